"""--model_reg: the numpy restatement the host and the GPU tests share (a plain module: no torch, no GPU), written from the definition

    R(m)    = (1/N) sum_{a in A} sum_{i : i + e_a inside} |m[i + e_a] - m[i]|          (A empty: (1/N) sum_i |m[i]|)
    dR/dm[i] = k[i] / N,  k[i] = sum_{a in A} ( sgn(m[i] - m[i - e_a]) [i_a >= 1] - sgn(m[i + e_a] - m[i]) [i_a < n_a - 1] )
               (A empty: k[i] = sgn(m[i]));  sgn(0) = 0

on m = [C][n0][n1][n2], N = m.size, A = the axes named by the bits of `axes` (bit k: n_k; the channel axis is never differenced).

Every |a - b| is formed in the dtype of m — float32 for what the kernel reads, so the terms are the kernel's own — and summed in float64;
the signs come from float64 differences of the values, which are exact for float32 inputs.  k is an integer array."""
import numpy as np

SHAPES = [(1, 5, 1, 1), (2, 7, 3, 1), (1, 1, 33, 65), (3, 9, 6, 5), (1, 130, 7, 10), (1, 257, 1, 129), (2, 4, 8, 8)]
# past 2048 workgroups of 256 quads: the kernel's grid-stride loop takes a second turn (65 * 129 * 65 = 545 025 quads > 524 288)
LARGE = (1, 65, 129, 260)
AXES = list(range(8))


def restate(m, axes):
    """(R, k, n_terms, sum of the terms) of m = [C][n0][n1][n2] (float32 or float64) for the bit mask `axes`."""
    m = np.asarray(m)
    assert m.ndim == 4 and 0 <= axes <= 7
    k = np.zeros(m.shape, dtype=np.int64)
    m64 = m.astype(np.float64)
    total, n_terms = 0.0, 0
    if axes == 0:
        k = np.sign(m64).astype(np.int64)
        total, n_terms = float(np.abs(m).astype(np.float64).sum()), m.size
    for a in range(3):
        if not axes >> a & 1:
            continue
        ax = a + 1
        s = np.sign(np.diff(m64, axis=ax)).astype(np.int64)          # sgn(m[i + e] - m[i]), i_a < n_a - 1
        lo = [slice(None)] * 4
        hi = [slice(None)] * 4
        lo[ax], hi[ax] = slice(None, -1), slice(1, None)
        k[tuple(hi)] += s
        k[tuple(lo)] -= s
        terms = np.abs(np.diff(m, axis=ax))                          # in the dtype of m
        total += float(terms.astype(np.float64).sum())
        n_terms += terms.size
    return total / m.size, k, n_terms, total


def grad32(k):
    """What the kernel stores: float32(k) / float32(N), one rounding."""
    return (k.astype(np.float32) / np.float32(k.size)).astype(np.float32)


def bar(m, axes):
    """(R, k, bar): the restatement and the bound on what another order of its double sum and the final division may change:
    n_terms * 2^-53 * sum|terms| + 2^-52 * |R|."""
    R, k, n_terms, total = restate(m, axes)
    return R, k, n_terms * 2.0 ** -53 * total + 2.0 ** -52 * abs(R)


def generic(shape, seed=0):
    """Normal values, float32: ties have probability ~0."""
    return np.random.RandomState(seed).standard_normal(shape).astype(np.float32)


def integers(shape, seed=1):
    """Small integers in [-2, 2]: neighbours tie often, zeros occur."""
    return np.random.RandomState(seed).randint(-2, 3, shape).astype(np.float32)


def dims_to_bits(dims, ndim):
    """Dims of the device tensor (1, C, n0, n1[, n2]) -> the bit mask of [C][n0][n1][n2], a 4-D tensor passed as n0 = 1."""
    return sum(1 << (d - 2 + 5 - ndim) for d in dims)


def as_4d(x):
    """The device tensor (1, C, a, b[, c]) as the [C][n0][n1][n2] array the entry point sees."""
    x = np.asarray(x)
    assert x.shape[0] == 1 and x.ndim in (4, 5)
    return x.reshape((x.shape[1],) + (1,) * (5 - x.ndim) + x.shape[2:])
