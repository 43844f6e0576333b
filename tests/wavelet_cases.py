"""Cases and the float64 reference of the --wavelet operator (dpi_wavelet_fwd / dpi_wavelet_adj), shared by tests/test_wavelet_host.py and
tests/test_gpu_wavelet.py.  A plain module: no GPU needed to import it.

The reference is composed from oracle.dpi_oracle.conv_same_axis_np and vertical_grad_np, both pinned against the reference's own
recordings (tests/test_oracle_golden.py), fed with the fp32-rounded taps and inputs.

Error bar, derived (nothing measured).  Every output is an fp32 fmaf chain of K terms; with diff = 1 each term of the forward pass holds one
more rounding (the difference) and the adjoint ends in one more addition.  Standard forward error analysis of such a chain gives
    |err| <= (K + 4) * 2^-24 * sum_k |taps_k| |u|
per element, with |u| = |m| (diff = 0) or |m[t + 1]| + |m[t]| (diff = 1, forward); for the adjoint with diff = 1 the magnitudes of the two
filtered rows that meet in an output add up.  The magnitude sums are computed with the same oracle functions on absolute values."""
import functools

import numpy as np

from oracle import dpi_oracle as O

U24 = 2.0 ** -24

# (C, T, S): T shorter than the half-width of the longer wavelets, row-tile seams (130 and 257 rows over 128-row tiles), S that is no
# multiple of 4 or of the 64-column strip, several channels
SHAPES = [(1, 5, 1), (2, 7, 3), (1, 33, 65), (3, 130, 70), (1, 257, 129)]
KS = [1, 3, 9, 65]
CASES = [(c, t, s, k) for (c, t, s) in SHAPES for k in KS] + [(1, 130, 64, 255)]          # + the longest wavelet (four chunks of taps)
IDS = ["%dx%dx%d-K%d" % c for c in CASES]


def taps_for(K, seed=0):
    """K asymmetric fp32 taps (convolution and correlation cannot be confused): white noise under a one-sided decay."""
    rng = np.random.RandomState(1000 + 7 * K + seed)
    w = rng.standard_normal(K) * np.exp(-np.arange(K) / max(K / 3.0, 1.0)) + 0.25 * np.linspace(-1.0, 0.5, K)
    w = w.astype(np.float32)
    assert K == 1 or not np.array_equal(w, w[::-1])
    return w


def vectors(C, T, S, seed=0):
    """(m, d): fp32 model- and data-side vectors of shape (1, C, T, S)."""
    rng = np.random.RandomState(seed + 13 * C + 101 * T + 7 * S)
    return rng.standard_normal((1, C, T, S)).astype(np.float32), rng.standard_normal((1, C, T, S)).astype(np.float32)


def forward64(m, taps, diff):
    """(d, magnitude) in float64 for m (1, C, T, ...): d = taps * (D m if diff else m) along axis 2."""
    m = np.asarray(m, dtype=np.float64)
    t = np.asarray(taps, dtype=np.float64)
    if diff:
        u = O.vertical_grad_np(m)
        mag = np.zeros_like(m)
        mag[:, :, :-1] = np.abs(m[:, :, 1:]) + np.abs(m[:, :, :-1])
    else:
        u, mag = m, np.abs(m)
    return O.conv_same_axis_np(u, t, 2), O.conv_same_axis_np(mag, np.abs(t), 2)


def adjoint64(d, taps, diff):
    """(m, magnitude) in float64: the transpose of forward64 — the correlation with the taps (= the convolution with the reversed taps, K
    odd), then D^T."""
    d = np.asarray(d, dtype=np.float64)
    t = np.asarray(taps, dtype=np.float64)[::-1]
    g, mag = O.conv_same_axis_np(d, t, 2), O.conv_same_axis_np(np.abs(d), np.abs(t), 2)
    if not diff:
        return g, mag
    both = np.zeros_like(mag)
    both[:, :, :-1] += mag[:, :, :-1]                          # |-g[t]| for t < T - 1
    both[:, :, 1:] += mag[:, :, :-1]                           # |g[t - 1]| for t >= 1
    return O.vertical_grad_np(g, adjoint=True), both


def bound(K, mag):
    return (K + 4) * U24 * mag


@functools.lru_cache(maxsize=None)
def case(C, T, S, K, diff):
    """Everything a test of one case needs, computed once: taps, the two vectors, both references and both bounds.  Read-only."""
    taps = taps_for(K)
    m, d = vectors(C, T, S)
    fwd, fmag = forward64(m, taps, diff)
    adj, amag = adjoint64(d, taps, diff)
    out = dict(taps=taps, m=m, d=d, fwd=fwd, fwd_bound=bound(K, fmag), adj=adj, adj_bound=bound(K, amag))
    for v in out.values():
        v.setflags(write=False)
    return out
