"""The trace-sampling operator of --trace_interp (K x K taps per trace: linear / cubic / sinc8) and its transpose, restated in float64 from
the definition in include/dpi_hip.h, and the case tables the host and the GPU tests share.  Independent of the library: the weights come
from numpy (np.sinc, np.i0), the forward pass is a gather, the adjoint a scatter, the dense matrix a third spelling; the dot test ties them.

Tensors are (C, T, X, Y), offsets (2, X, Y) with plane 0 = dx and plane 1 = dy, weight tables (2, K, X, Y): axis, tap, trace."""
import numpy as np

from trace_sampling_cases import OFFSET_KINDS, SHAPE_IDS as _IDS, SHAPES as _SHAPES, offsets_for          # noqa: F401

U23 = 2.0 ** -23
TAPS = {"linear": 2, "cubic": 4, "sinc8": 8}
KINDS = ["linear", "cubic", "sinc8"]                      # the library's kind numbers 0 / 1 / 2
SINC8_BETA = 6.0

# trace_sampling_cases.SHAPES (every tap clamps onto one node; the 2-D layout, once past a wavefront with a tail; narrower than K with
# both sides clamping; several tiles with odd tails; the block-index limit along t; aligned) and the first grid wider than K on both axes
SHAPES = list(_SHAPES) + [(1, 3, 9, 12)]
SHAPE_IDS = list(_IDS) + ["1x3x9x12"]


def _kernel(u, interp):
    s = np.abs(u)
    if interp == "linear":
        return 1.0 - s
    if interp == "cubic":
        # 1.5 s^3 - 2.5 s^2 + 1 and -0.5 s^3 + 2.5 s^2 - 4 s + 2, each in its factored spelling: as written, the cancellation between terms
        # of size ~6 alone puts 2.4e-15 on the sum of the four weights; factored, the sum is 1 within 4e-16
        return np.where(s <= 1.0, 1.0 - s * s * (2.5 - 1.5 * s), np.where(s < 2.0, -0.5 * (s - 1.0) * (s - 2.0) * (s - 2.0), 0.0))
    if interp == "sinc8":
        return np.sinc(u) * np.i0(SINC8_BETA * np.sqrt(np.maximum(0.0, 1.0 - (u / 4.0) ** 2))) / np.i0(SINC8_BETA)
    raise ValueError(interp)


def exact_sum(w, axis):
    """The sum of a few float64 values rounded once (taken in extended precision): what the weights sum to, not what summing them adds."""
    return np.asarray(w, dtype=np.longdouble).sum(axis=axis).astype(np.float64)


def weights64(off, interp):
    """(2, K, X, Y) float64: w(u) at u = (first + k) - (i + d) = (k - K/2 + (d >= 0)) - d from the fp32 offsets; sinc8 divided by the sum of
    its eight values; d == 0 the unit tap on the trace's own node with exact zeros around it."""
    K = TAPS[interp]
    d = np.asarray(off, dtype=np.float32).astype(np.float64)                     # (2, X, Y)
    k = np.arange(K, dtype=np.float64).reshape(1, K, 1, 1)
    u = (k - K // 2 + (d >= 0)[:, None]) - d[:, None]
    w = _kernel(u, interp)
    if interp == "sinc8":
        w = w / exact_sum(w, axis=1)[:, None]
    unit = (np.arange(K) == K // 2 - 1).astype(np.float64).reshape(1, K, 1, 1)
    return np.where((d == 0)[:, None], unit, w)


def tap_indices(off, K):
    """(tx, ty): (K, X, Y) integer arrays, clamp(i - K/2 + (d >= 0) + k, 0, n - 1) per axis."""
    off = np.asarray(off)
    _, X, Y = off.shape
    k = np.arange(K).reshape(K, 1, 1)
    tx = np.arange(X).reshape(1, X, 1) - K // 2 + (off[0] >= 0)[None].astype(np.int64) + k
    ty = np.arange(Y).reshape(1, 1, Y) - K // 2 + (off[1] >= 0)[None].astype(np.int64) + k
    return np.clip(tx, 0, X - 1), np.clip(ty, 0, Y - 1)


def forward64(x, off, interp, w=None):
    """y[c][t][x][y] = sum_kx wx[kx] * (sum_ky wy[ky] * in[c][t][tap_x][tap_y]) in float64; w: another table than weights64's."""
    x = np.asarray(x, dtype=np.float64)
    K = TAPS[interp]
    w = weights64(off, interp) if w is None else np.asarray(w, dtype=np.float64)
    tx, ty = tap_indices(off, K)
    out = np.zeros_like(x)
    for kx in range(K):
        inner = np.zeros_like(x)
        for ky in range(K):
            inner += w[1, ky] * x[:, :, tx[kx], ty[ky]]
        out += w[0, kx] * inner
    return out


def adjoint64(y, off, interp, w=None):
    """The transpose as a scatter: every trace adds wx * wy * y[c][t][trace] onto each of its K x K clamped taps, in float64."""
    y = np.asarray(y, dtype=np.float64)
    C, T, X, Y = y.shape
    K = TAPS[interp]
    w = weights64(off, interp) if w is None else np.asarray(w, dtype=np.float64)
    tx, ty = tap_indices(off, K)
    out = np.zeros((X * Y, C * T))                                               # node-major: np.add.at adds up nodes hit more than once
    flat = y.reshape(C * T, X * Y).T
    for kx in range(K):
        for ky in range(K):
            node = (tx[kx] * Y + ty[ky]).reshape(-1)
            np.add.at(out, node, flat * (w[0, kx] * w[1, ky]).reshape(-1, 1))
    return np.ascontiguousarray(out.T).reshape(C, T, X, Y)


def dense_matrix(off, interp, w=None):
    """R as an (X*Y) x (X*Y) float64 matrix, row = trace, column = node: entry = the sum of wx * wy over the taps of the trace on the node."""
    off = np.asarray(off)
    _, X, Y = off.shape
    K = TAPS[interp]
    w = weights64(off, interp) if w is None else np.asarray(w, dtype=np.float64)
    tx, ty = tap_indices(off, K)
    M = np.zeros((X * Y, X * Y))
    rows = np.arange(X * Y)
    for kx in range(K):
        for ky in range(K):
            np.add.at(M, (rows, (tx[kx] * Y + ty[ky]).reshape(-1)), (w[0, kx] * w[1, ky]).reshape(-1))
    return M


def structure(off, K):
    """Boolean (X*Y) x (X*Y): where a tap of the trace (row) lands on the node (column), whatever its weight."""
    off = np.asarray(off)
    _, X, Y = off.shape
    tx, ty = tap_indices(off, K)
    hit = np.zeros((X * Y, X * Y), dtype=bool)
    rows = np.arange(X * Y)
    for kx in range(K):
        for ky in range(K):
            hit[rows, (tx[kx] * Y + ty[ky]).reshape(-1)] = True
    return hit


def forward_tolerance(w32, x):
    """(K^2 + 2) * 2^-23 * A * max|x|: K^2 products and their sums, two roundings that form the weights; A = the largest sum |wx| |wy| over
    the traces, from the fp32 table (1 for linear: trace_sampling_cases.tolerance; <= 1.5625 cubic, <= 2.55 sinc8)."""
    w = np.abs(np.asarray(w32, dtype=np.float64))
    K = w.shape[1]
    A = float((w[0].sum(axis=0) * w[1].sum(axis=0)).max())
    return (K * K + 2) * U23 * A * float(np.abs(x).max())


def adjoint_counts(off, w32):
    """(n, B): the largest number of (trace, tap) pairs that land on one node, and the largest absolute coefficient sum of a node."""
    off = np.asarray(off)
    _, X, Y = off.shape
    w = np.abs(np.asarray(w32, dtype=np.float64))
    K = w.shape[1]
    tx, ty = tap_indices(off, K)
    n, B = np.zeros(X * Y), np.zeros(X * Y)
    for kx in range(K):
        for ky in range(K):
            node = (tx[kx] * Y + ty[ky]).reshape(-1)
            np.add.at(n, node, 1.0)
            np.add.at(B, node, (w[0, kx] * w[1, ky]).reshape(-1))
    return int(n.max()), float(B.max())


def adjoint_tolerance(off, w32, y):
    """(n + 2) * 2^-23 * B * max|y| with (n, B) = adjoint_counts of the case at hand."""
    n, B = adjoint_counts(off, w32)
    return (n + 2) * U23 * B * float(np.abs(y).max())


def plane_wave_error(interp, k_over_nyquist, steps=101):
    """Worst |R e^{ikx} - e^{ik(x + d)}| over d in [-0.5, 0.5] on one axis, away from the edges."""
    K = TAPS[interp]
    kk = np.pi * k_over_nyquist
    worst = 0.0
    for d in np.linspace(-0.5, 0.5, steps).astype(np.float32):
        w = weights64(np.full((2, 1, 1), d, dtype=np.float32), interp)[0, :, 0, 0]
        pos = np.arange(K) - K // 2 + (1 if d >= 0 else 0)
        worst = max(worst, abs(np.sum(w * np.exp(1j * kk * pos)) - np.exp(1j * kk * float(d))))
    return worst


def snr_db(ref, got):
    ref, got = np.asarray(ref, np.float64), np.asarray(got, np.float64)
    return float(10.0 * np.log10(np.sum(ref ** 2) / np.sum((ref - got) ** 2)))
