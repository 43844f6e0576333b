"""The trace-sampling operator R of --trace_offsets and its transpose, restated in float64 from the definition in include/dpi_hip.h, and the
case tables the host and the GPU tests share.  No reference code exists for R: this restatement is the yardstick.

Tensors are (C, T, X, Y), offsets (2, X, Y) with plane 0 = dx and plane 1 = dy.  `forward64` is the gather of the definition, `adjoint64`
scatters every trace's four weighted taps onto the grid (np.add.at): written independently of each other, tied together by the dot test."""
import numpy as np

U23 = 2.0 ** -23

# (C, T, X, Y): the smallest problem; the 2-D layout (Y = 1), one of them past a wavefront with a tail; odd 3-D sizes; more than one
# workgroup of trace columns with an odd tail; past the 65535 block-index limit along t; aligned
SHAPES = [(1, 1, 1, 1), (2, 3, 2, 1), (1, 5, 67, 1), (2, 3, 5, 7), (1, 2, 33, 67), (1, 70000, 2, 3), (3, 4, 16, 64)]
SHAPE_IDS = ["x".join(str(n) for n in s) for s in SHAPES]
OFFSET_KINDS = ["zero", "plus_half", "minus_half", "random"]
N_TERMS_FWD, N_TERMS_ADJ = 4, 36          # 2 x 2 taps; 9 traces with at most 4 taps each


def offsets_for(kind, X, Y, seed=0):
    """(2, X, Y) fp32: all zero, all +0.5, all -0.5 (every edge trace clamps), or uniform in [-0.5, 0.5] with exact zeros mixed in."""
    if kind == "zero":
        return np.zeros((2, X, Y), dtype=np.float32)
    if kind == "plus_half":
        return np.full((2, X, Y), 0.5, dtype=np.float32)
    if kind == "minus_half":
        return np.full((2, X, Y), -0.5, dtype=np.float32)
    if kind == "random":
        rng = np.random.RandomState(seed)
        off = rng.uniform(-0.5, 0.5, (2, X, Y)).astype(np.float32)
        off[rng.rand(2, X, Y) < 0.25] = 0.0
        return off
    raise ValueError(kind)


def tolerance(n_terms, x):
    """(n_terms + 2) * 2^-23 * max|input|: n_terms products of weights that sum to at most 1 per trace, their sum, and the two roundings
    that form a weight (1 - |d| and wx * wy)."""
    return (n_terms + 2) * U23 * float(np.abs(x).max())


def axis_taps(i, d, n):
    """The two taps of traces `i` (integer array) with offsets `d` on an axis of n nodes: (i0, i1, w0, w1), indices clamped to [0, n - 1].
    d >= 0: i, i + 1 with 1 - d, d;  d < 0: i - 1, i with -d, 1 + d.  Weights in float64 from the fp32 offset, exactly."""
    d = np.asarray(d, dtype=np.float64)
    i = np.broadcast_to(np.asarray(i, dtype=np.int64), d.shape)
    pos = d >= 0
    i0 = np.where(pos, i, i - 1)
    i1 = np.where(pos, i + 1, i)
    w0 = np.where(pos, 1.0 - d, -d)
    w1 = np.where(pos, d, 1.0 + d)
    return np.clip(i0, 0, n - 1), np.clip(i1, 0, n - 1), w0, w1


def trace_taps(off):
    """The 2 x 2 taps of every trace: a list of four (tap_x, tap_y, weight), each (X, Y)."""
    off = np.asarray(off)
    _, X, Y = off.shape
    x0, x1, wx0, wx1 = axis_taps(np.arange(X)[:, None], off[0], X)
    y0, y1, wy0, wy1 = axis_taps(np.arange(Y)[None, :], off[1], Y)
    return [(x0, y0, wx0 * wy0), (x0, y1, wx0 * wy1), (x1, y0, wx1 * wy0), (x1, y1, wx1 * wy1)]


def forward64(x, off):
    """y[c][t][x][y] = sum over the 2 x 2 taps of wx * wy * in[c][t][tap_x][tap_y], in float64."""
    x = np.asarray(x, dtype=np.float64)
    out = np.zeros_like(x)
    for tx, ty, w in trace_taps(off):
        out += w * x[:, :, tx, ty]
    return out


def adjoint64(y, off):
    """The transpose: every trace adds w * y[c][t][trace] onto each of its four taps, in float64."""
    y = np.asarray(y, dtype=np.float64)
    C, T, X, Y = y.shape
    out = np.zeros((C * T, X * Y))
    flat = y.reshape(C * T, X * Y)
    for tx, ty, w in trace_taps(off):
        contrib = flat * w.reshape(1, -1)
        node = (tx * Y + ty).reshape(-1)
        for s in range(X * Y):                           # one trace column at a time: nodes hit twice (clamped taps) add up
            out[:, node[s]] += contrib[:, s]
    return out.reshape(C, T, X, Y)
