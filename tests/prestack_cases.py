"""Cases and the float64 restatement of the pre-stack convolutional model (--wavelet_domain; operators.PrestackModelling), shared by tests/test_prestack_host.py and tests/test_gpu_prestack.py.  A plain module: no GPU needed to import it.

The restatement composes the float64 references of the two factors: moveout_cases.forward64 / adjoint64 (L) and wavelet_cases.forward64 /
adjoint64 (W), in the order of the domain: "data" d = W L m, "model" d = L W m.

Error bars, derived from the bars of the factors (nothing measured, no new tolerance).  Write A = B2 B1 and let b1 be the factor's own bar
on the first result, whose magnitude sum is mag1 (both from the factor's reference).  The fp32 result of the first stage is within b1 of
the float64 one, and |B1 m| <= mag1 (|w| <= 1 for every moveout weight; the wavelet's magnitude sum is the triangle inequality itself).
The second stage then sees an input of magnitude at most mag1 + b1, on which its own bar applies, and carries the first stage's error
through |B2|:
    |err| <= bar2(|B2| (mag1 + b1)) + |B2| b1
with |B2| x the factor's magnitude sum of x >= 0: wavelet_cases' convolution of |taps| with |x| (the two rows of the difference for an
impedance), moveout_cases' sum over the taps of a sample (each |w| <= 1 counted as 1).  The adjoint is the same statement on the
transposed factors in reverse order."""
import functools

import numpy as np

import moveout_cases as M
import wavelet_cases as W

DOMAINS = ["data", "model"]
KINDS = ["reflectivity", "impedance"]
INTERPS = ["linear", "cubic"]
TABLES = ["identity", "fractional_shift", "nmo_mutes", "constant", "mute_gap"]
# ((1, C, T, X[, Y]), K, table): every table once, 4-D and 5-D; T below a 128-row tile, one row past one and past two tiles; S of one
# lane, one short of, one past and two strips of 64 columns past; K = 65 fills one chunk of taps, 67 is the first length with two
OP_CASES = [((1, 1, 2, 1), 1, "constant"), ((1, 3, 33, 7, 9), 3, "nmo_mutes"), ((1, 1, 33, 65), 3, "fractional_shift"),
            ((1, 1, 129, 130), 65, "mute_gap"), ((1, 1, 257, 65), 67, "nmo_mutes"), ((1, 3, 1, 63), 1, "identity")]
OP_IDS = ["%s-K%d-%s" % ("x".join(str(n) for n in shape[1:]), K, family) for shape, K, family in OP_CASES]


def table_for(family, T, S):
    """The fp32 table (T, S) of one family."""
    t = np.arange(T, dtype=np.float64)[:, None] * np.ones((1, S))
    col = np.arange(S, dtype=np.float64)[None]
    if family == "identity":
        tab = t
    elif family == "fractional_shift":                            # a mute head of one or two rows, weights off the grid
        tab = t - 1.375
    elif family == "nmo_mutes":                                   # a top wedge that grows with the column and a stretch mute below it
        h = 0.7 * T * (col + 1.0) / S
        tab = np.where(t >= h, np.sqrt(np.maximum(t ** 2 - h ** 2, 0.0)), M.MUTE)
        with np.errstate(divide="ignore", invalid="ignore"):
            stretch = np.where(tab > 0, t / np.maximum(tab, 1e-30), np.inf)          # d tau / d t of the hyperbola
        tab = np.where((tab >= 0) & (stretch <= 2.5), tab, M.MUTE)
        tab[:, 0] = t[:, 0]                                       # the zero-offset trace stays whole
    elif family == "constant":
        tab = np.full((T, S), min(1.5, T - 1.0))
    elif family == "mute_gap":                                    # live, a gap inside the trace, live again; the gap moves with the column
        tab = 0.75 * t + 0.2
        lo = (T // 3 + (np.arange(S) % 5))[None]
        tab = np.where((t >= lo) & (t < lo + max(1, T // 8)), M.MUTE, tab)
    else:
        raise ValueError(family)
    return np.ascontiguousarray(tab.astype(np.float32))


def erode64(live, K, diff):
    """The live map of --wavelet_domain data by brute force: a loop over the samples and over the rows the wavelet reads for each."""
    live = np.asarray(live, dtype=bool)
    T = live.shape[0]
    flat = live.reshape(T, -1)
    out = np.zeros_like(flat)
    p = K // 2
    for s in range(flat.shape[1]):
        for t in range(T):
            rows = [q for q in range(t - p, t + p + diff + 1) if 0 <= q < T]
            out[t, s] = all(flat[q, s] for q in rows)
    return out.reshape(live.shape)


def _w_mag(x, taps, diff):
    return W.forward64(x, taps, diff)[1]


def _l_mag(x, table, interp):
    return M.forward64(x, table, interp)[1]


def forward64(m, taps, diff, table, interp, domain):
    """(d, bound) in float64 for m (1, C, T, S) and the fp32 taps and table as the operator holds them."""
    K = len(taps)
    if domain == "data":
        u, mag1 = M.forward64(m, table, interp)
        b1 = M.fwd_bound(interp, mag1)
        d, _ = W.forward64(u, taps, diff)
        return d, W.bound(K, _w_mag(mag1 + b1, taps, diff)) + _w_mag(b1, taps, diff)
    u, mag1 = W.forward64(m, taps, diff)
    b1 = W.bound(K, mag1)
    d, _ = M.forward64(u, table, interp)
    return d, M.fwd_bound(interp, _l_mag(mag1 + b1, table, interp)) + _l_mag(b1, table, interp)


def adjoint64(d, taps, diff, table, interp, domain):
    """(m, bound) in float64: the transposes in reverse order."""
    K = len(taps)
    if domain == "data":                                          # (W L)^T = L^T W^T
        g, mag1 = W.adjoint64(d, taps, diff)
        b1 = W.bound(K, mag1)
        m, _, n = M.adjoint64(g, table, interp)
        return m, M.adj_bound(interp, M.adjoint64(mag1 + b1, table, interp)[1], n[None, None]) + M.adjoint64(b1, table, interp)[1]
    g, mag1, n = M.adjoint64(d, table, interp)                    # (L W)^T = W^T L^T
    b1 = M.adj_bound(interp, mag1, n[None, None])
    m, _ = W.adjoint64(g, taps, diff)
    return m, W.bound(K, W.adjoint64(mag1 + b1, taps, diff)[1]) + W.adjoint64(b1, taps, diff)[1]


@functools.lru_cache(maxsize=None)
def vectors(C, T, S):
    m, d = M.vectors(C, T, S, seed=3)
    for v in (m, d):
        v.setflags(write=False)
    return m, d
