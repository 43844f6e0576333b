"""Cases and the float64 reference of the --moveout operator (dpi_moveout_fwd / dpi_moveout_adj), shared by tests/test_moveout_host.py
and tests/test_gpu_moveout.py.  A plain module: no GPU needed to import it.

The reference takes the fp32 table as given (the rounding of the table is the operator's definition, not its error) and forms the weights in
float64: forward64 is a gather with clamped taps, adjoint64 the scatter of the same taps with np.add.at, gather64 the adjoint written the
way the kernel walks it (per model row, over the ranges of operators.moveout.moveout_ranges).

Error bars, derived (nothing measured).  f = tau - floor(tau) is exact in fp32.  An fp32 weight is a Horner chain of at most 5 operations
on values of size <= 2.5, so it is within 6 * 2^-24 of the float64 weight, and |w| <= 1.  Each product rounds once and the K - 1 (forward)
or N - 1 (adjoint, N contributions to the row) additions round once each on partial sums bounded by sum |w x|.  Hence
    forward:  |err| <= (K + 12) * 2^-24 * sum_k |m_k|      over the K taps touched
    adjoint:  |err| <= (N + K + 12) * 2^-24 * sum |d_t|    over the N contributions of the row
with room to spare; a muted sample and a row nothing lands on have the bar 0: they must be exactly 0."""
import functools

import numpy as np

U24 = 2.0 ** -24
TAPS = {"linear": 2, "cubic": 4}
MUTE = -1.0

# (C, T, S): the wavelet cases' shapes — seams of any 64- or 128-wide tiling, S that is no multiple of 4, several channels
SHAPES = [(1, 5, 1), (2, 7, 3), (1, 33, 65), (3, 130, 70), (1, 257, 129)]
FAMILIES = ["identity", "shift", "stretch", "squeeze", "constant", "clamp_last", "sorted_gaps", "nmo", "all_muted"]
CASES = [(c, t, s, fam) for (c, t, s) in SHAPES for fam in FAMILIES]
IDS = ["%dx%dx%d-%s" % c for c in CASES]


def table_for(family, T, S, seed=0):
    """The fp32 table (T, S) of one family."""
    rng = np.random.RandomState(500 + 31 * T + 7 * S + seed)
    t = np.arange(T, dtype=np.float64)[:, None] * np.ones((1, S))
    if family == "identity":
        tab = t
    elif family == "shift":                                       # mute head, half-sample weights
        tab = t - 2.5
    elif family == "stretch":                                     # most model rows are never read
        tab = 3.0 * t + 0.25
    elif family == "squeeze":                                     # several t per row
        tab = 0.3 * t + 0.1
    elif family == "constant":                                    # the longest adjoint walk
        tab = np.full((T, S), 1.5)
    elif family == "clamp_last":                                  # taps clamped at the last row
        tab = np.minimum(t + 0.5, T - 1.0)
    elif family == "sorted_gaps":                                 # any monotone table, 30 % of it muted at random
        tab = np.sort(rng.uniform(0.0, T - 1.0, (T, S)), axis=0)
        tab[rng.uniform(size=(T, S)) < 0.3] = MUTE
    elif family == "nmo":                                         # sqrt(t^2 - h_s^2) behind a per-column mute head
        h = rng.uniform(0.0, 0.6 * T, (1, S))
        tab = np.where(t >= h, np.sqrt(np.maximum(t ** 2 - h ** 2, 0.0)), MUTE)
    elif family == "all_muted":
        tab = np.full((T, S), MUTE)
    else:
        raise ValueError(family)
    return np.ascontiguousarray(tab.astype(np.float32))


def vectors(C, T, S, seed=0):
    """(m, d): fp32 model- and data-side vectors of shape (1, C, T, S)."""
    rng = np.random.RandomState(seed + 13 * C + 101 * T + 7 * S)
    return rng.standard_normal((1, C, T, S)).astype(np.float32), rng.standard_normal((1, C, T, S)).astype(np.float32)


def taps64(table32, interp):
    """(live (T, S), rows (K, T, S) clamped, weights (K, T, S) float64) of the fp32 table; rows and weights of muted samples are 0."""
    tab = np.asarray(table32)
    assert tab.dtype == np.float32 and tab.ndim == 2
    T = tab.shape[0]
    tau = tab.astype(np.float64)
    live = (tau >= 0.0) & (tau <= T - 1.0)
    i0 = np.floor(np.where(live, tau, 0.0))
    f = np.where(live, tau, 0.0) - i0
    i0 = i0.astype(np.int64)
    if interp == "linear":
        first, w = 0, [1.0 - f, f]
    else:
        first = -1
        w = [((-.5 * f + 1.0) * f - .5) * f, (1.5 * f - 2.5) * f * f + 1.0, ((-1.5 * f + 2.0) * f + .5) * f, (.5 * f - .5) * f * f]
    rows = np.stack([np.clip(i0 + first + k, 0, T - 1) for k in range(len(w))])
    w = np.stack(w) * live[None]
    return live, rows * live[None], w


def forward64(m, table32, interp):
    """(d, magnitude) in float64 for m (1, C, T, S): the gather; magnitude = sum_k |m_k| over the taps of a live sample."""
    m = np.asarray(m, dtype=np.float64)
    live, rows, w = taps64(table32, interp)
    cols = np.arange(m.shape[3])[None]
    d, mag = np.zeros_like(m), np.zeros_like(m)
    for k in range(w.shape[0]):
        mk = m[:, :, rows[k], cols]
        d += w[k] * mk
        mag += np.abs(mk) * live
    return d, mag


def adjoint64(d, table32, interp):
    """(m, magnitude, N) in float64: the scatter of the same taps; magnitude = sum |d_t| and N = the count over the contributions of a
    row, a clamped tap counting like any other."""
    d = np.asarray(d, dtype=np.float64)
    live, rows, w = taps64(table32, interp)
    _, C, T, S = d.shape
    tt, ss = np.nonzero(live)
    m, mag, n = np.zeros_like(d), np.zeros_like(d), np.zeros((T, S))
    for k in range(w.shape[0]):
        r = rows[k][tt, ss]
        np.add.at(n, (r, ss), 1.0)
        for c in range(C):
            np.add.at(m[0, c], (r, ss), w[k][tt, ss] * d[0, c][tt, ss])
            np.add.at(mag[0, c], (r, ss), np.abs(d[0, c][tt, ss]))
    return m, mag, n


def gather64(d, table32, interp, ranges):
    """The adjoint the way the kernel walks it: row i of column s sums, in ascending t, the live samples ranges[0, i, s] <= t <
    ranges[1, i, s] whose tap lands on i."""
    d = np.asarray(d, dtype=np.float64)
    live, rows, w = taps64(table32, interp)
    _, C, T, S = d.shape
    m = np.zeros_like(d)
    for s in range(S):
        for i in range(T):
            for t in range(int(ranges[0, i, s]), int(ranges[1, i, s])):
                if live[t, s]:
                    for k in range(w.shape[0]):
                        if rows[k, t, s] == i:
                            m[0, :, i, s] += w[k, t, s] * d[0, :, t, s]
    return m


def fwd_bound(interp, mag):
    return (TAPS[interp] + 12) * U24 * mag


def adj_bound(interp, mag, n):
    return (n + TAPS[interp] + 12) * U24 * mag


@functools.lru_cache(maxsize=None)
def case(C, T, S, family, interp):
    """Everything a test of one case needs, computed once: the table, the two vectors, both references and both bounds.  Read-only."""
    table = table_for(family, T, S)
    m, d = vectors(C, T, S)
    fwd, fmag = forward64(m, table, interp)
    adj, amag, n = adjoint64(d, table, interp)
    out = dict(table=table, m=m, d=d, fwd=fwd, fwd_bound=fwd_bound(interp, fmag), adj=adj, adj_bound=adj_bound(interp, amag, n[None, None]))
    for v in out.values():
        v.setflags(write=False)
    return out
