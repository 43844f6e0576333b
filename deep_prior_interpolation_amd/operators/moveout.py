"""Moveout along the time axis (ours, --moveout: the reference warps no axis).  d = L m: the model m is the flattened gather the network
writes, d what the loss sees; a table tau[t][s] names, for every recorded sample, the fractional row of its own trace the sample is read
from.  forward / adjoint are dpi_moveout_fwd / dpi_moveout_adj (include/dpi_hip.h has the definition): linear or cubic (Keys) along t,
edges clamped, the adjoint a deterministic gather over ranges built here, once, from the monotone table.  `shift_table` and `nmo_table`
build the usual tables: statics / LMO / flattening on a horizon, and hyperbolic NMO with a stretch mute."""
import numpy as np
import torch

from .. import _lib
from .base import LinearOperator

__all__ = ["Moveout", "check_moveout_table", "MOVEOUT_TAPS", "MOVEOUT_MUTE", "shift_table", "nmo_table", "moveout_ranges"]

MOVEOUT_TAPS = {"linear": 2, "cubic": 4}       # taps along t; the position in this table is the library's interp number
MOVEOUT_MUTE = -1.0                            # what the table builders write for a muted sample (any finite value outside [0, T - 1] is one)
_TAP_SPAN = {"linear": (0, 1), "cubic": (-1, 2)}          # first and last tap row relative to floor(tau)


def shift_table(shape, shifts):
    """tau[t, x(, y)] = t - shifts[x(, y)], float64, for `shape` = (T, X) or (T, X, Y): a static, a linear moveout (shifts = offset /
    velocity) or flattening on a horizon (shifts = horizon - datum).  Samples that would be read from outside [0, T - 1] are muted by
    the operator itself."""
    shape = tuple(int(n) for n in shape)
    sh = np.asarray(shifts, dtype=np.float64)
    if len(shape) not in (2, 3) or sh.shape != shape[1:]:
        raise ValueError("shifts %s do not belong to a table of shape %s: expected %s" % (tuple(sh.shape), shape, shape[1:]))
    if not np.all(np.isfinite(sh)):
        raise ValueError("shifts hold non-finite values")
    t = np.arange(shape[0], dtype=np.float64).reshape((-1,) + (1,) * sh.ndim)
    return t - sh[None]


def nmo_table(shape, offset, velocity, stretch_mute=None):
    """The table of the hyperbolic travel time t(tau) = sqrt(tau^2 + (offset[x(, y)] / velocity(tau))^2), everything in samples and cells:
    tau[t, x(, y)] is the zero-offset time the recorded sample t belongs to, float64, MOVEOUT_MUTE where muted.  `velocity` is a callable
    of tau (float64 arrays) or T values at tau = 0 .. T - 1 (interpolated linearly between them), in cells per sample.  t(tau) is
    inverted on the branch where it increases after its minimum over tau = 0 .. T - 1: the unit interval that brackets t is found on
    that grid and bisected to the last bit.  Muted: where t(tau) does not increase across the bracket, before the first arrival (t below
    the minimum), past the last model row (t above t(T - 1)), and, with `stretch_mute`, where the stretch d tau / d t — one over the
    rise of t(tau) across the bracket — exceeds it."""
    shape = tuple(int(n) for n in shape)
    off = np.asarray(offset, dtype=np.float64)
    if len(shape) not in (2, 3) or off.shape != shape[1:]:
        raise ValueError("offset %s does not belong to a table of shape %s: expected %s" % (tuple(off.shape), shape, shape[1:]))
    if not np.all(np.isfinite(off)):
        raise ValueError("offset holds non-finite values")
    if stretch_mute is not None and not float(stretch_mute) > 0.0:
        raise ValueError("stretch_mute must be > 0, got %r" % (stretch_mute,))
    T = shape[0]
    if callable(velocity):
        vel = lambda tau: np.asarray(velocity(tau), dtype=np.float64)
    else:
        v = np.asarray(velocity, dtype=np.float64)
        if v.shape != (T,):
            raise ValueError("velocity must be a callable or %d values, got %s" % (T, tuple(v.shape)))
        vel = lambda tau: np.interp(tau, np.arange(T, dtype=np.float64), v)
    grid = np.arange(T, dtype=np.float64)
    vg = vel(grid)
    if vg.shape != (T,) or not np.all(np.isfinite(vg)) or not np.all(vg > 0.0):
        raise ValueError("velocity must be finite and > 0 at every tau = 0 .. %d" % (T - 1))
    off = off.reshape(1, -1)                                     # (1, S)
    S = off.shape[1]
    travel = lambda tau: np.sqrt(tau ** 2 + (off / vel(tau)) ** 2)
    if T == 1:
        return np.where(off == 0.0, 0.0, MOVEOUT_MUTE).reshape(shape)
    g = travel(grid[:, None])                                    # (T, S) on the grid of tau
    jmin = (T - 1) - np.argmin(g[::-1], axis=0)                  # the last minimum: the branch starts there
    rows = grid[:, None]
    branch = np.where(rows >= jmin[None], g, -np.inf)
    env = np.maximum.accumulate(branch, axis=0)                  # non-decreasing: searchable
    t = grid
    j = np.empty((T, S), dtype=np.int64)
    for s in range(S):
        j[:, s] = np.searchsorted(env[:, s], t, side="right") - 1
    j = np.clip(j, 0, T - 2)
    cols = np.arange(S)[None]
    g0, g1 = g[j, cols], g[j + 1, cols]
    live = (j >= jmin[None]) & (env[j, cols] == g0) & (env[j + 1, cols] == g1) & (g1 > g0) & (t[:, None] >= g0) & (t[:, None] <= g1)
    if stretch_mute is not None:
        with np.errstate(divide="ignore"):
            live &= 1.0 / (g1 - g0) <= float(stretch_mute)
    lo, hi = j.astype(np.float64), j.astype(np.float64) + 1.0
    want = np.broadcast_to(t[:, None], (T, S))
    for _ in range(56):                                          # the bracket is one sample wide: 2^-56 of it is below the last bit
        mid = 0.5 * (lo + hi)
        below = travel(mid) <= want
        lo = np.where(below, mid, lo)
        hi = np.where(below, hi, mid)
    # lo is the last tau found with t(tau) <= t, hi the first one above: a sample that sits on a grid value of t(tau) gets that row exactly
    tau = np.clip(np.where(travel(hi) == want, hi, lo), 0.0, float(T - 1))
    return np.where(live, tau, MOVEOUT_MUTE).reshape(shape)


def moveout_ranges(table32, interp):
    """The adjoint's walk: range[0, i, s] <= t < range[1, i, s] holds every live sample of column s with a tap on model row i, int32
    (2, T, S), for the fp32 table (T, S) whose live values do not decrease along t.  The live samples of a column are then sorted by
    floor(tau), so those with i - last <= floor(tau) <= i - first (first, last: the tap span; clamping makes the bounds of rows 0 and
    T - 1 one-sided by itself) are one run of the live samples: counted per column (the searchsorted of the sorted floors, for all rows
    at once) and mapped back to t through the order of the live samples.  An empty run is (0, 0)."""
    first, last = _TAP_SPAN[interp]
    T, S = table32.shape
    live = (table32 >= 0) & (table32 <= np.float32(T - 1))
    i0 = np.floor(np.where(live, table32, 0)).astype(np.int64)
    hist = np.zeros((T + 1, S), dtype=np.int64)
    tt, ss = np.nonzero(live)
    np.add.at(hist, (i0[tt, ss] + 1, ss), 1)
    below = np.cumsum(hist, axis=0)                              # below[j, s] = live samples of column s with floor(tau) < j, j = 0 .. T
    order = np.argsort(~live, axis=0, kind="stable")             # per column: the live t ascending, then the muted ones
    rows = np.arange(T, dtype=np.int64)[:, None]
    cols = np.arange(S)[None]
    a = below[np.clip(rows - last, 0, T), cols]                  # rank of the first live sample with floor(tau) >= i - last
    b = below[np.clip(rows - first + 1, 0, T), cols]             # one past the rank of the last one with floor(tau) <= i - first
    some = b > a
    t0 = np.where(some, order[np.minimum(a, T - 1), cols], 0)
    t1 = np.where(some, order[np.clip(b - 1, 0, T - 1), cols] + 1, 0)
    return np.ascontiguousarray(np.stack([t0, t1]).astype(np.int32))


def check_moveout_table(table, what="the moveout table"):
    """table (T, X) or (T, X, Y) -> (the contiguous fp32 table as the kernels read it, the boolean map of its live samples).  ValueError
    for a table that is not 2-D or 3-D real, for non-finite values and for live values that decrease along t within a trace (the first
    such trace is named)."""
    tab = table.detach().cpu().numpy() if torch.is_tensor(table) else np.asarray(table)
    if tab.ndim not in (2, 3) or tab.size < 1 or tab.dtype.kind not in "fiu":
        raise ValueError("%s must be a non-empty (T, X) or (T, X, Y) array of real numbers, got %s %s"
                         % (what, tab.dtype, tuple(tab.shape)))
    if not np.all(np.isfinite(tab)):
        raise ValueError("%s holds non-finite values (mute a sample with %g)" % (what, MOVEOUT_MUTE))
    with np.errstate(over="ignore"):
        tab32 = np.ascontiguousarray(tab, dtype=np.float32)                                   # the one rounding
    tab32 = np.where(np.isfinite(tab32), tab32, np.float32(MOVEOUT_MUTE))                     # beyond fp32: far outside, muted
    T = int(tab32.shape[0])
    if T > (1 << 24):
        raise ValueError("%s has %d rows: at most 2^24" % (what, T))
    flat = tab32.reshape(T, -1)
    live = (flat >= 0) & (flat <= np.float32(T - 1))
    # live values must not decrease along t: against the largest live value above each sample
    seen = np.maximum.accumulate(np.where(live, flat, -np.inf), axis=0)
    bad = np.zeros_like(live)
    bad[1:] = live[1:] & (flat[1:] < seen[:-1])
    if bad.any():
        s = int(np.argmax(bad.any(axis=0)))
        t = int(np.argmax(bad[:, s]))
        trace = np.unravel_index(s, tab32.shape[1:])
        raise ValueError("%s decreases along t in trace %s: %g at t = %d after %g (events would cross; the live values "
                         "of a trace must not decrease)" % (what, tuple(int(v) for v in trace), float(flat[t, s]), t, float(seen[t - 1, s])))
    return tab32, live.reshape(tab32.shape)


class Moveout(LinearOperator):
    """forward: the model (1, C, T, X[, Y]) -> the data of the same shape, d[t] read from row table[t] of its own trace, `interp` =
    "linear" (2 taps) or "cubic" (4 taps, Keys a = -1/2) along t, rows clamped to [0, T - 1]; adjoint: the exact transpose.  `table` is
    (T, X) or (T, X, Y), shared by the channels; a sample is live where 0 <= table <= T - 1 and muted (d = 0) for any other finite value.
    The table is rounded ONCE to fp32 (`table`), `live` is the boolean map of its live samples; table and walk ranges go to a device once
    (`upload`, or the first call on it), so a captured iteration replays the operator unchanged.  ValueError, before any launch, for a
    table that is not 2-D or 3-D real, non-finite values, live values that decrease along t within a trace, an unknown interp, a tensor
    whose (T, X[, Y]) differs from the table's and a batch other than 1."""

    def __init__(self, table, interp="linear"):
        super().__init__()
        if interp not in MOVEOUT_TAPS:
            raise ValueError("unknown interpolation %r: expected one of %s" % (interp, ", ".join(MOVEOUT_TAPS)))
        tab32, live = check_moveout_table(table)
        T = int(tab32.shape[0])
        flat = tab32.reshape(T, -1)
        self.interp = interp
        self.kind = list(MOVEOUT_TAPS).index(interp)
        self.table = tab32
        self.live = live
        self.T, self.S = T, int(flat.shape[1])
        self._ranges = moveout_ranges(flat, interp)

    def _to_device(self, device):
        """(table, ranges)"""
        return torch.from_numpy(self.table).to(device), torch.from_numpy(self._ranges).to(device)

    def _matvec(self, x, adjoint):
        self._check_patch(x, ValueError, "Moveout expects a (1, C, T, X) or (1, C, T, X, Y) tensor, got %d-D")
        if tuple(x.shape[2:]) != tuple(self.table.shape) or x.shape[1] < 1:
            raise ValueError("Moveout built from a table of shape %s got a tensor of shape %s: its (T, X[, Y]) must be the table's"
                             % (tuple(self.table.shape), tuple(x.shape)))
        tau, ranges = self.upload(x.device)
        y = torch.empty_like(x)
        L = _lib.load()
        C_ = int(x.shape[1])
        if adjoint:
            _lib.check(L.dpi_moveout_adj(_lib.ptr(x), _lib.ptr(tau), _lib.ptr(ranges), self.kind, C_, self.T, self.S, _lib.ptr(y),
                                         _lib.stream()), "dpi_moveout_adj")
        else:
            _lib.check(L.dpi_moveout_fwd(_lib.ptr(x), _lib.ptr(tau), self.kind, C_, self.T, self.S, _lib.ptr(y), _lib.stream()),
                       "dpi_moveout_fwd")
        return y
