"""Velocity estimation for --moveout (ours, --moveout_offset: the reference estimates no velocity).  A semblance scan over the known traces
of a gather (`semblance_sums`, dpi_semblance_sums on the device: include/dpi_hip.h has the definition), the panel of the sums
(`semblance_panel`), a picked law v(tau) per gather (`pick_velocity`, a Viterbi pass), optionally smoothed along tau (`smooth_law`,
--moveout_smooth) and the NMO table of the law (`scan_table`, through `nmo_table` on the host or `nmo_table_device`, dpi_nmo_table, on the
device).  Everything after the table is the path of --moveout.  The kernel sums in a fixed order and the host part is float64 numpy
in a fixed order as well: the same data give the same table on every device and every rank."""
import numpy as np
import torch

from .. import _lib
from .moveout import MOVEOUT_MUTE, check_moveout_table, nmo_table

__all__ = ["GATHERS", "TABLE_BUILDERS", "NMO_TABLE_DEVICE_ROWS", "gather_geometry", "semblance_sums", "semblance_panel", "pick_velocity", "smooth_law",
           "nmo_table_device", "scan_table", "velocity_windows"]

GATHERS = ("volume", "x", "y")
TABLE_BUILDERS = ("host", "device")
NMO_TABLE_DEVICE_ROWS = 4096                # dpi_nmo_table keeps a trace's travel times in LDS: at most this many rows


def gather_geometry(shape, gather="volume"):
    """(n_groups, group_stride, n_traces, trace_stride) of dpi_semblance_sums for a (T, X) section or a (T, X, Y) volume: `volume` = all
    traces are one gather, `y` = every y index is its own gather of X traces, `x` = every x index its own gather of Y traces.  A
    section has the one gather only."""
    shape = tuple(int(n) for n in shape)
    if len(shape) not in (2, 3) or min(shape) < 1:
        raise ValueError("a gather geometry needs a (T, X) or (T, X, Y) shape, got %s" % (shape,))
    if gather not in GATHERS:
        raise ValueError("gather must be one of %s, got %r" % (", ".join(GATHERS), gather))
    if len(shape) == 2:
        if gather != "volume":
            raise ValueError("a (T, X) section is one gather: gather must be volume, got %r" % (gather,))
        return 1, 0, shape[1], 1
    X, Y = shape[1:]
    return {"volume": (1, 0, X * Y, 1), "y": (Y, 1, X, Y), "x": (X, Y, Y, 1)}[gather]


def _check_velocities(velocities):
    vel = np.ascontiguousarray(np.asarray(velocities, dtype=np.float64).reshape(-1))
    if vel.size < 1 or not np.all(np.isfinite(vel)) or not np.all(vel > 0.0):
        raise ValueError("velocities must be at least one finite value > 0 (cells per sample), got %r" % (velocities,))
    return vel


def _check_offset(offset, shape):
    off = np.asarray(offset)
    if off.dtype.kind not in "fiu":
        raise ValueError("offset must hold real numbers, got %s" % off.dtype)
    if len(shape) == 2 and off.shape == (shape[1], 1):
        off = off[:, 0]
    if off.shape != tuple(shape[1:]):
        raise ValueError("offset %s does not belong to data of shape %s: expected %s" % (tuple(off.shape), tuple(shape), tuple(shape[1:])))
    off = np.ascontiguousarray(off, dtype=np.float64)
    if not np.all(np.isfinite(off)):
        raise ValueError("offset holds non-finite values")
    return off


def semblance_sums(data, mask, offset, velocities, gather="volume", stretch_mute=None, device=None):
    """(num, den, cnt) of dpi_semblance_sums as numpy, (G, NV, T) float64, float64 and int32: data and mask (T, X) or (T, X, Y) (mask:
    non-zero = known), offset (X,) / (X, 1) or (X, Y) in cells, velocities in cells per sample, `gather` as in gather_geometry,
    `stretch_mute` None = none, `device` the HIP device (None: the current one).  ValueError before any launch for shapes that do not
    belong together, non-finite offsets, velocities that are not finite and > 0, a stretch mute that is not > 0 and a gather the
    geometry does not have."""
    d = np.asarray(data)
    m = np.asarray(mask)
    if d.ndim not in (2, 3) or d.size < 1 or d.dtype.kind not in "fiu":
        raise ValueError("data must be a non-empty (T, X) or (T, X, Y) array of real numbers, got %s %s" % (d.dtype, tuple(d.shape)))
    if m.shape != d.shape:
        raise ValueError("mask %s does not belong to data of shape %s" % (tuple(m.shape), tuple(d.shape)))
    geo = gather_geometry(d.shape, gather)
    off = _check_offset(offset, d.shape)
    vel = _check_velocities(velocities)
    if stretch_mute is not None and not (float(stretch_mute) > 0.0 and np.isfinite(float(stretch_mute))):
        raise ValueError("stretch_mute must be a finite value > 0, got %r" % (stretch_mute,))
    T = int(d.shape[0])
    if T > (1 << 24):
        raise ValueError("data of %d rows: at most 2^24" % T)
    S = int(d.size // T)
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    with np.errstate(over="ignore", invalid="ignore"):
        d32 = np.ascontiguousarray(d, dtype=np.float32).reshape(T, S)
    known = np.ascontiguousarray((m != 0).reshape(T, S), dtype=np.float32)
    G, NV = geo[0], int(vel.size)
    with torch.cuda.device(dev):
        d_, m_ = torch.from_numpy(d32).to(dev), torch.from_numpy(known).to(dev)
        o_, v_ = torch.from_numpy(off.reshape(-1)).to(dev), torch.from_numpy(vel).to(dev)
        num = torch.empty((G, NV, T), dtype=torch.float64, device=dev)
        den = torch.empty_like(num)
        cnt = torch.empty((G, NV, T), dtype=torch.int32, device=dev)
        _lib.check(_lib.load().dpi_semblance_sums(_lib.ptr(d_), _lib.ptr(m_), _lib.ptr(o_), _lib.ptr(v_), NV,
                                                  0.0 if stretch_mute is None else float(stretch_mute), T, S, geo[0], geo[1], geo[2], geo[3],
                                                  _lib.ptr(num), _lib.ptr(den), _lib.ptr(cnt), _lib.stream()), "dpi_semblance_sums")
        return num.cpu().numpy(), den.cpu().numpy(), cnt.cpu().numpy()


def _box(a, window):
    """Sums over rows tau - window .. tau + window along the last axis, clipped at the ends, added in ascending row order."""
    T = a.shape[-1]
    out = np.zeros_like(a)
    for k in range(-window, window + 1):
        lo, hi = max(0, -k), min(T, T - k)
        if hi > lo:
            out[..., lo:hi] += a[..., lo + k:hi + k]
    return out


def semblance_panel(num, den, cnt, window=2, min_fold=4):
    """The sums (G, NV, T) -> the panel P (G, T, NV), float64: entries with cnt < min_fold are zeroed in all three arrays, then
    P = box(num^2) / box(cnt * den) with box the sum over the 2 * window + 1 rows around tau, clipped at the ends; P = 0 where the
    denominator is 0.  num^2 <= cnt * den row by row (Cauchy-Schwarz), so P lies in [0, 1] up to the rounding of the sums."""
    num, den = np.asarray(num, dtype=np.float64), np.asarray(den, dtype=np.float64)
    cnt = np.asarray(cnt)
    if num.ndim != 3 or den.shape != num.shape or cnt.shape != num.shape:
        raise ValueError("num, den and cnt must share one (G, NV, T) shape, got %s, %s, %s" % (num.shape, den.shape, cnt.shape))
    if int(window) != window or window < 0 or int(min_fold) != min_fold or min_fold < 0:
        raise ValueError("window and min_fold must be integers >= 0, got %r, %r" % (window, min_fold))
    keep = cnt >= int(min_fold)
    num, den, fold = np.where(keep, num, 0.0), np.where(keep, den, 0.0), np.where(keep, cnt, 0).astype(np.float64)
    top, bot = _box(num * num, int(window)), _box(fold * den, int(window))
    some = bot > 0.0
    return np.ascontiguousarray(np.swapaxes(np.where(some, top / np.where(some, bot, 1.0), 0.0), 1, 2))


def pick_velocity(panel, velocities, max_step=1, return_index=False):
    """The law v(tau) of every gather, (G, T) float64: per gather the path j(tau) over the columns of its panel (T, NV) that maximises
    sum_tau P[tau, j(tau)] subject to |j(tau + 1) - j(tau)| <= max_step, found by a Viterbi pass in float64 (the scores are added in
    ascending tau).  Ties go to the lowest index: at the last row, and at every step back among the admissible predecessors.  Nothing is
    smoothed across gathers.  `return_index`: (the law, the path j (G, T) int64) instead of the law alone."""
    P = np.asarray(panel, dtype=np.float64)
    vel = np.asarray(velocities, dtype=np.float64).reshape(-1)
    if P.ndim != 3 or P.shape[2] != vel.size or P.size < 1:
        raise ValueError("panel must be (G, T, NV) with NV = %d velocities, got %s" % (vel.size, tuple(P.shape)))
    if int(max_step) != max_step or max_step < 0:
        raise ValueError("max_step must be an integer >= 0, got %r" % (max_step,))
    path = _pick_index(P, int(max_step))
    return (vel[path], path) if return_index else vel[path]


def _pick_index(P, step):
    G, T, NV = P.shape
    score = P[:, 0].copy()                                       # (G, NV)
    back = np.zeros((G, T, NV), dtype=np.int64)
    cols = np.arange(NV)
    shifts = [k for k in range(-step, step + 1) if abs(k) < NV]  # ascending: np.argmax keeps the first = lowest predecessor
    for t in range(1, T):
        cand = np.full((len(shifts), G, NV), -np.inf)
        for n, k in enumerate(shifts):
            lo, hi = max(0, -k), min(NV, NV - k)
            cand[n, :, lo:hi] = score[:, lo + k:hi + k]
        best = np.argmax(cand, axis=0)                           # (G, NV)
        back[:, t] = cols[None] + np.asarray(shifts)[best]
        score = np.take_along_axis(cand, best[None], axis=0)[0] + P[:, t]
    path = np.empty((G, T), dtype=np.int64)
    j = np.argmax(score, axis=1)
    rows = np.arange(G)
    for t in range(T - 1, -1, -1):
        path[:, t] = j
        j = back[rows, t, j]
    return path


def smooth_law(law, weight, length):
    """The laws (G, T) smoothed along tau by a Gaussian of `length` = L rows weighted by `weight` (G, T) >= 0, float64: with K = ceil(3 L)
    and g_k = exp(-0.5 (k / L)^2), row tau becomes sum_k g_k w[r] v[r] / sum_k g_k w[r] over the rows r = tau + k, k = -K .. K, that lie
    inside [0, T - 1] (the window is clipped, not replicated), both sums added in ascending k; where the weights of a window are all zero,
    the unweighted sum_k g_k v[r] / sum_k g_k.  L = 0 returns `law` unchanged.  ValueError for shapes that do not match, negative or
    non-finite weights and a negative or non-finite L."""
    v = np.asarray(law, dtype=np.float64)
    w = np.asarray(weight, dtype=np.float64)
    if v.ndim != 2 or w.shape != v.shape or v.size < 1:
        raise ValueError("law and weight must share one (G, T) shape, got %s and %s" % (tuple(v.shape), tuple(w.shape)))
    L = float(length)
    if not (np.isfinite(L) and L >= 0.0):
        raise ValueError("the smoothing length must be finite and >= 0 (rows), got %r" % (length,))
    if not (np.all(np.isfinite(w)) and np.all(w >= 0.0)):
        raise ValueError("weight must be finite and >= 0")
    if L == 0.0:
        return v
    T = v.shape[1]
    K = min(int(np.ceil(3.0 * L)), T - 1)                        # rows further than T - 1 away lie outside every window
    num, den, plain, norm = (np.zeros_like(v) for _ in range(4))
    for k in range(-K, K + 1):
        gk = np.exp(-0.5 * (k / L) ** 2)
        lo, hi = max(0, -k), min(T, T - k)
        gw = gk * w[:, lo + k:hi + k]
        num[:, lo:hi] += gw * v[:, lo + k:hi + k]
        den[:, lo:hi] += gw
        plain[:, lo:hi] += gk * v[:, lo + k:hi + k]
        norm[:, lo:hi] += gk
    some = den > 0.0
    return np.where(some, num / np.where(some, den, 1.0), plain / norm)


def _check_laws(laws, G, T):
    v = np.asarray(laws, dtype=np.float64)
    if G == 1 and v.shape == (T,):
        v = v[None]
    if v.shape != (G, T):
        raise ValueError("velocity must be %d values for each of the %d gathers, got %s" % (T, G, tuple(v.shape)))
    if not np.all(np.isfinite(v)) or not np.all(v > 0.0):
        raise ValueError("velocity must be finite and > 0 at every tau = 0 .. %d" % (T - 1))
    return np.ascontiguousarray(v)


def nmo_table_device(shape, offset, laws, gather="volume", stretch_mute=None, device=None):
    """operators.nmo_table for sampled laws, built by dpi_nmo_table on the device (include/dpi_hip.h has the definition): the float64 table
    of `shape` = (T, X) or (T, X, Y) for the laws (G, T) of the gathers of `gather` (gather_geometry; (T,) will do for one gather),
    `offset` as in semblance_sums, one launch for all gathers.  The kernel forms the host's expressions in the host's order: the two
    tables can differ only where the device rounds an fp64 square root or division differently.  ValueError before any launch for what
    nmo_table refuses (shapes, non-finite offsets, a law that is not finite and > 0, a stretch mute that is not > 0) and for more than
    NMO_TABLE_DEVICE_ROWS rows, which names --moveout_table."""
    shape = tuple(int(n) for n in shape)
    geo = gather_geometry(shape, gather)
    off = _check_offset(offset, shape)
    if stretch_mute is not None and not (float(stretch_mute) > 0.0 and np.isfinite(float(stretch_mute))):
        raise ValueError("stretch_mute must be a finite value > 0, got %r" % (stretch_mute,))
    T = shape[0]
    S = int(np.prod(shape[1:]))
    law = _check_laws(laws, geo[0], T)
    if T > NMO_TABLE_DEVICE_ROWS:
        raise ValueError("--moveout_table device builds tables of at most %d rows (a trace's travel times are kept in on-chip memory), got "
                         "%d: use --moveout_table host" % (NMO_TABLE_DEVICE_ROWS, T))
    if S >= (1 << 31):
        raise ValueError("--moveout_table device: %d traces, at most 2^31 - 1: use --moveout_table host" % S)
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    with torch.cuda.device(dev):
        l_, o_ = torch.from_numpy(law).to(dev), torch.from_numpy(off.reshape(-1)).to(dev)
        tab = torch.full((T, S), MOVEOUT_MUTE, dtype=torch.float64, device=dev)
        _lib.check(_lib.load().dpi_nmo_table(_lib.ptr(l_), _lib.ptr(o_), 0.0 if stretch_mute is None else float(stretch_mute), T, S, geo[0], geo[1],
                                             geo[2], geo[3], _lib.ptr(tab), _lib.stream()), "dpi_nmo_table")
        return tab.cpu().numpy().reshape(shape)


def scan_table(data, mask, offset, vmin, vmax, nv, gather="volume", window=2, min_fold=4, max_step=1, stretch_mute=None, device=None,
               smooth=0.0, table="host"):
    """Scan, pick and build the table: {"table": the float64 moveout table in the shape of `data` (operators.nmo_table on the law, gather by
    gather, with the same `stretch_mute`; checked by check_moveout_table), "velocity": the laws as used (G, T), "pick": the picked
    staircase (G, T), "velocities": np.linspace(vmin, vmax, nv), "panel": (G, T, NV)}.  `smooth` = L > 0 (--moveout_smooth): the law as
    used is smooth_law of the pick over L rows, weighted by the panel along the picked path; 0: the pick itself.  `table`: "host" =
    nmo_table, "device" = nmo_table_device, one launch for all gathers.  ValueError before any launch for vmin <= 0, vmax < vmin, nv < 1,
    a negative or non-finite `smooth`, an unknown `table` and whatever semblance_sums refuses; a law that makes a trace's table decrease
    along t raises one that names --moveout_vscan."""
    smooth = float(smooth)
    if not (np.isfinite(smooth) and smooth >= 0.0):
        raise ValueError("smooth must be finite and >= 0 (rows), got %r" % (smooth,))
    if table not in TABLE_BUILDERS:
        raise ValueError("table must be one of %s, got %r" % (", ".join(TABLE_BUILDERS), table))
    if int(nv) != nv or nv < 1:
        raise ValueError("nv must be an integer >= 1, got %r" % (nv,))
    vmin, vmax = float(vmin), float(vmax)
    if not (np.isfinite(vmin) and vmin > 0.0):
        raise ValueError("vmin must be finite and > 0 (cells per sample), got %r" % (vmin,))
    if not (np.isfinite(vmax) and vmax >= vmin):
        raise ValueError("vmax must be finite and >= vmin = %g, got %r" % (vmin, vmax))
    vel = np.linspace(vmin, vmax, int(nv))
    shape = tuple(int(n) for n in np.shape(data))
    num, den, cnt = semblance_sums(data, mask, offset, vel, gather=gather, stretch_mute=stretch_mute, device=device)
    panel = semblance_panel(num, den, cnt, window=window, min_fold=min_fold)
    pick, path = pick_velocity(panel, vel, max_step=max_step, return_index=True)
    law = pick
    if smooth > 0.0:
        law = smooth_law(pick, np.take_along_axis(panel, path[:, :, None], axis=2)[:, :, 0], smooth)
    off = _check_offset(offset, shape)
    if table == "device":
        table = nmo_table_device(shape, off, law, gather=gather, stretch_mute=stretch_mute, device=device)
    elif gather == "volume":
        table = nmo_table(shape, off, law[0], stretch_mute)
    else:
        axis = 2 if gather == "y" else 1                         # the axis that numbers the gathers
        table = np.stack([nmo_table((shape[0], shape[3 - axis]), np.take(off, g, axis=axis - 1), law[g], stretch_mute)
                          for g in range(shape[axis])], axis=axis)
    try:
        check_moveout_table(table, what="the table of the picked law")
    except ValueError as e:
        raise ValueError("--moveout_vscan: %s; a law that changes more slowly keeps the events of a trace in order: try a smaller "
                         "--moveout_max_step or a narrower scan" % e) from e
    return {"table": table, "velocity": law, "pick": pick, "velocities": vel, "panel": panel}


def velocity_windows(law, gather, origins, dim):
    """The laws that belong to each patch window: (T,) for `volume`, else (T, G_window), the gathers the window's x (`x`) or y (`y`) range
    spans.  `origins` / `dim`: the windows' origins and extent in (t, x[, y])."""
    if gather == "volume":
        return [law[0].copy() for _ in origins]
    axis = 1 if gather == "x" else 2
    return [np.ascontiguousarray(law[int(o[axis]):int(o[axis]) + int(dim[axis])].T) for o in origins]
