"""The cases dpi_nmo_table is run on, the statements of operators.nmo_table behind every decision of a table with their distance from a
rounding boundary, the error bar of the comparison, the scalar restatement of the kernel, and the stand-in of the mechanism test.  A
plain module: no fixtures, no GPU needed to import it.

Bar.  The kernel and operators.nmo_table form the same float64 expressions in the same order without fused multiply-adds; they can
differ in the rounding of the division off / v and of the square root.  The host rounds both to half an ulp.  The HIP math tables give
1 ulp for the fp64 sqrt; the fp64 division is IEEE there (half an ulp) and is taken as 1 ulp as well.  With u = 2^-52 (an ulp is at most
u times the value): q = off / v differs by at most 1.5 u relatively, q^2 by 3 u (+ its own rounding, u / 2 each side), x^2 + q^2 by at
most that (x^2 is the same on both sides; + u / 2 each side), the root of it by half of that, (3 + 1 + 1) / 2 = 2.5 u, plus the root's own
1.5 u: the two travel(x) differ by at most E = 4 u t near travel = t; 5 u t is used.  Either side bisects to the last bit of ITS travel: its
result is the last x of the bracket with travel(x) <= t, where travel(x) is the exact, increasing travel time plus that side's rounding
noise of at most 2 u t (host) or 3.5 u t (device).  Two such crossings lie at most (E + noise) / slope <= 8 u t / slope apart, `slope` the
derivative of the exact travel time at the solution, plus an ulp of tau for where the bisection stops.  The derivative, not the mean rise
g1 - g0 of the bracket, is what divides: where t(tau) is curved (the bracket that starts at the minimum of a far trace has slope 0 at
its left end) the mean rise overstates the slope at the solution.  The slope is evaluated in float64 on the host at the host's tau,
    slope = (x - q^2 dv / v) / t,   q = off / v(x), dv = law[j + 1] - law[j],
and halved, which covers its change over an interval some 1e-9 of it wide (the generator keeps slope >= 1e-6):
    |tau_dev - tau_host| <= 16 u max(t, 1) / slope + 2 u T.
Exactly representable samples (zero offset: travel(x) = x) have tau = t on both sides and must be equal.

Decisions.  The live map must be equal, so every comparison behind it is kept at least MARGIN = 1e-9 (relative) from its boundary by
construction, for every trace with a non-zero offset: the ties of the minimum (g[j] against g[jmin]), the running maximum (g[j] against
env[j - 1]), the search (every finite env against every whole t), g1 > g0, t >= g0, t <= g1 and the stretch test.  A draw that comes
closer is replaced by the next seed's, never excluded."""
import functools

import numpy as np

from deep_prior_interpolation_amd.operators import nmo_table
from deep_prior_interpolation_amd.operators.moveout import MOVEOUT_MUTE

U = 2.0 ** -52
MARGIN = 1e-9
MIN_SLOPE = 1e-6
VELOCITIES = np.linspace(1.0, 1.8, 17)      # the grid the staircase laws step on (velocity_cases.EVENT_VELOCITIES)

LAWS = ("constant", "rising", "inversion", "staircase")
FLAT = [(T, S, law, stretch) for T in (1, 2, 33, 257) for S in (1, 63, 65) for law in LAWS for stretch in (None, 1.5)]
FLAT += [(33, 65, "far", None), (257, 63, "far", 1.5), (33, 63, "zero", 1.5), (2, 65, "zero", None)]
FLAT_IDS = ["T%d-S%d-%s-%s" % (T, S, law, "none" if st is None else "stretch%g" % st) for T, S, law, st in FLAT]
VOLUMES = [(33, X, Y, stretch) for (X, Y) in ((5, 7), (16, 16)) for stretch in (None, 1.5)]
VOLUME_IDS = ["T33-X%d-Y%d-%s" % (X, Y, "none" if st is None else "stretch%g" % st) for _, X, Y, st in VOLUMES]


def make_law(kind, T, rng):
    """One law (T,).  The inversion (fast above, slow below) makes t(tau) drop where the velocity does: the branch starts after the drop
    and the running maximum differs from t(tau) wherever the slow part has not caught up yet."""
    j = np.arange(T, dtype=np.float64)
    if kind in ("constant", "far", "zero"):
        return np.full(T, 1.0 + 0.5 * rng.rand())
    if kind == "rising":
        return 1.0 + rng.rand() * 0.2 + (0.5 + 0.5 * rng.rand()) * j / max(T - 1, 1)
    if kind == "inversion":
        cut = T // 3 + rng.randint(0, max(T // 4, 1))
        wobble = 1.0 + 0.02 * np.sin(0.9 * j + rng.rand())
        return np.where(j < cut, 3.0 + rng.rand(), 1.0 + 0.3 * rng.rand()) * wobble
    if kind == "staircase":                                      # a pick: a walk of at most one grid step per row
        idx = np.clip(np.cumsum(rng.randint(-1, 2, T)) + rng.randint(4, 12), 0, VELOCITIES.size - 1)
        return VELOCITIES[idx]
    raise ValueError(kind)


def make_offsets(kind, T, S, rng):
    if kind == "zero":
        return np.zeros(S)
    if kind == "far":                                            # t(0) = off / v > T - 1: every sample is muted
        return rng.uniform(3.0 * T + 10.0, 5.0 * T + 20.0, S)
    off = rng.uniform(0.0, 1.2 * T, S)
    off[rng.rand(S) < 0.2] = 0.0
    off[0] = 0.0                                                 # always one exactly representable trace
    if S > 2:
        off[S // 2] = 4.0 * T + 10.0                             # and one muted throughout
    return off


def _vel(law, x, j):
    """np.interp(x, arange(T), law) for j <= x <= j + 1: the node's value on a node, else slope * (x - j) + law[j]."""
    return np.where(x == j, law[j], np.where(x == j + 1.0, law[j + 1], (law[j + 1] - law[j]) * (x - j) + law[j]))


def decisions(law, off, stretch, table):
    with np.errstate(invalid="ignore"):                          # inf - inf where t(tau) overflows or a row is -inf: filtered where used
        return _decisions(law, off, stretch, table)


def _decisions(law, off, stretch, table):
    """(the least relative distance of a decision of operators.nmo_table from its boundary over the traces with a non-zero offset, the bar
    (T, S) of the module docstring, the least slope at a live solution) for one gather: law (T,), off (S,), table (T, S) from the host."""
    T, S = table.shape
    if T == 1:
        return np.inf, np.zeros((T, S)), np.inf
    grid = np.arange(T, dtype=np.float64)
    with np.errstate(over="ignore"):
        g = np.sqrt(grid[:, None] ** 2 + (off[None] / law[:, None]) ** 2)
    jmin = (T - 1) - np.argmin(g[::-1], axis=0)
    env = np.maximum.accumulate(np.where(grid[:, None] >= jmin[None], g, -np.inf), axis=0)
    inexact = off != 0.0
    rel = lambda a, b: np.abs(a - b) / np.maximum(np.maximum(np.abs(a), np.abs(b)), 1e-300)
    margin = np.inf
    if inexact.any():
        gi, ei, ji = g[:, inexact], env[:, inexact], jmin[inexact]
        fin = np.isfinite(gi)
        other = grid[:, None] != ji[None]
        d = rel(gi, gi[ji, np.arange(ji.size)][None])
        if (other & fin).any():
            margin = min(margin, float(d[other & fin].min()))                     # ties of the minimum
        up = (grid[1:, None] > ji[None]) & fin[1:]
        if up.any():
            margin = min(margin, float(rel(gi[1:], ei[:-1])[up].min()))            # the running maximum
        near = np.isfinite(ei) & (ei <= T)
        if near.any():
            margin = min(margin, float((np.abs(ei - np.rint(ei)) / np.maximum(ei, 1.0))[near].min()))       # env against every whole t
        if stretch is not None:
            j = np.empty((T, ji.size), dtype=np.int64)
            for s in range(ji.size):
                j[:, s] = np.searchsorted(ei[:, s], grid, side="right") - 1
            j = np.clip(j, 0, T - 2)
            c = np.arange(ji.size)[None]
            rise = gi[j + 1, c] - gi[j, c]
            ok = np.isfinite(rise) & (rise > 0)
            if ok.any():
                margin = min(margin, float(rel(1.0 / rise[ok], float(stretch)).min()))
    live = table != MOVEOUT_MUTE
    bar = np.zeros((T, S))
    slope_min = np.inf
    tt, ss = np.nonzero(live & inexact[None])
    if tt.size:
        x = table[tt, ss]
        j = np.minimum(np.floor(x), T - 2.0)
        ji = j.astype(np.int64)
        v = _vel(law, x, ji)
        q = off[ss] / v
        slope = (x - q * q * (law[ji + 1] - law[ji]) / v) / grid[tt].clip(1e-300)
        slope_min = float(slope.min())
        bar[tt, ss] = 16.0 * U * np.maximum(grid[tt], 1.0) / np.maximum(slope, 1e-300) + 2.0 * U * T
    return margin, bar, slope_min


def _build(T, shape, law_kinds, off_kind, stretch, geo_name, seed):
    """laws (G, T), offsets of `shape[1:]`, the host table, margin, bar."""
    rng = np.random.RandomState(seed)
    S = int(np.prod(shape[1:]))
    off = make_offsets(off_kind, T, S, rng).reshape(shape[1:])
    if geo_name == "volume":
        G = 1
    else:
        G = shape[2] if geo_name == "y" else shape[1]
    laws = np.stack([make_law(law_kinds[g % len(law_kinds)], T, rng) for g in range(G)])
    if geo_name == "volume":
        ref = nmo_table(shape, off, laws[0], stretch)
        parts = [(laws[0], off.reshape(-1), ref.reshape(T, -1))]
    else:
        axis = 2 if geo_name == "y" else 1
        tabs = [nmo_table((T, shape[3 - axis]), np.take(off, g, axis=axis - 1), laws[g], stretch) for g in range(G)]
        ref = np.stack(tabs, axis=axis)
        parts = [(laws[g], np.take(off, g, axis=axis - 1), tabs[g]) for g in range(G)]
    margin, slope_min, bars = np.inf, np.inf, []
    for law, o, tab in parts:
        m, b, sl = decisions(law, o, stretch, tab)
        margin, slope_min = min(margin, m), min(slope_min, sl)
        bars.append(b)
    if geo_name == "volume":
        bar = bars[0].reshape(shape)
    else:
        bar = np.stack(bars, axis=2 if geo_name == "y" else 1)
    return dict(laws=laws, offset=off, ref=ref, bar=bar, margin=margin, slope=slope_min, stretch=stretch, shape=shape, gather=geo_name, seed=seed)


def _first_that_keeps_the_margin(make):
    for seed in range(100):
        c = make(seed)
        if c["margin"] >= MARGIN and c["slope"] >= MIN_SLOPE:
            return c
    raise AssertionError("no draw keeps the margin")


@functools.lru_cache(maxsize=None)
def flat_case(T, S, law, stretch):
    """One gather of S traces on T rows: a (T, S) section."""
    off_kind = law if law in ("far", "zero") else "mixed"
    return _first_that_keeps_the_margin(lambda seed: _build(T, (T, S), (law,), off_kind, stretch, "volume", 1000 * seed + 13 * T + S))


@functools.lru_cache(maxsize=None)
def volume_case(T, X, Y, stretch, gather):
    """A (T, X, Y) volume under one of the three layouts, a different law per gather (the four kinds in turn)."""
    return _first_that_keeps_the_margin(lambda seed: _build(T, (T, X, Y), LAWS, "mixed", stretch, gather, 1000 * seed + 17 * T + X * Y))


def compare(got, c, what=""):
    """The live maps are equal, the live samples within the bar (zero-offset traces: equal).  Returns (bit-identical?, worst error / bar)."""
    ref, bar = c["ref"], c["bar"]
    assert got.shape == ref.shape and got.dtype == np.float64, what
    assert np.isfinite(got).all(), what
    live = ref != MOVEOUT_MUTE
    assert np.array_equal(got != MOVEOUT_MUTE, live), "%s: the live maps differ at %d samples" % (what, int(((got != MOVEOUT_MUTE) != live).sum()))
    err = np.abs(got - ref)
    exact = np.broadcast_to((c["offset"] == 0.0)[None], ref.shape)
    assert not err[exact].any(), "%s: a zero-offset trace differs" % what
    worst = float((err[live & ~exact] / bar[live & ~exact]).max()) if (live & ~exact).any() else 0.0
    same = bool(np.array_equal(got, ref))
    print("%s: %d live of %d, bit-identical %s, worst |tau_dev - tau_host| / bar = %.3g (largest error %.3g)" % (
        what, int(live.sum()), live.size, same, worst, float(err.max())))
    assert np.all(err <= bar), (what, worst)
    return same, worst


def rows64(law, off, stretch, T):
    """The scalar restatement of one trace of dpi_nmo_table (include/dpi_hip.h), the way the kernel walks it: an upper-bound search instead
    of searchsorted, the last minimum by comparison, the velocity of a bracket from its two nodes.  Returns the column (T,)."""
    if T == 1:
        return np.array([0.0 if off == 0.0 else MOVEOUT_MUTE])
    f = np.float64
    with np.errstate(over="ignore"):
        g = [np.sqrt(f(j) * f(j) + (f(off) / law[j]) * (f(off) / law[j])) for j in range(T)]
    mv, jmin = np.inf, 0
    for j in range(T):
        if g[j] <= mv:
            mv, jmin = g[j], j
    env, run = [], -np.inf
    for j in range(T):
        if j >= jmin and g[j] > run:
            run = g[j]
        env.append(run if j >= jmin else -np.inf)

    def travel(x, j):
        v = law[j] if x == j else (law[j + 1] if x == j + 1.0 else (law[j + 1] - law[j]) * (x - f(j)) + law[j])
        q = f(off) / v
        return np.sqrt(x * x + q * q)

    out = np.full(T, MOVEOUT_MUTE)
    for t in range(T):
        want = f(t)
        lo, hi = 0, T
        while lo < hi:
            m = (lo + hi) >> 1
            if env[m] <= want:
                lo = m + 1
            else:
                hi = m
        j = min(max(lo - 1, 0), T - 2)
        g0, g1 = g[j], g[j + 1]
        live = j >= jmin and env[j] == g0 and env[j + 1] == g1 and g1 > g0 and g0 <= want <= g1
        if live and stretch is not None:
            live = f(1.0) / (g1 - g0) <= stretch
        if not live:
            continue
        l, h = f(j), f(j) + 1.0
        for _ in range(56):
            mid = f(0.5) * (l + h)
            if travel(mid, j) <= want:
                l = mid
            else:
                h = mid
        out[t] = min(max(h if travel(h, j) == want else l, 0.0), f(T - 1))
    return out


# ---------------------------------------------------------------- the stand-in of the mechanism test ------------------------------
def roughness(table):
    """mean |d^2 tau / dt^2|: the absolute second difference of the table along t over triples of consecutive live samples of a trace."""
    tab = np.asarray(table, dtype=np.float64).reshape(table.shape[0], -1)
    live = (tab >= 0) & (tab <= tab.shape[0] - 1)
    ok = live[:-2] & live[1:-1] & live[2:]
    return float(np.abs(tab[2:] - 2.0 * tab[1:-1] + tab[:-2])[ok].mean())


STANDIN_SHAPE = (48, 32, 32)
STANDIN_VSCAN = (1.0, 1.8, 33)


@functools.lru_cache(maxsize=None)
def standin(mask_kind):
    """(the stand-in volume with its unknown traces zeroed, the known map, the offsets, the table of its mean law) at STANDIN_SHAPE, the
    set-up of tools/velocity_scan_quality.py: `random` = 66 % of the traces missing at random, `regular` = every third trace along x kept."""
    from deep_prior_interpolation_amd import utils as u
    nt, nx, ny = STANDIN_SHAPE
    vol = u.hyperbolic_volume(STANDIN_SHAPE, seed=0).astype(np.float64)
    if mask_kind == "random":
        known = np.broadcast_to(u.random_trace_mask(STANDIN_SHAPE, 0.66, seed=1), STANDIN_SHAPE) > 0
    else:
        known = np.zeros(STANDIN_SHAPE, dtype=bool)
        known[:, ::3] = True
    off = nt * np.sqrt((np.arange(nx)[:, None] / nx) ** 2 + (np.arange(ny)[None, :] / ny) ** 2)
    mean = nmo_table(STANDIN_SHAPE, off, lambda tau: 1.0 / (0.9 - 0.3 * tau / nt))
    return np.where(known, vol, 0.0), known, off, mean


def sums64_as_semblance_sums(data, mask, offset, velocities, gather="volume", stretch_mute=None, device=None):
    """velocity_cases.sums64 behind the signature of operators.semblance_sums: what the host tests put in the kernel's place."""
    import velocity_cases as V
    from deep_prior_interpolation_amd.operators import gather_geometry
    d = np.asarray(data)
    T = d.shape[0]
    r = V.sums64(d.astype(np.float32).reshape(T, -1), np.asarray(mask).reshape(T, -1), np.asarray(offset, dtype=np.float64).reshape(-1),
                 velocities, stretch_mute, gather_geometry(d.shape, gather))
    return r["num"], r["den"], r["cnt"]
