"""Synthetic seismic-like volumes for benchmarks and parity runs (the reference's hyperbolic3d dataset is absent
from its checkout).

`hyperbolic_volume` is the stand-in for `datasets/hyperbolic3d/original.npy` drawn after the figures and printed numbers of
the reference's notebook (proof_of_concept_3D.ipynb cells 13 / 15 / 20): a (t, x, y) cube of hyperbolic events with apex at
(x, y) = (0, 0); at the notebook's patch size (256, 128, 128) the first event has its apex near t = 50 and reaches the far
corner near t = 250, the following events come 18-32 samples apart and fill everything below the first one, the wavelet is a
Ricker whose central lobe is ~8 samples wide, and `std(gain * img * mask)` at gain 40 with 66 % of the traces missing is
3.94 / 5.16 on the notebook's two patches (cell 15 output) — the amplitude is scaled so that the stand-in lands in that band.
A weak band-limited background (2 % of the event RMS x 5; no exact zeros) keeps the empty part of the cube from being an
exactly-zero target.  Smaller volumes are the same picture at a coarser sampling (wavelet and spacing scale with nt / 256,
down to a quarter), so that (128, 64, 64) or (48, 32, 32) stand-ins hold as many events as the full patch.

`sparse_hyperbolic_volume` is the round-1/2 stand-in (5 narrow events, > 70 % of the cube exactly zero, std 1.5 at the
bench patch): kept because committed reference recordings (`tests/golden/plateau_96x64x64.npz`) were made on it."""
import numpy as np

__all__ = ["hyperbolic_volume", "tiled_hyperbolic_volume", "sparse_hyperbolic_volume", "random_trace_mask", "coarse_std", "avo_gathers",
           "hyperbolic_traces", "ricker"]

TARGET_RMS = 0.19          # std of the un-gained cube: 40 * 0.19 * sqrt(0.34) = 4.4, the middle of the notebook's 3.94 .. 5.16


def _binomial_smooth(a, passes):
    """Separable [1 4 6 4 1] / 16 low-pass along every axis, `passes` times (numpy only; zero-padded edges)."""
    k = np.array([1.0, 4.0, 6.0, 4.0, 1.0], dtype=np.float32) / 16.0
    for ax in range(a.ndim):
        n = a.shape[ax]
        for _ in range(passes):
            p = np.zeros_like(a)
            for j, w in enumerate(k):
                s = j - 2
                src = [slice(None)] * a.ndim
                dst = [slice(None)] * a.ndim
                src[ax] = slice(max(0, s), n + min(0, s))
                dst[ax] = slice(max(0, -s), n - max(0, s))
                p[tuple(dst)] += w * a[tuple(src)]
            a = p
    return a


def hyperbolic_volume(shape, seed=0, background=0.02, dtype=np.float32):
    rng = np.random.RandomState(seed)
    nt, nx, ny = shape
    s = min(1.0, max(0.25, nt / 256.0))          # sampling relative to the notebook's patch
    f0 = 0.055 / s                               # Ricker peak frequency, cycles per sample
    t = np.arange(nt, dtype=np.float32)[:, None, None]
    r2 = (np.arange(nx, dtype=np.float32)[None, :, None] / max(nx, 1)) ** 2 + \
         (np.arange(ny, dtype=np.float32)[None, None, :] / max(ny, 1)) ** 2
    vol = np.zeros(shape, dtype=np.float32)
    t0 = rng.uniform(0.12, 0.22) * nt
    while t0 < 1.05 * nt:
        c = 0.9 - 0.3 * min(t0 / nt, 1.0) + rng.uniform(-0.04, 0.04)     # moveout: slower (steeper) events on top
        amp = rng.uniform(0.5, 1.0) * rng.choice([-1.0, 1.0])
        tt = np.sqrt(t0 ** 2 + r2 * (nt * c) ** 2)
        a = (np.pi * f0 * (t - tt)) ** 2
        vol += (amp * (1.0 - 2.0 * a) * np.exp(-a)).astype(np.float32)
        t0 += rng.uniform(18.0, 32.0) * s
    vol *= TARGET_RMS / max(float(vol.std()), 1e-12)
    if background > 0:
        n = _binomial_smooth(rng.standard_normal(shape).astype(np.float32), 2)
        vol += (background * 5.0 * TARGET_RMS / max(float(n.std()), 1e-12)) * n
    return vol.astype(dtype)


def tiled_hyperbolic_volume(shape, tile=(128, 128), seed=0, dtype=np.float32):
    """Field-scale stand-in (BASELINE configs[4]: 512x512x1024): `hyperbolic_volume((nt, tile_x, tile_y))` mirror-tiled along x and y up to
    `shape` — continuous at the seams, the event density and amplitude statistics of the small cube everywhere, and seconds instead of
    minutes of host time for 2.7e8 voxels."""
    nt, nx, ny = shape
    tx, ty = min(tile[0], nx), min(tile[1], ny)
    v = hyperbolic_volume((nt, tx, ty), seed=seed, dtype=dtype)
    row = np.concatenate([v if i % 2 == 0 else v[:, ::-1, :] for i in range(-(-nx // tx))], axis=1)[:, :nx, :]
    return np.ascontiguousarray(np.concatenate([row if j % 2 == 0 else row[:, :, ::-1] for j in range(-(-ny // ty))], axis=2)[:, :, :ny])


def sparse_hyperbolic_volume(shape, seed=0, nev=5, dtype=np.float32):
    rng = np.random.RandomState(seed)
    nt, nx, ny = shape
    t = np.arange(nt, dtype=np.float32)[:, None, None]
    r2 = (np.arange(nx, dtype=np.float32)[None, :, None] / max(nx, 1)) ** 2 + \
         (np.arange(ny, dtype=np.float32)[None, None, :] / max(ny, 1)) ** 2
    vol = np.zeros(shape, dtype=np.float32)
    for _ in range(nev):
        t0 = rng.uniform(0.08, 0.6) * nt
        v = rng.uniform(0.6, 1.6)
        amp = rng.uniform(0.5, 1.0) * rng.choice([-1.0, 1.0])
        tt = np.sqrt(t0 ** 2 + r2 * (nt / v) ** 2)
        a = (np.pi * 0.25 * (t - tt)) ** 2
        vol += (amp * (1.0 - 2.0 * a) * np.exp(-a)).astype(np.float32)
    return (vol / np.abs(vol).max()).astype(dtype)


def avo_gathers(shape, theta, vsvp=0.5, seed=0, linearization="akirich", return_model=False, dtype=np.float32):
    """Stand-in for a pre-stack line (--avo_theta): a (T, X, ntheta) volume of angle gathers that obeys the linearised AVO equation
    exactly.  Three independent parameter sections (T, X) — the x-y plane 0 of `hyperbolic_volume((T, X, 1))` with the seeds 3 seed,
    3 seed + 1, 3 seed + 2: smooth hyperbolic events — are pushed through the float64 coefficients G(theta, vsvp) of
    operators/avo.py, d[t, x, a] = sum_k G[a, k] m_k[t, x], and rounded once to `dtype`.  return_model=True also gives the model
    (T, X, 3) in float64."""
    from ..operators.avo import avo_coefficients
    nt, nx = int(shape[0]), int(shape[1])
    if len(shape) == 3 and int(shape[2]) != len(theta):
        raise ValueError("shape %r names %d angle sections for %d angles" % (tuple(shape), shape[2], len(theta)))
    model = np.stack([hyperbolic_volume((nt, nx, 1), seed=3 * int(seed) + k, dtype=np.float64)[:, :, 0] for k in range(3)], axis=-1)
    G = avo_coefficients(theta, vsvp, 1, linearization)[:, :, 0]                  # (ntheta, 3)
    data = np.einsum("ak,txk->txa", G, model).astype(dtype)
    return (data, model) if return_model else data


def hyperbolic_traces(shape, offsets, seed=0, dtype=np.float32):
    """Stand-in for irregular acquisition (--trace_offsets): the events of `hyperbolic_volume(shape, seed, background=0)` evaluated
    analytically at the recorded positions (x + dx, y + dy) instead of the bin centres.  `offsets` is (X, Y, 2) in grid cells, the layout of
    the flag's file.  The generator is consumed exactly as `hyperbolic_volume` consumes it and the amplitude scale is that of the on-grid
    cube, so both are the same wavefield: at zero offsets the result equals `hyperbolic_volume(shape, seed, background=0)` bit for bit."""
    rng = np.random.RandomState(seed)
    nt, nx, ny = shape
    off = np.asarray(offsets, dtype=np.float32)
    if off.shape != (nx, ny, 2):
        raise ValueError("offsets must have the shape (X, Y, 2) = %r, got %r" % ((nx, ny, 2), tuple(off.shape)))
    s = min(1.0, max(0.25, nt / 256.0))
    f0 = 0.055 / s
    t = np.arange(nt, dtype=np.float32)[:, None, None]
    gx, gy = np.arange(nx, dtype=np.float32)[None, :, None], np.arange(ny, dtype=np.float32)[None, None, :]
    r2_grid = (gx / max(nx, 1)) ** 2 + (gy / max(ny, 1)) ** 2
    r2_rec = ((gx + off[None, :, :, 0]) / max(nx, 1)) ** 2 + ((gy + off[None, :, :, 1]) / max(ny, 1)) ** 2
    grid = np.zeros(shape, dtype=np.float32)
    rec = np.zeros(shape, dtype=np.float32)
    t0 = rng.uniform(0.12, 0.22) * nt
    while t0 < 1.05 * nt:
        c = 0.9 - 0.3 * min(t0 / nt, 1.0) + rng.uniform(-0.04, 0.04)
        amp = rng.uniform(0.5, 1.0) * rng.choice([-1.0, 1.0])
        for vol, r2 in ((grid, r2_grid), (rec, r2_rec)):
            tt = np.sqrt(t0 ** 2 + r2 * (nt * c) ** 2)
            a = (np.pi * f0 * (t - tt)) ** 2
            vol += (amp * (1.0 - 2.0 * a) * np.exp(-a)).astype(np.float32)
        t0 += rng.uniform(18.0, 32.0) * s
    rec *= TARGET_RMS / max(float(grid.std()), 1e-12)
    return rec.astype(dtype)


def ricker(f0, dt, K, dtype=np.float64):
    """Ricker wavelet of peak frequency f0 (Hz) sampled every dt (s) on K samples (odd) centred on time zero:
    w(t) = (1 - 2 a) exp(-a), a = (pi f0 t)^2 — symmetric, 1 at the centre sample.  The wavelet of `hyperbolic_volume` is
    ricker(0.055 / s, 1, K) (f0 in cycles per sample)."""
    K = int(K)
    if K < 1 or K % 2 == 0:
        raise ValueError("ricker: K must be odd and >= 1, got %r" % (K,))
    if not (f0 > 0 and dt > 0):
        raise ValueError("ricker: f0 and dt must be > 0, got %r, %r" % (f0, dt))
    t = (np.arange(K, dtype=np.float64) - K // 2) * float(dt)
    a = (np.pi * float(f0) * t) ** 2
    return ((1.0 - 2.0 * a) * np.exp(-a)).astype(dtype)


def random_trace_mask(shape, rate, seed=0, dtype=np.float32):
    """Binary mask with `rate` of the (x,y) traces deleted, constant along t (build_mask(regular=False) semantics)."""
    rng = np.random.RandomState(seed)
    ntr = int(np.prod(shape[1:]))
    keep = np.ones(ntr, dtype=dtype)
    keep[rng.choice(ntr, int(ntr * rate), replace=False)] = 0
    return np.broadcast_to(keep.reshape((1,) + tuple(shape[1:])), shape).copy()


def coarse_std(vol, mask, gain=40.0):
    """What the reference prints as "the std of coarse data" (main.py:118-139 `load_data`: unbiased std of img * mask)."""
    return float(np.std(np.asarray(vol, dtype=np.float64) * gain * np.asarray(mask, dtype=np.float64), ddof=1))
