"""Sampling-mask synthesis (drop-in for reference utils/mask.py build_mask / add_rand_mask).
Uses numpy's global legacy RNG exactly like the reference so that np.random.seed(s) reproduces its masks.
holdout_traces (ours, --holdout) draws from a private generator instead, so it leaves that stream alone."""
import numpy as np

__all__ = ["build_mask", "add_rand_mask", "holdout_traces", "holdout_masks"]


def build_mask(data, rate, regular=False):
    """Binary trace mask for a (t, x[, y]) cube with `rate` of the traces deleted (constant along t)."""
    if data.ndim == 2:
        nt, nx = data.shape
        ny = 1
    elif data.ndim == 3:
        nt, nx, ny = data.shape
    else:
        raise ValueError("data volume has to be either 2D or 3D")
    ntr = nx * ny
    ndel = int(ntr * rate)
    if regular:
        keep_few = rate >= 0.5
        n = ntr - ndel if keep_few else ndel
        m = int(np.ceil(ntr / n))
        tr = np.ones(ntr) if keep_few else np.zeros(ntr)
        for i in range(n):
            tr[i * m + 1:i * m + m] = 0 if keep_few else 1
    else:
        tr = np.ones(ntr)
        tr[np.random.choice(np.arange(ntr), ndel, replace=False)] = 0
    mask = np.broadcast_to(tr.astype(data.dtype)[None, :], (nt, ntr)).copy()
    return mask.reshape((nt, nx, ny)).squeeze()


def add_rand_mask(mask, perc=0.3):
    """Delete a further `perc` of the surviving traces (data.py:79-80, --adirandel)."""
    m = mask.copy()
    pts = np.argwhere(m[0] == 1)
    sel = np.random.choice(np.arange(pts.shape[0]), int(pts.shape[0] * perc), replace=False)
    for p in pts[sel]:
        m[(slice(None),) + tuple(p)] = 0
    return m


_HOLDOUT_STREAM = 0x686F6C64          # mixed into the seed: the split draws from a stream of its own


def holdout_traces(mask, frac, seed, name=None):
    """Per-trace selection of --holdout for a patch mask in numpy order (T, X[, Y], C): every trace (one t column) with at least one
    nonzero sample is held out with probability `frac`, an independent draw per trace from a private generator seeded with
    (seed, a fixed stream tag) — never numpy's global RNG nor torch's CPU generator, so the reference's mask draws and the initial weights
    do not move.  The draws are made in device order [C][X][Y], one per trace, known or not: the result depends on (seed, frac, mask) only.
    Returns a float32 0/1 array of shape mask.shape[1:] (the patch's numpy order without t).  Raises ValueError naming the patch when no
    trace is held out or no known trace is left for training."""
    frac = float(frac)
    if not 0.0 <= frac <= 0.5:
        raise ValueError("--holdout must lie in [0, 0.5], got %r" % frac)
    known = np.any(np.asarray(mask) != 0, axis=0)                     # (X[, Y], C)
    rng = np.random.Generator(np.random.PCG64(np.random.SeedSequence([int(seed) & 0xFFFFFFFFFFFFFFFF, _HOLDOUT_STREAM])))
    u = np.moveaxis(rng.random(np.moveaxis(known, -1, 0).shape), 0, -1)
    sel = known & (u < frac)
    patch = "patch %r" % (name,)
    if not sel.any():
        raise ValueError("%s: --holdout %g held out no known trace (%d known traces); raise --holdout or use a larger patch"
                         % (patch, frac, int(known.sum())))
    if not (known & ~sel).any():
        raise ValueError("%s: --holdout %g held out every known trace (%d): no training sample is left" % (patch, frac, int(known.sum())))
    return sel.astype(np.float32)


def holdout_masks(mask, sel):
    """(m_tr, m_ho) = (mask * (1 - h), mask * h) per sample, h = the selection of holdout_traces broadcast along t."""
    h = np.asarray(sel)[None]
    return mask * (1 - h), mask * h
