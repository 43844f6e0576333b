"""Linearised amplitude-versus-angle modelling (reference operators/avo.py:9-95): three elastic-parameter sections -> ntheta angle
sections with coefficients G(theta, vs/vp) of the Aki-Richards or the Fatti form.  forward / adjoint are dpi_avo_fwd / dpi_avo_adj.

The coefficients are a host matter: `avo_coefficients` evaluates the reference's formulas in float64, the operator rounds them ONCE to
fp32 and uploads them once per device.  `avo_model_from_data` is the other host piece: the per-time-sample pseudo-inverse of G in float64,
which takes a data-domain output of the deep-prior loop (--avo_theta) back to the three parameter sections."""
import numpy as np
import torch

from .. import _lib
from .base import LinearOperator

__all__ = ["AVOLinearModelling", "avo_coefficients", "avo_model_from_data", "AVO_LINEARIZATIONS"]

AVO_LINEARIZATIONS = ("akirich", "fatti")


def avo_coefficients(theta, vsvp=0.5, nt0=1, linearization="akirich"):
    """G (ntheta, 3, nt0) in float64 (avo.py:9-40): theta in degrees, vsvp a scalar or nt0 values.
    akirich: G1 = 1 / (2 cos^2), G2 = -4 r^2 sin^2, G3 = 1/2 - 2 r^2 sin^2;  fatti: G1 = (1 + tan^2) / 2, G2 = -4 r^2 sin^2,
    G3 = (4 r^2 sin^2 - tan^2) / 2, with r = vs/vp.  Raises for another linearization and for |theta| >= 90 (the reference falls back to
    Aki-Richards silently and returns the huge values of a cosine that is zero to rounding)."""
    if linearization not in AVO_LINEARIZATIONS:
        raise ValueError("linearization must be akirich or fatti, got %r" % (linearization,))
    th = np.asarray(theta.detach().cpu().numpy() if torch.is_tensor(theta) else theta, dtype=np.float64).reshape(-1)
    if th.size < 1 or not np.all(np.isfinite(th)) or np.any(np.abs(th) >= 90.0):
        raise ValueError("theta must hold at least one angle with |theta| < 90 degrees, got %r" % (th.tolist(),))
    r = np.asarray(vsvp.detach().cpu().numpy() if torch.is_tensor(vsvp) else vsvp, dtype=np.float64).reshape(-1)
    if r.size == 1:
        r = np.full(int(nt0), r[0])
    elif r.size != int(nt0):
        raise ValueError("vsvp holds %d values for nt0 = %d" % (r.size, int(nt0)))
    if r.size < 1 or not np.all(np.isfinite(r)):
        raise ValueError("vsvp must be finite and nt0 >= 1")
    th = np.deg2rad(th)[:, None]
    r2 = (r ** 2)[None, :]
    s2 = np.sin(th) ** 2
    if linearization == "akirich":
        g1 = 1.0 / (2.0 * np.cos(th) ** 2) + 0.0 * r2
        g2 = -4.0 * r2 * s2
        g3 = 0.5 - 2.0 * r2 * s2
    else:
        t2 = np.tan(th) ** 2
        g1 = 0.5 * (1.0 + t2) + 0.0 * r2
        g2 = -4.0 * r2 * s2
        g3 = 0.5 * (4.0 * r2 * s2 - t2)
    return np.stack([g1, g2, g3], axis=1)


def avo_model_from_data(data, G):
    """The three parameter sections of a data-domain patch: data (T, ..., ntheta) in the patch's numpy order, G (ntheta, 3, T) ->
    model (T, ..., 3) in float64, m_t = pinv(G_t) d_t per time sample (the least-squares model; exact for data in the range of G_t)."""
    G = np.asarray(G, dtype=np.float64)
    d = np.asarray(data, dtype=np.float64)
    if G.ndim != 3 or G.shape[1] != 3 or d.shape[0] != G.shape[2] or d.shape[-1] != G.shape[0]:
        raise ValueError("data %s does not match G %s: (T, ..., ntheta) against (ntheta, 3, T)" % (d.shape, G.shape))
    P = np.linalg.pinv(np.transpose(G, (2, 0, 1)))                     # (T, 3, ntheta)
    flat = d.reshape(d.shape[0], -1, d.shape[-1])                      # (T, S, ntheta)
    return np.einsum("tka,tsa->tsk", P, flat).reshape(d.shape[:-1] + (3,))


class AVOLinearModelling(LinearOperator):
    """forward: (1, 3, nt0, *spat) -> (1, ntheta, nt0, *spat); adjoint: back (avo.py:43-95).  `G` keeps the reference's shape
    (ntheta, 3, nt0, 1[, 1]) (fp32, on the host; also for nt0 = 1, where the reference drops the time axis).  Differences, all refusals of what
    the reference computes garbage for or fails on later: an unknown linearization and |theta| >= 90 raise ValueError; a batch other than 1,
    a channel count other than 3 / ntheta, a time axis other than nt0 and a number of spatial axes other than len(spatdims) raise before
    any launch."""

    def __init__(self, theta, vsvp=0.5, nt0=1, spatdims=None, linearization="akirich"):
        super().__init__()
        self.nt0 = int(nt0) if not torch.is_tensor(vsvp) else int(vsvp.numel())
        self.ntheta = len(theta)
        if spatdims is None:
            self.spatdims = ()
        else:
            self.spatdims = spatdims if isinstance(spatdims, tuple) else (spatdims,)
        self.linearization = linearization
        self.G64 = avo_coefficients(theta, vsvp, self.nt0, linearization)          # (ntheta, 3, nt0) float64
        self._g32 = np.ascontiguousarray(self.G64.astype(np.float32))              # the one rounding
        self.G = torch.from_numpy(self._g32.reshape(self._g32.shape + (1,) * len(self.spatdims)))
        self._ndim_msg = "AVOLinearModelling built for %d spatial axes got a %%d-D tensor" % len(self.spatdims)

    def _to_device(self, device):
        return torch.from_numpy(self._g32).to(device)

    def _matvec(self, x, adjoint):
        cin = self.ntheta if adjoint else 3
        self._check_patch(x, _lib.DpiError, self._ndim_msg, ndims=(3 + len(self.spatdims),))
        if x.shape[1] != cin:
            raise _lib.DpiError("AVOLinearModelling.%s expects %d channels, got %d" % ("adjoint" if adjoint else "forward", cin, x.shape[1]))
        if x.shape[2] != self.nt0:
            raise _lib.DpiError("AVOLinearModelling built for nt0 = %d got a time axis of %d samples" % (self.nt0, x.shape[2]))
        S = 1
        for n in x.shape[3:]:
            S *= int(n)
        if S < 1:
            raise _lib.DpiError("AVOLinearModelling: empty tensor %s" % (tuple(x.shape),))
        g = self.upload(x.device)
        y = torch.empty((1, 3 if adjoint else self.ntheta) + tuple(x.shape[2:]), dtype=torch.float32, device=x.device)
        L = _lib.load()
        fn, name = (L.dpi_avo_adj, "dpi_avo_adj") if adjoint else (L.dpi_avo_fwd, "dpi_avo_fwd")
        _lib.check(fn(_lib.ptr(x), _lib.ptr(g), self.ntheta, self.nt0, S, _lib.ptr(y), _lib.stream()), name)
        return y
