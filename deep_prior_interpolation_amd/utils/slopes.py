"""Local dips and the directional Laplacian (drop-in for reference utils/slopes.py) on the GPU, on 2-D sections and on both
families of vertical sections of a 3-D patch."""
import math
from typing import Tuple

import numpy as np
import torch

from .. import _lib
from ..operators.base import LinearOperator
from .processing import GaussianFilter, gaussian_kernel

__all__ = ["Hale2D", "Hale2DSections", "directional_laplacian", "structure_tensor_dips", "structure_tensor_dips_sections"]


def _planes(t):
    if t.ndim != 4:
        raise _lib.DpiError("expected a BCHW tensor")
    if not t.is_cuda or t.dtype != torch.float32:
        raise _lib.DpiError("slopes operators run on fp32 GPU tensors (no CPU path)")
    return t.contiguous(), t.shape[0] * t.shape[1], int(t.shape[2]), int(t.shape[3])


def _patch(t):
    if t.ndim != 5:
        raise _lib.DpiError("expected a (B,C,T,X,Y) patch")
    if not t.is_cuda or t.dtype != torch.float32:
        raise _lib.DpiError("slopes operators run on fp32 GPU tensors (no CPU path)")
    return t.contiguous(), t.shape[0] * t.shape[1], int(t.shape[2]), int(t.shape[3]), int(t.shape[4])


def _smooth_axes(fields, axes, std):
    """The Gaussian smoothing of structure_tensor_dips (kernel size 2*min(n_v, n_h)//2 + 1, std `std`, zero padded 'same') of the
    given [N][T][X][Y] fields along two of their axes, v first: dpi_fir_axis0 on the [outer][n][inner] view of each axis.  Where
    min(n_v, n_h) is odd the size is even (always for the (t,y) sections of a (T,X,1) volume): the kernel stays centred on K//2, and
    one zero tap past its end gives dpi_fir_axis0 the odd length it takes with the same sums."""
    sizes = fields[0].shape[1:]
    taps = gaussian_kernel(2 * min(sizes[axes[0]], sizes[axes[1]]) // 2 + 1, std, sym=True)
    if taps.size % 2 == 0:
        taps = np.append(taps, 0.0)
    K = int(taps.size)
    taps = torch.from_numpy(taps.astype(np.float32)).to(fields[0].device)
    L = _lib.load()
    out = []
    for f in fields:
        for ax in axes:
            outer, n = int(f.shape[0]) * math.prod(sizes[:ax]), int(sizes[ax])
            inner = f.numel() // (outer * n)
            y = torch.empty_like(f)
            for o0 in range(0, outer, 65535):                 # the outer index is the launch's grid y
                o1 = min(outer, o0 + 65535)
                off = o0 * n * inner * 4
                _lib.check(L.dpi_fir_axis0(_lib.ptr(f) + off, _lib.ptr(taps), K, o1 - o0, n, inner, _lib.ptr(y) + off, _lib.stream()),
                           "dpi_fir_axis0")
            f = y
        out.append(f)
    return out


def structure_tensor_dips_sections(in_content: torch.Tensor, smooth: float = 0., dt: float = 1., dx: float = 1.,
                                   dy: float = 1.) -> Tuple[torch.Tensor, torch.Tensor]:
    """Dips of both families of vertical sections of a (B,C,T,X,Y) patch: structure_tensor_dips on every (t,x) section (v = t,
    h = x) and on every (t,y) section (v = t, h = y), smoothing along the two axes of the section.  Returns (phi_tx, phi_ty), each
    of the patch's shape.  No gradient is propagated."""
    with torch.no_grad():
        x, N, T, X, Y = _patch(in_content)
        L = _lib.load()
        f = torch.empty((5,) + tuple(x.shape), dtype=torch.float32, device=x.device)
        gtt, gtx, gxx, gty, gyy = f.unbind(0)
        _lib.check(L.dpi_structure_tensor_sections(_lib.ptr(x), N, T, X, Y, float(dt), float(dx), float(dy), _lib.ptr(gtt), _lib.ptr(gtx),
                                                   _lib.ptr(gxx), _lib.ptr(gty), _lib.ptr(gyy), _lib.stream()),
                   "dpi_structure_tensor_sections")
        tx, ty = (gtt, gtx, gxx), (gtt, gty, gyy)
        if smooth > 0:
            v = [t.view(N, T, X, Y) for t in (gtt, gtx, gxx, gty, gyy)]
            tx = _smooth_axes(v[:3], (0, 1), float(smooth))
            ty = _smooth_axes([v[0], v[3], v[4]], (0, 2), float(smooth))
        phis = []
        aniso = torch.empty_like(x)
        for vv, vh, hh in (tx, ty):
            phi = torch.empty_like(x)
            _lib.check(L.dpi_dips(_lib.ptr(vv), _lib.ptr(vh), _lib.ptr(hh), x.numel(), _lib.ptr(phi), _lib.ptr(aniso), _lib.stream()),
                       "dpi_dips")
            phis.append(phi)
        return phis[0], phis[1]


def structure_tensor_dips(in_content: torch.Tensor, dv: float = 1., dh: float = 1, smooth: float = 0.) -> Tuple[torch.Tensor, torch.Tensor]:
    """Dip angle and anisotropy from the (optionally Gaussian-smoothed) structure tensor of a BCHW section
    (slopes.py:6-48).  No gradient is propagated: dips are a fixed field the regulariser is built on."""
    with torch.no_grad():
        x, N, H, W = _planes(in_content)
        L = _lib.load()
        gvv, gvh, ghh = (torch.empty_like(x) for _ in range(3))
        _lib.check(L.dpi_structure_tensor(_lib.ptr(x), N, H, W, float(dv), float(dh), _lib.ptr(gvv), _lib.ptr(gvh), _lib.ptr(ghh),
                                          _lib.stream()), "dpi_structure_tensor")
        if smooth > 0:
            G = GaussianFilter(channels=x.shape[1], kernel_size=2 * min(H, W) // 2 + 1, ndim=2, std=smooth)
            gvv, gvh, ghh = G(gvv), G(gvh), G(ghh)
        phi, aniso = torch.empty_like(x), torch.empty_like(x)
        _lib.check(L.dpi_dips(_lib.ptr(gvv), _lib.ptr(gvh), _lib.ptr(ghh), x.numel(), _lib.ptr(phi), _lib.ptr(aniso), _lib.stream()),
                   "dpi_dips")
        return phi, aniso


class Hale2D(LinearOperator):
    """Directional Laplacian built on a dip field (BCHW, same shape as the sections it is applied to) — slopes.py:72-105.
    forward(x) = -(Dh(a Dv x + b Dh x) + Dv(b Dv x + c Dh x)) with a = cos^2, b = -cos sin, c = sin^2; differentiable (the
    backward is the exact transpose kernel), plus an explicit `adjoint` the reference does not have."""

    def __init__(self, directions: torch.Tensor):
        super().__init__()
        with torch.no_grad():
            u1 = torch.cos(directions)
            u2 = -torch.sin(directions)
            self.a = (u1 * u1).contiguous()
            self.b = (u1 * u2).contiguous()
            self.c = (u2 * u2).contiguous()
            self.dips = directions

    def _matvec(self, x, adjoint):
        x, N, H, W = _planes(x)
        if tuple(x.shape) != tuple(self.a.shape):
            raise _lib.DpiError("Hale2D: tensor shape %s differs from the dip field %s" % (tuple(x.shape), tuple(self.a.shape)))
        y = torch.empty_like(x)
        _lib.check(_lib.load().dpi_hale2d(_lib.ptr(x), _lib.ptr(self.a), _lib.ptr(self.b), _lib.ptr(self.c), N, H, W, int(adjoint),
                                          _lib.ptr(y), _lib.stream()), "dpi_hale2d")
        return y


def directional_laplacian(in_content: torch.Tensor, theta: torch.Tensor) -> torch.Tensor:
    return Hale2D(theta)(in_content)


class Hale2DSections(LinearOperator):
    """Hale2D on both families of vertical sections of a (B,C,T,X,Y) patch: forward(x) = stack(L_tx x, L_ty x) of shape (2,B,C,T,X,Y),
    with L_tx = Hale2D(phi_tx) on every (t,x) section (v = t, h = x) and L_ty = Hale2D(phi_ty) on every (t,y) section (v = t, h = y).
    adjoint(g) = L_tx^T g[0] + L_ty^T g[1].  Differentiable (the backward is the transpose kernel); `dips` is (2, B*C, T, X, Y)."""

    def __init__(self, phi_tx: torch.Tensor, phi_ty: torch.Tensor):
        super().__init__()
        if tuple(phi_tx.shape) != tuple(phi_ty.shape) or phi_tx.ndim != 5:
            raise _lib.DpiError("Hale2DSections: the two dip fields must be (B,C,T,X,Y) of one shape, got %s and %s"
                                % (tuple(phi_tx.shape), tuple(phi_ty.shape)))
        with torch.no_grad():
            self.shape = tuple(phi_tx.shape)
            B, C, T, X, Y = self.shape
            self.dips = torch.stack((phi_tx, phi_ty)).reshape(2, B * C, T, X, Y)
            u1 = torch.cos(self.dips)
            u2 = -torch.sin(self.dips)
            # [a, b, c] of the (t,x) family, then of the (t,y) family
            self.coef = torch.stack((u1[0] * u1[0], u1[0] * u2[0], u2[0] * u2[0], u1[1] * u1[1], u1[1] * u2[1], u2[1] * u2[1])).contiguous()

    def _matvec(self, x, adjoint):
        if not x.is_cuda or x.dtype != torch.float32:
            raise _lib.DpiError("slopes operators run on fp32 GPU tensors (no CPU path)")
        if not self.coef.is_cuda or self.coef.device != x.device:
            raise _lib.DpiError("Hale2DSections: the dip field lives on %s, the tensor on %s" % (self.coef.device, x.device))
        want = ((2,) + self.shape) if adjoint else self.shape
        if tuple(x.shape) != want:
            raise _lib.DpiError("Hale2DSections: tensor shape %s, expected %s for the dip field %s" % (tuple(x.shape), want, self.shape))
        x = x.contiguous()
        B, C, T, X, Y = self.shape
        y = torch.empty(self.shape if adjoint else (2,) + self.shape, dtype=torch.float32, device=x.device)
        _lib.check(_lib.load().dpi_hale_sections(_lib.ptr(x), _lib.ptr(self.coef), B * C, T, X, Y, int(adjoint), _lib.ptr(y), _lib.stream()),
                   "dpi_hale_sections")
        return y
