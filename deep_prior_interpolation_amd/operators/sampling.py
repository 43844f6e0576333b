"""Sampling of a regular-grid tensor at the recorded trace positions (ours, --trace_offsets: the reference takes every known trace to
sit on a grid node).  forward / adjoint are dpi_trace_sample_fwd / dpi_trace_sample_adj (include/dpi_hip.h has the definition): bilinear
in (x, y) from the per-trace offsets, the same for every t and every channel, edges clamped, the adjoint a deterministic gather.  With
interp = "cubic" or "sinc8" (--trace_interp) the operator applies a table of K x K weights per trace, built on the host by
dpi_trace_interp_weights, through dpi_trace_resample_fwd / dpi_trace_resample_adj."""
import ctypes

import numpy as np
import torch

from .. import _lib
from .base import LinearOperator

__all__ = ["TraceSampling", "check_trace_offsets", "INTERP_TAPS", "interp_weights"]

INTERP_TAPS = {"linear": 2, "cubic": 4, "sinc8": 8}       # taps per axis; the position in this table is the library's kind number


def check_trace_offsets(offsets, what="offsets"):
    """offsets (2, X, Y) -> contiguous fp32 numpy array; ValueError for another shape, non-finite values and |d| > 0.5."""
    off = np.asarray(offsets.detach().cpu().numpy() if torch.is_tensor(offsets) else offsets)
    if off.ndim != 3 or off.shape[0] != 2 or off.shape[1] < 1 or off.shape[2] < 1:
        raise ValueError("%s must have the shape (2, X, Y) (plane 0 dx, plane 1 dy), got %s" % (what, tuple(off.shape)))
    off = np.ascontiguousarray(off, dtype=np.float32)
    if not np.all(np.isfinite(off)):
        raise ValueError("%s hold non-finite values" % what)
    if np.abs(off).max() > 0.5:
        raise ValueError("%s must lie in [-0.5, 0.5] grid cells (a trace belongs to the bin it is nearest to), got |d| up to %g"
                         % (what, float(np.abs(off).max())))
    return off


def interp_weights(offsets, interp):
    """offsets (2, X, Y) -> the weight table (2, K, X, Y) fp32 of `interp` (axis, tap, trace), from dpi_trace_interp_weights: float64
    arithmetic from the fp32 offsets, one rounding.  ValueError for an unknown name and for offsets check_trace_offsets refuses."""
    if interp not in INTERP_TAPS:
        raise ValueError("unknown interpolation %r: expected one of %s" % (interp, ", ".join(INTERP_TAPS)))
    off = check_trace_offsets(offsets)
    kind, K = list(INTERP_TAPS).index(interp), INTERP_TAPS[interp]
    L = _lib.load()
    if L.dpi_trace_interp_taps(kind) != K:
        raise _lib.DpiError("libdpi_hip.so has %d taps for %s, this binding %d" % (L.dpi_trace_interp_taps(kind), interp, K))
    w = np.empty((2, K) + off.shape[1:], dtype=np.float32)
    _lib.check(L.dpi_trace_interp_weights(off.ctypes.data_as(ctypes.c_void_p), kind, off.shape[1], off.shape[2],
                                          w.ctypes.data_as(ctypes.c_void_p)), "dpi_trace_interp_weights")
    return w


class TraceSampling(LinearOperator):
    """forward: (1, C, T, X[, Y]) on the grid -> the same shape at the trace positions; adjoint: its exact transpose.  `offsets` is
    (2, X, Y) — dx, dy per trace in grid cells, |d| <= 0.5 — as numpy array or tensor; a 4-D tensor (1, C, T, X) is the case Y = 1.  The
    offsets are checked here and uploaded once per device.  A tensor whose (X, Y) differs from the offsets and a batch other than 1 raise
    ValueError before any launch.  `interp` is "linear" (bilinear, today's kernels), "cubic" or "sinc8" (INTERP_TAPS): for the latter two
    the weight table is built here, once, and uploaded with the offsets; an unknown name raises ValueError."""

    def __init__(self, offsets, interp="linear"):
        super().__init__()
        if interp not in INTERP_TAPS:
            raise ValueError("unknown interpolation %r: expected one of %s" % (interp, ", ".join(INTERP_TAPS)))
        self.interp = interp
        self._off32 = check_trace_offsets(offsets)
        self.X, self.Y = int(self._off32.shape[1]), int(self._off32.shape[2])
        self.offsets = torch.from_numpy(self._off32)
        self.weights = None if interp == "linear" else torch.from_numpy(interp_weights(self._off32, interp))      # (2, K, X, Y)

    def _to_device(self, device):
        """(offsets, the weight table of a non-linear kind or None)"""
        return self.offsets.to(device), None if self.weights is None else self.weights.to(device)

    def _matvec(self, x, adjoint):
        self._check_patch(x, ValueError, "TraceSampling works on (1, C, T, X[, Y]) tensors, got %d axes")
        grid = (int(x.shape[3]), int(x.shape[4]) if x.ndim == 5 else 1)
        if grid != (self.X, self.Y):
            raise ValueError("TraceSampling built from offsets of a %d x %d (X, Y) grid got a tensor of %d x %d"
                             % (self.X, self.Y, grid[0], grid[1]))
        C_, T_ = int(x.shape[1]), int(x.shape[2])
        if C_ < 1 or T_ < 1:
            raise ValueError("TraceSampling: empty tensor %s" % (tuple(x.shape),))
        off, w = self.upload(x.device)
        y = torch.empty_like(x)
        L = _lib.load()
        if w is not None:
            fn, name = ((L.dpi_trace_resample_adj, "dpi_trace_resample_adj") if adjoint
                        else (L.dpi_trace_resample_fwd, "dpi_trace_resample_fwd"))
            _lib.check(fn(_lib.ptr(x), _lib.ptr(w), _lib.ptr(off), INTERP_TAPS[self.interp], C_, T_, self.X, self.Y, _lib.ptr(y),
                          _lib.stream()), name)
            return y
        fn, name = (L.dpi_trace_sample_adj, "dpi_trace_sample_adj") if adjoint else (L.dpi_trace_sample_fwd, "dpi_trace_sample_fwd")
        _lib.check(fn(_lib.ptr(x), _lib.ptr(off), C_, T_, self.X, self.Y, _lib.ptr(y), _lib.stream()), name)
        return y
