"""The convolutional model of seismic data (ours as an operator; the reference ships its pieces, operators/signal.py:8-45 VerticalConv and
operators/derivative.py:8-21 VerticalGrad, without a caller): a known wavelet maps a reflectivity or a log-impedance section to the traces.
forward / adjoint are dpi_wavelet_fwd / dpi_wavelet_adj: one launch each, on 4-D and 5-D tensors whose dim 2 is time."""
import numpy as np
import torch

from .. import _lib
from .base import LinearOperator

__all__ = ["ConvolutionalModelling", "WAVELET_MODEL_KINDS", "WAVELET_MAX_TAPS"]

WAVELET_MODEL_KINDS = ("reflectivity", "impedance")
WAVELET_MAX_TAPS = 255


class ConvolutionalModelling(LinearOperator):
    """forward: (1, C, T, X[, Y]) -> the same shape, every trace filtered along T ('same', zero padded); adjoint: the exact transpose.
        kind = "reflectivity":  d = w * r            taps = w,     no difference      (= 2 VerticalConv(w))
        kind = "impedance":     d = 0.5 w * D m      taps = w / 2, D = the forward difference along T with the last row zero
                                                     (= Chain([VerticalGrad(), VerticalConv(w)]), the post-stack model 0.5 W D ln(AI))
    The taps are rounded ONCE to fp32 on the host (`taps`) and go to a device once (`upload`, or the first call on it), so a captured
    iteration replays the operator unchanged.  ValueError, before any launch, for a wavelet that is not 1-D, empty, of even length, longer
    than 255 samples, not finite or all zero, for an unknown kind and for a batch other than 1."""

    def __init__(self, wavelet, kind="reflectivity"):
        super().__init__()
        if kind not in WAVELET_MODEL_KINDS:
            raise ValueError("kind must be reflectivity or impedance, got %r" % (kind,))
        w = wavelet.detach().cpu().numpy() if torch.is_tensor(wavelet) else np.asarray(wavelet)
        if w.ndim != 1 or w.size < 1 or w.dtype.kind not in "fiu":
            raise ValueError("the wavelet must be a non-empty 1-D array of real numbers, got %s %s" % (w.dtype, tuple(w.shape)))
        if w.size % 2 == 0:
            raise ValueError("the wavelet must have an odd length (its centre sample is time zero), got %d samples" % w.size)
        if w.size > WAVELET_MAX_TAPS:
            raise ValueError("the wavelet must have at most %d samples, got %d" % (WAVELET_MAX_TAPS, w.size))
        w = w.astype(np.float64)
        if not np.all(np.isfinite(w)):
            raise ValueError("the wavelet holds non-finite values")
        self.kind = kind
        self.diff = 1 if kind == "impedance" else 0
        self.taps = np.ascontiguousarray((w / 2 if self.diff else w).astype(np.float32))          # the one rounding
        if not np.all(np.isfinite(self.taps)) or not np.any(self.taps != 0):
            raise ValueError("the wavelet is all zero (or overflows fp32): nothing would reach the loss")

    def _to_device(self, device):
        return torch.from_numpy(self.taps).to(device)

    def _matvec(self, x, adjoint):
        self._check_patch(x, ValueError, "ConvolutionalModelling expects a (1, C, T, X) or (1, C, T, X, Y) tensor, got %d-D", nonempty=True)
        C_, T = int(x.shape[1]), int(x.shape[2])
        S = x.numel() // (C_ * T)
        taps = self.upload(x.device)
        y = torch.empty_like(x)
        L = _lib.load()
        fn, name = (L.dpi_wavelet_adj, "dpi_wavelet_adj") if adjoint else (L.dpi_wavelet_fwd, "dpi_wavelet_fwd")
        _lib.check(fn(_lib.ptr(x), _lib.ptr(taps), int(self.taps.size), self.diff, C_, T, S, _lib.ptr(y), _lib.stream()), name)
        return y
