"""The pre-stack convolutional model (ours, --wavelet_domain): the wavelet W of --wavelet and the moveout L of --moveout as one operator.
    domain = "data":   d = W L r   L moves the section out, W (behind D for a log-impedance) acts along recorded time: the wavelet is not
                                   stretched.  forward = dpi_moveout_fwd then dpi_wavelet_fwd; adjoint = dpi_wavelet_adj then
                                   dpi_moveout_adj.
    domain = "model":  d = L W r   W acts along zero-offset time, L moves the band-limited section out: the wavelet stretches with the
                                   events.  forward = dpi_wavelet_fwd then dpi_moveout_fwd; adjoint = dpi_moveout_adj then dpi_wavelet_adj.
Two launches each way, the kernels of the two parts and nothing else, so `first` applied to a model gives the tensor the iteration saw
(a forward pass that takes the moveout while the wavelet kernel stages its tile was built and measured slower: DESIGN.md §3.2)."""
import numpy as np

from .base import LinearOperator
from .moveout import Moveout
from .wavelet import ConvolutionalModelling

__all__ = ["PrestackModelling", "PRESTACK_DOMAINS", "erode_live"]

PRESTACK_DOMAINS = ("data", "model")


def erode_live(live, K, diff=0):
    """L's live map (T, X[, Y]) -> the map of the data samples W can be compared at behind L: sample t is live only if every row of L r
    inside [0, T) that a wavelet of K taps reads for it is live, rows t - K/2 .. t + K/2 and, behind the forward difference (diff = 1),
    row t + K/2 + 1 as well.  L writes 0 at a muted sample, so next to a mute the convolution is a truncated one.  Rows outside [0, T)
    are the zeros --wavelet alone assumes: they do not erode."""
    live = np.asarray(live, dtype=bool)
    T, p = int(live.shape[0]), int(K) // 2
    dead = np.zeros((T + 1,) + live.shape[1:], dtype=np.int64)
    np.cumsum(~live, axis=0, out=dead[1:])                       # dead[j] = muted rows below j
    t = np.arange(T)
    lo, hi = np.clip(t - p, 0, T), np.clip(t + p + int(diff) + 1, 0, T)
    return dead[hi] == dead[lo]


class PrestackModelling(LinearOperator):
    """forward: (1, C, T, X[, Y]) -> the same shape, d = W L x (domain "data") or d = L W x (domain "model"); adjoint: the exact
    transpose, the adjoints of the parts in reverse order.  `wavelet` is the wavelet (1-D, odd length <= 255) or a ready
    ConvolutionalModelling, `table` the moveout table (T, X[, Y]) or a ready Moveout: ready parts are used as they are (`interp` and
    `kind` then are theirs), so whoever holds them launches the same kernels on the same device tensors.  `first` / `second` are the
    parts in the order of the forward pass.  `live` is the boolean map of the data samples that count: L's live map under "model"; under
    "data" that map eroded along t by the reach of the wavelet (erode_live).  As one operator the pair is one autograd node: the tensor
    between the parts is not kept for the backward pass.  ValueError, before any launch, for what either part refuses and for an
    unknown domain."""

    def __init__(self, wavelet, table, interp="linear", kind="reflectivity", domain="data"):
        super().__init__()
        if domain not in PRESTACK_DOMAINS:
            raise ValueError("domain must be data or model, got %r" % (domain,))
        self.wavelet = wavelet if isinstance(wavelet, ConvolutionalModelling) else ConvolutionalModelling(wavelet, kind=kind)
        self.moveout = table if isinstance(table, Moveout) else Moveout(table, interp=interp)
        self.domain = domain
        self.kind, self.interp = self.wavelet.kind, self.moveout.interp
        self.first, self.second = (self.moveout, self.wavelet) if domain == "data" else (self.wavelet, self.moveout)
        self.live = erode_live(self.moveout.live, self.wavelet.taps.size, self.wavelet.diff) if domain == "data" else self.moveout.live

    def _to_device(self, device):
        """(taps, (table, ranges)): both parts go up, and stay with the parts"""
        return self.wavelet.upload(device), self.moveout.upload(device)

    def _matvec(self, x, adjoint):
        # what the second part would refuse is refused here, ahead of the first part's launch
        self._check_patch(x, ValueError, "PrestackModelling expects a (1, C, T, X) or (1, C, T, X, Y) tensor, got %d-D", nonempty=True)
        if tuple(x.shape[2:]) != tuple(self.moveout.table.shape):
            raise ValueError("PrestackModelling built from a table of shape %s got a tensor of shape %s: its (T, X[, Y]) must be the table's"
                             % (tuple(self.moveout.table.shape), tuple(x.shape)))
        a, b = (self.second, self.first) if adjoint else (self.first, self.second)
        return b._matvec(a._matvec(x, adjoint), adjoint)
