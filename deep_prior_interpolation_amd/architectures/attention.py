"""Attention-gated MultiRes-UNet, 2-D and 3-D (drop-in for AttMulResUnet2D of reference architectures/attention.py).

A MultiRes-UNet without ResPaths whose skip tensors pass through grid-attention gates: the decoder block of a level reads
cat[skip * gate, Upsample(deeper)], gate = Upsample(x2, linear)(sigmoid(psi(relu(W_g(deeper) + W_x(skip))))).  One implementation
parametrised by `nd`, like mulresunet.py; the reference has the 2-D net only, the 3-D one is this project's (trilinear gate,
3-D MultiRes blocks).  Child names, registration and construction order follow the reference (attention.py:86-113, 212-248) so
that state_dict keys and same-seed initial values coincide in 2-D.  The gate itself and the concatenation run as one HIP node
(ops.attention_gate); the one-channel map in front of it is composed from the existing conv / BatchNorm / add / ReLU nodes.
"""
from torch import nn

from .. import nn as hnn
from .. import ops
from .base import conv_nd, get_activation
from .mulresunet import DownPath, MultiResBlock

__all__ = ["AttMulResUnet", "AttMulResUnet2D", "AttMulResUnet3D", "GridAttentionBlock"]


def _bn(nd, f):
    return (hnn.BatchNorm3d if nd == 3 else hnn.BatchNorm2d)(f)


def _conv_bn(seq, x):
    """Sequential(conv, BatchNorm) without an activation: conv -> BN as ConvBnActFn with slope 1."""
    conv_m, bn = seq[0][0], seq[1]
    return ops.conv_bn_act(x, conv_m.weight, conv_m.bias, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.num_batches_tracked,
                           conv_m._s, 1.0)


class GridAttentionBlock(nn.Module):
    """attention.py:86-113.  g: the coarse (deeper) tensor, F_g channels; x: the skip tensor, F_l channels on the twice finer grid.
    psi[1] (Sigmoid) and psi[2] (Upsample) hold no parameters: they keep the reference's child positions, and run fused with the
    product inside ops.attention_gate.  The gate is always up-sampled linearly, whatever the net's --upsample."""

    def __init__(self, nd, F_g, F_l, F_int):
        super().__init__()
        self.nd = nd
        self.W_g = nn.Sequential(conv_nd(nd, F_g, F_int, 1, 1), _bn(nd, F_int))
        self.W_x = nn.Sequential(conv_nd(nd, F_l, F_int, 3, 2), _bn(nd, F_int))
        self.psi = nn.Sequential(conv_nd(nd, F_int, 1, 1, 1), hnn.Activation("Sigmoid"),
                                 hnn.Upsample(scale_factor=2, mode="trilinear" if nd == 3 else "bilinear"))
        self.relu = hnn.LeakyReLU(0.0)

    def gate_map(self, g, x):
        """q = psi[0](relu(W_g(g) + W_x(x))): one channel on g's grid, before the sigmoid."""
        return self.psi[0](self.relu(ops.add(_conv_bn(self.W_g, g), _conv_bn(self.W_x, x))))

    def forward(self, g, x):
        return ops.attention_gate(x, self.gate_map(g, x), None)


class AttMulResUnet(nn.Module):
    """attention.py:197-262 with `nd` as a parameter and any number n >= 2 of scales (the reference hard-codes five)."""

    def __init__(self, nd, num_input_channels=1, num_output_channels=3, num_channels_down=(16, 32, 64, 128, 256), alpha=1.67,
                 last_act_fun=None, need_bias=True, upsample_mode="nearest", act_fun="LeakyReLU", dropout=0.0):
        super().__init__()
        filters = list(num_channels_down)
        n = len(filters)
        if n < 2:
            raise ValueError("AttMulResUnet needs at least two scales (got --filters %s)" % (filters,))
        if not isinstance(upsample_mode, (list, tuple)):
            upsample_mode = [upsample_mode] * n
        self.nd, self.n_scales = nd, n
        depths = [num_input_channels]
        for i in range(n):
            mrb = MultiResBlock(nd, filters[i], depths[-1], alpha, act_fun, need_bias, dropout)
            depths.append(mrb.out_dim)
            setattr(self, "down_mb%d" % (i + 1), mrb)
        for i in range(1, n):
            # stride-2 conv -> BatchNorm -> act -> dropout: the BatchNorm is there in 2-D as well, unlike MulResUnet (attention.py:227-232)
            setattr(self, "down%d" % i, DownPath(conv_nd(nd, depths[i], depths[i], 3, stride=2, bias=need_bias), _bn(nd, depths[i]),
                                                 get_activation(act_fun), hnn.Dropout(dropout)))
            setattr(self, "up_mb%d" % i, MultiResBlock(nd, filters[-(i + 1)], depths[-i] + depths[-(i + 1)], alpha, act_fun, need_bias, dropout))
            setattr(self, "att%d" % i, GridAttentionBlock(nd, depths[-i], depths[-(i + 1)], filters[-i]))
            setattr(self, "up%d" % i, hnn.Upsample(scale_factor=2, mode=upsample_mode[i]))
        if isinstance(last_act_fun, str) and last_act_fun.lower() == "none":
            last_act_fun = None
        if last_act_fun is not None:
            self.outconv = nn.Sequential(conv_nd(nd, depths[1], num_output_channels, 1, 1, bias=need_bias), get_activation(last_act_fun))
        else:
            self.outconv = conv_nd(nd, depths[1], num_output_channels, 1, 1, bias=need_bias)

    def forward(self, inp):
        n = self.n_scales
        if inp.ndim != self.nd + 2:
            raise ValueError("AttMulResUnet%dD: expected a %d-D input (1, C, %s), got shape %s"
                             % (self.nd, self.nd + 2, "D, H, W" if self.nd == 3 else "H, W", tuple(inp.shape)))
        if any(s % (1 << (n - 1)) for s in inp.shape[2:]):
            raise ValueError("AttMulResUnet%dD with %d scales needs every spatial size divisible by %d (the gates join tensors of exactly "
                             "twice the size); got input shape %s" % (self.nd, n, 1 << (n - 1), tuple(inp.shape)))
        xs = [self.down_mb1(inp)]
        for k in range(1, n):
            xs.append(getattr(self, "down_mb%d" % (k + 1))(getattr(self, "down%d" % k)(xs[-1])))
        g = xs[-1]
        for i in range(1, n):
            skip, att = xs[n - 1 - i], getattr(self, "att%d" % i)
            g = getattr(self, "up_mb%d" % i)(ops.attention_gate(skip, att.gate_map(g, skip), g, getattr(self, "up%d" % i).mode))
        return self.outconv(g)


def AttMulResUnet2D(num_input_channels=1, num_output_channels=3, num_channels_down=(16, 32, 64, 128, 256), alpha=1.67, last_act_fun=None,
                    need_bias=True, upsample_mode="nearest", act_fun="LeakyReLU", dropout=0.0):
    """2-D attention MultiRes-UNet (reference attention.py:197-262)."""
    return AttMulResUnet(2, num_input_channels, num_output_channels, num_channels_down, alpha, last_act_fun, need_bias, upsample_mode,
                         act_fun, dropout)


def AttMulResUnet3D(num_input_channels=1, num_output_channels=1, num_channels_down=(16, 32, 64, 128, 256), alpha=1.67, last_act_fun=None,
                    need_bias=True, upsample_mode="nearest", act_fun="LeakyReLU", dropout=0.0):
    """3-D attention MultiRes-UNet (no reference counterpart: the 2-D net with 3-D blocks and a trilinear gate)."""
    return AttMulResUnet(3, num_input_channels, num_output_channels, num_channels_down, alpha, last_act_fun, need_bias, upsample_mode,
                         act_fun, dropout)
