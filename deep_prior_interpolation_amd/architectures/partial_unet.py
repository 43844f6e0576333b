"""Partial-convolution UNet, 2-D and 3-D (drop-in for PartialUNet / PartialUNet3D of reference architectures/partial_unet.py).

Five encoder blocks of a partial convolution (the result re-normalised by the number of known samples under the stencil, a shrinking hole
map handed on) and a learned stride-2 convolution, a decoder of plain convolutions and nearest up-sampling, the input concatenated in
front of the last four layers.  One implementation parametrised by `nd`.  Child names, registration and construction order follow the
reference (partial_unet.py:6-303), so state_dict keys and shapes coincide: 57 entries in 2-D, 62 in 3-D (Partial2DBlock does not hand
`bias` to its partial convolution, Partial3DBlock does: partial_unet.py:164,179).

The reference defines the net and cannot run it from its main.py.  What is fixed on purpose here:
  * `mask_conv` is a MaskWindow, not a convolution: its all-ones `weight` is a persistent BUFFER of the reference's shape.  The reference's
    init_weights re-draws every mask_conv.weight from N(0, gain) because the class name contains "Conv" (utils/torch.py:34-53), which turns the
    "number of known samples" into a random signed number; here init_weights passes it by.  It is out of parameters(), so num_params is lower than
    the reference's count by these five tensors, and a state_dict whose mask_conv.weight is not all ones is refused (the kernel assumes ones).
  * the mask may have one channel (broadcast over the input's); the reference's mask_conv expects the input's channels.
  * the hole map is carried as ONE channel (the reference's Cout channels are identical) and the learned `down` convolution is applied to it
    with down.weight summed over its input channels — the same numbers, without the 48-channel tensor.
  * sizes the five stride-2 levels cannot halve and double back raise ValueError before anything is launched (the reference fails in torch.cat).
"""
import torch
from torch import nn

from .. import nn as hnn
from .. import ops
from .base import get_activation

__all__ = ["MaskWindow", "PartialConv", "PartialConv2d", "PartialConv3d", "PartialBlock", "PartialBlock2d", "PartialBlock3d", "PartialNet",
           "PartialUNet", "PartialUNet3D"]

_LEVELS = 5


def _conv_cls(nd):
    return hnn.Conv3d if nd == 3 else hnn.Conv2d


class MaskWindow(nn.Module):
    """The reference's frozen all-ones `mask_conv` (partial_unet.py:26-28,35-36) as a buffer.  Construction draws from torch's generator exactly
    as nn.ConvNd(in, out, 3, 1, 1, bias=False) does, so the same-seed initial values of every later layer stay those of the reference class.
    The class name holds neither "Conv" nor "BatchNorm": init_weights leaves the ones alone."""

    def __init__(self, nd, in_channels, out_channels):
        super().__init__()
        drawn = (nn.Conv3d if nd == 3 else nn.Conv2d)(in_channels, out_channels, 3, 1, 1, bias=False)          # the reference's draw, discarded
        self.register_buffer("weight", torch.ones_like(drawn.weight.detach()))

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        w = state_dict.get(prefix + "weight")
        if w is not None and tuple(w.shape) == tuple(self.weight.shape) and not bool((w == 1).all()):
            raise ValueError("%sweight is not all ones: the partial-convolution kernel counts the known samples under the stencil and has no "
                             "weighted form (a reference checkpoint saved after init_weights holds N(0, gain) there)" % prefix)
        super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)


class PartialConv(nn.Module):
    """partial_unet.py:6-80 (2-D) / 83-157 (3-D): children input_conv, mask_conv, bn, act, dr in the reference's order."""

    def __init__(self, nd, in_channels, out_channels, bn=True, bias=False, sample="none-3", act_fun="ReLU", drop=0.0):
        super().__init__()
        if sample != "none-3":
            raise NotImplementedError("PartialConv: sample=%r (stride-2 stencils of 3 / 5 / 7) has no kernel; the nets use 'none-3' only" % (sample,))
        self.nd = nd
        self.input_conv = _conv_cls(nd)(in_channels, out_channels, 3, 1, 1, bias=bias)
        self.mask_conv = MaskWindow(nd, in_channels, out_channels)
        nn.init.kaiming_normal_(self.input_conv.weight, a=0, mode="fan_in")
        self.bn = (hnn.BatchNorm3d if nd == 3 else hnn.BatchNorm2d)(out_channels) if bn else None
        self.act = get_activation(act_fun)
        self.dr = hnn.Dropout(drop)

    def forward(self, input_x, mask):
        y, new_mask = ops.partial_conv(input_x, mask, self.input_conv.weight, self.input_conv.bias)
        fold = self.bn is not None and isinstance(self.act, hnn.LeakyReLU)
        if self.bn is not None:
            b = self.bn
            y = ops.batch_norm(y, b.weight, b.bias, b.running_mean, b.running_var, b.num_batches_tracked,
                               self.act.negative_slope if fold else 1.0)
        if not fold:
            y = self.act(y)
        return self.dr(y), new_mask


class PartialBlock(nn.Module):
    """partial_unet.py:160-187: partial convolution, then the learned stride-2 `down` on the tensor AND on the hole map."""

    def __init__(self, nd, input_channel, out_channels, bn, act_fun, bias, drop):
        super().__init__()
        if nd == 3:
            self.partialconv = PartialConv(3, input_channel, out_channels, bn=bn, act_fun=act_fun, bias=bias, drop=drop)
        else:
            self.partialconv = PartialConv(2, input_channel, out_channels, bn=bn, act_fun=act_fun, drop=drop)        # no bias: partial_unet.py:164
        self.down = _conv_cls(nd)(out_channels, out_channels, 3, 2, 1, bias=bias)
        self.dr = hnn.Dropout(drop)

    def forward(self, x, mask):
        x, new_mask = self.partialconv(x, mask)
        # down(new_mask) of the reference with its identical channels folded into the weight; autograd's expand hands every input channel of
        # down.weight the gradient
        mask = ops.conv(new_mask, self.down.weight.sum(dim=1, keepdim=True), self.down.bias, 2)
        return self.dr(self.down(x)), self.dr(mask)


def _plain(nd, cin, cout):
    return _conv_cls(nd)(cin, cout, 3, 1, 1, bias=False)


class PartialNet(nn.Module):
    """partial_unet.py:190-303 with `nd` as a parameter.  forward(input_x, mask): mask of input_x's shape or with one channel."""

    def __init__(self, nd, num_input_channels=1, num_output_channels=1, use_bn=True, need_bias=True, act_fun="LeakyReLU", dropout=0.0):
        super().__init__()
        self.nd = nd
        self.layers = _LEVELS
        cin = num_input_channels
        for i in range(1, _LEVELS + 1):
            setattr(self, "enc%d" % i, PartialBlock(nd, cin, 48, use_bn, act_fun, need_bias, dropout))
            cin = 48
        self.dec5 = hnn.Upsample(scale_factor=2, mode="nearest")
        for name, c in (("dec4", 96), ("dec3", 144), ("dec2", 144), ("dec1", 144)):
            setattr(self, name, nn.Sequential(_plain(nd, c, 96), _plain(nd, 96, 96), hnn.Upsample(scale_factor=2, mode="nearest"),
                                              hnn.Dropout(dropout)))
        self.last_kernel = nn.Sequential(_plain(nd, 96 + num_input_channels, 96), _plain(nd, 96, 64), _plain(nd, 64, 32),
                                         _plain(nd, 32, num_output_channels))

    def check_shapes(self, input_x, mask):
        name = "PartialUNet3D" if self.nd == 3 else "PartialUNet"
        if mask is None:
            raise TypeError("%s.forward(input_x, mask) needs the mask of known samples" % name)
        if input_x.ndim != self.nd + 2:
            raise ValueError("%s: expected a %d-D input (1, C, %s), got shape %s"
                             % (name, self.nd + 2, "D, H, W" if self.nd == 3 else "H, W", tuple(input_x.shape)))
        if any(s % (1 << _LEVELS) for s in input_x.shape[2:]):
            raise ValueError("%s needs every spatial size divisible by %d (five stride-2 levels, nearest x2 back up); got input shape %s"
                             % (name, 1 << _LEVELS, tuple(input_x.shape)))
        if mask.ndim != input_x.ndim or tuple(mask.shape[2:]) != tuple(input_x.shape[2:]) or mask.shape[1] not in (1, input_x.shape[1]):
            raise ValueError("%s: mask %s does not fit input %s (the input's grid, its channels or one)"
                             % (name, tuple(mask.shape), tuple(input_x.shape)))

    def forward(self, input_x, mask=None):
        self.check_shapes(input_x, mask)
        downs, x = [], input_x
        for i in range(1, _LEVELS + 1):
            x, mask = getattr(self, "enc%d" % i)(x, mask)
            downs.append(x)
        up = self.dec5(downs[4])
        for name, skip in (("dec4", downs[3]), ("dec3", downs[2]), ("dec2", downs[1]), ("dec1", downs[0])):
            up = getattr(self, name)(ops.concat_crop([skip, up]))
        return self.last_kernel(ops.concat_crop([input_x, up]))


def PartialConv2d(in_channels, out_channels, bn=True, bias=False, sample="none-3", act_fun="ReLU", drop=0.0):
    return PartialConv(2, in_channels, out_channels, bn, bias, sample, act_fun, drop)


def PartialConv3d(in_channels, out_channels, bn=True, bias=False, sample="none-3", act_fun="ReLU", drop=0.0):
    return PartialConv(3, in_channels, out_channels, bn, bias, sample, act_fun, drop)


def PartialBlock2d(input_channel, out_channels, bn, act_fun, bias, drop):
    return PartialBlock(2, input_channel, out_channels, bn, act_fun, bias, drop)


def PartialBlock3d(input_channel, out_channels, bn, act_fun, bias, drop):
    return PartialBlock(3, input_channel, out_channels, bn, act_fun, bias, drop)


def PartialUNet(num_input_channels=1, num_output_channels=1, use_bn=True, need_bias=True, act_fun="LeakyReLU", dropout=0.0):
    """2-D partial-convolution UNet (reference partial_unet.py:190-245)."""
    return PartialNet(2, num_input_channels, num_output_channels, use_bn, need_bias, act_fun, dropout)


def PartialUNet3D(num_input_channels=1, num_output_channels=1, use_bn=True, need_bias=True, act_fun="LeakyReLU", dropout=0.0):
    """3-D partial-convolution UNet (reference partial_unet.py:248-303)."""
    return PartialNet(3, num_input_channels, num_output_channels, use_bn, need_bias, act_fun, dropout)
