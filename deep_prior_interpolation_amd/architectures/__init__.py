"""Network factory — drop-in for reference architectures/__init__.py:10-86.

`get_net(args, outchannel)` consumes the same Namespace fields (datadim, net, inputdepth, filters, skip,
upsample, activation, last_activation, dropout) and returns an nn.Module whose state_dict keys equal the
reference's, built from HIP-backed leaf modules.  `build_net` is what the Interpolator calls: get_net plus `--datadim 3d --net part`,
a route of get_net that the host suite pins as refused, and `--datadim 3d --net unet`, which get_net (like the reference's) lets fall through to
MulResUnet3D and build_net routes to UNet3D.
"""
from .base import *            # noqa: F401,F403
from .mulresunet import *      # noqa: F401,F403
from .skip import *            # noqa: F401,F403
from .unet import *            # noqa: F401,F403
from .attention import *       # noqa: F401,F403
from .partial_unet import *    # noqa: F401,F403
from .unet import UNet, UNet3D
from .attention import AttMulResUnet2D, AttMulResUnet3D
from .mulresunet import MulResUnet, MulResUnet3D
from .partial_unet import PartialUNet, PartialUNet3D
from .skip import Skip, Skip3D


def _partial(cls, args, outchannel):
    return cls(args.inputdepth, outchannel, use_bn=True, need_bias=True, act_fun=args.activation, dropout=args.dropout)


def build_net(args, outchannel=1):
    """What the Interpolator builds: get_net, and the nets that get_net's pinned routes keep from it — `--datadim 3d --net part` and
    `--datadim 3d --net unet` (get_net keeps the reference's fall-through to MulResUnet3D there: its drop-in contract)."""
    if getattr(args, "net", "multiunet") == "part" and args.datadim == "3d":
        return _partial(PartialUNet3D, args, outchannel)
    if getattr(args, "net", "multiunet") == "unet" and args.datadim == "3d":
        return UNet3D(num_input_channels=args.inputdepth, num_output_channels=outchannel, filters=args.filters, upsample_mode=args.upsample,
                      need_bias=True, act_fun=args.activation, last_act_fun=args.last_activation, dropout=args.dropout)
    return get_net(args, outchannel)


def get_net(args, outchannel=1):
    net_name = getattr(args, "net", "multiunet")
    if net_name == "attmultiunet":
        # upstream routes 2d and 2.5d to AttMulResUnet2D (architectures/__init__.py:23-33) and has no 3-D attention net; AttMulResUnet3D is ours
        if args.datadim == "2d":
            raise NotImplementedError("--datadim 2d --net attmultiunet is held back on purpose: AttMulResUnet2D exists (architectures/attention.py), but the "
                                      "host suite pins the 2d route of this factory as refused (tests/test_host.py); --datadim 2.5d builds the same net")
        cls = AttMulResUnet3D if args.datadim == "3d" else AttMulResUnet2D
        return cls(num_input_channels=args.inputdepth, num_output_channels=outchannel, num_channels_down=args.filters,
                   upsample_mode=args.upsample, need_bias=True, act_fun=args.activation, last_act_fun=args.last_activation,
                   dropout=args.dropout)
    if net_name == "part":
        # upstream routes 2d and 2.5d to PartialUNet and 3d to PartialUNet3D (architectures/__init__.py) but calls them without their mask
        # (main.py:159): here Interpolator.net_forward passes it.  --filters / --skip / --upsample / --last_activation are ignored, as upstream
        if args.datadim == "2d":
            raise NotImplementedError("--datadim 2d --net part is held back on purpose: PartialUNet exists (architectures/partial_unet.py), but the "
                                      "host suite pins the 2d route of this factory as refused (tests/test_host.py); --datadim 2.5d builds the same net")
        if args.datadim == "3d":
            raise NotImplementedError("get_net holds its 3d route for --net part on purpose: the host suite pins it as refused "
                                      "(tests/test_attention_host.py).  PartialUNet3D exists (architectures/partial_unet.py) and "
                                      "architectures.build_net, which the Interpolator calls, builds it")
        return _partial(PartialUNet, args, outchannel)
    common = dict(num_input_channels=args.inputdepth, num_output_channels=outchannel, upsample_mode=args.upsample,
                  need_bias=True, act_fun=args.activation, last_act_fun=args.last_activation, dropout=args.dropout)
    if args.datadim in ("2d", "2.5d"):
        if net_name == "unet":
            # upstream names an undefined `UNetMod` here (architectures/__init__.py:13); the intended class is unet.UNet
            return UNet(num_input_channels=args.inputdepth, num_output_channels=outchannel, filters=args.filters,
                        upsample_mode=args.upsample, need_bias=True, act_fun=args.activation,
                        last_act_fun=args.last_activation, dropout=args.dropout)
        if net_name == "skip":
            # BASELINE configs[3] names the 2.5-D skip net.  Upstream cannot reach its 2-D `Skip` (architectures/skip.py:5-48): `--net` has
            # no such choice and get_net falls through to MulResUnet (architectures/__init__.py:41-53).  Documented deviation, like
            # `--net skip` in 3-D: same argument mapping as the Skip3D branch (architectures/__init__.py:62-72), which needs one skip
            # width per scale (len(--skip) == len(--filters))
            if len(args.skip) != len(args.filters):
                raise ValueError("--net skip needs one --skip width per --filters scale (got %d and %d)" % (len(args.skip), len(args.filters)))
            return Skip(num_channels_down=args.filters, num_channels_up=args.filters, num_channels_skip=args.skip, **common)
        return MulResUnet(num_channels_down=args.filters, num_channels_up=args.filters, num_channels_skip=args.skip, **common)
    if net_name == "skip":
        return Skip3D(num_channels_down=args.filters, num_channels_up=args.filters, num_channels_skip=args.skip, **common)
    return MulResUnet3D(num_channels_down=args.filters, num_channels_up=args.filters, num_channels_skip=args.skip, **common)
