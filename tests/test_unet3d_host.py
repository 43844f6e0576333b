"""CPU-side tests of the 3-D plain UNet: state_dict parity of UNet3D with the 2-D UNet, same-seed constructor values, the routing of
build_net / get_net, `--upsample deconv` in the parser, the size guard and the C-ABI bookkeeping of csrc/unet3d_ops.hip.  No GPU needed."""
import os
import re

import pytest
import torch
from torch import nn

from conftest import ROOT

from deep_prior_interpolation_amd import _lib
from deep_prior_interpolation_amd.architectures import MulResUnet3D, UNet, UNet3D, build_net, get_net
from deep_prior_interpolation_amd.parameter import parse_arguments

F = [2, 4, 8, 16, 32]
MODES = [("deconv", "deconv"), ("trilinear", "bilinear"), ("nearest", "nearest")]          # (3-D mode, its 2-D counterpart)
UNET3D_SYMBOLS = ["dpi_deconv4x4x4s2_bwd_data", "dpi_deconv4x4x4s2_bwd_weight", "dpi_deconv4x4x4s2_bwd_weight_ws_floats",
                  "dpi_deconv4x4x4s2_fwd", "dpi_maxpool2x2x2_bwd", "dpi_maxpool2x2x2_fwd"]


def _closed_form(cin, cout, f, mode):
    """Parameters of the tree, biases included: 3x3x3 convolutions 27 a b + b, transposed convolutions 64 a b + b, the 1x1x1 head."""
    c3 = lambda a, b: 27 * a * b + b
    n = c3(cin, f[0]) + c3(f[0], f[0])
    for i in range(1, 5):
        n += c3(f[i - 1], f[i]) + c3(f[i], f[i])
    for i in range(4, 0, -1):
        n += (64 * f[i] * f[i - 1] + f[i - 1]) if mode == "deconv" else c3(f[i], f[i - 1])
        n += c3(2 * f[i - 1], f[i - 1]) + c3(f[i - 1], f[i - 1])
    return n + f[0] * cout + cout


@pytest.mark.parametrize("mode,mode2d", MODES)
def test_state_dict_matches_the_2d_net_with_one_more_axis(mode, mode2d):
    m3 = UNet3D(6, 2, F, upsample_mode=mode, act_fun="LeakyReLU")
    m2 = UNet(6, 2, F, upsample_mode=mode2d, act_fun="LeakyReLU")
    k3, k2 = list(m3.state_dict().items()), list(m2.state_dict().items())
    assert [k for k, _ in k3] == [k for k, _ in k2]                                          # same names, same order
    assert k3[0][0] == "start.conv1.0.0.weight" and k3[-1][0].startswith("final.")
    for (k, a), (_, b) in zip(k3, k2):
        want = tuple(b.shape) if b.ndim < 4 else tuple(b.shape) + (b.shape[-1],)
        assert tuple(a.shape) == want, k
    assert sum(p.numel() for p in m3.parameters()) == _closed_form(6, 2, F, mode)
    assert [n for n, _ in m3.named_children()] == ["start", "down1", "down2", "down3", "down4", "up4", "up3", "up2", "up1", "final"]
    # one shared activation instance; no norm in the up blocks; a 1x1x1 head
    assert m3.start.conv1[2] is m3.down4.conv.conv2[2] is m3.up1.conv.conv1[1]
    assert len(m3.up2.conv.conv1) == 2 and type(m3.down2.conv.conv1[1]).__name__ == "InstanceNorm3d"
    assert tuple(m3.final[0].weight.shape) == (2, F[0], 1, 1, 1)
    if mode == "deconv":
        assert "Conv" in type(m3.up4.up).__name__ and isinstance(m3.up4.up, nn.ConvTranspose3d)


def test_widths_need_not_double():
    """The up blocks read the deeper level's width (the 2-D class assumes 2 * out_size)."""
    f = [16, 16, 32, 32, 32]
    m = UNet3D(8, 1, f, "deconv")
    assert tuple(m.up4.up.weight.shape) == (32, 32, 4, 4, 4) and tuple(m.up2.up.weight.shape) == (32, 16, 4, 4, 4)
    assert sum(p.numel() for p in m.parameters()) == _closed_form(8, 1, f, "deconv")


@pytest.mark.parametrize("mode", [m for m, _ in MODES])
def test_same_seed_constructor_values(mode):
    """The constructor draws what a tree of nn.Conv3d / nn.ConvTranspose3d built in the same order draws."""
    cin, cout = 3, 2
    torch.manual_seed(11)
    got = [v for v in UNet3D(cin, cout, F, upsample_mode=mode).state_dict().values()]
    torch.manual_seed(11)
    c3 = lambda a, b: nn.Conv3d(a, b, 3, padding=1)
    mods = [c3(cin, F[0]), c3(F[0], F[0])]
    for i in range(1, 5):
        mods += [c3(F[i - 1], F[i]), c3(F[i], F[i])]
    for i in range(4, 0, -1):
        mods.append(nn.ConvTranspose3d(F[i], F[i - 1], 4, stride=2, padding=1) if mode == "deconv" else c3(F[i], F[i - 1]))
        mods += [c3(2 * F[i - 1], F[i - 1]), c3(F[i - 1], F[i - 1])]
    mods.append(nn.Conv3d(F[0], cout, 1))
    want = [t for m in mods for t in (m.weight, m.bias)]
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert torch.equal(a, b.detach())


def _args(extra):
    return parse_arguments(["--imgdir", "x"] + list(extra))


def test_factory_routes():
    a = _args(["--datadim", "3d", "--net", "unet", "--inputdepth", "4", "--filters", "2", "4", "8", "16", "32", "--upsample", "deconv"])
    n = build_net(a, 1)
    assert type(n) is UNet3D and isinstance(n.up1.up, nn.ConvTranspose3d) and n.start.conv1[0][0].weight.shape[1] == 4
    b = _args(["--datadim", "3d", "--net", "unet", "--inputdepth", "4", "--filters", "2", "4", "8", "16", "32", "--upsample", "linear"])
    assert b.upsample == "trilinear" and type(build_net(b, 1)) is UNet3D
    # the drop-in factory keeps the reference's fall-through
    b.skip = [2, 4, 8, 16]
    ref = MulResUnet3D(num_input_channels=4, num_channels_down=F, num_channels_up=F, num_channels_skip=b.skip, upsample_mode="trilinear")
    got = get_net(b, 1)
    assert type(got) is type(ref) and type(got) is not UNet3D and list(got.state_dict()) == list(ref.state_dict())
    # the 2-D routes are get_net's own
    c = _args(["--datadim", "2d", "--net", "unet", "--upsample", "deconv"])
    assert type(build_net(c, 1)) is UNet and isinstance(build_net(c, 1).up1.up, nn.ConvTranspose2d)


def test_parser_accepts_deconv_with_unet_only():
    for dd, extra in (("2d", []), ("2.5d", ["--imgchannel", "3"]), ("3d", [])):
        a = _args(["--datadim", dd, "--net", "unet", "--upsample", "deconv"] + extra)
        assert a.upsample == "deconv"                                                          # post-processing leaves it
    for net in ("multiunet", "skip", "attmultiunet", "part"):
        with pytest.raises(ValueError) as e:
            _args(["--datadim", "3d", "--net", net, "--upsample", "deconv"])
        assert "--upsample" in str(e.value)
    # --net load: the saved args.txt decides the net, and net_args_are_same compares the flag with it, so the flag must parse
    assert _args(["--datadim", "3d", "--net", "load", "--netdir", "a/0_model.pth", "--upsample", "deconv"]).upsample == "deconv"
    with pytest.raises(ValueError) as e:
        _args(["--datadim", "3d", "--upsample", "deconv"])                                     # the default net
    assert "--upsample" in str(e.value)


def test_size_guard_raises_before_any_launch():
    """On the CPU a launch would fail for want of a device: the guard must come first."""
    m = UNet3D(2, 1, F, "deconv")
    for shape, word in (((1, 2, 24, 16, 16), "divisible by 16"), ((1, 2, 16, 16, 16), "single voxel"), ((1, 2, 32, 16, 8), "divisible by 16"),
                        ((1, 2, 32, 16), "(1, C, D, H, W)")):
        with pytest.raises(ValueError) as e:
            m(torch.zeros(shape))
        assert word in str(e.value) and str(shape[2]) in str(e.value), str(e.value)
    UNet3D.check_size((1, 2, 32, 16, 16))                                                      # accepted
    UNet3D.check_size((1, 2, 16, 16, 48))


def test_abi_lists_the_new_entry_points():
    txt = open(os.path.join(ROOT, "include", "dpi_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    header = set(re.findall(r"\b(dpi_[a-z0-9_]+)\s*\(", txt))
    new_h = sorted(s for s in header if "2x2x2" in s or "4x4x4" in s)
    new_t = sorted(s for s in _lib.SIGNATURES if "2x2x2" in s or "4x4x4" in s)
    assert new_h == new_t == UNET3D_SYMBOLS
    assert len(_lib.SIGNATURES["dpi_deconv4x4x4s2_bwd_weight"][1]) == 10 and len(_lib.SIGNATURES["dpi_maxpool2x2x2_fwd"][1]) == 7
