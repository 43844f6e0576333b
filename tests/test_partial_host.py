"""CPU-side tests of --net part: state_dict parity with the reference's PartialUNet / PartialUNet3D, same-seed constructor values, the frozen
mask window, the routing of get_net, the shape guard and the C-ABI bookkeeping of the partial-convolution kernels.  No GPU needed."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from conftest import ROOT, jstr

from deep_prior_interpolation_amd import utils as u
from deep_prior_interpolation_amd.architectures import build_net, get_net
from deep_prior_interpolation_amd.architectures.partial_unet import (MaskWindow, PartialConv2d, PartialConv3d, PartialNet, PartialUNet,
                                                                     PartialUNet3D)
from deep_prior_interpolation_amd.parameter import parse_arguments

PCONV_SYMBOLS = ["dpi_pconv_mask_bwd", "dpi_pconv_mask_fwd", "dpi_pconv_norm_bwd", "dpi_pconv_norm_bwd_ws_floats", "dpi_pconv_norm_fwd"]
NETS = {"net2d": lambda: PartialUNet(3, 2), "net3d": lambda: PartialUNet3D(2, 1)}


def _checksum(v):
    return np.concatenate([[v.double().sum().item()], v.double().reshape(-1)[:4].numpy()])


@pytest.mark.parametrize("name,count", [("net2d", 57), ("net3d", 62)])
def test_state_dict_keys_match_the_reference(golden, name, count):
    g = golden("partial")[name]
    m = NETS[name]()
    keys = [[k, list(v.shape)] for k, v in m.state_dict().items()]
    assert keys == jstr(g["keys"]) and len(keys) == count                       # same names, shapes AND order
    # the reference's quirk the keys depend on: Partial2DBlock does not hand `bias` to its partial convolution, Partial3DBlock does
    assert ("enc1.partialconv.input_conv.bias" in m.state_dict()) == (name == "net3d")


@pytest.mark.parametrize("name", ["net2d", "net3d"])
def test_same_seed_constructor_values_are_bit_identical(golden, name):
    g = golden("partial")[name]["checksums"]
    torch.manual_seed(int(golden("partial")["meta"]["seed"]))
    m = NETS[name]()
    sd = m.state_dict()
    assert sorted(sd) == sorted(g)
    for k, v in sd.items():
        assert np.array_equal(_checksum(v), g[k]), k


@pytest.mark.parametrize("name", ["net2d", "net3d"])
def test_mask_window_is_ones_frozen_and_not_a_parameter(name):
    m = NETS[name]()
    u.init_weights(m, "xavier", 0.02)
    windows = [(k, w) for k, w in m.named_modules() if isinstance(w, MaskWindow)]
    assert len(windows) == 5 and all("Conv" not in type(w).__name__ for _, w in windows)
    for k, w in windows:
        assert bool((w.weight == 1).all()), k
        assert not w.weight.requires_grad
    names = [k for k, _ in m.named_parameters()]
    assert not any("mask_conv" in k for k in names) and all(p.requires_grad for p in m.parameters())
    assert len(names) == len(m.state_dict()) - 5 - 15                             # 5 windows, 5 x (running_mean, running_var, num_batches_tracked)
    assert m.enc1.partialconv.mask_conv.weight.shape == m.enc1.partialconv.input_conv.weight.shape
    # init_weights did draw the convolutions (xavier, gain 0.02) and left no bias
    assert float(m.enc2.down.weight.detach().std()) < 0.01 and float(m.enc2.down.bias.detach().abs().max()) == 0.0


def test_loading_a_mask_window_that_is_not_ones_raises():
    m = PartialUNet(3, 2)
    sd = m.state_dict()
    m.load_state_dict(sd)                                                          # its own state loads
    sd = {k: v.clone() for k, v in sd.items()}
    sd["enc3.partialconv.mask_conv.weight"][0, 0, 1, 1] = 0.5
    with pytest.raises(ValueError) as e:
        m.load_state_dict(sd)
    assert "enc3.partialconv.mask_conv.weight" in str(e.value)


def test_only_the_default_stencil_exists():
    for sample in ("down-3", "down-5", "down-7"):
        with pytest.raises(NotImplementedError):
            PartialConv2d(3, 4, sample=sample)
        with pytest.raises(NotImplementedError):
            PartialConv3d(3, 4, sample=sample)


def _args(datadim, extra=()):
    return parse_arguments(["--imgdir", "x", "--datadim", datadim, "--net", "part", "--inputdepth", "4"] + list(extra))


def test_routing():
    """3d and 2.5d build, 2d is refused.  The 3-D net is built by build_net, which the Interpolator calls: get_net's own 3d route is pinned as
    refused by tests/test_attention_host.py and says where the net is."""
    n3 = build_net(_args("3d", ["--filters", "4", "8", "--upsample", "linear", "--last_activation", "Sigmoid"]), 1)          # ignored, as in the reference
    assert isinstance(n3, PartialNet) and n3.nd == 3
    assert [(k, tuple(v.shape)) for k, v in n3.state_dict().items()] == [(k, tuple(v.shape)) for k, v in PartialUNet3D(4, 1).state_dict().items()]
    assert type(n3.enc1.partialconv.bn).__name__ == "BatchNorm3d" and n3.enc1.down.bias is not None
    with pytest.raises(NotImplementedError) as e:
        get_net(_args("3d"), 1)
    assert "build_net" in str(e.value) and "PartialUNet3D" in str(e.value)
    for factory in (get_net, build_net):
        n25 = factory(_args("2.5d", ["--imgchannel", "3", "--activation", "ReLU"]), 3)
        assert isinstance(n25, PartialNet) and n25.nd == 2
        assert n25.last_kernel[3].weight.shape == (3, 32, 3, 3) and n25.enc1.partialconv.act.negative_slope == 0.0
        with pytest.raises(NotImplementedError) as e:             # the 2d route is held (tests/test_host.py), on purpose and saying so
            factory(_args("2d"), 1)
        assert "2.5d" in str(e.value) and "PartialUNet" in str(e.value)
    other = _args("3d")
    other.net = "multiunet"
    assert type(build_net(other, 1)) is type(get_net(other, 1))                   # every other net: get_net itself


@pytest.mark.parametrize("nd,shape", [(2, (1, 3, 34, 64)), (2, (1, 3, 32, 48)), (3, (1, 2, 32, 48, 32)), (3, (1, 2, 32, 32, 34)), (3, (1, 2, 32, 32))])
def test_shape_guard_raises_before_anything_is_launched(nd, shape):
    """Every spatial size must be divisible by 32.  The guard speaks first: on CPU tensors the first kernel call would raise DpiError instead."""
    m = PartialNet(nd, shape[1], 1)
    with pytest.raises(ValueError) as e:
        m(torch.zeros(shape), torch.zeros((1, 1) + tuple(shape[2:])))
    assert str(tuple(shape)) in str(e.value)
    with pytest.raises(TypeError):                                   # the reference's call, net(input_), says what is missing
        m(torch.zeros((1, shape[1]) + (32,) * nd))
    with pytest.raises(ValueError):                                  # a mask with one channel too many fits neither form
        m(torch.zeros((1, shape[1]) + (32,) * nd), torch.zeros((1, shape[1] + 1) + (32,) * nd))


def test_pconv_symbols_in_header_table_and_library():
    from deep_prior_interpolation_amd import _lib
    raw = open(os.path.join(ROOT, "include", "dpi_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = set(re.findall(r"\b(dpi_[a-z0-9_]+)\s*\(", txt))
    for name in PCONV_SYMBOLS:
        assert name in declared, name
        assert name in _lib.SIGNATURES, name
    assert [len(_lib.SIGNATURES[n][1]) for n in PCONV_SYMBOLS] == [9, 8, 8, 2, 11]
    assert raw.count("partial_unet.py:") >= 4                      # the declarations cite the reference lines they replace
    assert "partial_conv.hip" in open(os.path.join(ROOT, "deep_prior_interpolation_amd", "csrc", "Makefile")).read()
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    exported = set(re.findall(r"\bT (dpi_[a-z0-9_]+)", out))
    assert set(PCONV_SYMBOLS) <= exported, set(PCONV_SYMBOLS) - exported


def test_pconv_entry_points_validate_before_launching():
    """Argument checks of the C entry points (no device needed: a refused call launches nothing)."""
    from deep_prior_interpolation_amd import _lib
    L = _lib.load()
    assert L.dpi_pconv_norm_bwd_ws_floats(48, 1080) == 2 * 4 * 48                # 270 groups of 4 voxels: 2 blocks of 4 waves
    assert L.dpi_pconv_norm_bwd_ws_floats(48, 128 * 64 * 64) == 2048 * 48        # one row per 256 voxels
    assert L.dpi_pconv_norm_bwd_ws_floats(0, 10) == 0 and L.dpi_pconv_norm_bwd_ws_floats(3, 0) == 0
    assert L.dpi_pconv_norm_bwd_ws_floats(3, 1 << 31) == 0                       # beyond the kernels' 32-bit voxel indices
    a = 1 << 20                                                                  # any non-NULL, aligned address: never dereferenced by a refused call
    err = L.dpi_last_error
    assert L.dpi_pconv_mask_fwd(None, a, 3, 3, 10, a + 64, a + 128, None) == -1
    assert L.dpi_pconv_mask_fwd(a, a + 64, 3, 2, 10, a + 128, a + 256, None) == -1 and b"geometry" in err()        # Cm is Cin or 1
    assert L.dpi_pconv_mask_fwd(a, a + 64, 3, 3, 1 << 31, a + 128, a + 256, None) == -1 and b"geometry" in err()
    assert L.dpi_pconv_mask_fwd(a, a + 64, 3, 3, 10, a, a + 256, None) == -1 and b"in-place" in err()
    assert L.dpi_pconv_mask_fwd(a + 2, a + 64, 3, 3, 10, a + 128, a + 256, None) == -1 and b"aligned" in err()
    assert L.dpi_pconv_norm_fwd(a, a + 64, None, 3, 0, 2, 2, a, a + 128, a + 256, None) == -1 and b"geometry" in err()
    assert L.dpi_pconv_norm_fwd(a, None, None, 3, 1, 2, 2, a, a + 128, a + 256, None) == -1
    assert L.dpi_pconv_norm_fwd(a, a + 64, None, 3, 1, 2, 2, a, a + 64, a + 256, None) == -1 and b"alias" in err()  # new_mask on msum
    assert L.dpi_pconv_norm_fwd(a, a + 64, None, 3, 1 << 16, 1 << 16, 2, a, a + 128, a + 256, None) == -1
    assert L.dpi_pconv_norm_bwd(a, a + 64, 3, 10, a + 128, a + 256, None, None) == -1 and b"workspace" in err()
    assert L.dpi_pconv_norm_bwd(a, a + 64, 0, 10, a + 128, None, None, None) == -1 and b"geometry" in err()
    assert L.dpi_pconv_norm_bwd(a, a + 64, 3, 10, a + 64, None, None, None) == -1                                     # dc on S
    assert L.dpi_pconv_mask_bwd(a, None, a + 64, 3, 3, 10, a + 128, a + 256, None) == -1                              # dm needs x
    assert L.dpi_pconv_mask_bwd(a, a + 64, a + 128, 3, 1, 0, a + 256, None, None) == -1 and b"geometry" in err()
    assert L.dpi_pconv_mask_bwd(a, a + 64, a + 128, 3, 3, 10, a + 64, None, None) == -1 and b"alias" in err()        # dx on x
    assert L.dpi_pconv_mask_bwd(a + 1, a + 64, a + 128, 3, 3, 10, a + 256, None, None) == -1 and b"aligned" in err()


def test_no_cpu_fallback():
    from deep_prior_interpolation_amd import ops, _lib
    with pytest.raises(_lib.DpiError):
        ops.partial_conv(torch.zeros(1, 3, 4, 6), torch.ones(1, 1, 4, 6), torch.zeros(2, 3, 3, 3), None)
    with pytest.raises(_lib.DpiError):
        PartialUNet(3, 1)(torch.zeros(1, 3, 32, 32), torch.ones(1, 1, 32, 32))
