"""CPU-side tests of --net attmultiunet: state_dict parity with the reference's AttMulResUnet2D, same-seed initial values, the routing
of get_net, the shape guard and the C-ABI bookkeeping of the gate kernels.  No GPU needed."""
import os
import re
import subprocess
from argparse import Namespace

import numpy as np
import pytest
import torch

from conftest import ROOT, jstr

from deep_prior_interpolation_amd import utils as u
from deep_prior_interpolation_amd.architectures import get_net
from deep_prior_interpolation_amd.architectures.attention import AttMulResUnet, AttMulResUnet2D, AttMulResUnet3D, GridAttentionBlock
from deep_prior_interpolation_amd.parameter import parse_arguments

GATE_SYMBOLS = ["dpi_attn_gate_bwd", "dpi_attn_gate_bwd_ws_floats", "dpi_attn_gate_fwd"]


@pytest.mark.parametrize("mode", ["bilinear", "nearest"])
def test_state_dict_keys_match_the_reference(golden, mode):
    g = golden("attention")["net2d_" + mode]
    m = AttMulResUnet2D(num_input_channels=6, num_output_channels=2, num_channels_down=[4, 4, 8, 8, 8], upsample_mode=mode)
    assert [[k, list(v.shape)] for k, v in m.state_dict().items()] == jstr(g["keys"])          # same names, shapes AND order
    assert list(m.state_dict().keys()) == list(g["init_state"].keys())


def test_class_same_seed_init_is_bit_identical(golden):
    g = golden("attention")["net2d_bilinear"]
    u.set_seed(0)
    m = AttMulResUnet2D(num_input_channels=6, num_output_channels=2, num_channels_down=[4, 4, 8, 8, 8], upsample_mode="bilinear")
    u.init_weights(m, "xavier", 0.02)
    for k, v in m.state_dict().items():
        assert np.array_equal(v.numpy(), g["init_state"][k]), k
    u.set_seed(0)
    b = GridAttentionBlock(2, 6, 5, 4)
    u.init_weights(b, "xavier", 0.02)
    st = golden("attention")["gate2d"]["state"]
    assert list(b.state_dict().keys()) == list(st.keys())
    for k, v in b.state_dict().items():
        assert np.array_equal(v.numpy(), st[k]), k


def test_factory_same_seed_init_is_bit_identical(golden):
    """set_seed(0) + get_net + init_weights reproduces the initial state_dict of the reference's Interpolator (2.5-D fixture)."""
    g = golden("net_attmultiunet25d_tiny")
    ns = Namespace(**jstr(g["args"]))
    assert ns.datadim == "2.5d" and ns.net == "attmultiunet"
    u.set_seed(0)
    net = get_net(ns, g["image"].shape[-1] if ns.imgchannel is None else ns.imgchannel)
    u.init_weights(net, ns.inittype, ns.initgain)
    sd = net.state_dict()
    assert list(sd.keys()) == list(g["init_state"].keys())
    for k, v in g["init_state"].items():
        assert np.array_equal(sd[k].numpy(), v), k
    assert sum(p.numel() for p in net.parameters()) == int(g["num_params"])


def _args(datadim, extra=()):
    return parse_arguments(["--imgdir", "x", "--datadim", datadim, "--net", "attmultiunet", "--filters", "4", "8", "8", "--inputdepth", "4"] + list(extra))


def test_routing():
    n3 = get_net(_args("3d"), 1)
    assert isinstance(n3, AttMulResUnet) and n3.nd == 3 and n3.n_scales == 3
    assert type(n3.down1[1]).__name__ == "BatchNorm3d" and n3.att1.psi[2].mode == "trilinear"
    ref3 = AttMulResUnet3D(4, 1, [4, 8, 8])
    assert [(k, tuple(v.shape)) for k, v in n3.state_dict().items()] == [(k, tuple(v.shape)) for k, v in ref3.state_dict().items()]
    n25 = get_net(_args("2.5d", ["--imgchannel", "3"]), 3)
    assert isinstance(n25, AttMulResUnet) and n25.nd == 2
    assert type(n25.down1[1]).__name__ == "BatchNorm2d" and n25.att1.psi[2].mode == "bilinear"
    assert n25.outconv[0].weight.shape == (3, n25.down_mb1.out_dim, 1, 1)
    with pytest.raises(NotImplementedError) as e:                 # the 2d route of the factory is held (tests/test_host.py), on purpose and saying so
        get_net(_args("2d"), 1)
    assert "2.5d" in str(e.value) and "AttMulResUnet2D" in str(e.value)
    with pytest.raises(NotImplementedError):
        get_net(parse_arguments(["--imgdir", "x", "--datadim", "3d", "--net", "part"]), 1)


def test_gate_is_always_linear_and_last_activation_is_placed_like_the_reference():
    m = AttMulResUnet2D(3, 2, [4, 4], upsample_mode="nearest", last_act_fun="Sigmoid")
    assert m.up1.mode == "nearest" and m.att1.psi[2].mode == "bilinear"
    assert [k for k in m.state_dict() if k.startswith("outconv")] == ["outconv.0.0.weight", "outconv.0.0.bias"]
    m = AttMulResUnet2D(3, 2, [4, 4], last_act_fun="none")
    assert [k for k in m.state_dict() if k.startswith("outconv")] == ["outconv.0.weight", "outconv.0.bias"]
    with pytest.raises(ValueError):
        AttMulResUnet2D(3, 2, [4])


@pytest.mark.parametrize("nd,filters,shape", [(2, [4, 4, 8, 8, 8], (1, 6, 32, 40)), (2, [4, 4], (1, 6, 7, 8)), (3, [4, 8, 8], (1, 4, 16, 16, 18)),
                                              (3, [4, 8, 8], (1, 4, 16, 16))])
def test_shape_guard_raises_before_anything_is_launched(nd, filters, shape):
    """Every spatial size must be divisible by 2**(n-1); 32 x 40 with five scales is the reference's own shape error (5 against 6 in the gate).
    The guard speaks first: on CPU tensors the first kernel call would raise DpiError instead."""
    m = AttMulResUnet(nd, shape[1], 1, filters)
    with pytest.raises(ValueError) as e:
        m(torch.zeros(shape))
    assert str(tuple(shape)) in str(e.value)


def test_gate_symbols_in_header_table_and_library():
    from deep_prior_interpolation_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dpi_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(dpi_[a-z0-9_]+)\s*\(", txt))
    for name in GATE_SYMBOLS:
        assert name in declared, name
        assert name in _lib.SIGNATURES, name
    assert len(_lib.SIGNATURES["dpi_attn_gate_fwd"][1]) == 10 and len(_lib.SIGNATURES["dpi_attn_gate_bwd"][1]) == 12
    assert len(_lib.SIGNATURES["dpi_attn_gate_bwd_ws_floats"][1]) == 5
    assert _lib.ABI_VERSION == 406              # unchanged: a stale library fails on the unresolved symbols instead
    # the declarations cite the reference call they replace
    raw = open(os.path.join(ROOT, "include", "dpi_hip.h")).read()
    assert raw.count("attention.py:107-113") >= 2
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    exported = set(re.findall(r"\bT (dpi_[a-z0-9_]+)", out))
    assert set(GATE_SYMBOLS) <= exported, set(GATE_SYMBOLS) - exported


def test_gate_entry_points_validate_before_launching():
    """Argument checks of the C entry points (no device needed: a refused call launches nothing)."""
    from deep_prior_interpolation_amd import _lib
    L = _lib.load()
    assert L.dpi_attn_gate_bwd_ws_floats(25, 128, 64, 64, 1) == 256 * 128 * 128
    assert L.dpi_attn_gate_bwd_ws_floats(3, 1, 3, 5, 0) == 6 * 10
    assert L.dpi_attn_gate_bwd_ws_floats(0, 1, 3, 5, 0) == 0 and L.dpi_attn_gate_bwd_ws_floats(3, 1, 3, 5, 2) == 0
    assert L.dpi_attn_gate_bwd_ws_floats(1, 1024, 1024, 1024, 1) == 0          # 2^33 fine voxels: beyond the kernels' 32-bit indices
    a = 1 << 20                                                                  # any non-NULL, aligned address: never dereferenced by a refused call
    assert L.dpi_attn_gate_fwd(None, a, 3, 1, 3, 5, 0, a + 64, a + 128, None) == -1
    assert L.dpi_attn_gate_fwd(a, a + 64, 0, 1, 3, 5, 0, a + 128, a + 256, None) == -1
    assert L.dpi_attn_gate_fwd(a + 2, a + 64, 3, 1, 3, 5, 0, a + 128, a + 256, None) == -1 and b"aligned" in L.dpi_last_error()
    assert L.dpi_attn_gate_bwd(a, a + 64, a + 128, 3, 1, 3, 5, 0, a + 256, a + 512, None, None) == -1
    assert L.dpi_attn_gate_bwd(a, a + 64, a + 128, 3, 0, 3, 5, 0, a + 256, a + 512, a + 1024, None) == -1 and b"geometry" in L.dpi_last_error()


def test_no_cpu_fallback():
    from deep_prior_interpolation_amd import ops, _lib
    with pytest.raises(_lib.DpiError):
        ops.attention_gate(torch.zeros(1, 3, 4, 6), torch.zeros(1, 1, 2, 3), torch.zeros(1, 2, 2, 3), "nearest")
    with pytest.raises(_lib.DpiError):
        AttMulResUnet2D(3, 1, [4, 4])(torch.zeros(1, 3, 8, 8))
