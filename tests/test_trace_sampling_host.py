"""--trace_offsets without a GPU: the float64 restatement of the sampling operator checked against itself, the flag and its refusals, the
offset windows of extract_patches, the off-grid stand-in, checkpoints and the ABI table."""
import ctypes as C
import os
import subprocess
from argparse import Namespace

import numpy as np
import pytest
import torch

from conftest import ROOT
from trace_sampling_cases import OFFSET_KINDS, SHAPE_IDS, SHAPES, adjoint64, axis_taps, forward64, offsets_for, trace_taps

from deep_prior_interpolation_amd import _lib, utils as u
from deep_prior_interpolation_amd.data import extract_patches
from deep_prior_interpolation_amd.operators import TraceSampling
from deep_prior_interpolation_amd.parameter import net_args_are_same, parse_arguments

HOST_SHAPES = [s for s in SHAPES if s[1] < 1000]          # the long-t case says nothing new about the restatement
HOST_IDS = [i for s, i in zip(SHAPES, SHAPE_IDS) if s[1] < 1000]


# ---------------------------------------------------------------- the float64 restatement -----------------------------------------
@pytest.mark.parametrize("shape", HOST_SHAPES, ids=HOST_IDS)
@pytest.mark.parametrize("kind", OFFSET_KINDS)
def test_weights_sum_to_one_for_every_trace(shape, kind):
    _, _, X, Y = shape
    off = offsets_for(kind, X, Y)
    taps = trace_taps(off)
    total = sum(w for _, _, w in taps)
    assert total.shape == (X, Y) and np.abs(total - 1.0).max() <= 4e-16
    for tx, ty, w in taps:
        assert tx.min() >= 0 and tx.max() <= X - 1 and ty.min() >= 0 and ty.max() <= Y - 1 and w.min() >= 0.0
    np.testing.assert_allclose(forward64(np.ones(shape), off), 1.0, rtol=0, atol=4e-16)      # clamped edges included


def test_clamped_taps_both_count():
    i0, i1, w0, w1 = axis_taps(np.arange(3), np.float32([-0.5, 0.25, 0.5]), 3)
    assert i0.tolist() == [0, 1, 2] and i1.tolist() == [0, 2, 2]                 # trace 0 reaches left, trace 2 right: both clamp
    assert w0.tolist() == [0.5, 0.75, 0.5] and w1.tolist() == [0.5, 0.25, 0.5]
    y = forward64(np.arange(3.0).reshape(1, 1, 3, 1), np.stack([np.float32([-0.5, 0.25, 0.5]).reshape(3, 1), np.zeros((3, 1), np.float32)]))
    assert y.reshape(-1).tolist() == [0.0, 1.25, 2.0]


@pytest.mark.parametrize("shape", HOST_SHAPES, ids=HOST_IDS)
@pytest.mark.parametrize("kind", OFFSET_KINDS)
def test_restatement_passes_its_own_dot_test(shape, kind):
    rng = np.random.RandomState(1)
    off = offsets_for(kind, shape[2], shape[3], seed=2)
    d, r = rng.standard_normal(shape), rng.standard_normal(shape)
    lhs, rhs = np.vdot(forward64(d, off), r), np.vdot(d, adjoint64(r, off))
    assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), np.linalg.norm(d) * np.linalg.norm(r))


@pytest.mark.parametrize("shape", HOST_SHAPES, ids=HOST_IDS)
def test_zero_offsets_give_the_identity(shape):
    x = np.random.RandomState(3).standard_normal(shape)
    off = offsets_for("zero", shape[2], shape[3])
    assert np.array_equal(forward64(x, off), x) and np.array_equal(adjoint64(x, off), x)


# ---------------------------------------------------------------- the operator's refusals -----------------------------------------
def test_operator_refusals():
    op = TraceSampling(offsets_for("random", 5, 7))
    assert op.offsets.dtype == torch.float32 and tuple(op.offsets.shape) == (2, 5, 7)
    # refused from the shapes alone, before the library is even looked up (these are host tensors)
    with pytest.raises(ValueError, match="5 x 7"):
        op._matvec(torch.zeros(1, 2, 3, 7, 5), False)
    with pytest.raises(ValueError, match="5 x 7"):
        op._matvec(torch.zeros(1, 2, 3, 5), True)                       # a 4-D tensor is Y = 1
    with pytest.raises(ValueError, match="batch"):
        op._matvec(torch.zeros(2, 2, 3, 5, 7), False)
    bad = offsets_for("random", 5, 7)
    bad[1, 2, 3] = np.nan
    with pytest.raises(ValueError, match="non-finite"):
        TraceSampling(bad)
    bad[1, 2, 3] = np.inf
    with pytest.raises(ValueError, match="non-finite"):
        TraceSampling(bad)
    bad[1, 2, 3] = 0.50001
    with pytest.raises(ValueError, match=r"\[-0.5, 0.5\]"):
        TraceSampling(bad)
    with pytest.raises(ValueError, match="shape"):
        TraceSampling(np.zeros((5, 7, 2), dtype=np.float32))
    with pytest.raises(_lib.DpiError):                                 # no CPU path
        op.forward(torch.zeros(1, 2, 3, 5, 7))
    assert tuple(TraceSampling(np.zeros((2, 9, 1))).offsets.shape) == (2, 9, 1)


# ---------------------------------------------------------------- flags -----------------------------------------------------------
BASE3 = ["--imgdir", "x", "--datadim", "3d"]
FLAG = ["--trace_offsets", "off.npy"]


def test_flag_parses():
    assert parse_arguments(BASE3).trace_offsets is None
    assert parse_arguments(BASE3 + FLAG).trace_offsets == "off.npy"
    assert parse_arguments(["--imgdir", "x", "--datadim", "2d"] + FLAG).trace_offsets == "off.npy"
    assert parse_arguments(BASE3 + FLAG + ["--holdout", "0.2"]).holdout == 0.2            # composes


@pytest.mark.parametrize("argv", [
    ["--imgdir", "x", "--datadim", "2.5d", "--imgchannel", "3"] + FLAG,
    ["--imgdir", "x", "--datadim", "2.5d", "--slice", "tx", "--imgchannel", "5", "--avo_theta", "0", "10", "20", "30", "40"] + FLAG,
    BASE3 + FLAG + ["--out_ema", "0.9"],
    BASE3 + FLAG + ["--optimizer", "sgld"],
    BASE3 + FLAG + ["--optimizer", "psgld"],
], ids=["2.5d", "avo_theta", "out_ema", "sgld", "psgld"])
def test_flag_refusals(argv):
    with pytest.raises(ValueError, match="--trace_offsets"):
        parse_arguments(argv)


def test_main_pocs_refuses_the_flag():
    from deep_prior_interpolation_amd.main_pocs import Interpolator
    with pytest.raises(ValueError, match="--trace_offsets"):
        Interpolator(parse_arguments(BASE3 + FLAG), "/tmp", device="cpu")


def test_checkpoints():
    now = parse_arguments(BASE3)
    saved = Namespace(**{k: v for k, v in vars(parse_arguments(BASE3)).items() if k != "trace_offsets"})
    assert not hasattr(saved, "trace_offsets")
    assert net_args_are_same(now, saved) and net_args_are_same(saved, now)           # an args.txt without the key: off
    with_flag = parse_arguments(BASE3 + FLAG)
    assert not net_args_are_same(with_flag, saved) and not net_args_are_same(with_flag, now)
    assert net_args_are_same(with_flag, parse_arguments(BASE3 + FLAG))
    assert not net_args_are_same(with_flag, parse_arguments(BASE3 + ["--trace_offsets", "other.npy"]))


# ---------------------------------------------------------------- extract_patches -------------------------------------------------
def _volume(tmp_path, shape, off, seed=0):
    rng = np.random.RandomState(seed)
    np.save(tmp_path / "vol.npy", rng.standard_normal(shape).astype(np.float32))
    np.save(tmp_path / "mask.npy", u.random_trace_mask(shape, 0.5, seed=seed + 1).astype(np.float32))
    np.save(tmp_path / "off.npy", off)


def _args(tmp_path, datadim, extra=()):
    return parse_arguments(["--imgdir", str(tmp_path), "--imgname", "vol.npy", "--maskname", "mask.npy", "--datadim", datadim,
                            "--trace_offsets", "off.npy"] + list(extra))


@pytest.mark.parametrize("reassembly, npatches", [("crop", 8), ("cover", 27)])
def test_offset_windows_line_up_with_the_mask_windows(tmp_path, reassembly, npatches):
    """The offsets are made a function of the mask and of the position, offset = (mask ? +1 : -1) * (x * 19 + y + 1) / 1000 in dx and half of
    it in dy: a window cut at another origin than its mask window cannot reproduce it."""
    shape = (13, 12, 11)                                  # cover adds an edge-flush window on every axis
    mask = u.random_trace_mask(shape, 0.5, seed=1)
    pos = (np.arange(12)[:, None] * 19 + np.arange(11)[None, :] + 1) / 1000.0
    sign = np.where(mask[0] > 0, 1.0, -1.0)
    off = np.stack([sign * pos, 0.5 * sign * pos], axis=-1).astype(np.float32)
    _volume(tmp_path, shape, off)
    a = _args(tmp_path, "3d", ["--patch_shape", "8", "8", "8", "--patch_stride", "4", "3", "2", "--reassembly", reassembly])
    patches = extract_patches(a)
    origins = u.window_origins(shape, (8, 8, 8), (4, 3, 2), cover=reassembly == "cover")
    assert len(patches) == npatches == len(origins)
    for p, org in zip(patches, origins):
        o = p["offsets"]
        assert o.shape == (8, 8, 2) and o.dtype == np.float32 and p["mask"].shape == (8, 8, 8, 1)
        known = p["mask"][0, :, :, 0] > 0
        assert np.array_equal(o[..., 0] > 0, known)                           # lines up with the mask window
        assert np.array_equal(o, off[org[1]:org[1] + 8, org[2]:org[2] + 8])     # and sits at the window's origin
    assert "offsets" not in extract_patches(parse_arguments(["--imgdir", str(tmp_path), "--imgname", "vol.npy", "--maskname", "mask.npy",
                                                             "--datadim", "3d", "--patch_shape", "8", "8", "8"]))[0]


@pytest.mark.parametrize("file_shape", [(11,), (11, 1)])
def test_offset_windows_of_a_section(tmp_path, file_shape):
    shape = (13, 11)
    off = (np.arange(11) / 40.0 - 0.1).astype(np.float32).reshape(file_shape)
    _volume(tmp_path, shape, off)
    patches = extract_patches(_args(tmp_path, "2d", ["--patch_shape", "8", "4", "--patch_stride", "4", "3", "--reassembly", "cover"]))
    origins = u.window_origins(shape, (8, 4), (4, 3), cover=True)
    assert len(patches) == len(origins) == 12
    for p, org in zip(patches, origins):
        assert p["offsets"].shape == (4, 1, 2) and p["image"].shape == (8, 4, 1)
        assert np.array_equal(p["offsets"][:, 0, 0], off.reshape(-1)[org[1]:org[1] + 4]) and np.all(p["offsets"][..., 1] == 0)


def test_extract_patches_refusals(tmp_path):
    shape = (13, 11, 10)
    good = np.zeros((11, 10, 2), dtype=np.float32)
    for bad in (np.zeros((10, 11, 2), np.float32), np.zeros((11, 10), np.float32), np.zeros((2, 11, 10), np.float32), np.zeros(11, np.float32)):
        _volume(tmp_path, shape, bad)
        with pytest.raises(ValueError, match="--trace_offsets"):
            extract_patches(_args(tmp_path, "3d"))
    for value in (0.51, -0.75, np.nan, np.inf):
        bad = good.copy()
        bad[3, 4, 1] = value
        _volume(tmp_path, shape, bad)
        with pytest.raises(ValueError, match="--trace_offsets"):
            extract_patches(_args(tmp_path, "3d"))
    # a 2d run on a 3-D file: the last axis becomes channels
    _volume(tmp_path, shape, good)
    with pytest.raises(ValueError, match="--trace_offsets"):
        extract_patches(_args(tmp_path, "2d"))
    _volume(tmp_path, (13, 11), np.zeros(10, np.float32))
    with pytest.raises(ValueError, match="--trace_offsets"):
        extract_patches(_args(tmp_path, "2d"))
    _volume(tmp_path, shape, good)
    assert len(extract_patches(_args(tmp_path, "3d"))) == 1


# ---------------------------------------------------------------- the stand-in ----------------------------------------------------
@pytest.mark.parametrize("shape", [(48, 32, 32), (24, 7, 5)])
def test_hyperbolic_traces_at_zero_offsets_is_the_volume(shape):
    for seed in (0, 3):
        vol = u.hyperbolic_volume(shape, seed, background=0)
        tr = u.hyperbolic_traces(shape, np.zeros(shape[1:] + (2,), dtype=np.float32), seed)
        assert tr.dtype == vol.dtype and np.array_equal(tr, vol)


def test_hyperbolic_traces_off_the_grid():
    shape = (48, 16, 16)
    off = np.random.RandomState(0).uniform(-0.5, 0.5, (16, 16, 2)).astype(np.float32)
    vol, tr = u.hyperbolic_volume(shape, 1, background=0), u.hyperbolic_traces(shape, off, 1)
    assert tr.shape == vol.shape and not np.array_equal(tr, vol) and np.isfinite(tr).all()
    off[3, 4] = 0.0                                      # a trace that sits on its node is the volume's
    assert np.array_equal(u.hyperbolic_traces(shape, off, 1)[:, 3, 4], vol[:, 3, 4])
    with pytest.raises(ValueError, match="offsets"):
        u.hyperbolic_traces(shape, off[:8], 1)


# ---------------------------------------------------------------- ABI -------------------------------------------------------------
def test_abi_table_header_exports_and_makefile_name_the_entry_points():
    assert _lib.ABI_VERSION == 406
    h = open(os.path.join(ROOT, "include", "dpi_hip.h")).read()
    assert "int dpi_trace_sample_fwd(const float* x, const float* off, int C, int T, int X, int Y, float* y, void* stream);" in h
    assert "int dpi_trace_sample_adj(const float* y, const float* off, int C, int T, int X, int Y, float* x, void* stream);" in h
    for name in ("dpi_trace_sample_fwd", "dpi_trace_sample_adj"):
        res, args = _lib.SIGNATURES[name]
        assert res is C.c_int and args == [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    assert "trace_sample.hip" in open(os.path.join(ROOT, "deep_prior_interpolation_amd", "csrc", "Makefile")).read()
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    exported = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    for name in ("dpi_trace_sample_fwd", "dpi_trace_sample_adj"):
        assert (" T " + name + "\n") in exported
    assert _lib.load().dpi_version() == 406
