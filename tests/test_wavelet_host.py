"""--wavelet without a GPU: the flags and their refusals, the operator's constructor and taps, the Ricker helper, old checkpoints, the
re-assembly of the model sections, the float64 reference the GPU tests use, and the ABI table."""
import ctypes as C
import os
import subprocess
from argparse import Namespace

import numpy as np
import pytest
import torch

from conftest import ROOT

import wavelet_cases as W
from deep_prior_interpolation_amd import _lib, utils as u
from deep_prior_interpolation_amd.operators import ConvolutionalModelling
from deep_prior_interpolation_amd.parameter import net_args_are_same, parse_arguments

BASE = ["--imgdir", "x"]
WAV = ["--wavelet", "w.npy"]


# ---------------------------------------------------------------- flags -----------------------------------------------------------
def test_flags_parse():
    off = parse_arguments(BASE)
    assert off.wavelet is None and off.wavelet_model == "reflectivity"
    a = parse_arguments(BASE + WAV)
    assert a.wavelet == "w.npy" and a.wavelet_model == "reflectivity"
    a = parse_arguments(BASE + WAV + ["--wavelet_model", "impedance"])
    assert a.wavelet_model == "impedance"
    # time is dim 2 of the device tensor for all of these
    for extra in (["--datadim", "2d"], ["--datadim", "3d"], ["--datadim", "2.5d", "--slice", "tx", "--imgchannel", "3"],
                  ["--datadim", "2.5d", "--slice", "ty", "--imgchannel", "3"]):
        assert parse_arguments(BASE + WAV + extra).wavelet == "w.npy"
    # behind the AVO operator
    a = parse_arguments(BASE + WAV + ["--datadim", "2.5d", "--slice", "tx", "--imgchannel", "4", "--avo_theta", "0", "10", "20", "30"])
    assert a.wavelet == "w.npy" and a.avo_theta == [0.0, 10.0, 20.0, 30.0]


@pytest.mark.parametrize("argv, flag", [
    (BASE + ["--wavelet_model", "impedance"], "--wavelet_model"),                       # would silently do nothing
    (BASE + WAV + ["--datadim", "2.5d", "--slice", "xy", "--imgchannel", "3"], "--wavelet"),
    (BASE + WAV + ["--datadim", "2.5d", "--imgchannel", "3"], "--slice"),               # xy is the default slice
])
def test_flag_refusals(argv, flag):
    with pytest.raises(ValueError, match=flag):
        parse_arguments(argv)


def test_unknown_model_kind_is_refused():
    with pytest.raises(SystemExit):
        parse_arguments(BASE + WAV + ["--wavelet_model", "velocity"])
    a = parse_arguments(BASE + WAV)
    a.wavelet_model = "velocity"
    from deep_prior_interpolation_amd.parameter import check_wavelet
    with pytest.raises(ValueError, match="--wavelet_model"):
        check_wavelet(a)


def test_time_axis_is_dim_2_for_the_allowed_slices():
    """What the refusal of --slice xy rests on: data.transpose_patches_25d leaves t in front for tx and ty, and moves it to the end (the
    channel stack) for xy.  load_data then turns (T, A, channels) into (1, channels, T, A)."""
    from deep_prior_interpolation_amd.data import transpose_patches_25d
    p = np.zeros((2, 5, 6, 7))                                  # (patches, T, X, Y)
    assert transpose_patches_25d(p, "tx").shape == (2, 5, 6, 7)
    assert transpose_patches_25d(p, "ty").shape == (2, 5, 7, 6)
    assert transpose_patches_25d(p, "xy").shape == (2, 6, 7, 5)


def test_main_pocs_refuses_the_flag():
    from deep_prior_interpolation_amd.main_pocs import Interpolator
    with pytest.raises(ValueError, match="--wavelet"):
        Interpolator(parse_arguments(BASE + WAV), "/tmp", device="cpu")


def test_interpolator_names_the_flag_for_a_bad_file(tmp_path):
    from deep_prior_interpolation_amd.main import Interpolator
    np.save(tmp_path / "even.npy", np.ones(4))
    np.save(tmp_path / "good.npy", u.ricker(25.0, 0.004, 9))
    with pytest.raises(ValueError, match="--wavelet"):
        Interpolator(parse_arguments(["--imgdir", str(tmp_path), "--wavelet", "even.npy"]), "/tmp", device="cpu")
    with pytest.raises(ValueError, match="--wavelet"):
        Interpolator(parse_arguments(["--imgdir", str(tmp_path), "--wavelet", "missing.npy"]), "/tmp", device="cpu")
    T = Interpolator(parse_arguments(["--imgdir", str(tmp_path), "--wavelet", "good.npy", "--wavelet_model", "impedance"]), "/tmp",
                     device="cpu")
    assert T.forward_model.stage("wavelet").op.kind == "impedance" and T.forward_model.stage("wavelet").op.taps.size == 9 and T.wavelet_model() is None
    assert Interpolator(parse_arguments(["--imgdir", str(tmp_path)]), "/tmp", device="cpu").forward_model.stage("wavelet") is None


# ---------------------------------------------------------------- operator --------------------------------------------------------
@pytest.mark.parametrize("bad", [np.ones(4), np.ones(0), np.ones((3, 3)), np.array([1.0, np.nan, 0.5]), np.array([1.0, np.inf, 0.5]),
                                 np.zeros(5), np.ones(257), np.array(2.0)])
def test_operator_refuses_the_wavelet(bad):
    with pytest.raises(ValueError, match="wavelet"):
        ConvolutionalModelling(bad)


def test_operator_refuses_kind_and_batch():
    with pytest.raises(ValueError, match="kind"):
        ConvolutionalModelling(np.ones(3), kind="velocity")
    op = ConvolutionalModelling(np.ones(3))
    # refused from the shape alone, before the library is even looked up (these are host tensors)
    with pytest.raises(ValueError, match="batch"):
        op._matvec(torch.zeros(2, 1, 6, 5), False)
    with pytest.raises(ValueError, match="batch"):
        op._matvec(torch.zeros(3, 1, 6, 5, 2), True)
    with pytest.raises(ValueError):
        op._matvec(torch.zeros(1, 6, 5), False)
    with pytest.raises(_lib.DpiError):                           # no CPU path
        op.forward(torch.zeros(1, 1, 6, 5))
    assert ConvolutionalModelling(np.ones(255)).taps.size == 255


def test_taps_for_both_kinds():
    w = np.array([0.1, -0.7, 1.0 / 3.0, 0.25, 1e-3])
    r = ConvolutionalModelling(w)
    assert r.kind == "reflectivity" and r.diff == 0 and r.taps.dtype == np.float32 and np.array_equal(r.taps, w.astype(np.float32))
    i = ConvolutionalModelling(torch.from_numpy(w), kind="impedance")
    assert i.diff == 1 and i.taps.dtype == np.float32 and np.array_equal(i.taps, (w / 2).astype(np.float32))
    # the taps of VerticalConv(w): impedance = Chain([VerticalGrad(), VerticalConv(w)]), reflectivity = 2 VerticalConv(w)
    from deep_prior_interpolation_amd.operators import VerticalConv
    assert np.array_equal(i.taps, VerticalConv(w)._taps_fwd)


def test_ricker():
    w = u.ricker(25.0, 0.004, 65)
    assert w.shape == (65,) and w.dtype == np.float64
    assert np.array_equal(w, w[::-1]) and int(np.argmax(w)) == 32 and w[32] == 1.0
    assert abs(w.sum()) < 1e-6 and w.min() < -0.4                  # zero mean, side lobes of -2 exp(-3/2)
    # the first zero crossing sits at t = 1 / (pi f0 sqrt(2))
    t0 = 1.0 / (np.pi * 25.0 * np.sqrt(2.0)) / 0.004
    assert w[32 + int(np.floor(t0))] > 0 > w[32 + int(np.ceil(t0))]
    assert u.ricker(0.055, 1.0, 9, dtype=np.float32).dtype == np.float32
    for bad in (dict(K=8), dict(K=0), dict(f0=0.0), dict(dt=-1.0)):
        with pytest.raises(ValueError):
            u.ricker(**{**dict(f0=25.0, dt=0.004, K=9), **bad})
    ConvolutionalModelling(w)


# ---------------------------------------------------------------- the float64 reference -------------------------------------------
@pytest.mark.parametrize("diff", [0, 1])
def test_reference_is_the_formula_of_the_header_and_its_transpose(diff):
    C_, T, S, K = 2, 7, 3, 9                                     # T shorter than K: most taps fall outside
    c = W.case(C_, T, S, K, diff)
    m, d, taps = c["m"].astype(np.float64), c["d"].astype(np.float64), c["taps"].astype(np.float64)
    un = np.zeros_like(m)
    if diff:
        un[:, :, :-1] = m[:, :, 1:] - m[:, :, :-1]
    else:
        un = m
    fwd = np.zeros_like(m)
    for t in range(T):
        for k in range(K):
            q = t + K // 2 - k
            if 0 <= q < T:
                fwd[:, :, t] += taps[k] * un[:, :, q]
    np.testing.assert_allclose(c["fwd"], fwd, rtol=0, atol=1e-12)
    g = np.zeros_like(d)
    for t in range(T):
        for k in range(K):
            q = t - K // 2 + k
            if 0 <= q < T:
                g[:, :, t] += taps[k] * d[:, :, q]
    adj = g
    if diff:
        adj = np.zeros_like(g)
        for t in range(T):
            adj[:, :, t] = (-g[:, :, t] if t < T - 1 else 0.0) + (g[:, :, t - 1] if t >= 1 else 0.0)
    np.testing.assert_allclose(c["adj"], adj, rtol=0, atol=1e-12)
    # <A m, d> = <m, A^T d> in float64
    assert abs(np.vdot(c["fwd"], d) - np.vdot(m, c["adj"])) <= 1e-12 * np.abs(c["fwd"]).sum()
    assert np.all(c["fwd_bound"] >= 0) and np.all(c["adj_bound"] >= 0) and c["fwd_bound"].max() < 1e-4


def test_cases_cover_what_the_issue_names():
    assert len(W.CASES) == 21 and (1, 130, 64, 255) in W.CASES
    assert {c[:3] for c in W.CASES[:20]} == {(1, 5, 1), (2, 7, 3), (1, 33, 65), (3, 130, 70), (1, 257, 129)}
    assert {c[3] for c in W.CASES[:20]} == {1, 3, 9, 65}


# ---------------------------------------------------------------- checkpoints -----------------------------------------------------
def test_net_args_are_same():
    now = parse_arguments(BASE)
    saved = Namespace(**{k: v for k, v in vars(parse_arguments(BASE)).items() if not k.startswith("wavelet")})
    assert not hasattr(saved, "wavelet") and not hasattr(saved, "wavelet_model")
    assert net_args_are_same(now, saved) and net_args_are_same(saved, now)            # an old args.txt reads as off
    on = parse_arguments(BASE + WAV)
    assert net_args_are_same(on, parse_arguments(BASE + WAV))
    assert not net_args_are_same(on, saved) and not net_args_are_same(on, now)
    assert not net_args_are_same(on, parse_arguments(BASE + ["--wavelet", "other.npy"]))
    assert not net_args_are_same(on, parse_arguments(BASE + WAV + ["--wavelet_model", "impedance"]))


# ---------------------------------------------------------------- re-assembly -----------------------------------------------------
@pytest.mark.parametrize("reassembly, vol_shape, out_shape", [("crop", (20, 14), (20, 14)), ("crop", (21, 15), (20, 14)),
                                                              ("cover", (21, 15), (21, 15))])
@pytest.mark.parametrize("blend", ["flat", "taper"])
def test_reassembly_returns_a_constant_model_exactly(tmp_path, reassembly, vol_shape, out_shape, blend):
    from deep_prior_interpolation_amd.data import reconstruct_patches
    np.save(tmp_path / "vol.npy", np.zeros(vol_shape, dtype=np.float32))
    a = Namespace(imgdir=str(tmp_path), imgname="vol.npy", outdir="run", datadim="2d", slice="xy", imgchannel=None, gain=2.0,
                  patch_shape=[8, 8], patch_stride=[4, 6], reassembly=reassembly, blend=blend)
    origins = u.window_origins(vol_shape, (8, 8), (4, 6), cover=reassembly == "cover")
    assert len(origins) == (15 if reassembly == "cover" else 8)
    os.makedirs(tmp_path / "run")
    model = np.full((8, 8, 1), 1.5 * a.gain, dtype=np.float32)
    for i in range(len(origins)):
        np.save(tmp_path / "run" / ("%02d_run.npy" % i), {"output": np.zeros((8, 8, 1), dtype=np.float32), "history": None,
                                                         "wavelet": np.ones(3, np.float32), "wavelet_model": model})
    rec = reconstruct_patches(a, results_root=str(tmp_path), field="wavelet_model")
    assert rec.shape == out_shape and np.array_equal(rec, np.full(out_shape, 1.5))
    # a skipped patch (wavelet_model None) counts as zeros in its window; files of a run without --wavelet are refused
    np.save(tmp_path / "run" / "00_run.npy", {"output": np.zeros((8, 8, 1), dtype=np.float32), "history": None,
                                              "wavelet": np.ones(3, np.float32), "wavelet_model": None})
    rec = reconstruct_patches(a, results_root=str(tmp_path), field="wavelet_model")
    assert rec[0, 0] == 0.0 and rec[-1, -1] == 1.5
    np.save(tmp_path / "run" / "00_run.npy", {"output": np.zeros((8, 8, 1), dtype=np.float32), "history": None})
    with pytest.raises(ValueError, match="wavelet"):
        reconstruct_patches(a, results_root=str(tmp_path), field="wavelet_model")
    with pytest.raises(ValueError, match="field"):
        reconstruct_patches(a, results_root=str(tmp_path), field="wavelet")


# ---------------------------------------------------------------- ABI -------------------------------------------------------------
def test_abi_table_header_exports_and_makefile_name_the_entry_points():
    assert _lib.ABI_VERSION == 406
    I, P, Z = C.c_int, C.c_void_p, C.c_size_t
    for name in ("dpi_wavelet_fwd", "dpi_wavelet_adj"):
        assert _lib.SIGNATURES[name] == (I, [P, P, I, I, I, I, Z, P, P])
    h = open(os.path.join(ROOT, "include", "dpi_hip.h")).read()
    assert "int dpi_wavelet_fwd(const float* m, const float* taps, int K, int diff, int C, int T, size_t S, float* d, void* stream);" in h
    assert "int dpi_wavelet_adj(const float* d, const float* taps, int K, int diff, int C, int T, size_t S, float* m, void* stream);" in h
    assert "operators/signal.py:8-45" in h and "operators/derivative.py:8-21" in h
    assert "wavelet.hip" in open(os.path.join(ROOT, "deep_prior_interpolation_amd", "csrc", "Makefile")).read()
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    exported = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    for name in ("dpi_wavelet_fwd", "dpi_wavelet_adj"):
        assert (" T " + name + "\n") in exported
    assert _lib.load().dpi_version() == 406
