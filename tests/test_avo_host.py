"""--avo_theta without a GPU: the host-built coefficients against the reference's recorded ones (tests/golden/avo.npz, recorded by
tools/record_avo_golden.py), the flags and their refusals, the float64 pseudo-inverse that recovers the parameter sections, their
re-assembly, old checkpoints and the ABI table."""
import os
from argparse import Namespace

import numpy as np
import pytest
import torch

from conftest import ROOT

from deep_prior_interpolation_amd import _lib, utils as u
from deep_prior_interpolation_amd.operators import AVOLinearModelling, avo_coefficients, avo_model_from_data
from deep_prior_interpolation_amd.parameter import net_args_are_same, parse_arguments

BASE = ["--imgdir", "x", "--datadim", "2.5d", "--slice", "tx", "--imgchannel", "5"]
THETA = ["--avo_theta", "0", "10", "20", "30", "40"]
U24 = 2.0 ** -24


def _cases(g, kind):
    return [g[kind][k] for k in sorted(g[kind])]


def _operator(c, spatdims=None):
    vsvp = c["vsvp"]
    vsvp = float(vsvp[0]) if vsvp.size == 1 else torch.from_numpy(vsvp)
    return AVOLinearModelling(c["theta"].tolist(), vsvp=vsvp, nt0=int(c["nt0"]), spatdims=spatdims, linearization=str(c["lin"]))


# ---------------------------------------------------------------- coefficients ----------------------------------------------------
def test_fixture_holds_the_cases_and_its_own_measurements(golden):
    g = golden("avo")
    coef, vec = _cases(g, "coef"), _cases(g, "vec")
    assert len(coef) == 32 and len(vec) == 16
    assert {tuple(c["theta"].tolist()) for c in coef} == {(0, 10, 20, 30, 40), (5, 15, 25), tuple(range(0, 50, 7)), (0, 60, 75)}
    assert {str(c["lin"]) for c in coef} == {"akirich", "fatti"} and {int(c["nt0"]) for c in coef} == {37, 8}
    assert {c["vsvp"].size for c in coef} == {1, 37, 8}
    assert {v["x"].shape[2:] for v in vec} == {(37, 19), (8, 7, 9)}
    # what the recorder measured: the reference's fp32 G sits a few fp32 roundings from the float64 formula, cond(G_t) is moderate
    assert 0.0 < float(g["gap_max"]) < 1e-6 and 1.0 < float(g["cond_min"]) < float(g["cond_max"]) < 1e3


def test_host_coefficients_match_the_reference(golden):
    g = golden("avo")
    gap = float(g["gap_max"])
    for c in _cases(g, "coef"):
        op = _operator(c, spatdims=(19,))
        ref = c["G"]
        assert op.G.dtype == torch.float32 and tuple(op.G.shape) == ref.shape + (1,)          # the reference's shape (ntheta, 3, nt0, 1)
        err = np.abs(op.G.numpy()[..., 0].astype(np.float64) - ref.astype(np.float64)).max()
        assert err <= 4.0 * gap * np.abs(ref).max(), (c["theta"], str(c["lin"]), err)
        assert op.G64.dtype == np.float64 and np.array_equal(op.G64.astype(np.float32), op.G.numpy()[..., 0])    # rounded once
    assert tuple(_operator(_cases(g, "coef")[0], spatdims=(7, 9)).G.shape)[3:] == (1, 1)


def test_operator_refusals():
    with pytest.raises(ValueError, match="linearization"):
        AVOLinearModelling([0, 10, 20], linearization="shuey")
    for bad in ([0, 10, 90], [-95, 0, 10]):
        with pytest.raises(ValueError, match="theta"):
            AVOLinearModelling(bad)
    with pytest.raises(ValueError, match="vsvp"):
        avo_coefficients([0, 10, 20], np.linspace(0.4, 0.6, 5), 7)
    op = AVOLinearModelling([0, 10, 20, 30], nt0=6, spatdims=(5,))
    # refused from the shapes alone, before the library is even looked up (these are host tensors)
    with pytest.raises(_lib.DpiError, match="batch"):
        op._matvec(torch.zeros(2, 3, 6, 5), False)
    with pytest.raises(_lib.DpiError, match="nt0"):
        op._matvec(torch.zeros(1, 3, 7, 5), False)
    with pytest.raises(_lib.DpiError, match="channels"):
        op._matvec(torch.zeros(1, 3, 6, 5), True)
    with pytest.raises(_lib.DpiError, match="spatial"):
        op._matvec(torch.zeros(1, 3, 6, 5, 2), False)
    with pytest.raises(_lib.DpiError):                       # no CPU path
        op.forward(torch.zeros(1, 3, 6, 5))


# ---------------------------------------------------------------- flags -----------------------------------------------------------
def test_flags_parse():
    a = parse_arguments(BASE + THETA)
    assert a.avo_theta == [0.0, 10.0, 20.0, 30.0, 40.0] and a.avo_vsvp == 0.5 and a.avo_linearization == "akirich"
    a = parse_arguments(BASE + THETA + ["--avo_vsvp", "0.45", "--avo_linearization", "fatti"])
    assert a.avo_vsvp == 0.45 and a.avo_linearization == "fatti"
    off = parse_arguments(BASE)
    assert off.avo_theta is None


@pytest.mark.parametrize("argv, flag", [
    (["--imgdir", "x", "--datadim", "3d", "--imgchannel", "5"] + THETA, "--datadim"),
    (["--imgdir", "x", "--datadim", "2.5d", "--slice", "xy", "--imgchannel", "5"] + THETA, "--slice"),
    (["--imgdir", "x", "--datadim", "2.5d", "--slice", "tx", "--imgchannel", "4"] + THETA, "--imgchannel"),
    (["--imgdir", "x", "--datadim", "2.5d", "--slice", "tx"] + THETA, "--imgchannel"),
    (["--imgdir", "x", "--datadim", "2.5d", "--slice", "tx", "--imgchannel", "3", "--avo_theta", "10", "10", "20"], "--avo_theta"),
    (["--imgdir", "x", "--datadim", "2.5d", "--slice", "tx", "--imgchannel", "2", "--avo_theta", "10", "20"], "--avo_theta"),
    (BASE + THETA + ["--avo_vsvp", "0"], "--avo_vsvp"),
    (BASE + THETA + ["--avo_vsvp", "-0.5"], "--avo_vsvp"),
    # distinct angles, equal sin^2: two columns' worth of information only
    (["--imgdir", "x", "--datadim", "2.5d", "--slice", "tx", "--imgchannel", "3", "--avo_theta", "-10", "10", "20"], "--avo_theta"),
    (["--imgdir", "x", "--datadim", "2.5d", "--slice", "tx", "--imgchannel", "3", "--avo_theta", "0", "45", "90"], "--avo_theta"),
])
def test_flag_refusals(argv, flag):
    with pytest.raises(ValueError, match=flag):
        parse_arguments(argv)


def test_unknown_linearization_is_refused_by_the_parser():
    with pytest.raises(SystemExit):
        parse_arguments(BASE + THETA + ["--avo_linearization", "shuey"])


def test_main_pocs_refuses_the_flag():
    from deep_prior_interpolation_amd.main_pocs import Interpolator
    with pytest.raises(ValueError, match="--avo_theta"):
        Interpolator(parse_arguments(BASE + THETA), "/tmp", device="cpu")


# ---------------------------------------------------------------- model recovery --------------------------------------------------
def test_pseudo_inverse_recovers_the_model(golden):
    """float64 m -> fp32 (G m) -> pinv: each (t, s) model vector comes back within 8 cond(G_t) 2^-24 |m| — the data's rounding, at most
    2^-24 sigma_max |m|, divided by sigma_min."""
    rng = np.random.RandomState(5)
    for c in _cases(golden("avo"), "coef"):
        G = c["G"].astype(np.float64)                                     # (ntheta, 3, nt0)
        nt0 = G.shape[2]
        m = rng.standard_normal((nt0, 11, 3))
        d = np.einsum("akt,tsk->tsa", G, m).astype(np.float32)
        got = avo_model_from_data(d, G)
        assert got.dtype == np.float64 and got.shape == m.shape
        cond = np.array([np.linalg.cond(G[:, :, t]) for t in range(nt0)])
        err = np.linalg.norm(got - m, axis=-1)
        bound = 8.0 * cond[:, None] * U24 * np.linalg.norm(m, axis=-1)
        assert np.all(err <= bound), float((err / bound).max())


def test_avo_gathers_obey_the_avo_equation():
    theta = [0, 10, 20, 30, 40]
    d, m = u.avo_gathers((24, 16, 5), theta, vsvp=0.5, seed=2, return_model=True)
    assert d.shape == (24, 16, 5) and d.dtype == np.float32 and m.shape == (24, 16, 3) and m.dtype == np.float64
    G = avo_coefficients(theta, 0.5, 1)[:, :, 0]
    np.testing.assert_allclose(d, np.einsum("ak,txk->txa", G, m), rtol=0, atol=U24 * np.abs(d).max())
    assert np.linalg.matrix_rank(np.corrcoef(m.reshape(-1, 3).T), tol=1e-2) == 3           # three independent sections
    assert np.array_equal(d, u.avo_gathers((24, 16, 5), theta, vsvp=0.5, seed=2))
    assert not np.array_equal(d, u.avo_gathers((24, 16, 5), theta, vsvp=0.5, seed=3))
    with pytest.raises(ValueError):
        u.avo_gathers((24, 16, 4), theta)


# ---------------------------------------------------------------- re-assembly -----------------------------------------------------
@pytest.mark.parametrize("reassembly, vol_shape, out_shape", [("crop", (20, 14, 5), (20, 14, 3)), ("crop", (21, 15, 5), (20, 14, 3)),
                                                              ("cover", (21, 15, 5), (21, 15, 3))])
@pytest.mark.parametrize("blend", ["flat", "taper"])
def test_reassembly_returns_a_constant_model_exactly(tmp_path, reassembly, vol_shape, out_shape, blend):
    from deep_prior_interpolation_amd.data import reconstruct_patches
    np.save(tmp_path / "vol.npy", np.zeros(vol_shape, dtype=np.float32))
    a = Namespace(imgdir=str(tmp_path), imgname="vol.npy", outdir="run", datadim="2.5d", slice="tx", imgchannel=5, gain=2.0,
                  patch_shape=[8, 8, 5], patch_stride=[4, 6, 5], reassembly=reassembly, blend=blend)
    origins = u.window_origins(vol_shape, (8, 8, 5), (4, 6, 5), cover=reassembly == "cover")
    assert len(origins) == (15 if reassembly == "cover" else 8)            # overlapping windows along t (and, under cover, along x)
    os.makedirs(tmp_path / "run")
    c = np.array([1.5, -2.0, 0.3], dtype=np.float32)
    model = np.broadcast_to(c * np.float32(a.gain), (8, 8, 3)).astype(np.float32)
    for i in range(len(origins)):
        np.save(tmp_path / "run" / ("%02d_run.npy" % i),
                {"output": np.zeros((8, 8, 5), dtype=np.float32), "history": None, "avo_theta": [0, 10, 20, 30, 40], "avo_model": model})
    rec = reconstruct_patches(a, results_root=str(tmp_path), field="avo_model")
    assert rec.shape == out_shape and rec.dtype == np.float32
    assert np.array_equal(rec, np.broadcast_to(c, out_shape))
    # a skipped patch (avo_model None) counts as zeros in its window; files of a run without --avo_theta are refused
    np.save(tmp_path / "run" / "00_run.npy", {"output": np.zeros((8, 8, 5), dtype=np.float32), "history": None, "avo_theta": [0], "avo_model": None})
    rec = reconstruct_patches(a, results_root=str(tmp_path), field="avo_model")
    assert rec[0, 0, 0] == 0.0 and np.array_equal(rec[-1, -1], c)
    np.save(tmp_path / "run" / "00_run.npy", {"output": np.zeros((8, 8, 5), dtype=np.float32), "history": None})
    with pytest.raises(ValueError, match="avo"):
        reconstruct_patches(a, results_root=str(tmp_path), field="avo_model")


def test_reassembly_blends_differing_models_like_the_data(tmp_path):
    """Two overlapping windows with different constants: the overlap is their mean (flat) / their ramp-weighted mean (taper), as
    field="output" gives for the same numbers."""
    from deep_prior_interpolation_amd.data import reconstruct_patches
    np.save(tmp_path / "vol.npy", np.zeros((12, 8, 5), dtype=np.float32))
    os.makedirs(tmp_path / "run")
    for i, v in enumerate((1.0, 3.0)):
        np.save(tmp_path / "run" / ("%d_run.npy" % i), {"output": np.full((8, 8, 5), v, dtype=np.float32), "history": None, "elapsed": None,
                                                       "avo_theta": [0, 10, 20, 30, 40], "avo_model": np.full((8, 8, 3), v, dtype=np.float32)})
    for blend in ("flat", "taper"):
        a = Namespace(imgdir=str(tmp_path), imgname="vol.npy", outdir="run", datadim="2.5d", slice="tx", imgchannel=5, gain=1.0,
                      patch_shape=[8, 8, 5], patch_stride=[4, 8, 5], reassembly="cover", blend=blend)
        model = reconstruct_patches(a, results_root=str(tmp_path), field="avo_model")
        data = reconstruct_patches(a, results_root=str(tmp_path))
        assert model.shape == (12, 8, 3) and data.shape == (12, 8, 5)
        np.testing.assert_array_equal(model[:, :, 0], data[:, :, 0])
        assert np.all(model[:4] == 1.0) and np.all(model[8:] == 3.0) and np.all((model[4:8] > 1.0) & (model[4:8] < 3.0))


# ---------------------------------------------------------------- checkpoints, ABI ------------------------------------------------
def test_old_checkpoints_without_the_keys_are_accepted():
    now = parse_arguments(BASE)
    saved = Namespace(**{k: v for k, v in vars(parse_arguments(BASE)).items() if not k.startswith("avo_")})
    assert not hasattr(saved, "avo_theta")
    assert net_args_are_same(now, saved)
    assert net_args_are_same(saved, now)
    with_avo = parse_arguments(BASE + THETA)
    assert not net_args_are_same(with_avo, saved)                      # the net of an --avo_theta run writes three parameter sections
    assert not net_args_are_same(with_avo, now)
    assert net_args_are_same(with_avo, parse_arguments(BASE + THETA))
    assert not net_args_are_same(with_avo, parse_arguments(BASE + ["--avo_theta", "0", "10", "20", "30", "41"]))


def test_abi_table_header_and_makefile_name_the_entry_points():
    import ctypes as C
    for name in ("dpi_avo_fwd", "dpi_avo_adj"):
        res, args = _lib.SIGNATURES[name]
        assert res is C.c_int and args == [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_size_t, C.c_void_p, C.c_void_p]
    h = open(os.path.join(ROOT, "include", "dpi_hip.h")).read()
    assert "int dpi_avo_fwd(const float* x, const float* G, int ntheta, int T, size_t S, float* y, void* stream);" in h
    assert "int dpi_avo_adj(const float* y, const float* G, int ntheta, int T, size_t S, float* x, void* stream);" in h
    assert "operators/avo.py:67-95" in h
    assert "avo.hip" in open(os.path.join(ROOT, "deep_prior_interpolation_amd", "csrc", "Makefile")).read()
