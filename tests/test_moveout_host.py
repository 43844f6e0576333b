"""--moveout without a GPU: the float64 reference the GPU tests use, the table builders, the operator's refusals and walk ranges, the flags
and their refusals, old checkpoints, the table windows of data.extract_patches, the Interpolator's mask, the re-assembly field and the
ABI table."""
import ctypes as C
import os
import subprocess
from argparse import Namespace

import numpy as np
import pytest
import torch

from conftest import ROOT

import moveout_cases as M
from deep_prior_interpolation_amd import _lib, utils as u
from deep_prior_interpolation_amd.operators import Moveout, moveout_ranges, nmo_table, shift_table
from deep_prior_interpolation_amd.parameter import check_moveout, net_args_are_same, parse_arguments

BASE = ["--imgdir", "x"]
MOV = ["--moveout", "tau.npy"]


def standin_nmo(shape, **kw):
    """The NMO table of utils.hyperbolic_volume's MEAN law c(tau) = 0.9 - 0.3 tau / nt: apex at (0, 0), offset = nt * r, velocity = 1 / c."""
    nt, nx, ny = shape
    off = nt * np.sqrt((np.arange(nx)[:, None] / nx) ** 2 + (np.arange(ny)[None] / ny) ** 2)
    return nmo_table(shape, off, lambda tau: 1.0 / (0.9 - 0.3 * tau / nt), **kw), off


# ---------------------------------------------------------------- the float64 reference -------------------------------------------
@pytest.mark.parametrize("interp", ["linear", "cubic"])
@pytest.mark.parametrize("C_, T, S, family", M.CASES[:27], ids=M.IDS[:27])
def test_reference_dot_test_gather_and_identity(C_, T, S, family, interp):
    """<L m, d> = <m, L^T d> at 1e-12, the gather over the operator's ranges equals the scatter, the identity table returns its input."""
    c = M.case(C_, T, S, family, interp)
    m, d = c["m"].astype(np.float64), c["d"].astype(np.float64)
    a, b = np.vdot(c["fwd"], d), np.vdot(m, c["adj"])
    assert abs(a - b) <= 1e-12 * max(1.0, np.abs(c["fwd"]).sum())
    ranges = moveout_ranges(c["table"], interp)
    assert ranges.shape == (2, T, S) and ranges.dtype == np.int32 and ranges.min() >= 0 and ranges.max() <= T
    if T * S <= 33 * 65:
        np.testing.assert_allclose(M.gather64(d, c["table"], interp, ranges), c["adj"], rtol=0, atol=1e-12)
    if family == "identity":
        assert np.array_equal(c["fwd"], m) and np.array_equal(c["adj"], d)
    if family == "all_muted":
        assert not c["fwd"].any() and not c["adj"].any() and not c["fwd_bound"].any() and not ranges.any()
    assert np.all(c["fwd_bound"] >= 0) and np.all(c["adj_bound"] >= 0) and c["fwd_bound"].max() < 1e-4


@pytest.mark.parametrize("interp", ["linear", "cubic"])
@pytest.mark.parametrize("C_, T, S, family", M.CASES[27:], ids=M.IDS[27:])
def test_ranges_hold_every_contribution_at_the_large_shapes(C_, T, S, family, interp):
    table = M.table_for(family, T, S)
    live, rows, _ = M.taps64(table, interp)
    r = moveout_ranges(table, interp)
    tt, ss = np.nonzero(live)
    for k in range(rows.shape[0]):
        i = rows[k][tt, ss]
        assert np.all(r[0][i, ss] <= tt) and np.all(tt < r[1][i, ss])
    if family == "constant":
        assert r[1].max() - r[0].min() == T                     # the longest walk: one thread, all T samples


def test_weights_are_exact_at_f_0_and_sum_to_one():
    tab = np.array([[0.0], [1.0], [2.25], [3.0]], dtype=np.float32)
    for interp, at0 in (("linear", [1, 0]), ("cubic", [0, 1, 0, 0])):
        live, rows, w = M.taps64(tab, interp)
        assert live.all() and np.array_equal(w[:, 0, 0], at0) and np.array_equal(w[:, 3, 0], at0)
        np.testing.assert_allclose(w.sum(axis=0), 1.0, rtol=0, atol=1e-15)
    assert np.array_equal(M.taps64(tab, "cubic")[1][:, 0, 0], [0, 0, 1, 2]) and np.array_equal(M.taps64(tab, "cubic")[1][:, 3, 0], [2, 3, 3, 3])


def test_cases_cover_what_the_issue_names():
    assert len(M.CASES) == 45 and {c[:3] for c in M.CASES} == {(1, 5, 1), (2, 7, 3), (1, 33, 65), (3, 130, 70), (1, 257, 129)}
    assert len(M.FAMILIES) == 9
    t = M.table_for("sorted_gaps", 130, 70)
    assert 0.2 < (t == M.MUTE).mean() < 0.4
    assert (M.table_for("stretch", 33, 65) <= 32).mean() < 0.4 and (M.table_for("nmo", 33, 65)[0] == M.MUTE).any()


# ---------------------------------------------------------------- the table builders ----------------------------------------------
def test_shift_table():
    sh = np.array([[0.0, 0.5, -1.25], [2.0, 3.75, 0.1]])
    tab = shift_table((6, 2, 3), sh)
    assert tab.shape == (6, 2, 3) and tab.dtype == np.float64
    assert np.array_equal(tab, np.arange(6.0)[:, None, None] - sh[None])
    assert np.array_equal(shift_table((4, 3), [0.5, 1.0, 0.0]), np.arange(4.0)[:, None] - np.array([0.5, 1.0, 0.0])[None])
    for bad in (np.zeros(3), np.zeros((3, 2))):
        with pytest.raises(ValueError, match="shifts"):
            shift_table((6, 2, 3), bad)
    with pytest.raises(ValueError, match="non-finite"):
        shift_table((4, 2), [0.0, np.nan])
    op = Moveout(tab)
    assert np.array_equal(op.live, (tab >= 0) & (tab <= 5)) and op.table.dtype == np.float32


@pytest.mark.parametrize("velocity", ["callable", "values"])
def test_nmo_table_inverts_its_travel_time(velocity):
    T, X = 64, 24
    off = np.linspace(0.0, 60.0, X)
    law = lambda tau: 1.5 + 0.02 * tau
    vel = law if velocity == "callable" else law(np.arange(T, dtype=np.float64))          # the law is linear: its interpolated values are the law
    tab = nmo_table((T, X), off, vel)
    assert tab.shape == (T, X) and tab.dtype == np.float64
    live = tab != -1.0
    assert np.all((tab[live] >= 0) & (tab[live] <= T - 1)) and 0.3 < live.mean() < 1.0
    t = np.arange(T, dtype=np.float64)[:, None] * np.ones((1, X))
    back = np.sqrt(tab ** 2 + (off[None] / law(tab)) ** 2)
    assert np.abs(back - t)[live].max() <= 1e-9
    # monotone per trace; muted before the first arrival (the minimum of t(tau), which a velocity that rises with tau puts behind tau = 0 on
    # the far traces) and past t(T - 1), live everywhere between: t(tau) rises all the way behind its minimum under this law
    g = np.sqrt(np.arange(T)[:, None] ** 2.0 + (off[None] / law(np.arange(T)[:, None])) ** 2)
    for x in range(X):
        col = tab[:, x][live[:, x]]
        assert np.all(np.diff(col) > 0)
        assert np.all(np.diff(g[int(np.argmin(g[:, x])):, x]) > 0)
        assert not live[t[:, x] < g[:, x].min(), x].any() and not live[t[:, x] > g[T - 1, x], x].any()
        assert live[(t[:, x] >= g[:, x].min()) & (t[:, x] <= g[T - 1, x]), x].all()
    assert np.array_equal(tab[:, 0], np.arange(T))              # zero offset: the identity, to the bit
    Moveout(tab)                                                # monotone after the rounding to fp32 as well
    muted = nmo_table((T, X), off, vel, stretch_mute=1.5)
    assert (muted != -1.0).sum() < live.sum() and np.array_equal(muted[muted != -1.0], tab[muted != -1.0])
    j = np.floor(muted[muted != -1.0]).astype(int)
    xs = np.nonzero(muted != -1.0)[1]
    j = np.minimum(j, T - 2)
    assert np.all(1.0 / (g[j + 1, xs] - g[j, xs]) <= 1.5 + 1e-12)


def test_nmo_table_on_the_stand_in_law():
    tab, off = standin_nmo((48, 32, 32))
    live = tab != -1.0
    assert 0.3 < live.mean() < 0.4
    c = lambda tau: 0.9 - 0.3 * tau / 48
    back = np.sqrt(tab ** 2 + (off[None] * c(tab)) ** 2)
    assert np.abs(back - np.arange(48.0)[:, None, None])[live].max() <= 1e-9
    # c falls with tau: t(tau) has its minimum inside the axis on the far traces; everything before it is muted
    g = np.sqrt(np.arange(48.0)[:, None, None] ** 2 + (off[None] * c(np.arange(48.0)[:, None, None])) ** 2)
    assert not live[np.arange(48.0)[:, None, None] < g.min(axis=0)[None]].any()
    op = Moveout(tab, "cubic")
    assert op.live.mean() == live.mean()


def test_nmo_table_refusals():
    for kw, match in ((dict(offset=np.zeros(3)), "offset"), (dict(velocity=np.ones(5)), "velocity"), (dict(velocity=lambda t: 0.0 * t), "velocity"),
                      (dict(stretch_mute=0.0), "stretch_mute"), (dict(offset=np.array([0.0, np.inf])), "offset")):
        args = dict(shape=(8, 2), offset=np.zeros(2), velocity=np.ones(8))
        args.update(kw)
        with pytest.raises(ValueError, match=match):
            nmo_table(**args)


# ---------------------------------------------------------------- the operator ----------------------------------------------------
@pytest.mark.parametrize("bad, match", [
    (np.zeros(5), "2-D|\\(T, X\\)"), (np.zeros((2, 3, 4, 5)), "\\(T, X\\)"), (np.zeros((4, 3), dtype=complex), "real"), (np.zeros((0, 3)), "non-empty"),
    (np.array([[0.0], [np.nan]]), "non-finite"), (np.array([[0.0], [np.inf]]), "non-finite"),
])
def test_operator_refuses_the_table(bad, match):
    with pytest.raises(ValueError, match=match):
        Moveout(bad)


def test_operator_names_the_first_decreasing_trace():
    tab = np.arange(6.0)[:, None, None] * np.ones((1, 3, 4))
    tab[2, 1, 2] = -1.0                                          # a mute gap is fine
    Moveout(tab)
    tab[4, 2, 1] = 2.5                                           # after 3: decreases
    tab[3, 2, 3] = 0.0
    with pytest.raises(ValueError, match=r"trace \(2, 1\)"):
        Moveout(tab)
    gap = np.array([[3.0], [-1.0], [2.0], [4.0]])                # decreasing across a gap counts too
    with pytest.raises(ValueError, match=r"trace \(0,\)"):
        Moveout(gap)
    Moveout(np.array([[2.0], [2.0], [9.0], [2.0]]))              # equal values and a muted sample (9 > T - 1) between them


def test_operator_refuses_interp_batch_and_shape():
    with pytest.raises(ValueError, match="interpolation"):
        Moveout(np.zeros((4, 3)), interp="sinc8")
    op = Moveout(np.zeros((6, 5)))
    # refused from the shape alone, before the library is even looked up (these are host tensors)
    with pytest.raises(ValueError, match="batch"):
        op._matvec(torch.zeros(2, 1, 6, 5), False)
    with pytest.raises(ValueError, match="table"):
        op._matvec(torch.zeros(1, 1, 6, 4), False)
    with pytest.raises(ValueError, match="table"):
        op._matvec(torch.zeros(1, 1, 6, 5, 1), True)
    with pytest.raises(ValueError):
        op._matvec(torch.zeros(1, 6, 5), False)
    with pytest.raises(_lib.DpiError):                           # no CPU path
        op.forward(torch.zeros(1, 1, 6, 5))
    op3 = Moveout(torch.zeros(6, 5, 2), interp="cubic")
    assert op3.table.shape == (6, 5, 2) and op3.live.shape == (6, 5, 2) and op3.live.all() and op3.kind == 1 and op.kind == 0
    assert op.table.dtype == np.float32 and op.live.dtype == bool


# ---------------------------------------------------------------- flags -----------------------------------------------------------
def test_flags_parse():
    off = parse_arguments(BASE)
    assert off.moveout is None and off.moveout_interp == "linear" and check_moveout(off) is None
    assert check_moveout(Namespace(datadim="3d")) is None       # an old args.txt
    a = parse_arguments(BASE + MOV + ["--datadim", "3d"])
    assert a.moveout == "tau.npy" and check_moveout(a) == ("tau.npy", "linear")
    a = parse_arguments(BASE + MOV + ["--datadim", "2d", "--moveout_interp", "cubic"])
    assert check_moveout(a) == ("tau.npy", "cubic")
    # everything that sees a data-domain tensor combines
    for extra in (["--holdout", "0.2"], ["--out_ema", "0.9"], ["--optimizer", "sgld"], ["--aa_weight", "0.1"], ["--trace_offsets", "o.npy"],
                  ["--trace_offsets", "o.npy", "--trace_interp", "cubic"], ["--net", "unet"], ["--net", "attmultiunet"], ["--precision", "bf16"]):
        assert parse_arguments(BASE + MOV + ["--datadim", "3d"] + extra).moveout == "tau.npy"
    with pytest.raises(SystemExit):
        parse_arguments(BASE + MOV + ["--datadim", "3d", "--moveout_interp", "sinc8"])


@pytest.mark.parametrize("argv, flag", [
    (BASE + ["--moveout_interp", "cubic"], "--moveout_interp"),                                       # would silently do nothing
    (BASE + MOV + ["--datadim", "2.5d", "--slice", "tx", "--imgchannel", "3"], "--moveout"),
    (BASE + MOV + ["--datadim", "2.5d", "--slice", "tx", "--imgchannel", "4", "--avo_theta", "0", "10", "20", "30"], "--moveout"),
    (BASE + MOV + ["--datadim", "3d", "--wavelet", "w.npy"], "--wavelet"),
    (BASE + MOV + ["--datadim", "3d", "--net", "part"], "--net part"),
    (BASE + MOV + ["--datadim", "3d", "--data_forgetting_factor", "3"], "--data_forgetting_factor"),
])
def test_flag_refusals(argv, flag):
    with pytest.raises(ValueError, match=flag):
        parse_arguments(argv)


def test_avo_and_bad_interp_are_refused_by_the_check_itself():
    a = parse_arguments(BASE + MOV + ["--datadim", "3d"])
    a.avo_theta = [0.0, 10.0, 20.0]
    with pytest.raises(ValueError, match="--avo_theta"):
        check_moveout(a)
    a.avo_theta, a.moveout_interp = None, "sinc8"
    with pytest.raises(ValueError, match="--moveout_interp"):
        check_moveout(a)


def test_main_pocs_refuses_the_flag():
    from deep_prior_interpolation_amd.main_pocs import Interpolator
    with pytest.raises(ValueError, match="--moveout"):
        Interpolator(parse_arguments(BASE + MOV + ["--datadim", "3d"]), "/tmp", device="cpu")


def test_net_args_are_same():
    now = parse_arguments(BASE)
    saved = Namespace(**{k: v for k, v in vars(parse_arguments(BASE)).items() if not k.startswith("moveout")})
    assert not hasattr(saved, "moveout") and not hasattr(saved, "moveout_interp")
    assert net_args_are_same(now, saved) and net_args_are_same(saved, now)            # an old args.txt reads as off / linear
    on = parse_arguments(BASE + MOV)
    assert net_args_are_same(on, parse_arguments(BASE + MOV))
    assert not net_args_are_same(on, saved) and not net_args_are_same(on, now)
    assert not net_args_are_same(on, parse_arguments(BASE + ["--moveout", "other.npy"]))
    assert not net_args_are_same(on, parse_arguments(BASE + MOV + ["--moveout_interp", "cubic"]))


# ---------------------------------------------------------------- data.extract_patches --------------------------------------------
def _volume(tmp_path, shape, table, datadim, patch_shape, patch_stride=None, extra=()):
    rng = np.random.RandomState(0)
    vol = rng.standard_normal(shape).astype(np.float32)
    np.save(tmp_path / "vol.npy", vol)
    np.save(tmp_path / "msk.npy", (rng.uniform(size=shape) < 0.5).astype(np.float32))
    if table is not None:
        np.save(tmp_path / "tau.npy", table)
    argv = ["--imgdir", str(tmp_path), "--imgname", "vol.npy", "--maskname", "msk.npy", "--datadim", datadim, "--patch_shape"] + \
        [str(n) for n in patch_shape]
    if patch_stride is not None:
        argv += ["--patch_stride"] + [str(n) for n in patch_stride]
    return parse_arguments(argv + (MOV if table is not None else []) + list(extra)), vol


@pytest.mark.parametrize("reassembly", ["crop", "cover"])
def test_extract_patches_cuts_the_table_window_3d(tmp_path, reassembly):
    from deep_prior_interpolation_amd.data import extract_patches
    shape = (6, 9, 7)
    table = np.arange(6.0)[:, None, None] - np.random.RandomState(1).uniform(0, 2, (1, 9, 7))
    a, vol = _volume(tmp_path, shape, table, "3d", (-1, 4, 4), (-1, 3, 3), extra=("--reassembly", reassembly))
    patches = extract_patches(a)
    origins = u.window_origins(shape, (6, 4, 4), (6, 3, 3), cover=reassembly == "cover")
    assert len(patches) == len(origins) == (6 if reassembly == "cover" else 4)
    for p, o in zip(patches, origins):
        win = (slice(None), slice(int(o[1]), int(o[1]) + 4), slice(int(o[2]), int(o[2]) + 4))
        assert p["moveout"].shape == (6, 4, 4) and p["moveout"].dtype == np.float32
        assert np.array_equal(p["moveout"], table.astype(np.float32)[win])
        assert np.array_equal(p["image"][..., 0], vol[win] * a.gain)
    b, _ = _volume(tmp_path, shape, None, "3d", (-1, 4, 4), (-1, 3, 3))
    assert all("moveout" not in p for p in extract_patches(b))


def test_extract_patches_cuts_the_table_window_2d(tmp_path):
    from deep_prior_interpolation_amd.data import extract_patches
    table = np.arange(8.0)[:, None] - np.linspace(0, 3, 10)[None]
    a, _ = _volume(tmp_path, (8, 10), table, "2d", (-1, 5))
    patches = extract_patches(a)
    assert len(patches) == 2 and np.array_equal(patches[1]["moveout"], table.astype(np.float32)[:, 5:])


def test_extract_patches_refusals(tmp_path):
    from deep_prior_interpolation_amd.data import extract_patches
    good = np.arange(6.0)[:, None, None] * np.ones((1, 9, 7))
    a, _ = _volume(tmp_path, (6, 9, 7), good, "3d", (3, 4, 4))          # a time-tiled patch
    with pytest.raises(ValueError, match="--moveout.*time axis"):
        extract_patches(a)
    for bad, match in ((good[:, :, :6], "--moveout.*shape"), (good[:5], "--moveout.*shape"), (good[0], "--moveout.*shape"),
                       (np.where(good == 3, np.nan, good), "--moveout.*non-finite"), (good[::-1].copy(), r"--moveout.*trace \(0, 0\)"),
                       (good.astype(complex), "--moveout.*real")):
        a, _ = _volume(tmp_path, (6, 9, 7), bad, "3d", (-1, 4, 4))
        with pytest.raises(ValueError, match=match):
            extract_patches(a)
    a, _ = _volume(tmp_path, (6, 9, 7), good, "2d", (-1, 4, -1))        # a 3-D volume under --datadim 2d: its last axis is channels
    with pytest.raises(ValueError, match="--moveout"):
        extract_patches(a)


# ---------------------------------------------------------------- the Interpolator, on the host -----------------------------------
def test_load_data_takes_muted_samples_out_of_the_device_mask(tmp_path):
    from deep_prior_interpolation_amd.main import Interpolator
    a = parse_arguments(["--imgdir", str(tmp_path), "--datadim", "3d", "--holdout", "0.3"] + MOV)
    T = Interpolator(a, str(tmp_path), device="cpu")
    rng = np.random.RandomState(2)
    table = (np.arange(6.0)[:, None, None] - rng.randint(0, 4, (1, 5, 4))).astype(np.float64)
    table[:, 0, 0] = -1.0                                        # one fully muted trace
    img, mask = rng.standard_normal((6, 5, 4, 1)), (rng.uniform(size=(1, 5, 4, 1)) < 0.7) * np.ones((6, 1, 1, 1))
    mask[:, 0, 0] = 1.0
    std = T.load_data({"image": img, "mask": mask, "name": "0", "moveout": table})
    live = table >= 0
    assert np.array_equal(T.forward_model.stage("moveout").op.live, live) and np.array_equal(T.mask, mask)             # the host mask stays the file's
    assert np.array_equal(T.mask_[0, 0].numpy(), (mask[..., 0] * live).astype(np.float32)) and std > 0
    assert np.array_equal(T.known_mask(), mask * live[..., None])
    T.begin_patch(0)
    T.build_holdout()
    assert T.holdout_sel.shape == (5, 4, 1) and T.holdout_sel.sum() > 0 and T.holdout_sel[0, 0, 0] == 0      # nothing live to hold out
    assert not (T.mask_[0, 0].numpy() * T.holdout_sel[None, ..., 0])[~live].any()
    # no live known sample: std 0, the patch is skipped like an all-masked one; the result file names the table and no model
    assert T.load_data({"image": img, "mask": mask, "name": "1", "moveout": np.full((6, 5, 4), -1.0)}) == 0.0
    T.out_best, T.elapsed = T.img * T.mask, 0.0
    T.save_result()
    run = np.load(tmp_path / "1_run.npy", allow_pickle=True).item()
    assert run["moveout_model"] is None and run["moveout_interp"] == "linear" and np.array_equal(run["moveout"], np.full((6, 5, 4), -1.0, np.float32))
    for bad, match in ((None, "carries no table"), (table[:5], "shape"), (table[::-1].copy(), "decreases")):
        with pytest.raises(ValueError, match="--moveout.*" + match):
            T.load_data({"image": img, "mask": mask, "name": "0", "moveout": bad})
    T0 = Interpolator(parse_arguments(["--imgdir", str(tmp_path), "--datadim", "3d"]), str(tmp_path), device="cpu")
    with pytest.raises(ValueError, match="--moveout is off"):
        T0.load_data({"image": img, "mask": mask, "name": "0", "moveout": table})
    T0.load_data({"image": img, "mask": mask, "name": "0"})
    assert T0.forward_model.stage("moveout") is None and T0.known_mask() is T0.mask and T0.moveout_model() is None


def test_interpolator_refuses_what_the_parser_refuses():
    from deep_prior_interpolation_amd.main import Interpolator
    a = parse_arguments(BASE + MOV + ["--datadim", "3d"])
    a.net = "part"
    with pytest.raises(ValueError, match="--net part"):
        Interpolator(a, "/tmp", device="cpu")


# ---------------------------------------------------------------- re-assembly -----------------------------------------------------
def test_reassembly_of_the_model_sections(tmp_path):
    from deep_prior_interpolation_amd.data import reconstruct_patches
    np.save(tmp_path / "vol.npy", np.zeros((8, 14), dtype=np.float32))
    a = Namespace(imgdir=str(tmp_path), imgname="vol.npy", outdir="run", datadim="2d", slice="xy", imgchannel=None, gain=2.0,
                  patch_shape=[-1, 8], patch_stride=[-1, 6], reassembly="crop", blend="flat")
    os.makedirs(tmp_path / "run")
    tab = np.zeros((8, 8), np.float32)
    for i in range(2):
        np.save(tmp_path / "run" / ("%d_run.npy" % i), {"output": np.zeros((8, 8, 1), dtype=np.float32), "history": None, "moveout": tab,
                                                        "moveout_model": np.full((8, 8, 1), (i + 1) * a.gain, dtype=np.float32)})
    rec = reconstruct_patches(a, results_root=str(tmp_path), field="moveout_model")
    assert rec.shape == (8, 14) and np.array_equal(rec[:, :6], np.full((8, 6), 1.0)) and np.array_equal(rec[:, 6:8], np.full((8, 2), 1.5))
    assert np.array_equal(rec[:, 8:], np.full((8, 6), 2.0))
    np.save(tmp_path / "run" / "0_run.npy", {"output": np.zeros((8, 8, 1), dtype=np.float32), "history": None, "moveout": tab,
                                             "moveout_model": None})          # a skipped patch counts as zeros
    assert reconstruct_patches(a, results_root=str(tmp_path), field="moveout_model")[0, 0] == 0.0
    np.save(tmp_path / "run" / "0_run.npy", {"output": np.zeros((8, 8, 1), dtype=np.float32), "history": None})
    with pytest.raises(ValueError, match="moveout"):
        reconstruct_patches(a, results_root=str(tmp_path), field="moveout_model")


# ---------------------------------------------------------------- ABI -------------------------------------------------------------
def test_abi_table_header_exports_and_makefile_name_the_entry_points():
    assert _lib.ABI_VERSION == 406
    I, P, Z = C.c_int, C.c_void_p, C.c_size_t
    assert _lib.SIGNATURES["dpi_moveout_fwd"] == (I, [P, P, I, I, I, Z, P, P])
    assert _lib.SIGNATURES["dpi_moveout_adj"] == (I, [P, P, P, I, I, I, Z, P, P])
    h = open(os.path.join(ROOT, "include", "dpi_hip.h")).read()
    assert "int dpi_moveout_fwd(const float* m, const float* tau, int interp, int C, int T, size_t S, float* d, void* stream);" in h
    assert ("int dpi_moveout_adj(const float* d, const float* tau, const int* range, int interp, int C, int T, size_t S, float* m, "
            "void* stream);") in h
    assert "moveout.hip" in open(os.path.join(ROOT, "deep_prior_interpolation_amd", "csrc", "Makefile")).read()
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    exported = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    for name in ("dpi_moveout_fwd", "dpi_moveout_adj"):
        assert (" T " + name + "\n") in exported
    assert _lib.load().dpi_version() == 406
