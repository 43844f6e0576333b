"""--moveout_offset without a GPU: the picker against exhaustive search, the panel, recovery of one analytic event through the float64
restatement of the scan, the flags and every refusal, old checkpoints, what stays as it was with the flags off, and the ABI table."""
import ctypes as C
import itertools
import os
import subprocess
from argparse import Namespace

import numpy as np
import pytest

from conftest import ROOT

import velocity_cases as V
from deep_prior_interpolation_amd import _lib
from deep_prior_interpolation_amd.operators import (gather_geometry, nmo_table, pick_velocity, scan_table, semblance_panel, semblance_sums,
                                                    velocity_windows)
from deep_prior_interpolation_amd.parameter import check_moveout, check_moveout_scan, net_args_are_same, parse_arguments

BASE = ["--imgdir", "x"]
SCAN = ["--moveout_offset", "off.npy", "--moveout_vscan", "1.0", "1.8", "9"]


# ---------------------------------------------------------------- the picker ------------------------------------------------------
def _exhaustive(P, step):
    """Every admissible path, its score added in ascending tau; the best one, ties to the lowest index at the last row, then at the row
    before it, and so on: what a Viterbi pass that breaks its ties towards the lowest index returns."""
    T, NV = P.shape
    best = None
    for path in itertools.product(range(NV), repeat=T):
        if any(abs(path[t + 1] - path[t]) > step for t in range(T - 1)):
            continue
        s = P[0, path[0]]
        for t in range(1, T):
            s = s + P[t, path[t]]
        key = (-s,) + tuple(reversed(path))
        if best is None or key < best[0]:
            best = (key, path, s)
    return np.array(best[1]), best[2]


@pytest.mark.parametrize("step", [1, 2])
@pytest.mark.parametrize("T, NV", [(1, 1), (1, 4), (2, 3), (4, 4), (6, 4), (6, 2), (5, 1)])
def test_pick_velocity_against_exhaustive_search(T, NV, step):
    vel = np.linspace(1.0, 2.0, NV) if NV > 1 else np.array([1.5])
    rng = np.random.RandomState(100 * T + 10 * NV + step)
    panels = [rng.rand(T, NV) for _ in range(6)]
    # ties: few distinct dyadic values (every sum exact, so equal scores are equal floats), a constant panel, an all-zero panel
    panels += [rng.randint(0, 3, (T, NV)) / 4.0 for _ in range(8)] + [np.full((T, NV), 0.5), np.zeros((T, NV))]
    got = pick_velocity(np.stack(panels), vel, max_step=step)
    assert got.shape == (len(panels), T) and got.dtype == np.float64
    for P, law in zip(panels, got):
        want, _ = _exhaustive(P, step)
        assert np.array_equal(law, vel[want]), (P, law, vel[want])
    assert np.array_equal(got[-1], np.full(T, vel[0])) and np.array_equal(got[-2], np.full(T, vel[0]))       # all tied: the lowest index


def test_pick_velocity_follows_a_ridge_no_faster_than_max_step():
    P = np.zeros((1, 8, 9))
    ridge = [0, 0, 4, 4, 4, 8, 8, 8]
    P[0, np.arange(8), ridge] = 1.0
    vel = np.arange(9.0) + 1.0
    for step in (1, 2, 4):
        j = (pick_velocity(P, vel, max_step=step)[0] - 1.0).astype(int)
        assert np.abs(np.diff(j)).max() <= step
    assert np.array_equal(pick_velocity(P, vel, max_step=4)[0] - 1.0, ridge)
    assert len(set(pick_velocity(P, vel, max_step=0)[0])) == 1
    with pytest.raises(ValueError, match="panel"):
        pick_velocity(P, vel[:-1])
    with pytest.raises(ValueError, match="max_step"):
        pick_velocity(P, vel, max_step=-1)


# ---------------------------------------------------------------- the panel -------------------------------------------------------
def test_semblance_panel_bounds_fold_window_and_zero_denominator():
    c = V.flat_case(33, 130, 3, "holes")
    r = c["ref"]
    P = semblance_panel(r["num"], r["den"], r["cnt"], window=2, min_fold=4)
    assert P.shape == (1, 33, 3) and P.dtype == np.float64
    # Cauchy-Schwarz row by row; the sums of up to 130 terms and the box of 5 rows are rounded: (130 + 5 + 4) 2^-53 relative, each side
    assert P.min() >= 0.0 and P.max() <= 1.0 + 4 * 139 * 2.0 ** -53 and P.max() > 0.0
    # the restatement of the panel, row by row with explicit clipping
    keep = r["cnt"] >= 4
    n, d, k = np.where(keep, r["num"], 0), np.where(keep, r["den"], 0), np.where(keep, r["cnt"], 0)
    for tau in (0, 1, 2, 16, 30, 31, 32):
        lo, hi = max(0, tau - 2), min(33, tau + 3)
        top, bot = (n[0, :, lo:hi] ** 2).sum(1), (k[0, :, lo:hi] * d[0, :, lo:hi]).sum(1)
        np.testing.assert_allclose(P[0, tau], np.where(bot > 0, top / np.where(bot > 0, bot, 1), 0), rtol=1e-14, atol=0)
    # window 0 is the row's own ratio; a fold above every count empties the panel
    P0 = semblance_panel(r["num"], r["den"], r["cnt"], window=0, min_fold=1)
    some = (r["cnt"] >= 1) & (r["den"] > 0)
    np.testing.assert_allclose(P0[0].T[some[0]], (r["num"] ** 2 / np.where(some, r["cnt"] * r["den"], 1))[0][some[0]], rtol=1e-15)
    assert not semblance_panel(r["num"], r["den"], r["cnt"], window=2, min_fold=131).any()
    # min_fold zeroes all three arrays: a row below the fold adds nothing to its neighbours' windows
    num, den, cnt = np.ones((1, 1, 5)) * 3.0, np.ones((1, 1, 5)) * 3.0, np.full((1, 1, 5), 3, dtype=np.int32)
    cnt[0, 0, 2], num[0, 0, 2], den[0, 0, 2] = 2, 100.0, 1e4
    assert np.array_equal(semblance_panel(num, den, cnt, window=1, min_fold=3)[0, :, 0], np.ones(5))
    # a zero denominator (nothing live, or live zeros) is 0, not NaN
    z = semblance_panel(np.zeros((2, 3, 4)), np.zeros((2, 3, 4)), np.full((2, 3, 4), 9, dtype=np.int32))
    assert z.shape == (2, 4, 3) and not z.any()
    with pytest.raises(ValueError, match="shape"):
        semblance_panel(np.zeros((2, 3, 4)), np.zeros((2, 3, 4)), np.zeros((2, 3, 5), dtype=np.int32))
    with pytest.raises(ValueError, match="window"):
        semblance_panel(num, den, cnt, window=-1)


# ---------------------------------------------------------------- recovery --------------------------------------------------------
@pytest.mark.parametrize("stretch", V.EVENT_STRETCH)
@pytest.mark.parametrize("mask_kind", V.EVENT_MASKS)
@pytest.mark.parametrize("tau0, index", V.EVENTS)
def test_the_scan_recovers_one_hyperbolic_event(tau0, index, mask_kind, stretch):
    law = V.event_pick((64, 16, 16), tau0, index, mask_kind, stretch)
    assert law.shape == (1, 64) and law[0, tau0] == V.EVENT_VELOCITIES[index]


@pytest.mark.parametrize("tau0, index", V.EVENTS)
def test_the_scan_recovers_the_event_on_a_section(tau0, index):
    assert V.event_pick((64, 16), tau0, index, "full", None)[0, tau0] == V.EVENT_VELOCITIES[index]


def test_gather_geometry_and_velocity_windows():
    assert gather_geometry((9, 5), "volume") == (1, 0, 5, 1)
    assert gather_geometry((9, 5, 7), "volume") == (1, 0, 35, 1) == V.layouts((9, 5, 7))["volume"]
    assert gather_geometry((9, 5, 7), "y") == (7, 1, 5, 7) == V.layouts((9, 5, 7))["y"]
    assert gather_geometry((9, 5, 7), "x") == (5, 7, 7, 1) == V.layouts((9, 5, 7))["x"]
    for bad in ("x", "y"):
        with pytest.raises(ValueError, match="section"):
            gather_geometry((9, 5), bad)
    with pytest.raises(ValueError, match="gather"):
        gather_geometry((9, 5, 7), "z")
    law = np.arange(5 * 9.0).reshape(5, 9)                      # the x layout of (9, 5, 7): one law per x
    origins, dim = [(0, 0, 0), (0, 2, 3)], (9, 3, 4)
    w = velocity_windows(law, "x", origins, dim)
    assert w[0].shape == (9, 3) and np.array_equal(w[1], law[2:5].T)
    w = velocity_windows(np.arange(7 * 9.0).reshape(7, 9), "y", origins, dim)
    assert w[1].shape == (9, 4) and np.array_equal(w[1], np.arange(7 * 9.0).reshape(7, 9)[3:7].T)
    w = velocity_windows(law[:1], "volume", origins, dim)
    assert w[0].shape == (9,) and np.array_equal(w[1], law[0])


# ---------------------------------------------------------------- refusals before any launch --------------------------------------
def test_scan_table_and_semblance_sums_refuse_bad_arguments_before_any_launch(monkeypatch):
    """None of these reaches the library: loading it is made an error."""
    monkeypatch.setattr(_lib, "load", lambda: (_ for _ in ()).throw(AssertionError("reached the library")))
    d, m, off = np.zeros((8, 4, 3), np.float32), np.ones((8, 4, 3), np.float32), np.ones((4, 3))
    for kw, match in ((dict(vmin=0.0), "vmin"), (dict(vmin=-1.0), "vmin"), (dict(vmin=float("nan")), "vmin"), (dict(vmax=0.5), "vmax"),
                      (dict(vmax=float("inf")), "vmax"), (dict(nv=0), "nv"), (dict(nv=2.5), "nv"), (dict(gather="z"), "gather"),
                      (dict(offset=np.where(off > 0, np.nan, off)), "non-finite"), (dict(offset=np.full((4, 3), np.inf)), "non-finite"),
                      (dict(offset=off[:, :2]), "offset"), (dict(mask=m[:7]), "mask"), (dict(stretch_mute=0.0), "stretch_mute"),
                      (dict(data=np.zeros((8,), np.float32), mask=np.ones((8,), np.float32)), "data")):
        a = dict(data=d, mask=m, offset=off, vmin=1.0, vmax=2.0, nv=3)
        a.update(kw)
        with pytest.raises(ValueError, match=match):
            scan_table(**a)
    with pytest.raises(ValueError, match="section"):              # a gather the geometry does not have
        scan_table(d[:, :, 0], m[:, :, 0], off[:, 0], 1.0, 2.0, 3, gather="y")
    for vel in ([], [1.0, 0.0], [1.0, -2.0], [float("nan")]):
        with pytest.raises(ValueError, match="velocities"):
            semblance_sums(d, m, off, vel)


def test_a_table_that_decreases_names_the_flag(monkeypatch):
    """nmo_table inverts t(tau) on its increasing branch, so its tables do not decrease whatever the law (checked here for a law that
    jumps both ways); should a table builder ever return one that does, the ValueError names --moveout_vscan and --moveout_max_step."""
    from deep_prior_interpolation_amd.operators import check_moveout_table, velocity as mod
    T, X = 32, 8
    off = np.linspace(0.0, 40.0, X)
    for law in (np.where(np.arange(T) < 16, 3.0, 1.0), np.where(np.arange(T) < 16, 1.0, 3.0)):
        check_moveout_table(nmo_table((T, X), off, law))
    sums = lambda *a, **kw: (np.ones((1, 2, T)), np.ones((1, 2, T)), np.full((1, 2, T), 8, dtype=np.int32))
    monkeypatch.setattr(mod, "semblance_sums", sums)
    res = scan_table(np.zeros((T, X), np.float32), np.ones((T, X)), off, 1.0, 3.0, 2)
    assert np.array_equal(res["velocity"], np.ones((1, T))) and np.array_equal(res["table"], nmo_table((T, X), off, np.ones(T)))
    monkeypatch.setattr(mod, "nmo_table", lambda shape, *a: np.arange(T - 1.0, -1.0, -1.0)[:, None] * np.ones((1, X)))
    with pytest.raises(ValueError, match=r"--moveout_vscan.*decreases.*--moveout_max_step"):
        scan_table(np.zeros((T, X), np.float32), np.ones((T, X)), off, 1.0, 3.0, 2)


# ---------------------------------------------------------------- flags -----------------------------------------------------------
def test_flags_parse():
    off = parse_arguments(BASE)
    for k in ("moveout_offset", "moveout_vscan", "moveout_gather", "moveout_stretch", "moveout_window", "moveout_min_fold", "moveout_max_step"):
        assert getattr(off, k) is None, k
    assert check_moveout_scan(off) is None and check_moveout(off) is None
    assert check_moveout_scan(Namespace(datadim="3d")) is None and check_moveout(Namespace(datadim="3d")) is None      # an old args.txt
    a = parse_arguments(BASE + SCAN + ["--datadim", "3d"])
    assert a.moveout_offset == "off.npy" and a.moveout_vscan == [1.0, 1.8, 9.0] and a.moveout is None
    assert check_moveout(a) == ("scan:off.npy", "linear")
    assert check_moveout_scan(a) == {"file": "off.npy", "vmin": 1.0, "vmax": 1.8, "nv": 9, "gather": "volume", "stretch_mute": None,
                                     "window": 2, "min_fold": 4, "max_step": 1}
    a = parse_arguments(BASE + SCAN + ["--datadim", "3d", "--moveout_gather", "y", "--moveout_stretch", "1.5", "--moveout_window", "3",
                                       "--moveout_min_fold", "6", "--moveout_max_step", "2", "--moveout_interp", "cubic"])
    assert check_moveout(a) == ("scan:off.npy", "cubic")
    assert check_moveout_scan(a) == {"file": "off.npy", "vmin": 1.0, "vmax": 1.8, "nv": 9, "gather": "y", "stretch_mute": 1.5,
                                     "window": 3, "min_fold": 6, "max_step": 2}
    assert check_moveout(parse_arguments(BASE + SCAN + ["--datadim", "2d"])) == ("scan:off.npy", "linear")
    # --moveout_interp goes with either flag; everything that sees a data-domain tensor combines
    assert check_moveout(parse_arguments(BASE + ["--moveout", "tau.npy", "--moveout_interp", "cubic"])) == ("tau.npy", "cubic")
    for extra in (["--holdout", "0.2"], ["--out_ema", "0.9"], ["--optimizer", "sgld"], ["--trace_offsets", "o.npy"], ["--net", "unet"]):
        assert parse_arguments(BASE + SCAN + ["--datadim", "3d"] + extra).moveout_offset == "off.npy"
    with pytest.raises(SystemExit):
        parse_arguments(BASE + SCAN + ["--moveout_gather", "z"])
    with pytest.raises(SystemExit):
        parse_arguments(BASE + ["--moveout_offset", "off.npy", "--moveout_vscan", "1.0", "1.8"])


@pytest.mark.parametrize("argv, flag", [
    (BASE + SCAN + ["--moveout", "tau.npy"], "--moveout_offset.*--moveout"),
    (BASE + ["--moveout_vscan", "1.0", "1.8", "9"], "--moveout_vscan needs --moveout_offset"),
    (BASE + ["--moveout_gather", "x"], "--moveout_gather needs --moveout_offset"),
    (BASE + ["--moveout_gather", "volume"], "--moveout_gather needs --moveout_offset"),
    (BASE + ["--moveout_stretch", "1.5"], "--moveout_stretch needs --moveout_offset"),
    (BASE + ["--moveout_window", "2"], "--moveout_window needs --moveout_offset"),
    (BASE + ["--moveout_min_fold", "4"], "--moveout_min_fold needs --moveout_offset"),
    (BASE + ["--moveout_max_step", "1"], "--moveout_max_step needs --moveout_offset"),
    (BASE + ["--moveout", "tau.npy", "--moveout_stretch", "1.5"], "--moveout_stretch needs --moveout_offset"),
    (BASE + ["--moveout_offset", "off.npy"], "--moveout_offset needs --moveout_vscan"),
    (BASE + ["--moveout_offset", "off.npy", "--moveout_vscan", "0", "1.8", "9"], "--moveout_vscan"),
    (BASE + ["--moveout_offset", "off.npy", "--moveout_vscan", "2.0", "1.8", "9"], "--moveout_vscan"),
    (BASE + ["--moveout_offset", "off.npy", "--moveout_vscan", "1.0", "1.8", "0"], "--moveout_vscan"),
    (BASE + ["--moveout_offset", "off.npy", "--moveout_vscan", "1.0", "1.8", "2.5"], "--moveout_vscan"),
    (BASE + SCAN + ["--moveout_stretch", "0"], "--moveout_stretch"),
    (BASE + SCAN + ["--moveout_window", "-1"], "--moveout_window"),
    (BASE + SCAN + ["--moveout_min_fold", "-1"], "--moveout_min_fold"),
    (BASE + SCAN + ["--moveout_max_step", "-1"], "--moveout_max_step"),
    (BASE + SCAN + ["--datadim", "2d", "--moveout_gather", "x"], "--moveout_gather"),
    # everything --moveout refuses, through the same checks
    (BASE + SCAN + ["--datadim", "2.5d", "--slice", "tx", "--imgchannel", "3"], "--moveout_offset"),
    (BASE + SCAN + ["--datadim", "2.5d", "--slice", "tx", "--imgchannel", "4", "--avo_theta", "0", "10", "20", "30"], "--moveout_offset"),
    (BASE + SCAN + ["--datadim", "3d", "--wavelet", "w.npy"], "--moveout_offset.*--wavelet"),
    (BASE + SCAN + ["--datadim", "3d", "--net", "part"], "--moveout_offset.*--net part"),
    (BASE + SCAN + ["--datadim", "3d", "--data_forgetting_factor", "3"], "--moveout_offset.*--data_forgetting_factor"),
])
def test_flag_refusals(argv, flag):
    with pytest.raises(ValueError, match=flag):
        parse_arguments(argv)


def test_main_pocs_refuses_the_flag():
    from deep_prior_interpolation_amd.main_pocs import Interpolator
    with pytest.raises(ValueError, match="--moveout_offset"):
        Interpolator(parse_arguments(BASE + SCAN + ["--datadim", "3d"]), "/tmp", device="cpu")


def test_net_args_are_same():
    now = parse_arguments(BASE)
    saved = Namespace(**{k: v for k, v in vars(parse_arguments(BASE)).items() if not k.startswith("moveout_") or k == "moveout_interp"})
    assert not hasattr(saved, "moveout_offset") and not hasattr(saved, "moveout_vscan") and not hasattr(saved, "moveout_gather")
    assert net_args_are_same(now, saved) and net_args_are_same(saved, now)            # an old args.txt reads as off
    on = parse_arguments(BASE + SCAN)
    assert net_args_are_same(on, parse_arguments(BASE + SCAN)) and net_args_are_same(on, parse_arguments(BASE + SCAN + ["--moveout_gather", "volume"]))
    assert not net_args_are_same(on, saved) and not net_args_are_same(on, now) and not net_args_are_same(saved, on)
    assert not net_args_are_same(on, parse_arguments(BASE + ["--moveout_offset", "other.npy", "--moveout_vscan", "1.0", "1.8", "9"]))
    assert not net_args_are_same(on, parse_arguments(BASE + ["--moveout_offset", "off.npy", "--moveout_vscan", "1.0", "1.8", "17"]))
    assert not net_args_are_same(on, parse_arguments(BASE + SCAN + ["--datadim", "3d", "--moveout_gather", "x"]))
    assert not net_args_are_same(on, parse_arguments(BASE + SCAN + ["--moveout_stretch", "1.5"]))
    assert not net_args_are_same(on, parse_arguments(BASE + ["--moveout", "off.npy"]))
    # what only tunes the pick does not decide whether weights fit
    assert net_args_are_same(on, parse_arguments(BASE + SCAN + ["--moveout_window", "3", "--moveout_min_fold", "2", "--moveout_max_step", "2"]))


# ---------------------------------------------------------------- data.load_moveout -----------------------------------------------
def _volume(tmp_path, shape, offset, datadim, patch_shape, extra=()):
    rng = np.random.RandomState(0)
    np.save(tmp_path / "vol.npy", rng.standard_normal(shape).astype(np.float32))
    np.save(tmp_path / "msk.npy", (rng.uniform(size=shape) < 0.5).astype(np.float32))
    if offset is not None:
        np.save(tmp_path / "off.npy", offset)
    argv = ["--imgdir", str(tmp_path), "--imgname", "vol.npy", "--maskname", "msk.npy", "--datadim", datadim, "--patch_shape"] + \
        [str(n) for n in patch_shape]
    return parse_arguments(argv + (SCAN if offset is not None else []) + list(extra))


def test_extract_patches_refuses_the_file_before_any_launch(tmp_path, monkeypatch):
    from deep_prior_interpolation_amd.data import extract_patches
    monkeypatch.setattr(_lib, "load", lambda: (_ for _ in ()).throw(AssertionError("reached the library")))
    good = np.ones((9, 7))
    with pytest.raises(ValueError, match="--moveout_offset.*time axis"):
        extract_patches(_volume(tmp_path, (6, 9, 7), good, "3d", (3, 4, 4)))
    for bad, match in ((good[:, :6], "--moveout_offset.*shape"), (good[:8], "--moveout_offset.*shape"), (np.ones((6, 9, 7)), "--moveout_offset.*shape"),
                       (good[0], "--moveout_offset.*shape"), (np.where(np.arange(7) == 3, np.nan, good), "--moveout_offset.*non-finite"),
                       (np.where(np.arange(7) == 3, np.inf, good), "--moveout_offset.*non-finite"), (good.astype(complex), "--moveout_offset.*real")):
        with pytest.raises(ValueError, match=match):
            extract_patches(_volume(tmp_path, (6, 9, 7), bad, "3d", (-1, 4, 4)))
    with pytest.raises(ValueError, match="--moveout_offset"):     # a 3-D volume under --datadim 2d: its last axis is channels
        extract_patches(_volume(tmp_path, (6, 9, 7), good, "2d", (-1, 4, -1)))
    for bad in (np.ones((9, 2)), np.ones((8,)), np.ones((1, 9))):
        with pytest.raises(ValueError, match="--moveout_offset.*shape"):
            extract_patches(_volume(tmp_path, (6, 9), bad, "2d", (-1, 4)))


def test_load_moveout_and_check_moveout_are_unchanged_with_the_flags_off(tmp_path):
    from deep_prior_interpolation_amd.data import extract_patches, load_moveout, patch_extractor_for
    a = _volume(tmp_path, (6, 9, 7), None, "3d", (-1, 4, 4))
    assert check_moveout(a) is None and load_moveout(a, (6, 9, 7)) is None
    assert load_moveout(Namespace(datadim="3d"), (6, 9, 7)) is None                   # a Namespace without the keys
    patches = extract_patches(a)
    assert all("moveout" not in p and "moveout_velocity" not in p for p in patches)
    table = np.arange(6.0)[:, None, None] - np.random.RandomState(1).uniform(0, 2, (1, 9, 7))
    np.save(tmp_path / "tau.npy", table)
    b = parse_arguments(["--imgdir", str(tmp_path), "--imgname", "vol.npy", "--maskname", "msk.npy", "--datadim", "3d", "--patch_shape", "-1", "4",
                         "4", "--moveout", "tau.npy"])
    assert check_moveout(b) == ("tau.npy", "linear")
    pe = patch_extractor_for((6, 9, 7), b.patch_shape, b.patch_stride, b.datadim, b.imgchannel)
    got = load_moveout(b, (6, 9, 7), pe)
    assert got.dtype == np.float32 and np.array_equal(got, table.astype(np.float32))
    assert np.array_equal(load_moveout(b, (6, 9, 7)), got)                            # the two-argument call of before
    assert all("moveout" in p and "moveout_velocity" not in p for p in extract_patches(b))


def test_the_result_file_names_the_law_and_the_scan(tmp_path):
    """A patch dict as extract_patches builds it under --moveout_offset, through the Interpolator on the host (a skipped patch)."""
    from deep_prior_interpolation_amd.main import Interpolator
    a = parse_arguments(["--imgdir", str(tmp_path), "--datadim", "3d"] + SCAN)
    T = Interpolator(a, str(tmp_path), device="cpu")
    assert T.forward_model.flags["moveout"] == ("scan:off.npy", "linear") and T.forward_model.stage("moveout") is not None
    rng = np.random.RandomState(2)
    img, mask = rng.standard_normal((6, 5, 4, 1)), np.ones((6, 5, 4, 1))
    law = np.linspace(1.0, 1.8, 6)
    assert T.load_data({"image": img, "mask": mask, "name": "1", "moveout": np.full((6, 5, 4), -1.0), "moveout_velocity": law}) == 0.0
    T.out_best, T.elapsed = T.img * T.mask, 0.0
    T.save_result()
    run = np.load(tmp_path / "1_run.npy", allow_pickle=True).item()
    assert np.array_equal(run["moveout_velocity"], law) and run["moveout_vscan"] == [1.0, 1.8, 9.0]
    assert run["moveout_interp"] == "linear" and run["moveout_model"] is None and run["moveout"].shape == (6, 5, 4)
    # a run of --moveout on a file gains neither key
    b = parse_arguments(["--imgdir", str(tmp_path), "--datadim", "3d", "--moveout", "tau.npy"])
    T = Interpolator(b, str(tmp_path), device="cpu")
    T.load_data({"image": img, "mask": mask, "name": "2", "moveout": np.full((6, 5, 4), -1.0)})
    T.out_best, T.elapsed = T.img * T.mask, 0.0
    T.save_result()
    run = np.load(tmp_path / "2_run.npy", allow_pickle=True).item()
    assert "moveout" in run and "moveout_velocity" not in run and "moveout_vscan" not in run


# ---------------------------------------------------------------- ABI -------------------------------------------------------------
def test_abi_table_header_exports_and_makefile_name_the_entry_point():
    assert _lib.ABI_VERSION == 406
    I, P, Z, D = C.c_int, C.c_void_p, C.c_size_t, C.c_double
    assert _lib.SIGNATURES["dpi_semblance_sums"] == (I, [P, P, P, P, I, D, I, Z, I, Z, I, Z, P, P, P, P])
    h = " ".join(open(os.path.join(ROOT, "include", "dpi_hip.h")).read().split())
    assert ("int dpi_semblance_sums(const float* d, const float* mask, const double* offset, const double* vel, int NV, double stretch, int T, "
            "size_t S, int n_groups, size_t group_stride, int n_traces, size_t trace_stride, double* num, double* den, int* cnt, void* stream);") in h
    assert "semblance.hip" in open(os.path.join(ROOT, "deep_prior_interpolation_amd", "csrc", "Makefile")).read()
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    exported = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    assert " T dpi_semblance_sums\n" in exported
    assert _lib.load().dpi_version() == 406
