"""--moveout_smooth and --moveout_table without a GPU: smooth_law and its refusals, the smoothed law on one analytic event, the mechanism (a
smoothed law gives a table at most half as rough), the flags, old checkpoints, what stays as it was with the flags off, the ABI table, and
the scalar restatement of dpi_nmo_table against operators.nmo_table on the cases the GPU test runs."""
import ctypes as C
import os
import subprocess
from argparse import Namespace

import numpy as np
import pytest

from conftest import ROOT

import nmo_table_cases as N
import velocity_cases as V
from deep_prior_interpolation_amd import _lib
from deep_prior_interpolation_amd.operators import (check_moveout_table, nmo_table, nmo_table_device, pick_velocity, scan_table,
                                                    smooth_law, velocity as mod)
from deep_prior_interpolation_amd.parameter import check_moveout, check_moveout_scan, net_args_are_same, parse_arguments

BASE = ["--imgdir", "x"]
SCAN = ["--moveout_offset", "off.npy", "--moveout_vscan", "1.0", "1.8", "9"]


# ---------------------------------------------------------------- smooth_law ------------------------------------------------------
def _written_out(v, w, L):
    K = int(np.ceil(3 * L))
    T = len(v)
    out = np.empty(T)
    for tau in range(T):
        num = den = plain = norm = 0.0
        for k in range(-K, K + 1):
            r = tau + k
            if 0 <= r <= T - 1:
                g = np.exp(-0.5 * (k / L) ** 2)
                num += g * w[r] * v[r]
                den += g * w[r]
                plain += g * v[r]
                norm += g
        out[tau] = num / den if den != 0 else plain / norm
    return out


def test_smooth_law_length_zero_and_the_written_out_loop():
    rng = np.random.RandomState(0)
    v, w = 1.0 + rng.rand(2, 9), rng.rand(2, 9)
    w[1, 3:6] = 0.0
    assert np.array_equal(smooth_law(v, w, 0), v) and np.array_equal(smooth_law(v, w, 0.0), v)
    for L in (0.5, 1.0, 2.5, 40.0):                                # K = 2, 3, 8 and beyond the ends
        got = smooth_law(v, w, L)
        assert got.shape == v.shape and got.dtype == np.float64
        for g in range(2):
            assert np.array_equal(got[g], _written_out(v[g], w[g], L)), L
    lone = smooth_law(np.array([[1.5]]), np.array([[0.0]]), 3.0)   # T = 1, no weight: the value itself
    assert lone.shape == (1, 1) and lone[0, 0] == 1.5


def test_smooth_law_keeps_a_constant_and_stays_inside_the_range_of_its_input():
    rng = np.random.RandomState(1)
    T = 40
    for L in (1.0, 4.0, 12.0):
        K = int(np.ceil(3 * L))
        eps = (2 * K + 1) * 2.0 ** -52
        w = rng.rand(3, T)
        w[2] = 0.0                                               # the unweighted fall-back keeps both properties too
        const = smooth_law(np.full((3, T), 1.37), w, L)
        assert np.all(np.abs(const - 1.37) <= eps * 1.37), L
        v = 1.0 + rng.rand(3, T)
        got = smooth_law(v, w, L)
        lo, hi = v.min(axis=1, keepdims=True), v.max(axis=1, keepdims=True)
        assert np.all(got >= lo * (1 - eps)) and np.all(got <= hi * (1 + eps)), L


def test_smooth_law_with_all_weight_on_one_row():
    T, row, L = 30, 11, 2.0
    K = 6
    v = np.linspace(1.0, 2.0, T)[None]
    w = np.zeros((1, T))
    w[0, row] = 0.7
    got = smooth_law(v, w, L)[0]
    near = np.abs(np.arange(T) - row) <= K
    assert np.all(np.abs(got[near] - v[0, row]) <= 2.0 ** -52 * v[0, row])          # g w v / (g w): two roundings
    plain = smooth_law(v, np.zeros((1, T)), L)[0]
    assert np.array_equal(got[~near], plain[~near]) and not np.array_equal(got[near], plain[near])
    assert np.array_equal(plain, _written_out(v[0], np.zeros(T), L))


def test_smooth_law_refusals():
    v, w = np.ones((2, 5)), np.ones((2, 5))
    for bad_w in (np.ones((2, 4)), np.ones(5), np.ones((1, 2, 5))):
        with pytest.raises(ValueError, match="shape"):
            smooth_law(v, bad_w, 1.0)
    with pytest.raises(ValueError, match="shape"):
        smooth_law(np.ones(5), np.ones(5), 1.0)
    for bad in (-1.0, np.nan, np.inf):
        with pytest.raises(ValueError, match="weight"):
            smooth_law(v, np.where(np.arange(5) == 2, bad, w), 1.0)
    for bad in (-0.5, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="length"):
            smooth_law(v, w, bad)


def test_pick_velocity_returns_its_path_on_request():
    rng = np.random.RandomState(2)
    P, vel = rng.rand(3, 12, 5), np.linspace(1.0, 2.0, 5)
    law = pick_velocity(P, vel, max_step=1)
    assert isinstance(law, np.ndarray) and law.shape == (3, 12)
    law2, path = pick_velocity(P, vel, max_step=1, return_index=True)
    assert np.array_equal(law, law2) and path.shape == (3, 12) and path.dtype == np.int64 and np.array_equal(vel[path], law)


# ---------------------------------------------------------------- one event -------------------------------------------------------
@pytest.mark.parametrize("L", [2.0, 4.0])
@pytest.mark.parametrize("tau0, index", V.EVENTS)
def test_the_smoothed_law_stays_on_the_event(tau0, index, L, monkeypatch):
    shape = (64, 16, 16)
    d, off = V.event_gather(shape, tau0, index)
    monkeypatch.setattr(mod, "semblance_sums", N.sums64_as_semblance_sums)
    res = scan_table(d, np.ones(shape), off, 1.0, 1.8, 17, smooth=L)
    assert np.array_equal(res["pick"], V.event_pick(shape, tau0, index, "full", None))
    err = abs(res["velocity"][0, tau0] - V.EVENT_VELOCITIES[index])
    print("tau0 %d L %g: smoothed law off by %.4f" % (tau0, L, err))
    assert err <= 0.05
    raw = scan_table(d, np.ones(shape), off, 1.0, 1.8, 17)
    assert np.array_equal(raw["velocity"], raw["pick"]) and np.array_equal(raw["pick"], res["pick"])
    assert np.array_equal(raw["table"], nmo_table(shape, off, raw["pick"][0]))        # smooth = 0: today's bits
    path = pick_velocity(res["panel"], res["velocities"], return_index=True)[1]
    weight = np.take_along_axis(res["panel"], path[:, :, None], axis=2)[:, :, 0]
    assert np.array_equal(res["velocity"], smooth_law(res["pick"], weight, L))
    assert np.array_equal(res["table"], nmo_table(shape, off, res["velocity"][0]))


# ---------------------------------------------------------------- the mechanism ---------------------------------------------------
@pytest.mark.parametrize("mask_kind", ["random", "regular"])
def test_a_smoothed_law_gives_a_table_at_most_half_as_rough(mask_kind, monkeypatch):
    data, known, off, mean = N.standin(mask_kind)
    monkeypatch.setattr(mod, "semblance_sums", N.sums64_as_semblance_sums)
    kw = dict(gather="volume", window=2, min_fold=4, max_step=1)
    raw = scan_table(data, known, off, *N.STANDIN_VSCAN, **kw)
    smooth = scan_table(data, known, off, *N.STANDIN_VSCAN, smooth=4.0, **kw)
    assert np.array_equal(raw["pick"], smooth["pick"]) and np.array_equal(raw["velocity"], raw["pick"])
    r0, r4, rm = N.roughness(raw["table"]), N.roughness(smooth["table"]), N.roughness(mean)
    region = (mean >= 0) & (mean <= mean.shape[0] - 1)
    live = lambda t: (t >= 0) & (t <= t.shape[0] - 1)
    share0, share4 = (live(raw["table"]) & region).sum(), (live(smooth["table"]) & region).sum()
    print("%s: mean |d2 tau / dt2| %.3f as picked, %.3f smoothed over 4 rows, %.3f for the mean law; live in the mean law's region %.3f / %.3f"
          % (mask_kind, r0, r4, rm, share0 / region.sum(), share4 / region.sum()))
    assert r4 <= 0.5 * r0
    check_moveout_table(smooth["table"])
    assert share4 >= share0


# ---------------------------------------------------------------- flags -----------------------------------------------------------
def test_flags_parse_and_reach_the_scan():
    off = parse_arguments(BASE)
    assert off.moveout_smooth is None and off.moveout_table is None and check_moveout_scan(off) is None
    plain = check_moveout_scan(parse_arguments(BASE + SCAN))
    assert "smooth" not in plain and "table" not in plain
    for extra in (["--moveout_smooth", "0"], ["--moveout_table", "host"], ["--moveout_smooth", "0.0", "--moveout_table", "host"]):
        assert check_moveout_scan(parse_arguments(BASE + SCAN + extra)) == plain, extra         # the defaults spelled out: today's path
    a = parse_arguments(BASE + SCAN + ["--moveout_smooth", "4", "--moveout_table", "device", "--datadim", "3d"])
    assert a.moveout_smooth == 4.0 and a.moveout_table == "device"
    assert check_moveout_scan(a) == dict(plain, smooth=4.0, table="device") and check_moveout(a) == ("scan:off.npy", "linear")
    assert check_moveout_scan(parse_arguments(BASE + SCAN + ["--moveout_smooth", "2.5"])) == dict(plain, smooth=2.5)
    with pytest.raises(SystemExit):
        parse_arguments(BASE + SCAN + ["--moveout_table", "gpu"])


@pytest.mark.parametrize("argv, flag", [
    (BASE + ["--moveout_smooth", "4"], "--moveout_smooth needs --moveout_offset"),
    (BASE + ["--moveout_smooth", "0"], "--moveout_smooth needs --moveout_offset"),
    (BASE + ["--moveout", "tau.npy", "--moveout_smooth", "4"], "--moveout_smooth needs --moveout_offset"),
    (BASE + ["--moveout_table", "device"], "--moveout_table needs --moveout_offset"),
    (BASE + ["--moveout_table", "host"], "--moveout_table needs --moveout_offset"),
    (BASE + ["--moveout", "tau.npy", "--moveout_table", "device"], "--moveout_table needs --moveout_offset"),
    (BASE + SCAN + ["--moveout_smooth", "-1"], "--moveout_smooth"),
    (BASE + SCAN + ["--moveout_smooth", "nan"], "--moveout_smooth"),
    (BASE + SCAN + ["--moveout_smooth", "inf"], "--moveout_smooth"),
])
def test_flag_refusals(argv, flag):
    with pytest.raises(ValueError, match=flag):
        parse_arguments(argv)


def test_a_namespace_with_an_unknown_builder_is_refused():
    a = parse_arguments(BASE + SCAN)
    a.moveout_table = "gpu"
    with pytest.raises(ValueError, match="--moveout_table"):
        check_moveout_scan(a)


def test_main_pocs_keeps_refusing():
    from deep_prior_interpolation_amd.main_pocs import Interpolator
    with pytest.raises(ValueError, match="--moveout_offset"):
        Interpolator(parse_arguments(BASE + SCAN + ["--datadim", "3d", "--moveout_smooth", "4", "--moveout_table", "device"]), "/tmp", device="cpu")


def test_net_args_are_same():
    on = parse_arguments(BASE + SCAN)
    saved = Namespace(**{k: v for k, v in vars(on).items() if k not in ("moveout_smooth", "moveout_table")})       # an args.txt of before
    assert not hasattr(saved, "moveout_smooth") and not hasattr(saved, "moveout_table")
    assert net_args_are_same(on, saved) and net_args_are_same(saved, on)
    for same in (["--moveout_smooth", "0"], ["--moveout_table", "host"]):
        assert net_args_are_same(parse_arguments(BASE + SCAN + same), saved) and net_args_are_same(saved, parse_arguments(BASE + SCAN + same))
    smooth, device = parse_arguments(BASE + SCAN + ["--moveout_smooth", "4"]), parse_arguments(BASE + SCAN + ["--moveout_table", "device"])
    for other in (smooth, device):
        assert not net_args_are_same(other, saved) and not net_args_are_same(saved, other) and not net_args_are_same(other, on)
        assert net_args_are_same(other, Namespace(**vars(other)))
    assert not net_args_are_same(smooth, parse_arguments(BASE + SCAN + ["--moveout_smooth", "8"]))
    assert net_args_are_same(smooth, parse_arguments(BASE + SCAN + ["--moveout_smooth", "4.0", "--moveout_table", "host"]))


def test_scan_table_and_nmo_table_device_refuse_before_any_launch(monkeypatch):
    """None of these reaches the library: loading it is made an error."""
    monkeypatch.setattr(_lib, "load", lambda: (_ for _ in ()).throw(AssertionError("reached the library")))
    d, m, off = np.zeros((8, 4, 3), np.float32), np.ones((8, 4, 3), np.float32), np.ones((4, 3))
    for kw, match in ((dict(smooth=-1.0), "smooth"), (dict(smooth=float("nan")), "smooth"), (dict(smooth=float("inf")), "smooth"),
                      (dict(table="gpu"), "table")):
        with pytest.raises(ValueError, match=match):
            scan_table(d, m, off, 1.0, 2.0, 3, **kw)
    law = np.ones((1, 8))
    for args, kw, match in ((((8, 4, 3), off[:, :2], law), {}, "offset"), (((8,), off, law), {}, "shape"),
                            (((8, 4, 3), np.where(off > 0, np.nan, off), law), {}, "non-finite"),
                            (((8, 4, 3), off, law), dict(stretch_mute=0.0), "stretch_mute"), (((8, 4, 3), off, law), dict(stretch_mute=-1.0), "stretch_mute"),
                            (((8, 4, 3), off, law[:, :7]), {}, "velocity"), (((8, 4, 3), off, np.ones((4, 8))), {}, "velocity"),
                            (((8, 4, 3), off, np.ones((3, 8))), dict(gather="x"), "velocity"), (((8, 4, 3), off, law), dict(gather="z"), "gather"),
                            (((8, 4), off[:, 0], law), dict(gather="y"), "section"),
                            (((8, 4, 3), off, np.where(np.arange(8) == 3, 0.0, law)), {}, "velocity must be finite and > 0"),
                            (((8, 4, 3), off, np.where(np.arange(8) == 3, -1.0, law)), {}, "velocity must be finite and > 0"),
                            (((8, 4, 3), off, np.where(np.arange(8) == 3, np.nan, law)), {}, "velocity must be finite and > 0"),
                            (((8, 4, 3), off, np.where(np.arange(8) == 3, np.inf, law)), {}, "velocity must be finite and > 0")):
        with pytest.raises(ValueError, match=match):
            nmo_table_device(*args, **kw)
    with pytest.raises(ValueError, match=r"--moveout_table.*host"):                # more rows than the kernel keeps on chip
        nmo_table_device((4097, 2), np.ones(2), np.ones(4097))


# ---------------------------------------------------------------- the result file -------------------------------------------------
def _saved_run(tmp_path, name, extra, patch):
    from deep_prior_interpolation_amd.main import Interpolator
    a = parse_arguments(["--imgdir", str(tmp_path), "--datadim", "3d"] + SCAN + extra)
    T = Interpolator(a, str(tmp_path), device="cpu")
    rng = np.random.RandomState(2)
    img, mask = rng.standard_normal((6, 5, 4, 1)), np.ones((6, 5, 4, 1))
    assert T.load_data(dict({"image": img, "mask": mask, "name": name, "moveout": np.full((6, 5, 4), -1.0)}, **patch)) == 0.0
    T.out_best, T.elapsed = T.img * T.mask, 0.0
    T.save_result()
    return np.load(tmp_path / (name + "_run.npy"), allow_pickle=True).item()


def test_the_result_file_gains_its_keys_only_with_the_flags(tmp_path):
    law, pick = np.linspace(1.0, 1.8, 6), np.array([1.0, 1.0, 1.2, 1.4, 1.8, 1.8])
    plain = _saved_run(tmp_path, "1", [], {"moveout_velocity": pick})
    assert "moveout_velocity" in plain and not {"moveout_smooth", "moveout_pick", "moveout_table"} & set(plain)
    spelled = _saved_run(tmp_path, "2", ["--moveout_smooth", "0", "--moveout_table", "host"], {"moveout_velocity": pick})
    assert set(spelled) == set(plain)
    both = _saved_run(tmp_path, "3", ["--moveout_smooth", "4", "--moveout_table", "device"], {"moveout_velocity": law, "moveout_pick": pick})
    assert set(both) == set(plain) | {"moveout_smooth", "moveout_pick", "moveout_table"}
    assert both["moveout_smooth"] == 4.0 and both["moveout_table"] == "device"
    assert np.array_equal(both["moveout_pick"], pick) and np.array_equal(both["moveout_velocity"], law)
    only = _saved_run(tmp_path, "4", ["--moveout_table", "device"], {"moveout_velocity": pick})
    assert set(only) == set(plain) | {"moveout_table"}


def test_extract_patches_passes_the_flags_and_hands_out_the_pick(tmp_path, monkeypatch):
    from deep_prior_interpolation_amd.data import extract_patches
    shape = (16, 8, 6)
    rng = np.random.RandomState(0)
    vol = rng.standard_normal(shape).astype(np.float32)
    np.save(tmp_path / "vol.npy", vol)
    np.save(tmp_path / "msk.npy", np.where(rng.rand(1, 8, 6) < 0.7, vol, np.nan))
    np.save(tmp_path / "off.npy", 16 * np.sqrt((np.arange(8)[:, None] / 8) ** 2 + (np.arange(6)[None] / 6) ** 2))
    monkeypatch.setattr(mod, "semblance_sums", N.sums64_as_semblance_sums)
    seen = []
    real = mod.scan_table
    monkeypatch.setattr(mod, "scan_table", lambda *a, **kw: seen.append(kw) or real(*a, **dict(kw, table="host")))
    argv = ["--imgdir", str(tmp_path), "--imgname", "vol.npy", "--maskname", "msk.npy", "--datadim", "3d", "--patch_shape", "-1", "4", "6",
            "--moveout_min_fold", "2"] + SCAN
    plain = extract_patches(parse_arguments(argv))
    assert seen[-1]["smooth"] == 0.0 and seen[-1]["table"] == "host"
    assert all(set(p) == {"image", "mask", "name", "moveout", "moveout_velocity"} for p in plain)           # the keys of before
    smooth = extract_patches(parse_arguments(argv + ["--moveout_smooth", "3", "--moveout_table", "device", "--moveout_gather", "x"]))
    assert seen[-1]["smooth"] == 3.0 and seen[-1]["table"] == "device"
    assert len(smooth) == 2 and all(set(p) == {"image", "mask", "name", "moveout", "moveout_velocity", "moveout_pick"} for p in smooth)
    for p in smooth:
        assert p["moveout_pick"].shape == p["moveout_velocity"].shape == (16, 4)
        assert np.isin(p["moveout_pick"], np.linspace(1.0, 1.8, 9)).all() and not np.array_equal(p["moveout_pick"], p["moveout_velocity"])


# ---------------------------------------------------------------- the kernel's statement and the ABI ------------------------------
def test_every_case_of_the_gpu_test_finds_a_seed_and_is_not_empty():
    some_live = some_muted = 0
    for c in N.FLAT:
        k = N.flat_case(*c)
        assert k["margin"] >= N.MARGIN and k["slope"] >= N.MIN_SLOPE and np.isfinite(k["bar"]).all(), c
        live = k["ref"] != -1.0
        some_live += live.any()
        some_muted += (~live).any()
        if c[2] == "far":
            assert not live.any()
        if c[2] == "zero":                                       # tau == t exactly
            assert np.array_equal(k["ref"], np.broadcast_to(np.arange(c[0], dtype=np.float64)[:, None], k["ref"].shape))
        if c[2] == "inversion" and c[0] >= 33 and c[1] > 1:      # the branch starts after the drop: rows live under the constant law are muted
            assert (~live[:, k["offset"] < 1.2 * c[0]]).any()
    assert some_live > len(N.FLAT) // 2 and some_muted > len(N.FLAT) // 2
    for v in N.VOLUMES:
        for gather in ("volume", "x", "y"):
            k = N.volume_case(*v, gather)
            assert k["margin"] >= N.MARGIN and k["slope"] >= N.MIN_SLOPE, (v, gather)
            assert k["laws"].shape[0] == {"volume": 1, "x": v[1], "y": v[2]}[gather]


@pytest.mark.parametrize("T, S, law, stretch", [c for c in N.FLAT if c[0] <= 33 and c[1] != 63], ids=[i for c, i in zip(N.FLAT, N.FLAT_IDS) if c[0] <= 33 and c[1] != 63])
def test_the_kernels_statement_gives_the_hosts_bits(T, S, law, stretch):
    """What dpi_nmo_table is written to (include/dpi_hip.h), as a scalar loop over a few traces of every case: the bits of nmo_table, so
    the two can differ on the device only in how a square root or a division rounds."""
    c = N.flat_case(T, S, law, stretch)
    off = c["offset"].reshape(-1)
    for s in sorted(set(range(0, S, 7)) | {S // 2, S - 1}):
        assert np.array_equal(N.rows64(c["laws"][0], off[s], stretch, T), c["ref"][:, s]), s


def test_abi_table_header_exports_and_makefile_name_the_entry_point():
    I, P, D = C.c_int, C.c_void_p, C.c_double
    assert _lib.SIGNATURES["dpi_nmo_table"] == (I, [P, P, D, I, I, I, I, I, I, P, P])
    h = " ".join(open(os.path.join(ROOT, "include", "dpi_hip.h")).read().split())
    assert ("int dpi_nmo_table(const double* law, const double* offset, double stretch, int T, int S, int n_groups, int group_stride, "
            "int n_traces, int trace_stride, double* table, void* stream);") in h
    make = open(os.path.join(ROOT, "deep_prior_interpolation_amd", "csrc", "Makefile")).read()
    srcs = next(line for line in make.splitlines() if line.startswith("SRCS :="))
    assert "nmo_table.hip" in srcs.split()                       # the one list the library and the sanitizer build both take
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    exported = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    assert " T dpi_nmo_table\n" in exported
