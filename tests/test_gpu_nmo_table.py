"""--moveout_table device and --moveout_smooth on the GPU: dpi_nmo_table against operators.nmo_table on the cases of tests/nmo_table_cases.py
(equal live maps, live samples within the bar derived there), inside guard bands, on aligned and one-double-offset views; repeatability;
the refusals; scan_table(table="device"); and the deep-prior loop on a smoothed, device-built table against the same run on that table
read from a file."""
import os

import numpy as np
import pytest
import torch

import nmo_table_cases as N
import velocity_cases as V
from gpu_guard import guard
from deep_prior_interpolation_amd import _lib, utils as u
from deep_prior_interpolation_amd.operators import check_moveout_table, gather_geometry, nmo_table, nmo_table_device, scan_table

pytestmark = pytest.mark.gpu
DEV = "cuda"


class Launch:
    """The inputs and the output of one call in guard bands, `shift` doubles behind a 256-byte boundary."""

    def __init__(self, c, shift=0):
        self.T = c["shape"][0]
        self.S = int(np.prod(c["shape"][1:]))
        self.geo = gather_geometry(c["shape"], c["gather"])
        self.stretch = 0.0 if c["stretch"] is None else float(c["stretch"])
        self.src = {"law": torch.from_numpy(c["laws"].copy()).reshape(-1), "offset": torch.from_numpy(c["offset"].copy()).reshape(-1)}
        self.g = {"law": guard(c["laws"].size, torch.float64, DEV, fill=self.src["law"], offset=shift),
                  "offset": guard(self.S, torch.float64, DEV, fill=self.src["offset"], offset=(3 * shift) % 2),
                  "table": guard(self.T * self.S, torch.float64, DEV, offset=shift)}
        assert self.g["table"].payload.data_ptr() % 16 == 8 * shift

    def run(self, T=None):
        p = {k: _lib.ptr(g.payload) for k, g in self.g.items()}
        code = _lib.load().dpi_nmo_table(p["law"], p["offset"], self.stretch, self.T if T is None else T, self.S, self.geo[0], self.geo[1],
                                         self.geo[2], self.geo[3], p["table"], _lib.stream())
        torch.cuda.synchronize()
        return code

    def out(self, shape):
        return self.g["table"].payload.cpu().numpy().reshape(shape)

    def check(self, what):
        for k, g in self.g.items():
            g.check("%s: %s" % (what, k))
        for k, want in self.src.items():                         # the inputs are read only
            assert torch.equal(self.g[k].payload.cpu().reshape(-1), want), "%s: %s changed" % (what, k)


def _run_case(c, shift, what):
    L = Launch(c, shift)
    assert L.run() == 0, _lib.load().dpi_last_error()
    L.check(what)
    got = L.out(c["shape"])
    assert not np.isnan(got).any(), "%s: %d elements were not written" % (what, int(np.isnan(got).sum()))       # the payload starts as NaN
    return got, N.compare(got, c, what)


# ---------------------------------------------------------------- the entry point -------------------------------------------------
@pytest.mark.parametrize("shift", [0, 1], ids=["aligned", "plus8bytes"])
@pytest.mark.parametrize("T, S, law, stretch", N.FLAT, ids=N.FLAT_IDS)
def test_one_gather_against_the_host(T, S, law, stretch, shift):
    c = N.flat_case(T, S, law, stretch)
    got, _ = _run_case(c, shift, "T%d S%d %s %s +%d" % (T, S, law, stretch, 8 * shift))
    if law == "far":
        assert np.array_equal(got, np.full(c["shape"], -1.0))
    if law == "zero":
        assert np.array_equal(got, np.broadcast_to(np.arange(T, dtype=np.float64)[:, None], c["shape"]))
    # the wrapper gives the bits of the ctypes path
    assert np.array_equal(nmo_table_device(c["shape"], c["offset"], c["laws"], stretch_mute=stretch, device=DEV), got)


@pytest.mark.parametrize("gather", ["volume", "x", "y"])
@pytest.mark.parametrize("T, X, Y, stretch", N.VOLUMES, ids=N.VOLUME_IDS)
def test_the_three_layouts_against_the_host(T, X, Y, stretch, gather):
    c = N.volume_case(T, X, Y, stretch, gather)
    for shift in (0, 1):
        got, _ = _run_case(c, shift, "T%d X%d Y%d %s %s +%d" % (T, X, Y, stretch, gather, 8 * shift))
    assert np.array_equal(nmo_table_device(c["shape"], c["offset"], c["laws"], gather=gather, stretch_mute=stretch, device=DEV), got)


@pytest.mark.parametrize("T, S, law, stretch", [(257, 65, "inversion", 1.5), (33, 63, "staircase", None), (2, 65, "rising", None)])
def test_two_launches_give_the_same_bits_on_every_view(T, S, law, stretch):
    c = N.flat_case(T, S, law, stretch)
    first = None
    for shift in (0, 0, 1):
        L = Launch(c, shift)
        assert L.run() == 0
        got = L.out(c["shape"]).copy()
        assert L.run() == 0                                      # once more into the same buffer
        L.check("+%d, again" % (8 * shift))
        first = got if first is None else first
        assert np.array_equal(first, got) and np.array_equal(first, L.out(c["shape"]))


def test_more_rows_than_the_kernel_holds_and_other_bad_arguments_are_refused_before_any_launch():
    """Error returns only: every call below is refused by the argument checks, and the output keeps its bits."""
    lib = _lib.load()
    T, S = 4097, 2
    law, off = torch.ones(T, dtype=torch.float64, device=DEV), torch.zeros(S, dtype=torch.float64, device=DEV)        # zero offsets: tau = t exactly
    tab = guard(T * S, torch.float64, DEV)
    bits = tab.bits()
    P = _lib.ptr
    assert lib.dpi_nmo_table(P(law), P(off), 0.0, T, S, 1, 0, S, 1, P(tab.payload), _lib.stream()) != 0
    assert b"4096" in lib.dpi_last_error() and b"nmo_table" in lib.dpi_last_error()
    with pytest.raises(ValueError, match=r"--moveout_table.*host"):
        nmo_table_device((T, S), np.ones(S), np.ones(T), device=DEV)
    # (law, offset, stretch, T, S, n_groups, group_stride, n_traces, trace_stride, table, stream)
    good = (P(law), P(off), 0.0, 8, 2, 1, 0, 2, 1, P(tab.payload), _lib.stream())
    bad = [(0, None), (1, None), (9, None), (9, P(law)), (9, P(off)), (2, -1.0), (2, float("nan")), (2, float("inf")), (3, 0), (3, -1), (4, 0), (4, -2),
           (5, 0), (7, 0), (7, -1), (7, 3), (8, 2), (8, 0), (8, -1), (5, 2), (6, -1)]
    for i, v in bad:
        args = list(good)
        args[i] = v
        assert lib.dpi_nmo_table(*args) != 0, (i, v)
        assert b"nmo_table" in lib.dpi_last_error(), (i, v)
    for geo in ((2, 1, 2, 1), (2, 2, 1, 1), (1, 0, 2, 2), (2, 1 << 30, 1, 1), (2, 1, 2, (1 << 31) - 1)):      # gathers reaching past S = 2
        args = list(good)
        args[5:9] = geo
        assert lib.dpi_nmo_table(*args) != 0, geo
        assert b"reach past" in lib.dpi_last_error(), geo
    torch.cuda.synchronize()
    assert tab.untouched(bits)
    tab.check("refused launches")
    args = list(good)
    args[5:9] = (2, 1, 1, 0)                                     # two gathers of one trace each: exactly the two columns
    law2 = torch.ones(16, dtype=torch.float64, device=DEV)
    args[0] = P(law2)
    assert lib.dpi_nmo_table(*args) == 0
    torch.cuda.synchronize()
    tab.check("an accepted launch")
    want = nmo_table((8, 2), np.zeros(2), np.ones(8))
    assert np.array_equal(tab.payload[:16].cpu().numpy().reshape(8, 2), want) and tab.untouched(bits) is False
    assert torch.isnan(tab.payload[16:]).all()


# ---------------------------------------------------------------- scan_table ------------------------------------------------------
@pytest.mark.parametrize("smooth", [0.0, 4.0], ids=["pick", "smooth4"])
def test_scan_table_builds_the_table_of_one_event_on_the_device(smooth):
    shape = (64, 16, 16)
    for (tau0, index), stretch in zip(V.EVENTS, (None, 1.5, None)):
        d, off = V.event_gather(shape, tau0, index)
        kw = dict(gather="volume", window=2, min_fold=4, max_step=1, stretch_mute=stretch, device=DEV, smooth=smooth)
        host = scan_table(d, np.ones(shape), off, 1.0, 1.8, 17, table="host", **kw)
        dev = scan_table(d, np.ones(shape), off, 1.0, 1.8, 17, table="device", **kw)
        for k in ("velocity", "pick", "panel", "velocities"):
            assert np.array_equal(host[k], dev[k]), k
        assert np.array_equal(dev["pick"], V.event_pick(shape, tau0, index, "full", stretch))
        assert (smooth > 0) != np.array_equal(dev["velocity"], dev["pick"])
        check_moveout_table(dev["table"])
        law = host["velocity"][0]
        bar = N.decisions(law, off.reshape(-1), stretch, host["table"].reshape(shape[0], -1))[1]
        c = dict(ref=host["table"], bar=bar.reshape(shape), offset=off)
        N.compare(dev["table"], c, "event %d, smooth %g" % (tau0, smooth))
    # per gather: every slice from its own law
    d2, _ = V.event_gather(shape, 32, 12)
    data = np.where(np.arange(16).reshape(1, 16, 1) < 8, d, d2)
    host = scan_table(data, np.ones(shape), off, 1.0, 1.8, 17, gather="x", device=DEV, smooth=smooth)
    dev = scan_table(data, np.ones(shape), off, 1.0, 1.8, 17, gather="x", device=DEV, smooth=smooth, table="device")
    assert np.array_equal(host["velocity"], dev["velocity"]) and dev["velocity"].shape == (16, 64)
    bars = [N.decisions(host["velocity"][g], off[g], None, host["table"][:, g])[1] for g in range(16)]
    N.compare(dev["table"], dict(ref=host["table"], bar=np.stack(bars, axis=1), offset=off), "gather x, smooth %g" % smooth)


# ---------------------------------------------------------------- the run ---------------------------------------------------------
FLAGS = ["--datadim", "3d", "--upsample", "linear", "--filters", "4", "8", "--skip", "4", "--inputdepth", "8", "--gain", "40", "--epochs", "4", "--gpu", "0",
         "--imgname", "vol.npy", "--maskname", "msk.npy"]
SCAN = ["--moveout_offset", "off.npy", "--moveout_vscan", "1.0", "1.8", "9"]


def _files(folder, shape):
    os.makedirs(folder, exist_ok=True)
    vol = u.hyperbolic_volume(shape, seed=3)
    known = np.broadcast_to(u.random_trace_mask(shape, 0.5, seed=4), shape) > 0
    np.save(os.path.join(folder, "vol.npy"), vol)
    np.save(os.path.join(folder, "msk.npy"), np.where(known, vol, np.nan))
    T, X, Y = shape
    off = T * np.sqrt((np.arange(X)[:, None] / X) ** 2 + (np.arange(Y)[None, :] / Y) ** 2)
    np.save(os.path.join(folder, "off.npy"), off)
    return vol, known, off


def _optimise(a, patch, out):
    from deep_prior_interpolation_amd.main import Interpolator
    os.makedirs(out)
    T = Interpolator(a, str(out))
    assert T.load_data(patch) > 0
    T.begin_patch(0)
    T.build_model()
    T.build_input()
    T.optimize(verbose=False, mode="eager", check_every=2)
    T.save_result()
    run = np.load(os.path.join(str(out), patch["name"] + "_run.npy"), allow_pickle=True).item()
    h = T.history
    return [np.array(c) for c in (h.loss, h.snr, h.pcorr, h.lr)], run


def test_a_smoothed_device_built_run_is_the_run_on_the_table_it_built(tmp_path):
    """--moveout_offset --moveout_smooth 4 --moveout_table device, then --moveout on the table that run built, written to a file: the same
    histories and output bit for bit; the file of the first names the length, the staircase and the builder."""
    from deep_prior_interpolation_amd.data import extract_patches
    from deep_prior_interpolation_amd.parameter import parse_arguments
    shape = (32, 16, 16)
    vol, known, off = _files(tmp_path, shape)
    a = parse_arguments(["--imgdir", str(tmp_path)] + FLAGS + SCAN + ["--moveout_smooth", "4", "--moveout_table", "device"])
    patches = extract_patches(a)
    res = scan_table(np.where(known, vol * a.gain, 0.0), known, off, 1.0, 1.8, 9, device=DEV, smooth=4.0, table="device")
    assert len(patches) == 1 and np.array_equal(patches[0]["moveout"], res["table"].astype(np.float32))
    assert np.array_equal(patches[0]["moveout_velocity"], res["velocity"][0]) and np.array_equal(patches[0]["moveout_pick"], res["pick"][0])
    assert not np.array_equal(res["velocity"], res["pick"])
    hist_scan, run_scan = _optimise(a, patches[0], tmp_path / "scan")
    np.save(tmp_path / "tau.npy", res["table"])
    b = parse_arguments(["--imgdir", str(tmp_path)] + FLAGS + ["--moveout", "tau.npy"])
    read = extract_patches(b)
    assert np.array_equal(read[0]["moveout"], patches[0]["moveout"])
    hist_file, run_file = _optimise(b, read[0], tmp_path / "file")
    assert len(hist_scan[0]) == 4 and np.isfinite(hist_scan[0]).all()
    for x, y in zip(hist_scan, hist_file):
        np.testing.assert_array_equal(x, y)
    assert np.array_equal(run_scan["output"], run_file["output"]) and np.array_equal(run_scan["moveout_model"], run_file["moveout_model"])
    assert run_scan["moveout_smooth"] == 4.0 and run_scan["moveout_table"] == "device"
    assert np.array_equal(run_scan["moveout_pick"], res["pick"][0]) and np.array_equal(run_scan["moveout_velocity"], res["velocity"][0])
    assert not {"moveout_smooth", "moveout_pick", "moveout_table"} & set(run_file)
    live = (run_scan["moveout"] >= 0) & (run_scan["moveout"] <= shape[0] - 1)
    assert 0 < live.mean() < 1


def test_the_defaults_spelled_out_are_todays_scanned_run(tmp_path):
    """--moveout_smooth 0 --moveout_table host against the run without either flag: the same patch, histories, output and result keys."""
    from deep_prior_interpolation_amd.data import extract_patches
    from deep_prior_interpolation_amd.parameter import parse_arguments
    shape = (32, 16, 16)
    vol, known, off = _files(tmp_path, shape)
    a = parse_arguments(["--imgdir", str(tmp_path)] + FLAGS + SCAN)
    b = parse_arguments(["--imgdir", str(tmp_path)] + FLAGS + SCAN + ["--moveout_smooth", "0", "--moveout_table", "host"])
    pa, pb = extract_patches(a), extract_patches(b)
    assert set(pa[0]) == set(pb[0]) and "moveout_pick" not in pa[0]
    for k in ("image", "mask", "moveout", "moveout_velocity"):
        assert np.array_equal(pa[0][k], pb[0][k]), k
    res = scan_table(np.where(known, vol * a.gain, 0.0), known, off, 1.0, 1.8, 9, device=DEV)
    assert np.array_equal(res["table"], nmo_table(shape, off, res["pick"][0])) and np.array_equal(res["velocity"], res["pick"])
    assert np.array_equal(pa[0]["moveout"], res["table"].astype(np.float32))
    hist_a, run_a = _optimise(a, pa[0], tmp_path / "plain")
    hist_b, run_b = _optimise(b, pb[0], tmp_path / "spelled")
    for x, y in zip(hist_a, hist_b):
        np.testing.assert_array_equal(x, y)
    assert set(run_a) == set(run_b) and np.array_equal(run_a["output"], run_b["output"])
    assert not {"moveout_smooth", "moveout_pick", "moveout_table"} & set(run_a)
