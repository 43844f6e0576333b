"""--wavelet_domain without a GPU: the flag and its refusals, old checkpoints, the stage order and the one pre / best pair with recording
stand-ins, the eroded live map against a brute-force loop, the skipped patch and the keys of the result file."""
import os
from argparse import Namespace

import numpy as np
import pytest
import torch

import prestack_cases as P
from deep_prior_interpolation_amd import utils as u
from deep_prior_interpolation_amd.forward_model import ForwardModel, Stage
from deep_prior_interpolation_amd.operators import ConvolutionalModelling, Moveout, PrestackModelling, erode_live
from deep_prior_interpolation_amd.parameter import check_wavelet_domain, net_args_are_same, parse_arguments

BASE = ["--imgdir", "x"]
WAV, MOV = ["--wavelet", "w.npy"], ["--moveout", "tau.npy"]
SCAN = ["--moveout_offset", "off.npy", "--moveout_vscan", "1.0", "3.0", "21"]
D3 = ["--datadim", "3d"]
TODAY = "does not combine with --wavelet: which of the two operators comes first is not decided yet"


# ---------------------------------------------------------------- the flag ---------------------------------------------------------
@pytest.mark.parametrize("partners", [[], WAV, MOV, SCAN], ids=["alone", "wavelet", "moveout", "moveout_offset"])
@pytest.mark.parametrize("domain", P.DOMAINS)
def test_the_flag_without_both_partners_is_refused(partners, domain):
    with pytest.raises(ValueError, match="--wavelet_domain"):
        parse_arguments(BASE + D3 + partners + ["--wavelet_domain", domain])


@pytest.mark.parametrize("mov, flag", [(MOV, "--moveout"), (SCAN, "--moveout_offset")])
def test_both_partners_without_the_flag_keep_the_message_and_point_to_the_flag(mov, flag):
    with pytest.raises(ValueError) as e:
        parse_arguments(BASE + D3 + WAV + mov)
    msg = str(e.value)
    assert msg.startswith(flag + " " + TODAY) and "--wavelet_domain data | model" in msg[len(flag) + 1 + len(TODAY):]


@pytest.mark.parametrize("mov", [MOV, SCAN, MOV + ["--moveout_interp", "cubic"]], ids=["moveout", "moveout_offset", "cubic"])
@pytest.mark.parametrize("kind", P.KINDS)
@pytest.mark.parametrize("domain", P.DOMAINS)
def test_both_values_are_accepted(domain, kind, mov):
    a = parse_arguments(BASE + D3 + WAV + ["--wavelet_model", kind] + mov + ["--wavelet_domain", domain])
    assert a.wavelet_domain == domain and check_wavelet_domain(a) == domain
    assert parse_arguments(BASE + ["--datadim", "2d"] + WAV + mov + ["--wavelet_domain", domain]).wavelet_domain == domain


def test_absent_means_undecided_and_a_third_value_is_refused():
    assert parse_arguments(BASE).wavelet_domain is None and check_wavelet_domain(Namespace(datadim="3d")) is None      # an old args.txt
    with pytest.raises(SystemExit):
        parse_arguments(BASE + D3 + WAV + MOV + ["--wavelet_domain", "both"])
    a = parse_arguments(BASE + D3 + WAV + MOV + ["--wavelet_domain", "data"])
    a.wavelet_domain = "both"
    with pytest.raises(ValueError, match="--wavelet_domain"):
        check_wavelet_domain(a)


@pytest.mark.parametrize("extra, match", [
    (["--datadim", "2.5d", "--slice", "tx", "--imgchannel", "3"], "2.5d"),
    (["--datadim", "2.5d", "--slice", "tx", "--imgchannel", "4", "--avo_theta", "0", "10", "20", "30"], "--moveout"),
    (D3 + ["--net", "part"], "--net part"),
    (D3 + ["--data_forgetting_factor", "3"], "--data_forgetting_factor"),
])
@pytest.mark.parametrize("domain", P.DOMAINS)
def test_what_either_flag_refuses_alone_stays_refused(domain, extra, match):
    with pytest.raises(ValueError, match=match):
        parse_arguments(BASE + WAV + MOV + ["--wavelet_domain", domain] + extra)


def test_time_tiled_patches_stay_refused(tmp_path):
    from deep_prior_interpolation_amd.data import extract_patches
    rng = np.random.RandomState(0)
    np.save(tmp_path / "vol.npy", rng.standard_normal((6, 9, 7)).astype(np.float32))
    np.save(tmp_path / "msk.npy", (rng.uniform(size=(6, 9, 7)) < 0.5).astype(np.float32))
    np.save(tmp_path / "tau.npy", np.arange(6.0)[:, None, None] * np.ones((1, 9, 7)))
    np.save(tmp_path / "w.npy", u.ricker(0.12, 1.0, 5))
    a = parse_arguments(["--imgdir", str(tmp_path), "--imgname", "vol.npy", "--maskname", "msk.npy", "--patch_shape", "3", "4", "4"] + D3
                        + WAV + MOV + ["--wavelet_domain", "data"])
    with pytest.raises(ValueError, match="--moveout.*time axis"):
        extract_patches(a)


def test_main_pocs_refuses_the_flag():
    from deep_prior_interpolation_amd.main_pocs import Interpolator
    with pytest.raises(ValueError, match="--wavelet_domain"):
        Interpolator(parse_arguments(BASE + D3 + WAV + MOV + ["--wavelet_domain", "data"]), "/tmp", device="cpu")


def test_net_args_are_same_reports_the_domain(capsys):
    data = parse_arguments(BASE + D3 + WAV + MOV + ["--wavelet_domain", "data"])
    model = parse_arguments(BASE + D3 + WAV + MOV + ["--wavelet_domain", "model"])
    capsys.readouterr()
    assert not net_args_are_same(data, model)
    assert capsys.readouterr().out.splitlines()[-1] == "wavelet_domain"
    assert net_args_are_same(data, Namespace(**vars(data))) and not net_args_are_same(model, data)
    # an args.txt without the key reads as undecided: the same as a run without the pair, different from either value
    now = parse_arguments(BASE)
    saved = Namespace(**{k: v for k, v in vars(now).items() if k != "wavelet_domain"})
    assert not hasattr(saved, "wavelet_domain") and net_args_are_same(now, saved) and net_args_are_same(saved, now)
    old = Namespace(**{k: v for k, v in vars(data).items() if k != "wavelet_domain"})
    capsys.readouterr()
    assert not net_args_are_same(data, old) and capsys.readouterr().out.splitlines()[-1] == "wavelet_domain"


# ---------------------------------------------------------------- stage order and tracking -----------------------------------------
class Affine:
    """A pure-torch stand-in that records its calls; a x + b per stage, so the two do not commute."""
    COEF = {"avo": (2.0, 0.0), "wavelet": (3.0, 1.0), "moveout": (5.0, -2.0), "sampling": (7.0, 0.0)}

    def __init__(self, name, calls):
        self.name, self.calls = name, calls

    def __call__(self, x):
        self.calls.append((self.name, x))
        a, b = self.COEF[self.name]
        return x * a + b


def _args(tmp_path, domain, extra=()):
    np.save(tmp_path / "w.npy", u.ricker(0.12, 1.0, 5))
    dom = [] if domain is None else ["--wavelet_domain", domain]
    return parse_arguments(["--imgdir", str(tmp_path)] + D3 + WAV + MOV + dom + list(extra))


def _stand_ins(args, names=("sampling", "moveout", "wavelet"), tracked=("wavelet", "moveout")):
    calls = []
    stages = [Stage(n, Affine(n, calls), "data" if n == "sampling" else "model", n in tracked) for n in names]
    return ForwardModel(args, stages=stages), calls


@pytest.mark.parametrize("domain, order", [("data", ["moveout", "wavelet"]), ("model", ["wavelet", "moveout"])])
def test_stage_order_pre_and_the_second_model(tmp_path, domain, order):
    fm, calls = _stand_ins(_args(tmp_path, domain))
    assert [s.name for s in fm.stages] == order + ["sampling"] and fm.domain == domain
    x = torch.arange(6.0).reshape(1, 1, 3, 2).requires_grad_()
    out = fm.apply_model(x)
    assert [n for n, _ in calls] == order
    first, second = (Affine(n, []) for n in order)
    assert torch.equal(out, second(first(x)))
    # one pre: the tensor the network writes, detached, in front of the FIRST of the two
    assert torch.equal(fm.pre, x.detach()) and not fm.pre.requires_grad and calls[0][1] is x
    assert fm.model(order[0]) is None and fm.model(order[1]) is None          # nothing selected yet
    fm.select()
    assert fm.best is fm.pre
    fm.apply_model(x + 1.0)                                       # the next iterate does not touch the selected one
    del calls[:]
    want = x.detach()[0].permute(1, 2, 0).numpy()
    assert np.array_equal(fm.model(order[0]), want) and calls == []
    second_model = fm.model(order[1])
    assert [n for n, _ in calls] == [order[0]] and calls[0][1] is fm.best          # the first operator, once, on `best`
    assert np.array_equal(second_model, first(x.detach())[0].permute(1, 2, 0).numpy())
    fm.clean()
    assert fm.pre is None and fm.best is None and fm.model(order[0]) is None and fm.model(order[1]) is None


def test_two_tracked_stand_ins_without_a_domain_raise():
    with pytest.raises(ValueError, match="wavelet and moveout"):
        _stand_ins(parse_arguments(BASE))
    _stand_ins(parse_arguments(BASE), tracked=("moveout",))


@pytest.mark.parametrize("extra", [["--out_ema", "0.9"], ["--optimizer", "sgld"]])
@pytest.mark.parametrize("domain", P.DOMAINS)
def test_an_average_of_iterates_has_neither_model(tmp_path, domain, extra):
    fm, _ = _stand_ins(_args(tmp_path, domain, extra))
    fm.apply_model(torch.ones(1, 1, 3, 4))
    fm.select()
    assert fm.best is not None and fm.model("wavelet") is None and fm.model("moveout") is None and fm.volumes() == []


# ---------------------------------------------------------------- the eroded live map ----------------------------------------------
def _hand_made_table(T=24, X=5, Y=3):
    """A top wedge mute that grows with x and a mute gap inside every trace whose place moves with y; one trace is whole."""
    t = np.arange(T, dtype=np.float64)[:, None, None] * np.ones((1, X, Y))
    tab = t * 0.9
    wedge = np.arange(X)[None, :, None] * 2
    tab = np.where(t < wedge, -1.0, tab)
    gap = 12 + np.arange(Y)[None, None, :]
    tab = np.where((t >= gap) & (t < gap + 2), -1.0, tab)
    tab[:, 0, 0] = t[:, 0, 0] * 0.9
    return tab


@pytest.mark.parametrize("K, kind", [(1, "reflectivity"), (5, "reflectivity"), (1, "impedance"), (5, "impedance")])
def test_erosion_equals_the_brute_force_loop(K, kind):
    table = _hand_made_table()
    live = Moveout(table).live
    assert 0.5 < live.mean() < 1 and live[:, 0, 0].all() and not live[0, 1:].any() and not live[12:14, 1, 0].any() and live[14, 1, 0]
    diff = int(kind == "impedance")
    got = erode_live(live, K, diff)
    assert got.dtype == bool and got.shape == live.shape and np.array_equal(got, P.erode64(live, K, diff))
    assert not (got & ~live).any()                                # erosion only removes
    if K == 1 and not diff:
        assert np.array_equal(got, live)                          # a single tap reads the sample itself: no erosion
    else:
        assert got.sum() < live.sum()
        assert got[:, 0, 0].all()                                 # rows outside [0, T) do not erode: the whole trace stays whole
    op = PrestackModelling(np.ones(K), table, kind=kind, domain="data")
    assert np.array_equal(op.live, got)
    assert np.array_equal(PrestackModelling(np.ones(K), table, kind=kind, domain="model").live, live)


def test_one_more_row_for_the_impedance():
    live = np.ones((9, 1), dtype=bool)
    live[5] = False
    assert np.flatnonzero(~erode_live(live, 3, 0)[:, 0]).tolist() == [4, 5, 6]
    assert np.flatnonzero(~erode_live(live, 3, 1)[:, 0]).tolist() == [3, 4, 5, 6]          # D reads row t + K/2 + 1 as well
    assert np.flatnonzero(~erode_live(live, 1, 1)[:, 0]).tolist() == [4, 5]


@pytest.mark.parametrize("domain", P.DOMAINS)
def test_load_patch_returns_the_map_of_the_domain(tmp_path, domain):
    table = _hand_made_table()
    fm = ForwardModel(_args(tmp_path, domain, ["--wavelet_model", "impedance"]))
    assert [s.name for s in fm.stages] == (["moveout", "wavelet"] if domain == "data" else ["wavelet", "moveout"])
    live = fm.load_patch({"moveout": table}, table.shape + (1,), np.ones(table.shape + (1,)), torch.device("cpu"), "0")
    L = fm.stage("moveout").op.live
    assert np.array_equal(live, P.erode64(L, 5, 1) if domain == "data" else L) and live is fm.live
    assert isinstance(fm.pair, PrestackModelling) and fm.pair.domain == domain and fm.pair.kind == "impedance"
    assert fm.pair.wavelet is fm.stage("wavelet").op and fm.pair.moveout is fm.stage("moveout").op        # the same operator objects
    assert [s.name for s in fm._model] == ["prestack"] and fm._model[0].op is fm.pair and fm._model[0].tracked


def test_a_patch_whose_live_known_samples_all_fall_to_the_erosion_is_skipped(tmp_path):
    from deep_prior_interpolation_amd.main import Interpolator
    T_, X, Y = 8, 3, 2
    t = np.arange(T_, dtype=np.float64)[:, None, None] * np.ones((1, X, Y))
    table = np.where((t == 2) | (t == 6), -1.0, t)               # no live sample has four live neighbours: a 5-tap wavelet leaves none
    table[:, 1, 1] = t[:, 1, 1]                                   # but for one whole trace, which the mask does not know
    rng = np.random.RandomState(1)
    img = rng.standard_normal((T_, X, Y, 1))
    mask = np.ones((T_, X, Y, 1))
    mask[:, 1, 1] = 0.0
    data = {"image": img, "mask": mask, "name": "0", "moveout": table}
    runs = {}
    for domain in P.DOMAINS:
        out = tmp_path / domain
        os.makedirs(out)
        I = Interpolator(_args(out, domain), str(out), device="cpu")
        std = I.load_data(dict(data))
        runs[domain] = (I, std)
    I, std = runs["model"]
    assert std > 0 and I.mask_.sum().item() == (mask[..., 0] * (table >= 0)).sum()          # L's map: plenty left
    I, std = runs["data"]
    assert std == 0.0 and I.mask_.sum().item() == 0 and I.known_mask().sum() == 0 and I.mask.sum() > 0       # skipped like an all-masked one
    assert I.forward_model.live[:, 1, 1].all()                    # the unknown whole trace is live, and counts nowhere
    I.out_best, I.elapsed = I.img * I.mask, 0.0                  # what main() does for a flat patch
    I.save_result()
    run = np.load(tmp_path / "data" / "0_run.npy", allow_pickle=True).item()
    assert run["wavelet_model"] is None and run["moveout_model"] is None and run["wavelet_domain"] == "data"


# ---------------------------------------------------------------- result keys ------------------------------------------------------
WAV_KEYS = {"wavelet", "wavelet_model_kind", "wavelet_model"}
MOV_KEYS = {"moveout", "moveout_interp", "moveout_model"}
SCAN_KEYS = MOV_KEYS | {"moveout_velocity", "moveout_vscan"}


@pytest.mark.parametrize("mov, mov_keys", [(MOV, MOV_KEYS), (SCAN, SCAN_KEYS)], ids=["moveout", "moveout_offset"])
@pytest.mark.parametrize("domain", P.DOMAINS)
def test_run_fields_and_volumes(tmp_path, domain, mov, mov_keys):
    np.save(tmp_path / "w.npy", u.ricker(0.12, 1.0, 5))
    fm = ForwardModel(parse_arguments(["--imgdir", str(tmp_path)] + D3 + WAV + mov + ["--wavelet_domain", domain]))
    table = _hand_made_table()
    fm.load_patch({"moveout": table}, table.shape + (1,), np.ones(table.shape + (1,)), torch.device("cpu"), "0")
    run = fm.run_fields()
    assert set(run) == WAV_KEYS | mov_keys | {"wavelet_domain"} and run["wavelet_domain"] == domain
    assert run["wavelet_model"] is None and run["moveout_model"] is None          # nothing was optimised
    assert fm.volumes() == [("wavelet_model", "reconstructed_model.npy"), ("moveout_model", "reconstructed_flat.npy")]


@pytest.mark.parametrize("argv, keys, volumes", [
    (WAV, WAV_KEYS, [("wavelet_model", "reconstructed_model.npy")]),
    (MOV, MOV_KEYS, [("moveout_model", "reconstructed_flat.npy")]),
    ([], set(), []),
], ids=["wavelet", "moveout", "none"])
def test_one_flag_alone_keeps_its_key_set(tmp_path, argv, keys, volumes):
    np.save(tmp_path / "w.npy", u.ricker(0.12, 1.0, 5))
    fm = ForwardModel(parse_arguments(["--imgdir", str(tmp_path)] + D3 + argv))
    table = _hand_made_table()
    data = {"moveout": table} if argv == MOV else {}
    live = fm.load_patch(data, table.shape + (1,), np.ones(table.shape + (1,)), torch.device("cpu"), "0")
    assert set(fm.run_fields()) == keys and fm.volumes() == volumes and fm.pair is None and fm.domain is None
    assert (live is None) == (argv != MOV) and (live is None or np.array_equal(live, fm.stage("moveout").op.live))


def test_reassembly_takes_both_fields(tmp_path):
    from deep_prior_interpolation_amd.data import reconstruct_patches
    rng = np.random.RandomState(0)
    np.save(tmp_path / "vol.npy", rng.standard_normal((8, 8)).astype(np.float32))
    np.save(tmp_path / "msk.npy", np.ones((8, 8), dtype=np.float32))
    np.save(tmp_path / "w.npy", u.ricker(0.12, 1.0, 5))
    a = parse_arguments(["--imgdir", str(tmp_path), "--imgname", "vol.npy", "--maskname", "msk.npy", "--datadim", "2d", "--outdir", "run",
                         "--gain", "2"] + WAV + MOV + ["--wavelet_domain", "data"])
    os.makedirs(tmp_path / "run")
    r, lr = rng.standard_normal((8, 8, 1)).astype(np.float32), rng.standard_normal((8, 8, 1)).astype(np.float32)
    np.save(tmp_path / "run" / "0_run.npy", {"output": np.zeros((8, 8, 1), dtype=np.float32), "history": None, "wavelet": np.ones(5, np.float32),
                                             "moveout": np.zeros((8, 8), np.float32), "wavelet_domain": "data", "moveout_model": r,
                                             "wavelet_model": lr})
    for field, want in (("moveout_model", r), ("wavelet_model", lr)):
        rec = reconstruct_patches(a, results_root=str(tmp_path), field=field)
        np.testing.assert_allclose(rec, want[..., 0].astype(np.float64) / 2.0, rtol=1e-6)


# ---------------------------------------------------------------- the operator, on the host ----------------------------------------
def test_operator_parts_and_refusals():
    table = _hand_made_table()
    w = u.ricker(0.12, 1.0, 5)
    op = PrestackModelling(w, table, interp="cubic", kind="impedance", domain="data")
    assert (op.first, op.second) == (op.moveout, op.wavelet) and op.interp == "cubic" and op.kind == "impedance"
    op = PrestackModelling(w, table, domain="model")
    assert (op.first, op.second) == (op.wavelet, op.moveout)
    ready = PrestackModelling(ConvolutionalModelling(w), Moveout(table, "cubic"), domain="data")
    assert ready.interp == "cubic" and ready.kind == "reflectivity"
    taps, (tau, ranges) = ready.upload("cpu")
    assert taps is ready.wavelet.upload("cpu") and tau is ready.moveout.upload("cpu")[0] and ranges.dtype == torch.int32
    assert ready.float() is ready and ready.to("cpu") is ready
    for bad, match in ((dict(domain="both"), "domain"), (dict(kind="velocity"), "kind"), (dict(interp="sinc8"), "interp")):
        with pytest.raises(ValueError, match=match):
            PrestackModelling(w, table, **bad)
    with pytest.raises(ValueError, match="odd"):
        PrestackModelling(np.ones(4), table)
    with pytest.raises(ValueError, match="decreases"):
        PrestackModelling(w, table[::-1].copy())


def test_restatement_is_the_product_of_the_factors_and_its_own_transpose():
    """The float64 restatement: the product of the two references in the order of the domain, and <A x, y> = <x, A^T y> to rounding."""
    import moveout_cases as M
    import wavelet_cases as W
    C_, T, S = 2, 33, 7
    m, d = P.vectors(C_, T, S)
    taps = W.taps_for(9)
    for family in P.TABLES:
        table = P.table_for(family, T, S)
        for interp in P.INTERPS:
            for diff in (0, 1):
                for domain in P.DOMAINS:
                    fwd, fb = P.forward64(m, taps, diff, table, interp, domain)
                    adj, ab = P.adjoint64(d, taps, diff, table, interp, domain)
                    assert (fb >= 0).all() and (ab >= 0).all() and np.isfinite(fb).all() and np.isfinite(ab).all()
                    lhs, rhs = float((fwd * d).sum()), float((m.astype(np.float64) * adj).sum())
                    assert abs(lhs - rhs) <= 1e-12 * max(np.abs(fwd * d).sum(), 1.0), (family, interp, diff, domain)
                if family == "identity":
                    # L = 1: both domains are the wavelet alone
                    want = W.forward64(m, taps, diff)[0]
                    for domain in P.DOMAINS:
                        np.testing.assert_allclose(P.forward64(m, taps, diff, table, interp, domain)[0], want, rtol=0, atol=1e-13)
    # K = 1, tap 1: both domains are the moveout alone
    for domain in P.DOMAINS:
        table = P.table_for("nmo_mutes", T, S)
        np.testing.assert_array_equal(P.forward64(m, np.ones(1, np.float32), 0, table, "cubic", domain)[0], M.forward64(m, table, "cubic")[0])


def test_cases_cover_what_the_issue_names():
    assert {f for _, _, f in P.OP_CASES} == set(P.TABLES) and {K for _, K, _ in P.OP_CASES} == {1, 3, 65, 67}
    assert {len(shape) for shape, _, _ in P.OP_CASES} == {4, 5}
    for family in P.TABLES:
        for T, S in ((33, 65), (257, 130)):
            tab = P.table_for(family, T, S)
            live = (tab >= 0) & (tab <= T - 1)
            Moveout(tab)                                          # a table the operator takes: live values do not decrease along t
            if family == "identity":
                assert np.array_equal(tab, np.arange(T, dtype=np.float32)[:, None] * np.ones((1, S), np.float32))
            if family == "fractional_shift":
                assert not live[:2].any() and live[2:].all() and (tab[2:] % 1 != 0).all()
            if family == "nmo_mutes":
                assert live[:, 0].all() and not live[0, 1:].any() and 0.1 < live.mean() < 0.9
                first = np.argmax(live, axis=0)
                assert first[-1] > first[1] > 0                   # the wedge grows with the column
            if family == "constant":
                assert live.all() and (tab == tab[0, 0]).all()
            if family == "mute_gap":
                dead = ~live[:, 3]
                inside = np.flatnonzero(dead)
                assert dead.any() and live[inside[0] - 1, 3] and live[inside[-1] + 1, 3]          # live on both sides of the gap
