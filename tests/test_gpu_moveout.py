"""--moveout on the GPU: dpi_moveout_fwd / dpi_moveout_adj against the float64 reference of tests/moveout_cases.py within its derived bars,
inside guard bands; the identity and the all-muted table, repeatability, offset views, the refusals, the dot test and autograd; and the
deep-prior loop with the operator behind the network, eager and captured."""
import os

import numpy as np
import pytest
import torch

import moveout_cases as M
from gpu_guard import guard
from deep_prior_interpolation_amd import _lib, utils as u
from deep_prior_interpolation_amd.operators import Moveout, dottest, nmo_table, shift_table

pytestmark = pytest.mark.gpu
DEV = "cuda"
INTERPS = ["linear", "cubic"]


def _check(got, ref, bound, what):
    got = got.detach().cpu().numpy().astype(np.float64).reshape(ref.shape)
    err = np.abs(got - ref)
    worst = float((err / np.maximum(bound, 1e-300)).max())
    print("%s: worst error / bound = %.3f" % (what, worst))
    assert np.isfinite(got).all() and np.all(err <= bound), (what, worst)


def _call(adjoint, src, op, C_, dst):
    """The ctypes-direct path: the entry points themselves on the operator's uploaded table and ranges."""
    L = _lib.load()
    tau, ranges = op.upload(DEV)
    if adjoint:
        code = L.dpi_moveout_adj(_lib.ptr(src), _lib.ptr(tau), _lib.ptr(ranges), op.kind, C_, op.T, op.S, _lib.ptr(dst), _lib.stream())
    else:
        code = L.dpi_moveout_fwd(_lib.ptr(src), _lib.ptr(tau), op.kind, C_, op.T, op.S, _lib.ptr(dst), _lib.stream())
    torch.cuda.synchronize()
    return code


# ---------------------------------------------------------------- the entry points ------------------------------------------------
@pytest.mark.parametrize("interp", INTERPS)
@pytest.mark.parametrize("C_, T, S, family", M.CASES, ids=M.IDS)
def test_forward_and_adjoint_against_float64(C_, T, S, family, interp):
    c = M.case(C_, T, S, family, interp)
    op = Moveout(c["table"], interp)
    for adjoint, src, ref, bound in ((False, c["m"], c["fwd"], c["fwd_bound"]), (True, c["d"], c["adj"], c["adj_bound"])):
        what = "%s %s %s" % ("adjoint" if adjoint else "forward", family, interp)
        gin = guard(src.size, torch.float32, DEV, fill=torch.from_numpy(src.copy()))
        gout = guard(src.size, torch.float32, DEV)
        assert _call(adjoint, gin.payload, op, C_, gout.payload) == 0, _lib.load().dpi_last_error()
        gin.check(what + " input")
        gout.check(what + " output")
        assert torch.equal(gin.payload.cpu(), torch.from_numpy(src.copy()).reshape(-1))          # the input is read only
        _check(gout.payload, ref, bound, what)


@pytest.mark.parametrize("interp", INTERPS)
@pytest.mark.parametrize("C_, T, S", [(2, 7, 3), (3, 130, 70)])
def test_identity_and_all_muted_tables(C_, T, S, interp):
    """The identity table returns the input bit for bit, both directions; the all-muted table returns zeros."""
    for family, same in (("identity", True), ("all_muted", False)):
        c = M.case(C_, T, S, family, interp)
        op = Moveout(c["table"].reshape(T, S, 1), interp)           # as a 5-D operator
        for src, fn in ((c["m"], op.forward), (c["d"], op.adjoint)):
            got = fn(torch.from_numpy(src.copy()).reshape(1, C_, T, S, 1).to(DEV)).cpu().numpy().reshape(src.shape)
            assert np.array_equal(got, src if same else np.zeros_like(src))


@pytest.mark.parametrize("interp", INTERPS)
@pytest.mark.parametrize("family", ["squeeze", "constant", "sorted_gaps", "nmo"])
def test_adjoint_is_repeatable_and_paths_agree(family, interp):
    """The adjoint run twice gives identical bits; inputs and outputs 4, 8 and 12 bytes off a 16-byte boundary and the ctypes-direct
    path give the bits of the operator path, forward and adjoint."""
    C_, T, S = 3, 130, 70
    c = M.case(C_, T, S, family, interp)
    op = Moveout(c["table"], interp)
    for adjoint, src in ((False, c["m"]), (True, c["d"])):
        x = torch.from_numpy(src.copy()).to(DEV)
        first = (op.adjoint if adjoint else op.forward)(x)
        again = (op.adjoint if adjoint else op.forward)(x)
        assert torch.equal(first, again)
        for off in (0, 1, 2, 3):
            gin = guard(src.size, torch.float32, DEV, fill=torch.from_numpy(src.copy()), offset=off)
            gout = guard(src.size, torch.float32, DEV, offset=(off * 3) % 4)
            assert gin.payload.data_ptr() % 16 == 4 * off
            assert _call(adjoint, gin.payload, op, C_, gout.payload) == 0
            gin.check("input at +%d bytes" % (4 * off))
            gout.check("output, input at +%d bytes" % (4 * off))
            assert torch.equal(gout.payload, first.reshape(-1)), "ctypes path at +%d bytes differs from the operator path" % (4 * off)
        # a view with a storage offset goes through the operator as it is (contiguous, not 16-byte aligned)
        big = torch.zeros(src.size + 3, device=DEV)
        big[3:] = x.reshape(-1)
        view = big[3:].view(x.shape)
        assert view.storage_offset() == 3 and torch.equal((op.adjoint if adjoint else op.forward)(view), first)


def test_entry_points_refuse_bad_arguments():
    L = _lib.load()
    src = torch.ones(64, device=DEV)
    tau = torch.zeros(32, device=DEV)
    ranges = torch.zeros(64, dtype=torch.int32, device=DEV)
    g = guard(64, torch.float32, DEV)
    bits = g.bits()
    dst = g.payload
    P = _lib.ptr
    good_f = (P(src), P(tau), 0, 2, 4, 8, P(dst), _lib.stream())
    for i, bad in ((0, None), (1, None), (6, None), (6, P(src)), (2, 2), (2, -1), (3, 0), (4, 0), (5, 0), (3, -1), (4, (1 << 24) + 1), (3, 65536)):
        args = list(good_f)
        args[i] = bad
        assert L.dpi_moveout_fwd(*args) != 0, (i, bad)
        assert b"moveout_fwd" in L.dpi_last_error()
    good_a = (P(src), P(tau), P(ranges), 1, 2, 4, 8, P(dst), _lib.stream())
    for i, bad in ((0, None), (1, None), (2, None), (7, None), (7, P(src)), (3, 2), (3, -1), (4, 0), (5, 0), (6, 0), (5, -3), (4, 65536)):
        args = list(good_a)
        args[i] = bad
        assert L.dpi_moveout_adj(*args) != 0, (i, bad)
        assert b"moveout_adj" in L.dpi_last_error()
    torch.cuda.synchronize()
    assert g.untouched(bits)
    g.check("refused launches")
    assert L.dpi_moveout_fwd(*good_f) == 0 and L.dpi_moveout_adj(*good_a) == 0
    torch.cuda.synchronize()


def test_a_wrong_range_table_stays_in_bounds():
    """Ranges far outside [0, T] are clamped by the kernel: the walk is longer, the result the same bits, the guard bands untouched."""
    C_, T, S = 2, 7, 3
    c = M.case(C_, T, S, "squeeze", "cubic")
    op = Moveout(c["table"], "cubic")
    tau, _ = op.upload(DEV)
    wide = torch.stack([torch.full((T, S), -1000, dtype=torch.int32), torch.full((T, S), 1 << 30, dtype=torch.int32)]).to(DEV)
    gin = guard(c["d"].size, torch.float32, DEV, fill=torch.from_numpy(c["d"].copy()))
    gout = guard(c["d"].size, torch.float32, DEV)
    assert _lib.load().dpi_moveout_adj(_lib.ptr(gin.payload), _lib.ptr(tau), _lib.ptr(wide), 1, C_, T, S, _lib.ptr(gout.payload),
                                       _lib.stream()) == 0
    torch.cuda.synchronize()
    gin.check("input")
    gout.check("output")
    assert torch.equal(gout.payload, op.adjoint(torch.from_numpy(c["d"].copy()).to(DEV)).reshape(-1))


# ---------------------------------------------------------------- the operator ----------------------------------------------------
def _nmo(shape):
    """An NMO table on (T, X[, Y]) that leaves about half of the patch live."""
    T = shape[0]
    grid = np.meshgrid(*[np.arange(n) / n for n in shape[1:]], indexing="ij")
    off = 0.8 * T * np.sqrt(sum(g ** 2 for g in grid))
    return nmo_table(shape, off, lambda tau: 1.0 / (0.9 - 0.3 * tau / T))


def _shifts(shape, seed=5):
    return shift_table(shape, np.random.RandomState(seed).uniform(0.0, 3.0, shape[1:]))


@pytest.mark.parametrize("interp", INTERPS)
@pytest.mark.parametrize("shape", [(1, 2, 37, 19), (1, 2, 33, 7, 9), (1, 1, 140, 8, 9)], ids=["4d", "5d", "5d-long"])
def test_dottest(shape, interp):
    for name, table in (("nmo", _nmo(shape[2:])), ("shift", _shifts(shape[2:]))):
        op = Moveout(table, interp)
        assert 0.2 < op.live.mean() <= 1.0
        z = torch.zeros(shape, device=DEV)
        _, rel = dottest(op, z, z, verbose=False, generator=torch.Generator().manual_seed(3))
        print("dottest %s relative error %.3e" % (name, rel))
        assert rel <= 1e-5                                       # the level tests/test_gpu_avo.py accepts


@pytest.mark.parametrize("interp", INTERPS)
def test_operator_on_5d_against_float64_and_refusals(interp):
    """(1, 2, 33, 7, 9) is the [C][T][S = 63] layout of the entry points."""
    op = Moveout(_nmo((33, 7, 9)), interp)
    rng = np.random.RandomState(8)
    m = rng.standard_normal((1, 2, 33, 7, 9)).astype(np.float32)
    tab = op.table.reshape(33, 63)
    ref, mag = M.forward64(m.reshape(1, 2, 33, 63), tab, interp)
    _check(op.forward(torch.from_numpy(m).to(DEV)), ref, M.fwd_bound(interp, mag), "forward " + interp)
    ref, mag, n = M.adjoint64(m.reshape(1, 2, 33, 63), tab, interp)
    _check(op.adjoint(torch.from_numpy(m).to(DEV)), ref, M.adj_bound(interp, mag, n[None, None]), "adjoint " + interp)
    with pytest.raises(ValueError, match="batch"):
        op.forward(torch.zeros(2, 1, 33, 7, 9, device=DEV))
    with pytest.raises(ValueError, match="table"):
        op.forward(torch.zeros(1, 1, 33, 7, 8, device=DEV))


@pytest.mark.parametrize("interp", INTERPS)
def test_autograd_backward_is_the_other_kernel(interp):
    op = Moveout(_nmo((37, 19)), interp)
    gen = torch.Generator().manual_seed(4)
    x = torch.randn((1, 2, 37, 19), generator=gen).to(DEV).requires_grad_(True)
    y = torch.randn((1, 2, 37, 19), generator=gen).to(DEV).requires_grad_(True)
    op.forward(x).backward(y.detach())
    want = torch.empty_like(y)
    assert _call(True, y.detach(), op, 2, want) == 0             # dpi_moveout_adj itself
    assert torch.equal(x.grad, want) and torch.equal(x.grad, op.adjoint(y.detach()))
    op.adjoint(y).backward(x.detach())
    assert torch.equal(y.grad, op.forward(x.detach()))


# ---------------------------------------------------------------- the loop --------------------------------------------------------
CONFIGS = {       # flags, patch shape (numpy order, channels last)
    "2d": (["--datadim", "2d"], (32, 32, 1)),
    "3d": (["--datadim", "3d", "--upsample", "linear"], (16, 16, 16, 1)),
}
TABLES = {"shift": _shifts, "nmo": _nmo, "identity": lambda shape: shift_table(shape, np.zeros(shape[1:])),
          "muted": lambda shape: np.full(shape, -1.0)}


def _run(tmp_path, config, mode, table=None, interp="linear", extra=(), epochs=4, data_extra=None, tag="", optimise=True):
    """The tiny multiunet of tests/test_gpu_wavelet.py (filters 4 8, skip 4, 8 input channels) on a tiny patch of the hyperbolic stand-in,
    half the traces missing."""
    from deep_prior_interpolation_amd.main import Interpolator
    from deep_prior_interpolation_amd.parameter import parse_arguments
    flags, shape = CONFIGS[config]
    out = tmp_path / ("%s_%s_%s_%s%s" % (config, mode, table or "off", interp, tag))
    os.makedirs(out)
    mov = ["--moveout", "tau.npy", "--moveout_interp", interp] if table is not None else []
    a = parse_arguments(["--imgdir", str(out), "--filters", "4", "8", "--skip", "4", "--inputdepth", "8", "--gain", "40", "--epochs", str(epochs),
                         "--gpu", "0"] + flags + mov + list(extra))
    traces = u.random_trace_mask(shape[:3] if config == "3d" else shape[:2] + (1,), 0.5, seed=4)          # constant along t
    if config == "3d":
        vol, traces = u.hyperbolic_volume(shape[:3], seed=3)[..., None], traces[..., None]
    else:
        vol = u.hyperbolic_volume(shape, seed=3)                 # (T, X, channels)
    vol = vol.astype(np.float64) * a.gain
    mask = np.broadcast_to(traces, vol.shape).astype(np.float64)
    data = {"image": vol, "mask": mask, "name": "0"}
    if table is not None:
        data["moveout"] = TABLES[table](shape[:-1])
    data.update(data_extra or {})
    T = Interpolator(a, str(out))
    std = T.load_data(data)
    if optimise:
        T.begin_patch(0)
        T.build_model()
        T.build_input()
        T.optimize(verbose=False, mode=mode, check_every=2)
    else:
        assert np.isclose(std, 0.0, atol=1e-12)
        T.out_best, T.elapsed = T.img * T.mask, 0.0              # what main() does for a flat patch
    T.save_result()
    return T, np.load(out / "0_run.npy", allow_pickle=True).item()


def _history(T):
    h = T.history
    return [np.array(c) for c in (h.loss, h.snr, h.pcorr, h.lr)]


def _model_reproduces_output(T, run, is_3d, what):
    """L(moveout_model) = output within the forward bar (a model snapshot of another iteration than the output's cannot pass); muted
    samples of the output are exactly 0 and are out of the device mask, so they carry no loss."""
    out, model, table, interp = run["output"], run["moveout_model"], run["moveout"], run["moveout_interp"]
    assert model is not None and model.shape == out.shape and model.dtype == np.float32 and np.isfinite(model).all()
    assert table.dtype == np.float32 and table.shape == out.shape[:table.ndim] and np.array_equal(table, T.forward_model.stage("moveout").op.table)
    dev = (lambda v: v[None, None]) if is_3d else (lambda v: np.moveaxis(v, -1, 0)[None])
    flat = lambda v: dev(v).reshape(1, -1, table.shape[0], table[0].size)
    ref, mag = M.forward64(flat(model), table.reshape(table.shape[0], -1), interp)
    err = np.abs(flat(out).astype(np.float64) - ref)
    bound = M.fwd_bound(interp, mag)
    print("%s: worst |L(model) - output| / bound = %.3f" % (what, float((err / np.maximum(bound, 1e-300)).max())))
    assert np.all(err <= bound) and np.abs(ref).max() > 0
    live = T.forward_model.stage("moveout").op.live
    assert 0 < live.mean() < 1 and np.array_equal(live, (table >= 0) & (table <= table.shape[0] - 1))
    muted = np.broadcast_to(~live.reshape(flat(out).shape[2:])[None, None], flat(out).shape)
    assert not flat(out)[muted].any()
    assert not T.mask_.cpu().numpy().reshape(flat(out).shape)[muted].any() and T.mask_.sum().item() > 0
    assert np.array_equal(run["mask"], T.mask) and run["mask"].reshape(-1).sum() > T.mask_.sum().item()      # the saved mask is the file's


@pytest.mark.parametrize("config, table, interp", [("2d", "shift", "linear"), ("2d", "nmo", "cubic"), ("3d", "shift", "cubic"),
                                                   ("3d", "nmo", "linear")])
def test_loop_eager_and_graph(tmp_path, config, table, interp):
    """Eager and captured runs of one seed agree to the bar of tests/test_gpu_wavelet.py::test_loop_eager_and_graph, and in both the saved
    model is the one behind the saved output."""
    res = {}
    for mode in ("eager", "graph"):
        T, run = _run(tmp_path, config, mode, table, interp)
        assert len(T.history.loss) == 4 and np.isfinite(T.history.loss).all()
        assert run["moveout_interp"] == interp and run["output"].shape == CONFIGS[config][1][:3]
        _model_reproduces_output(T, run, config == "3d", "%s %s %s" % (config, table, mode))
        res[mode] = (_history(T), run["output"], run["moveout_model"])
    np.testing.assert_allclose(res["graph"][0][0], res["eager"][0][0], rtol=1e-12)
    np.testing.assert_allclose(res["graph"][0][1], res["eager"][0][1], rtol=1e-12)
    np.testing.assert_array_equal(res["graph"][1], res["eager"][1])
    np.testing.assert_array_equal(res["graph"][2], res["eager"][2])


@pytest.mark.parametrize("interp", INTERPS)
@pytest.mark.parametrize("mode", ["eager", "graph"])
def test_the_identity_table_reproduces_the_run_without_the_flag(tmp_path, mode, interp):
    """tau = t: the weights are 1, 0 / 0, 1, 0, 0 exactly, forward and adjoint, and nothing is muted, so the history and the output are
    those of the run without the flag bit for bit — and the model is the output."""
    T0, run0 = _run(tmp_path, "3d", mode, None, epochs=6)
    T1, run1 = _run(tmp_path, "3d", mode, "identity", interp, epochs=6)
    assert T0.forward_model.stage("moveout") is None and T1.forward_model.stage("moveout").op is not None and T1.forward_model.stage("moveout").op.live.all() and len(T1.history.loss) == 6
    for a, b in zip(_history(T0), _history(T1)):
        np.testing.assert_array_equal(a, b)
    assert np.array_equal(run0["output"], run1["output"])
    assert np.array_equal(run1["moveout_model"], run1["output"])
    assert not any(k.startswith("moveout") for k in run0)


@pytest.mark.parametrize("mode", ["eager", "graph"])
def test_loop_with_holdout_draws_no_muted_sample(tmp_path, mode):
    T, run = _run(tmp_path, "2d", mode, "nmo", extra=("--holdout", "0.2"))
    assert len(T.history.loss) == 4 and run["holdout"] is not None and run["best_iter"] == T.best_iter
    _model_reproduces_output(T, run, False, "holdout " + mode)
    live, sel = T.forward_model.stage("moveout").op.live, T.holdout_sel                # (T, X), (X, C)
    assert sel.sum() > 0
    held = T.mask_.cpu().numpy()[0] * np.moveaxis(sel, -1, 0)[:, None]          # (C, T, X): the samples the validation misfit sees
    assert held.sum() > 0 and not held[:, ~live].any()
    assert all((T.mask[:, x, c] * live[:, x]).any() for x, c in zip(*np.nonzero(sel)))          # every held-out trace has a live known sample
    assert np.isfinite(T.history.val_loss).all()


@pytest.mark.parametrize("mode", ["eager", "graph"])
def test_loop_with_out_ema_tracks_no_model(tmp_path, mode):
    T, run = _run(tmp_path, "2d", mode, "shift", extra=("--out_ema", "0.9"))
    assert len(T.history.loss) == 4 and np.isfinite(run["output"]).all() and run["out_ema"] == 0.9
    assert "moveout_model" in run and run["moveout_model"] is None and run["moveout_interp"] == "linear" and run["moveout"].shape == (32, 32)


@pytest.mark.parametrize("mode", ["eager", "graph"])
def test_loop_with_trace_offsets(tmp_path, mode):
    off = np.random.RandomState(11).uniform(-0.5, 0.5, (16, 16, 2)).astype(np.float32)
    T, run = _run(tmp_path, "3d", mode, "nmo", "cubic", extra=("--trace_offsets", "off.npy"), data_extra={"offsets": off})
    assert len(T.history.loss) == 4 and np.isfinite(T.history.loss).all() and run["trace_offsets"].shape == (16, 16, 2)
    _model_reproduces_output(T, run, True, "trace_offsets " + mode)


def test_fully_muted_patch_is_skipped(tmp_path):
    T, run = _run(tmp_path, "3d", "eager", "muted", optimise=False)
    assert run["moveout_model"] is None and run["moveout_interp"] == "linear" and not (run["moveout"] != -1.0).any()
    assert T.mask_.sum().item() == 0 and T.mask.sum() > 0


def test_reassembly_of_a_two_patch_job(tmp_path, monkeypatch):
    """main() on a (32, 48) section cut into two (32, 32) patches 16 traces apart: reconstruct_patches(field="moveout_model") returns the
    flattened sections of the result files, averaged where the windows overlap and divided by gain."""
    from deep_prior_interpolation_amd import main as main_mod
    from deep_prior_interpolation_amd.data import reconstruct_patches
    from deep_prior_interpolation_amd.parameter import parse_arguments
    monkeypatch.chdir(tmp_path)
    vol = u.hyperbolic_volume((32, 48, 1), seed=3)[..., 0]
    known = u.random_trace_mask((32, 48, 1), 0.5, seed=4)[..., 0]
    np.save(tmp_path / "vol.npy", vol)
    np.save(tmp_path / "msk.npy", np.where(np.broadcast_to(known, vol.shape) > 0, vol, np.nan))
    table = _shifts((32, 48))
    np.save(tmp_path / "tau.npy", table)
    argv = ["--imgdir", str(tmp_path), "--imgname", "vol.npy", "--maskname", "msk.npy", "--datadim", "2d", "--patch_shape", "-1", "32",
            "--patch_stride", "-1", "16", "--filters", "4", "8", "--skip", "4", "--inputdepth", "8", "--gain", "40", "--epochs", "3",
            "--gpu", "0", "--outdir", "job", "--moveout", "tau.npy"]
    main_mod.main(argv)
    runs = [np.load(tmp_path / "results" / "job" / ("%d_run.npy" % i), allow_pickle=True).item() for i in range(2)]
    for i, r in enumerate(runs):
        assert np.array_equal(r["moveout"], table.astype(np.float32)[:, 16 * i:16 * i + 32]) and r["moveout_model"].shape == (32, 32, 1)
    rec = reconstruct_patches(parse_arguments(argv), field="moveout_model")
    m0, m1 = (r["moveout_model"][..., 0].astype(np.float64) / 40.0 for r in runs)
    want = np.concatenate([m0[:, :16], 0.5 * (m0[:, 16:] + m1[:, :16]), m1[:, 16:]], axis=1)
    assert rec.shape == (32, 48) and np.abs(rec).max() > 0
    np.testing.assert_allclose(rec, want, rtol=1e-6, atol=1e-7 * np.abs(want).max())
    out = reconstruct_patches(parse_arguments(argv))
    assert out.shape == (32, 48) and not np.array_equal(out, rec)
