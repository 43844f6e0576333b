"""--wavelet on the GPU: dpi_wavelet_fwd / dpi_wavelet_adj against the float64 reference of tests/wavelet_cases.py within its derived bar,
inside guard bands; offset views, the dot test, autograd, the equalities with the reference's VerticalConv / VerticalGrad chain, the
refusals; and the deep-prior loop with the operator behind the network, eager and captured."""
import os
from argparse import Namespace

import numpy as np
import pytest
import torch

from conftest import jstr

import wavelet_cases as W
from gpu_guard import guard
from deep_prior_interpolation_amd import _lib, utils as u
from deep_prior_interpolation_amd.operators import Chain, ConvolutionalModelling, VerticalConv, VerticalGrad, dottest

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _check(got, ref, bound, what):
    got = got.detach().cpu().numpy().astype(np.float64).reshape(ref.shape)
    err = np.abs(got - ref)
    worst = float((err / np.maximum(bound, 1e-300)).max())
    print("%s: worst error / bound = %.3f" % (what, worst))
    assert np.isfinite(got).all() and np.all(err <= bound), (what, worst)


def _call(adjoint, src, taps, K, diff, C_, T, S, dst):
    L = _lib.load()
    fn = L.dpi_wavelet_adj if adjoint else L.dpi_wavelet_fwd
    code = fn(_lib.ptr(src), _lib.ptr(taps), K, diff, C_, T, S, _lib.ptr(dst), _lib.stream())
    torch.cuda.synchronize()
    return code


# ---------------------------------------------------------------- the entry points ------------------------------------------------
@pytest.mark.parametrize("diff", [0, 1])
@pytest.mark.parametrize("C_, T, S, K", W.CASES, ids=W.IDS)
def test_forward_and_adjoint_against_float64(C_, T, S, K, diff):
    c = W.case(C_, T, S, K, diff)
    taps = torch.from_numpy(c["taps"].copy()).to(DEV)
    for adjoint, src, ref, bound in ((False, c["m"], c["fwd"], c["fwd_bound"]), (True, c["d"], c["adj"], c["adj_bound"])):
        what = "%s diff=%d" % ("adjoint" if adjoint else "forward", diff)
        gin = guard(src.size, torch.float32, DEV, fill=torch.from_numpy(src.copy()))
        gout = guard(src.size, torch.float32, DEV)
        assert _call(adjoint, gin.payload, taps, K, diff, C_, T, S, gout.payload) == 0, _lib.load().dpi_last_error()
        gin.check(what + " input")
        gout.check(what + " output")
        assert torch.equal(gin.payload.cpu(), torch.from_numpy(src.copy()).reshape(-1))          # the input is read only
        _check(gout.payload, ref, bound, what)


@pytest.mark.parametrize("diff", [0, 1])
def test_offset_views_and_both_paths_give_the_same_bits(diff):
    """(2, 130, 68), K = 9: S % 4 == 0, so a 16-byte-aligned input takes the 16-byte loads and the same numbers 4, 8 and 12 bytes off a
    16-byte boundary take the element path — same values staged, same bits out.  The output is moved as well."""
    C_, T, S, K = 2, 130, 68, 9
    c = W.case(C_, T, S, K, diff)
    taps = torch.from_numpy(c["taps"].copy()).to(DEV)
    for adjoint, src, ref, bound in ((False, c["m"], c["fwd"], c["fwd_bound"]), (True, c["d"], c["adj"], c["adj_bound"])):
        res = []
        for off in (0, 1, 2, 3):
            gin = guard(src.size, torch.float32, DEV, fill=torch.from_numpy(src.copy()), offset=off)
            gout = guard(src.size, torch.float32, DEV, offset=(off * 3) % 4)
            assert gin.payload.data_ptr() % 16 == 4 * off
            assert _call(adjoint, gin.payload, taps, K, diff, C_, T, S, gout.payload) == 0
            gin.check("input at +%d bytes" % (4 * off))
            gout.check("output, input at +%d bytes" % (4 * off))
            res.append(gout.payload.clone())
        _check(res[0], ref, bound, "aligned")
        for off in (1, 2, 3):
            assert torch.equal(res[0], res[off]), "element path at +%d bytes differs from the 16-byte path" % (4 * off)


def test_entry_points_refuse_bad_arguments():
    L = _lib.load()
    src = torch.ones(64, device=DEV)
    taps = torch.ones(257, device=DEV)
    g = guard(64, torch.float32, DEV)
    bits = g.bits()
    dst = g.payload
    P = _lib.ptr
    for fn in (L.dpi_wavelet_fwd, L.dpi_wavelet_adj):
        good = (P(src), P(taps), 3, 0, 2, 4, 8, P(dst), _lib.stream())
        for i, bad in ((2, 2), (2, 0), (2, 257), (2, -1), (3, 2), (3, -1), (0, None), (1, None), (7, None), (4, 0), (5, 0), (6, 0), (4, -1),
                       (7, P(src))):
            args = list(good)
            args[i] = bad
            assert fn(*args) != 0, (i, bad)
            assert b"wavelet" in L.dpi_last_error()
    torch.cuda.synchronize()
    assert g.untouched(bits)
    g.check("refused launches")
    assert L.dpi_wavelet_fwd(*good) == 0
    torch.cuda.synchronize()


# ---------------------------------------------------------------- the operator ----------------------------------------------------
def _wavelet(K=9):
    return W.taps_for(K, seed=5).astype(np.float64)


@pytest.mark.parametrize("kind", ["reflectivity", "impedance"])
@pytest.mark.parametrize("shape", [(1, 2, 37, 19), (1, 2, 33, 7, 9), (1, 1, 140, 8, 9)], ids=["4d", "5d", "5d-two-tiles"])
def test_dottest(kind, shape):
    op = ConvolutionalModelling(_wavelet(9 if shape[2] < 100 else 65), kind=kind)
    z = torch.zeros(shape, device=DEV)
    _, rel = dottest(op, z, z, verbose=False, generator=torch.Generator().manual_seed(3))
    print("dottest relative error %.3e" % rel)
    assert rel <= 1e-5                                          # the level tests/test_gpu_avo.py accepts


@pytest.mark.parametrize("kind", ["reflectivity", "impedance"])
def test_operator_on_5d_against_float64(kind):
    """(1, 2, 33, 7, 9) is the [C][T][S = 63] layout of the entry points."""
    op = ConvolutionalModelling(_wavelet(), kind=kind)
    rng = np.random.RandomState(8)
    m = rng.standard_normal((1, 2, 33, 7, 9)).astype(np.float32)
    ref, mag = W.forward64(m, op.taps, op.diff)
    _check(op.forward(torch.from_numpy(m).to(DEV)), ref, W.bound(9, mag), "forward " + kind)
    ref, mag = W.adjoint64(m, op.taps, op.diff)
    _check(op.adjoint(torch.from_numpy(m).to(DEV)), ref, W.bound(9, mag), "adjoint " + kind)
    with pytest.raises(ValueError, match="batch"):
        op.forward(torch.zeros(2, 1, 8, 4, device=DEV))


@pytest.mark.parametrize("kind", ["reflectivity", "impedance"])
def test_autograd_backward_is_the_other_kernel(kind):
    op = ConvolutionalModelling(_wavelet(), kind=kind)
    gen = torch.Generator().manual_seed(4)
    x = torch.randn((1, 2, 37, 19), generator=gen).to(DEV).requires_grad_(True)
    y = torch.randn((1, 2, 37, 19), generator=gen).to(DEV).requires_grad_(True)
    op.forward(x).backward(y.detach())
    taps = op.upload(DEV)
    want = torch.empty_like(y)
    assert _call(True, y.detach(), taps, 9, op.diff, 2, 37, 19, want) == 0               # dpi_wavelet_adj itself
    assert torch.equal(x.grad, want) and torch.equal(x.grad, op.adjoint(y.detach()))
    op.adjoint(y).backward(x.detach())
    assert torch.equal(y.grad, op.forward(x.detach()))


def test_equals_the_chain_of_the_reference_operators():
    """impedance = Chain([VerticalGrad(), VerticalConv(w)]) and reflectivity = 2 VerticalConv(w) on a 4-D tensor, within the bar."""
    w = _wavelet()
    rng = np.random.RandomState(9)
    m = rng.standard_normal((1, 2, 37, 19)).astype(np.float32)
    x = torch.from_numpy(m).to(DEV)
    imp = ConvolutionalModelling(w, kind="impedance")
    chain = Chain([VerticalGrad(), VerticalConv(w)])
    _, mag = W.forward64(m, imp.taps, 1)
    a, b = imp.forward(x), chain.forward(x)
    print("impedance vs chain: identical = %s" % torch.equal(a, b))
    _check(a, b.cpu().numpy().astype(np.float64), W.bound(9, mag), "impedance forward vs chain")
    _, mag = W.adjoint64(m, imp.taps, 1)
    _check(imp.adjoint(x), chain.adjoint(x).cpu().numpy().astype(np.float64), W.bound(9, mag), "impedance adjoint vs chain")
    ref = ConvolutionalModelling(w, kind="reflectivity")
    _, mag = W.forward64(m, ref.taps, 0)
    _check(ref.forward(x), 2.0 * VerticalConv(w).forward(x).cpu().numpy().astype(np.float64), W.bound(9, mag), "reflectivity forward")
    _, mag = W.adjoint64(m, ref.taps, 0)
    _check(ref.adjoint(x), 2.0 * VerticalConv(w).adjoint(x).cpu().numpy().astype(np.float64), W.bound(9, mag), "reflectivity adjoint")


# ---------------------------------------------------------------- the loop --------------------------------------------------------
THETA = [0.0, 10.0, 20.0, 30.0]
CONFIGS = {       # flags, patch shape (numpy order, channels last)
    "2d": (["--datadim", "2d"], (32, 32, 1)),
    "3d": (["--datadim", "3d", "--upsample", "linear"], (16, 16, 16, 1)),
    "2.5d": (["--datadim", "2.5d", "--slice", "tx", "--imgchannel", "3"], (32, 32, 3)),
    "avo": (["--datadim", "2.5d", "--slice", "tx", "--imgchannel", "4", "--avo_theta"] + [str(t) for t in THETA], (32, 32, 4)),
}


def _run(tmp_path, config, mode, wavelet=None, kind="reflectivity", extra=(), epochs=4, data_extra=None, tag=""):
    """A tiny multiunet (filters 4 8, skip 4, 8 input channels) on a tiny patch of the hyperbolic stand-in, half the traces missing."""
    from deep_prior_interpolation_amd.main import Interpolator
    from deep_prior_interpolation_amd.parameter import parse_arguments
    flags, shape = CONFIGS[config]
    out = tmp_path / ("%s_%s_%s%s" % (config, mode, "off" if wavelet is None else kind, tag))
    os.makedirs(out)
    wav = []
    if wavelet is not None:
        np.save(out / "w.npy", np.asarray(wavelet))
        wav = ["--wavelet", "w.npy", "--wavelet_model", kind]
    a = parse_arguments(["--imgdir", str(out), "--filters", "4", "8", "--skip", "4", "--inputdepth", "8", "--gain", "40", "--epochs", str(epochs),
                         "--gpu", "0"] + flags + wav + list(extra))
    traces = u.random_trace_mask(shape[:3] if config == "3d" else shape[:2] + (1,), 0.5, seed=4)          # constant along t
    if config == "avo":
        vol = u.avo_gathers(shape, THETA, vsvp=0.5, seed=0)
    elif config == "3d":
        vol, traces = u.hyperbolic_volume(shape[:3], seed=3)[..., None], traces[..., None]
    else:
        vol = u.hyperbolic_volume(shape, seed=3)                 # (T, X, channels)
    vol = vol.astype(np.float64) * a.gain
    mask = np.broadcast_to(traces, vol.shape).astype(np.float64)
    data = {"image": vol, "mask": mask, "name": "0"}
    data.update(data_extra or {})
    T = Interpolator(a, str(out))
    T.load_data(data)
    T.begin_patch(0)
    T.build_model()
    T.build_input()
    T.optimize(verbose=False, mode=mode, check_every=2)
    T.save_result()
    return T, np.load(out / "0_run.npy", allow_pickle=True).item()


def _history(T):
    h = T.history
    return [np.array(c) for c in (h.loss, h.snr, h.pcorr, h.lr)]


def _model_reproduces_output(run, is_3d, what):
    """W(wavelet_model) = output within the operator's bar: a model snapshot taken at another iteration than the output's cannot pass."""
    out, model, taps = run["output"], run["wavelet_model"], run["wavelet"]
    assert model is not None and model.shape == out.shape and model.dtype == np.float32 and np.isfinite(model).all()
    dev = (lambda v: v[None, None]) if is_3d else (lambda v: np.moveaxis(v, -1, 0)[None])
    diff = 1 if run["wavelet_model_kind"] == "impedance" else 0
    ref, mag = W.forward64(dev(model), taps, diff)
    err = np.abs(dev(out).astype(np.float64) - ref)
    bound = W.bound(len(taps), mag)
    print("%s: worst |W(model) - output| / bound = %.3f" % (what, float((err / np.maximum(bound, 1e-300)).max())))
    assert np.all(err <= bound) and np.abs(ref).max() > 0


@pytest.mark.parametrize("config, kind", [("2d", "reflectivity"), ("3d", "impedance"), ("2.5d", "impedance")])
def test_loop_eager_and_graph(tmp_path, config, kind):
    """Eager and captured runs of one seed agree to the bar of tests/test_gpu_avo.py::test_loop_eager_and_graph, and in both the saved
    model is the one behind the saved output."""
    wavelet = u.ricker(0.12, 1.0, 9)
    res = {}
    for mode in ("eager", "graph"):
        T, run = _run(tmp_path, config, mode, wavelet, kind)
        assert len(T.history.loss) == 4 and np.isfinite(T.history.loss).all()
        assert run["wavelet_model_kind"] == kind and run["wavelet"].dtype == np.float32
        assert np.array_equal(run["wavelet"], (wavelet / 2 if kind == "impedance" else wavelet).astype(np.float32))
        assert run["output"].shape == CONFIGS[config][1][:3]
        _model_reproduces_output(run, config == "3d", "%s %s" % (config, mode))
        res[mode] = (_history(T), run["output"], run["wavelet_model"])
    np.testing.assert_allclose(res["graph"][0][0], res["eager"][0][0], rtol=1e-12)
    np.testing.assert_allclose(res["graph"][0][1], res["eager"][0][1], rtol=1e-12)
    np.testing.assert_array_equal(res["graph"][1], res["eager"][1])
    np.testing.assert_array_equal(res["graph"][2], res["eager"][2])


@pytest.mark.parametrize("mode", ["eager", "graph"])
def test_loop_with_holdout(tmp_path, mode):
    T, run = _run(tmp_path, "2d", mode, u.ricker(0.12, 1.0, 9), extra=("--holdout", "0.2"))
    assert len(T.history.loss) == 4 and run["holdout"] is not None and run["best_iter"] == T.best_iter
    _model_reproduces_output(run, False, "holdout " + mode)


@pytest.mark.parametrize("mode", ["eager", "graph"])
def test_loop_with_out_ema_tracks_no_model(tmp_path, mode):
    T, run = _run(tmp_path, "2d", mode, u.ricker(0.12, 1.0, 9), extra=("--out_ema", "0.9"))
    assert len(T.history.loss) == 4 and np.isfinite(run["output"]).all() and run["out_ema"] == 0.9
    assert "wavelet_model" in run and run["wavelet_model"] is None and run["wavelet_model_kind"] == "reflectivity"


@pytest.mark.parametrize("mode", ["eager", "graph"])
def test_loop_with_trace_offsets(tmp_path, mode):
    off = np.random.RandomState(11).uniform(-0.5, 0.5, (16, 16, 2)).astype(np.float32)
    T, run = _run(tmp_path, "3d", mode, u.ricker(0.12, 1.0, 9), extra=("--trace_offsets", "off.npy"), data_extra={"offsets": off})
    assert len(T.history.loss) == 4 and np.isfinite(T.history.loss).all() and run["trace_offsets"].shape == (16, 16, 2)
    _model_reproduces_output(run, True, "trace_offsets " + mode)


@pytest.mark.parametrize("mode", ["eager", "graph"])
def test_loop_behind_the_avo_operator(tmp_path, mode):
    """d = W G m: the wavelet model is the four angle sections before the wavelet, avo_model the three (wavelet-filtered) parameter
    sections derived from the output."""
    T, run = _run(tmp_path, "avo", mode, u.ricker(0.12, 1.0, 9))
    assert T.net_outchannel() == 3 and len(T.history.loss) == 4 and np.isfinite(T.history.loss).all()
    assert run["output"].shape == (32, 32, 4) and run["avo_model"].shape == (32, 32, 3) and np.isfinite(run["avo_model"]).all()
    _model_reproduces_output(run, False, "avo " + mode)


def test_skipped_patch_has_no_model(tmp_path):
    from deep_prior_interpolation_amd.main import Interpolator
    from deep_prior_interpolation_amd.parameter import parse_arguments
    np.save(tmp_path / "w.npy", u.ricker(0.12, 1.0, 9))
    a = parse_arguments(["--imgdir", str(tmp_path), "--datadim", "2d", "--epochs", "3", "--gpu", "0", "--wavelet", "w.npy"])
    T = Interpolator(a, str(tmp_path))
    T.load_data({"image": np.ones((8, 8, 1)), "mask": np.zeros((8, 8, 1)), "name": "0"})          # all masked
    T.out_best, T.elapsed = T.img * T.mask, 0.0            # what main() does for a flat patch
    T.save_result()
    run = np.load(tmp_path / "0_run.npy", allow_pickle=True).item()
    assert run["wavelet_model"] is None and run["wavelet_model_kind"] == "reflectivity" and run["wavelet"].shape == (9,)


@pytest.mark.parametrize("mode", ["eager", "graph"])
def test_the_unit_wavelet_reproduces_the_run_without_the_flag(tmp_path, mode):
    """--wavelet on the single tap [1.0], reflectivity: fmaf(1, m, 0) is exact, forward and adjoint, so the history and the output are
    those of the run without the flag bit for bit — and the model is the output."""
    T0, run0 = _run(tmp_path, "3d", mode, None, epochs=6)
    T1, run1 = _run(tmp_path, "3d", mode, np.array([1.0]), epochs=6)
    assert T0.forward_model.stage("wavelet") is None and T1.forward_model.stage("wavelet").op is not None and len(T1.history.loss) == 6
    for a, b in zip(_history(T0), _history(T1)):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(run0["output"], run1["output"])
    np.testing.assert_array_equal(run1["wavelet_model"], run1["output"])
    assert not any(k.startswith("wavelet") for k in run0)


def test_without_the_flag_nothing_changes(golden, tmp_path):
    """The 2.5-D trajectory fixture of tests/test_gpu_nets.py, eager, with its tolerances: the hook in net_forward is inert and the result
    file has no new field."""
    from deep_prior_interpolation_amd.main import Interpolator
    g = golden("net_mulresunet25d_tiny")
    a = Namespace(**jstr(g["args"]))
    K = len(g["loss"])
    a.epochs, a.gpu = K, 0
    assert not hasattr(a, "wavelet")
    T = Interpolator(a, str(tmp_path))
    T.load_data({"image": g["image"], "mask": g["mask"], "name": "0"})
    T.build_model()
    assert T.forward_model.stage("wavelet") is None and T.net_outchannel() == g["image"].shape[-1]
    T.net.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in g["init_state"].items()})
    T.net.to(DEV)
    T.input_ = torch.from_numpy(np.array(g["z"], dtype=np.float32)).to(DEV)
    T.optimize(net_inputs=[torch.from_numpy(np.array(x, dtype=np.float32)).to(DEV) for x in g["net_inputs"]], verbose=False, mode="eager")
    np.testing.assert_allclose(T.history.loss, g["loss"], rtol=5e-3)
    np.testing.assert_allclose(T.history.snr, g["snr"], atol=0.1)
    np.testing.assert_allclose(T.history.pcorr, g["pcorr"], atol=1e-2)
    assert np.argmin(T.history.loss) == np.argmin(g["loss"])
    ref = np.asarray(g["out_best"], np.float64)
    assert T.out_best.shape == ref.shape and np.linalg.norm(T.out_best - ref) < 1e-2 * np.linalg.norm(ref)
    assert T.forward_model.best is None and T.wavelet_model() is None
    T.save_result()
    run = np.load(tmp_path / "0_run.npy", allow_pickle=True).item()
    assert not any(k.startswith("wavelet") for k in run)
