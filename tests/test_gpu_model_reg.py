"""--model_reg on the GPU: dpi_model_reg against the numpy restatement of tests/model_reg_cases.py — grad bit for bit, the value within the
bar of re-ordering a double sum — inside guard bands, on aligned and one-float-offset views; repeatability, the refusals, autograd; and the
deep-prior loop with the penalty on what the network writes."""
import os

import numpy as np
import pytest
import torch

import model_reg_cases as MR
from gpu_guard import guard
from deep_prior_interpolation_amd import _lib, ops, utils as u
from deep_prior_interpolation_amd.operators import shift_table

pytestmark = pytest.mark.gpu
DEV = "cuda"
INPUTS = {"generic": MR.generic, "integers": MR.integers}


def _launch(m, shape, axes, grad, ws=None, res=None):
    """The entry point itself on device buffers; returns (code, res)."""
    L = _lib.load()
    C_, n0, n1, n2 = shape
    ws = torch.empty(L.dpi_model_reg_ws_doubles(int(np.prod(shape))), dtype=torch.float64, device=DEV) if ws is None else ws
    res = torch.full((1,), float("nan"), dtype=torch.float64, device=DEV) if res is None else res
    code = L.dpi_model_reg(_lib.ptr(m), C_, n0, n1, n2, axes, _lib.ptr(grad), _lib.ptr(ws), _lib.ptr(res), _lib.stream())
    torch.cuda.synchronize()
    return code, res


def _guarded(values, offset):
    """The values inside guard bands, `offset` floats behind a 256-byte boundary, and a NaN-filled guarded output placed the same way."""
    gin = guard(values.size, torch.float32, DEV, fill=torch.from_numpy(values.copy()), offset=offset)
    gout = guard(values.size, torch.float32, DEV, offset=offset)
    assert gin.payload.data_ptr() % 16 == 4 * offset and gout.payload.data_ptr() % 16 == 4 * offset
    return gin, gout


def _run_guarded(values, axes, offset, what):
    gin, gout = _guarded(values, offset)
    code, res = _launch(gin.payload, values.shape, axes, gout.payload)
    assert code == 0, _lib.load().dpi_last_error()
    gin.check(what + ": m")
    gout.check(what + ": grad")
    assert torch.equal(gin.payload.cpu(), torch.from_numpy(values.copy()).reshape(-1))          # the input is read only
    return gout.payload.cpu().numpy().reshape(values.shape), float(res.item())


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---------------------------------------------------------------- the entry point -------------------------------------------------
@pytest.mark.parametrize("inputs", sorted(INPUTS))
@pytest.mark.parametrize("shape", MR.SHAPES, ids=["x".join(map(str, s)) for s in MR.SHAPES])
def test_entry_point_against_the_restatement(shape, inputs):
    values = INPUTS[inputs](shape)
    worst = 0.0
    for axes in MR.AXES:
        R, k, bar = MR.bar(values, axes)
        for offset in (0, 1):
            what = "%s %s axes %d at +%d bytes" % (inputs, shape, axes, 4 * offset)
            grad, res = _run_guarded(values, axes, offset, what)
            assert _same_bits(grad, MR.grad32(k)), what
            ratio = abs(res - R) / bar if bar > 0 else (0.0 if res == R else np.inf)
            worst = max(worst, ratio)
            assert np.isfinite(res) and abs(res - R) <= bar, (what, res, R, bar)
        if inputs == "integers" and (axes == 0 or any(axes >> a & 1 and shape[a + 1] > 1 for a in range(3))) and np.prod(shape) > 5:
            assert (k == 0).any()                                # ties occurred
    print("%s %s: worst |res - R| / bar = %.3e" % (inputs, shape, worst))


def test_the_grid_stride_turn_on_both_paths():
    """MR.LARGE holds more quads than one turn of the grid covers; n2 % 4 == 0, so the aligned view takes the 16-byte path and the view
    one float in the 4-byte path."""
    values = MR.generic(MR.LARGE, seed=5)
    for axes in (7, 0):
        R, k, bar = MR.bar(values, axes)
        want = MR.grad32(k)
        got = {}
        for offset in (0, 1):
            grad, res = _run_guarded(values, axes, offset, "large axes %d at +%d bytes" % (axes, 4 * offset))
            assert _same_bits(grad, want)
            print("large axes %d at +%d bytes: |res - R| / bar = %.3e" % (axes, 4 * offset, abs(res - R) / bar))
            assert abs(res - R) <= bar
            got[offset] = res
        assert np.float64(got[0]).tobytes() == np.float64(got[1]).tobytes()


@pytest.mark.parametrize("shape", [(1, 130, 7, 10), (2, 4, 8, 8)])
def test_two_launches_give_identical_bits(shape):
    values = MR.generic(shape, seed=2)
    for axes in MR.AXES:
        a = _run_guarded(values, axes, 0, "first")
        b = _run_guarded(values, axes, 0, "second")
        assert _same_bits(a[0], b[0]) and np.float64(a[1]).tobytes() == np.float64(b[1]).tobytes()


@pytest.mark.parametrize("inputs", sorted(INPUTS))
@pytest.mark.parametrize("shape", [(2, 4, 8, 8), (3, 9, 6, 8), (1, 33, 5, 132), (1, 1, 1, 4)])
def test_vector_and_scalar_paths_give_identical_bits(shape, inputs):
    """n2 % 4 == 0: an aligned tensor takes the 16-byte path, a view one float into a larger buffer the 4-byte path; so does an aligned m
    with an offset grad."""
    values = INPUTS[inputs](shape, seed=3)
    m = torch.from_numpy(values.copy()).to(DEV)
    for axes in MR.AXES:
        vec = _run_guarded(values, axes, 0, "aligned")
        sca = _run_guarded(values, axes, 1, "offset")
        assert _same_bits(vec[0], sca[0]) and np.float64(vec[1]).tobytes() == np.float64(sca[1]).tobytes(), axes
        gout = guard(values.size, torch.float32, DEV, offset=3)
        assert m.data_ptr() % 16 == 0 and gout.payload.data_ptr() % 16 == 12
        code, res = _launch(m, shape, axes, gout.payload)
        assert code == 0
        gout.check("offset grad")
        assert _same_bits(gout.payload.cpu().numpy().reshape(shape), vec[0]) and np.float64(res.item()).tobytes() == np.float64(vec[1]).tobytes()


def test_entry_point_refuses_bad_arguments():
    L = _lib.load()
    m = torch.ones(64, device=DEV)
    ws = torch.empty(L.dpi_model_reg_ws_doubles(64), dtype=torch.float64, device=DEV)
    res = torch.zeros(1, dtype=torch.float64, device=DEV)
    g = guard(64, torch.float32, DEV)
    bits = g.bits()
    P = _lib.ptr
    good = (P(m), 2, 2, 4, 4, 7, P(g.payload), P(ws), P(res), _lib.stream())
    for i, bad in ((0, None), (6, None), (7, None), (8, None), (6, P(m)), (5, 8), (5, -1), (1, 0), (2, 0), (3, 0), (4, 0), (1, -1),
                   (2, 1 << 33), (4, 1 << 40)):
        args = list(good)
        args[i] = bad
        assert L.dpi_model_reg(*args) != 0, (i, bad)
        assert b"model_reg" in L.dpi_last_error()
    torch.cuda.synchronize()
    assert g.untouched(bits) and res.item() == 0.0
    g.check("refused launches")
    assert L.dpi_model_reg(*good) == 0
    torch.cuda.synchronize()
    assert not g.untouched(bits) and res.item() == 0.0           # a constant tensor: every difference is 0


# ---------------------------------------------------------------- autograd --------------------------------------------------------
@pytest.mark.parametrize("shape, dims", [((1, 2, 9, 7), ()), ((1, 2, 9, 7), (2, 3)), ((1, 2, 9, 8), (3,)), ((1, 3, 5, 6, 7), (2, 3, 4)),
                                         ((1, 1, 6, 5, 8), (3, 4)), ((1, 1, 6, 5, 8), (2,))])
def test_autograd(shape, dims):
    values = MR.integers(shape, seed=7) + (0 if dims else 0.5) * MR.generic(shape, seed=8)
    R, k, bar = MR.bar(MR.as_4d(values), MR.dims_to_bits(dims, len(shape)))
    want = MR.grad32(k).reshape(shape)
    for scale in (1.0, 3.0):
        m = torch.from_numpy(values.copy()).to(DEV).requires_grad_(True)
        r = ops.model_reg(m, dims)
        assert r.dtype == torch.float32 and r.ndim == 0 and abs(r.item() - R) <= bar + 2.0 ** -24 * abs(R)      # the scalar is rounded to fp32
        (r * scale).backward()
        assert _same_bits(m.grad.cpu().numpy(), want * np.float32(scale))


def test_autograd_refusals():
    with pytest.raises(_lib.DpiError):
        ops.model_reg(torch.zeros(1, 1, 4, 4), (2,))             # a CPU tensor
    with pytest.raises(_lib.DpiError):
        ops.model_reg(torch.zeros(1, 1, 4, 4, device=DEV, dtype=torch.float64), (2,))
    with pytest.raises(_lib.DpiError):
        ops.model_reg(torch.zeros(1, 1, 4, 8, device=DEV)[..., ::2], (2,))
    with pytest.raises(_lib.DpiError):
        ops.model_reg(torch.zeros(1, 1, 4, 4, device=DEV), (1,))             # channels are never differenced
    with pytest.raises(_lib.DpiError):
        ops.model_reg(torch.zeros(2, 1, 4, 4, device=DEV), (2,))


# ---------------------------------------------------------------- the loop --------------------------------------------------------
CONFIGS = {       # flags, patch shape (numpy order, channels last)
    "2d": (["--datadim", "2d"], (32, 32, 1)),
    "3d": (["--datadim", "3d", "--upsample", "linear"], (16, 16, 16, 1)),
}
W = 0.5
CASES = {         # config, operator flags, kind
    "wavelet-l1": ("3d", ["--wavelet", "w.npy"], "l1"),
    "moveout-tv_x": ("3d", ["--moveout", "tau.npy"], "tv_x"),
    "plain-tv": ("2d", [], "tv"),
}


def _run(tmp_path, case, reg=True, extra=(), mode=None, tag="", optimise=True):
    """The tiny multiunet of tests/test_gpu_wavelet.py (filters 4 8, skip 4, 8 input channels) on a tiny patch of the hyperbolic stand-in,
    half the traces missing, 4 iterations; mode None: "auto" with the flag (which must choose eager), "eager" without.  Returns (Interpolator, run file, the network's own output of every iteration)."""
    from deep_prior_interpolation_amd.main import Interpolator
    from deep_prior_interpolation_amd.parameter import parse_arguments
    config, op_flags, kind = CASES[case]
    flags, shape = CONFIGS[config]
    out = tmp_path / ("%s_%s%s" % (case, "on" if reg else "off", tag))
    os.makedirs(out)
    np.save(out / "w.npy", u.ricker(0.12, 1.0, 9))
    a = parse_arguments(["--imgdir", str(out), "--filters", "4", "8", "--skip", "4", "--inputdepth", "8", "--gain", "40", "--epochs", "4",
                         "--gpu", "0"] + flags + op_flags + (["--model_reg", kind, "--model_reg_weight", str(W)] if reg else []) + list(extra))
    traces = u.random_trace_mask(shape[:3] if config == "3d" else shape[:2] + (1,), 0.5, seed=4)
    if config == "3d":
        vol, traces = u.hyperbolic_volume(shape[:3], seed=3)[..., None], traces[..., None]
    else:
        vol = u.hyperbolic_volume(shape, seed=3)
    vol = vol.astype(np.float64) * a.gain
    data = {"image": vol, "mask": np.broadcast_to(traces, vol.shape).astype(np.float64), "name": "0"}
    if "--moveout" in op_flags:
        data["moveout"] = shift_table(shape[:-1], np.random.RandomState(5).uniform(0.0, 3.0, shape[1:-1]))
    u.set_seed(0)
    T = Interpolator(a, str(out))
    T.load_data(data)
    T.begin_patch(0)
    T.build_model()
    T.build_input()
    T.build_regularizer()
    seen = []
    inner = T._net_forward

    def spy(z):
        out = inner(z)
        seen.append(out.detach().clone())
        return out
    T._net_forward = spy
    if not optimise:
        return T, None, seen
    T.optimize(verbose=False, mode=mode or ("auto" if reg else "eager"))
    T.save_result()
    return T, np.load(out / "0_run.npy", allow_pickle=True).item(), seen


def _weights(T):
    return {k: v.detach().cpu().numpy().copy() for k, v in T.net.state_dict().items()}


@pytest.mark.parametrize("case", sorted(CASES))
def test_loop_adds_the_weighted_penalty(tmp_path, case):
    from deep_prior_interpolation_amd.parameter import model_reg_axes
    config, _, kind = CASES[case]
    T, run, seen = _run(tmp_path, case)
    h = T.history
    assert type(h) is u.HistoryModelReg and len(h) == 4 and len(seen) == 4
    loss, df, mreg = np.array(h.loss), np.array(h.df), np.array(h.model_reg)
    assert np.isfinite(loss).all() and (mreg > 0).all() and (df > 0).all()
    # total = fl(fl32(misfit) + fl(W * R)): three roundings, each at most 2^-24 of a quantity no larger than the total
    assert np.all(np.abs(loss - (df + W * mreg)) <= 4 * 2.0 ** -24 * loss)
    assert h.reg == [0.0] * 4
    assert "MREG" in h.log_message(3)
    # iteration 0: the penalty of the tensor the network itself wrote, before any operator
    m0 = seen[0].cpu().numpy()
    dims = model_reg_axes(kind, config, "xy")
    assert T.model_reg == (kind, W, dims)
    R, _, bar = MR.bar(MR.as_4d(m0), MR.dims_to_bits(dims, m0.ndim))
    print("%s: model_reg[0] = %.6e, restatement %.6e, bar %.3e (+ one fp32 rounding)" % (case, mreg[0], R, bar))
    assert abs(mreg[0] - R) <= bar + 2.0 ** -24 * abs(R)         # R comes back as an fp32 scalar: one more rounding than the bar counts
    if CASES[case][1]:                                           # behind an operator the penalised tensor is not the output
        assert T.forward_model.pre is not None and T.forward_model.pre.shape == seen[0].shape
    # the term reaches the weights
    T0, run0, seen0 = _run(tmp_path, case, reg=False)
    assert type(T0.history) is u.History and seen0 and "model_reg" not in run0
    w1, w0 = _weights(T), _weights(T0)
    assert any(not np.array_equal(w1[k], w0[k]) for k in w0 if w0[k].dtype.kind == "f")
    assert np.array(T0.history.loss)[0] == df[0]                 # the same seed: iteration 0 sees the same misfit
    # never captured, and said so
    assert T.has_regularizer() and not T.graph_capable() and "regulariser" in T._eager_reasons() and T0.graph_capable()
    assert run["model_reg"] == kind and run["model_reg_weight"] == W and type(run["history"]) is u.HistoryModelReg
    assert run["history"].model_reg == h.model_reg


def test_explicit_graph_mode_is_refused(tmp_path):
    T, _, _ = _run(tmp_path, "plain-tv", optimise=False)
    with pytest.raises(ValueError, match="--model_reg"):
        T.optimize(verbose=False, mode="graph")
    ops.set_weight_grad_overlap(False, in_graph=False)
    with pytest.raises(ValueError, match="--model_reg"):
        T.graph_prepare()
    assert len(T.history.loss) == 0


@pytest.mark.parametrize("case", ["plain-tv", "wavelet-l1"])
def test_loop_with_aa_weight_holds_all_three_terms(tmp_path, case):
    T, run, _ = _run(tmp_path, case, extra=("--aa_weight", "0.5", "--aa_smooth", "2"))
    h = T.history
    loss, df, reg, mreg = (np.array(c) for c in (h.loss, h.df, h.reg, h.model_reg))
    assert type(h) is u.HistoryModelReg and (reg > 0).all() and (mreg > 0).all()
    # fl32(misfit), fl(aa * R_aa), their sum, fl(W * R), the total: five roundings, each at most 2^-24 of a quantity no larger than the total
    assert np.all(np.abs(loss - (df + 0.5 * reg + W * mreg)) <= 5 * 2.0 ** -24 * loss)
    # the anti-aliasing column is what a run without --model_reg records at iteration 0 (same seed, same weights there)
    T0, _, _ = _run(tmp_path, case, reg=False, extra=("--aa_weight", "0.5", "--aa_smooth", "2"))
    assert type(T0.history) is u.HistoryReg and T0.history.reg[0] == reg[0] and T0.history.df[0] == df[0]


def test_loop_with_holdout_and_out_ema(tmp_path):
    T, run, _ = _run(tmp_path, "plain-tv", extra=("--holdout", "0.2", "--out_ema", "0.9"))
    h = T.history
    assert type(h) is u.HistoryModelRegHoldoutEma and len(h) == 4
    loss, df, mreg = np.array(h.loss), np.array(h.df), np.array(h.model_reg)
    assert np.all(np.abs(loss - (df + W * mreg)) <= 4 * 2.0 ** -24 * loss)
    # val_loss stays the pure misfit: that of the run without the flag at iteration 0 (same seed, same split, same weights there)
    T0, _, _ = _run(tmp_path, "plain-tv", reg=False, extra=("--holdout", "0.2", "--out_ema", "0.9"))
    assert h.val_loss[0] == T0.history.val_loss[0] and h.ema_loss[0] == T0.history.ema_loss[0]
    assert run["best_iter"] == T.best_iter and np.isfinite(run["output"]).all()
