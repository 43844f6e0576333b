"""GPU tests of --out_ema (the output selected from an exponential running average of the iterates): the streaming pass against a
float64 recursion and against the loss passes run on the stored average, the device loop control against a host model, graph against
eager, the untouched trajectory, the selection rule and the recursion end to end."""
import os
from argparse import Namespace

import numpy as np
import pytest
import torch

import iteration_cases as I
from conftest import jstr
from gpu_guard import guard

pytestmark = pytest.mark.gpu
DEV = "cuda"
BETA = 0.9


# ---------------------------------------------------------------- the pass ---------------------------------------------------------------
def _view(data, off):
    """`data` flattened on the device, `off` floats behind an allocation's (at least 256-byte aligned) start."""
    flat = torch.as_tensor(np.ascontiguousarray(data, dtype=np.float32).ravel())
    buf = torch.empty(flat.numel() + 4, dtype=torch.float32, device=DEV)
    v = buf[off:off + flat.numel()]
    v.copy_(flat)
    assert v.data_ptr() % 16 == 4 * off
    return v


def _fields(shape, seed, off, sel_p=0.3):
    """img, mask, sel of a patch (1, C, T, S...): random traces with a few dropped samples, a random 0/1 per known trace."""
    rng = np.random.RandomState(seed)
    C_, S_ = shape[1], shape[3:]
    img = rng.randn(*shape)
    tr = (rng.rand(1, C_, 1, *S_) > 0.4)
    m = np.broadcast_to(tr, shape) * (rng.rand(*shape) > 0.05)
    sel = (rng.rand(C_, *S_) < sel_p) & tr[0, :, 0]
    return _view(img, off), _view(m, off), _view(sel, off), rng


def _ema_call(shape, out, avg, img, mask, sel, kind, beta, it, active=None, res=None):
    from deep_prior_interpolation_amd import _lib
    L = _lib.load()
    n = out.numel()
    C_, T_ = shape[1], shape[2]
    step_lr = torch.tensor([float(it), 1e-3], dtype=torch.float32, device=DEV)
    ws = torch.empty(2 * L.dpi_loss_ws_doubles(n), dtype=torch.float64, device=DEV)
    if res is None:
        res = torch.full((11,), -7.0, dtype=torch.float64, device=DEV)
    _lib.check(L.dpi_ema_loss(out.data_ptr(), avg.data_ptr(), img.data_ptr(), mask.data_ptr(), None if sel is None else sel.data_ptr(),
                              C_, T_, n // (C_ * T_), kind, float(beta), step_lr.data_ptr(), None if active is None else active.data_ptr(),
                              ws.data_ptr(), res.data_ptr(), _lib.stream()), "dpi_ema_loss")
    torch.cuda.synchronize()
    return res


def _loss_call(shape, out, img, mask, sel, kind):
    """result doubles of dpi_masked_loss (sel None) / dpi_masked_loss_holdout on `out`."""
    from deep_prior_interpolation_amd import _lib
    L = _lib.load()
    n = out.numel()
    C_, T_ = shape[1], shape[2]
    dout = torch.empty(n, dtype=torch.float32, device=DEV)
    ws = torch.empty(2 * L.dpi_loss_ws_doubles(n), dtype=torch.float64, device=DEV)
    res = torch.full((11,), -7.0, dtype=torch.float64, device=DEV)
    if sel is None:
        _lib.check(L.dpi_masked_loss(out.data_ptr(), img.data_ptr(), mask.data_ptr(), n, kind, 1.0, dout.data_ptr(), ws.data_ptr(),
                                     res.data_ptr(), _lib.stream()))
    else:
        _lib.check(L.dpi_masked_loss_holdout(out.data_ptr(), img.data_ptr(), mask.data_ptr(), sel.data_ptr(), C_, T_, n // (C_ * T_), kind,
                                             1.0, dout.data_ptr(), ws.data_ptr(), res.data_ptr(), _lib.stream()))
    torch.cuda.synchronize()
    return res.cpu().numpy()


# odd 3-D, 2-D [C][T][X], tiny with several channels, several sweeps of a multi-block grid with two channels
SHAPES = [(1, 1, 17, 13, 11), (1, 3, 19, 23), (1, 3, 7, 5, 3), (1, 2, 24, 96, 64)]
STEPS = 5


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("shape", SHAPES)
def test_recursion_against_float64(shape, off):
    """Five calls (it = 0..4) on fresh outputs against avg_0 = out_0, avg_k = avg + w (out_k - avg) in float64 with the kernel's w.
    Bar: per step three fp32 roundings (the difference, the product, the sum) of at most 2^-24 relative on magnitudes <= 2 max|out|,
    under 2^-21 max|out|; over K steps at most K times that (the recursion contracts earlier errors)."""
    n = int(np.prod(shape))
    img, mask, sel, rng = _fields(shape, 11, off)
    g = guard(n, torch.float32, DEV, offset=off)                    # payload NaN: nothing of it may survive iteration 0
    avg = g.payload
    assert avg.data_ptr() % 16 == 4 * off and bool(torch.isnan(avg).all())
    w = float(np.float32(1.0 - float(np.float32(BETA))))
    ref, top = None, 0.0
    for it in range(STEPS):
        o = rng.randn(n).astype(np.float32) * 3.0
        top = max(top, float(np.abs(o).max()))
        out = _view(o, off)
        _ema_call(shape, out, avg, img, mask, sel, it % 2, BETA, it)
        got = avg.cpu().numpy()
        if it == 0:
            np.testing.assert_array_equal(got.view(np.uint32), o.view(np.uint32))
            ref = o.astype(np.float64)
        else:
            ref = ref + w * (o.astype(np.float64) - ref)
        err = float(np.abs(got.astype(np.float64) - ref).max())
        bar = (it + 1) * 2.0 ** -21 * top
        print("shape %s off %d it %d: max err %.3e, bar %.3e" % (shape, off, it, err, bar))
        assert err <= bar
    g.check("avg")


def _agree(a, b, scale=None):
    tol = 1e-9 * (abs(b) if scale is None else scale)
    assert abs(a - b) <= tol, (a, b, tol)


@pytest.mark.parametrize("with_sel", [False, True])
@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("shape", SHAPES[:2] + [SHAPES[3], (1, 2, 48, 96, 260)])        # the last one fills the capped grid of 1024 blocks
def test_metrics_are_those_of_the_loss_pass_on_the_average(shape, kind, with_sel):
    n = int(np.prod(shape))
    off = 1 if shape == SHAPES[1] else 0
    img, mask, sel, rng = _fields(shape, 5, off)
    if not with_sel:
        sel = None
    avg = _view(np.full(n, np.nan), off)
    base = img.cpu().numpy()
    for it in range(3):          # outputs correlated with the target: a PCORR of order one
        out = _view(0.6 * base + 0.8 * rng.randn(n), off)
        res = _ema_call(shape, out, avg, img, mask, sel, kind, BETA, it).cpu().numpy()
        ref = _loss_call(shape, avg, img, mask, sel, kind)
        a64, t64 = avg.double(), img.double()
        mags = {5: float(a64.abs().sum()), 6: float(t64.abs().sum())}       # signed sums: relative to the sum of magnitudes
        for k in range(7):
            _agree(res[k], ref[k], mags.get(k))
        if with_sel:
            _agree(res[8], ref[8])
            _agree(res[9], ref[9])
            assert res[10] == ref[10] and res[10] > 0
            mh = (mask.view(shape) * sel.view((1, shape[1], 1) + tuple(shape[3:]))) != 0
            assert res[10] == float(mh.sum())
        else:
            np.testing.assert_array_equal(res[8:], [-7.0, -7.0, -7.0])     # only [0..7] are written
    # and it is the average the numbers speak of, not the last output
    raw = _loss_call(shape, out, img, mask, sel, kind)
    assert abs(raw[0] - res[0]) > 1e-3 * abs(res[0])


@pytest.mark.parametrize("with_sel", [False, True])
def test_inactive_leaves_average_and_result_alone(with_sel):
    shape = SHAPES[0]
    n = int(np.prod(shape))
    img, mask, sel, rng = _fields(shape, 2, 0)
    g = guard(n, torch.float32, DEV, fill=torch.from_numpy(rng.randn(n).astype(np.float32)))
    out = _view(rng.randn(n), 0)
    res = torch.arange(11, dtype=torch.float64, device=DEV) + 0.5
    before, res_before = g.bits(), res.clone()
    active = torch.zeros(1, dtype=torch.int32, device=DEV)
    for it in (0, 3):
        _ema_call(shape, out, g.payload, img, mask, sel if with_sel else None, 0, BETA, it, active=active, res=res)
        assert g.untouched(before) and torch.equal(res.view(torch.int64), res_before.view(torch.int64))
    g.check("avg")
    active.fill_(1)
    _ema_call(shape, out, g.payload, img, mask, sel if with_sel else None, 0, BETA, 3, active=active, res=res)
    assert not g.untouched(before) and not torch.equal(res[:7], res_before[:7])
    g.check("avg")


# ---------------------------------------------------------------- loop control ----------------------------------------------------------
SCRIPTS = I.EMA_SCRIPTS          # shared with the host tests (tests/iteration_cases.py), as is the model of the eager rules


@pytest.mark.parametrize("ho", [0, 1])
@pytest.mark.parametrize("name", sorted(SCRIPTS))
def test_loop_control_against_host_model(name, ho):
    from deep_prior_interpolation_amd import _lib
    L = _lib.load()
    rows, plateau, es = SCRIPTS[name]
    lr0, cols = 1e-3, 10 if ho else 6
    ref = I.eager_loop_model(rows, lr0, plateau, es)
    metrics = torch.zeros(11, dtype=torch.float64, device=DEV)
    ema = torch.zeros(11, dtype=torch.float64, device=DEV)
    state = torch.zeros(12, dtype=torch.float64, device=DEV)
    state[2] = float("inf")
    hist = torch.zeros(cols * len(rows), dtype=torch.float64, device=DEV)
    step_lr = torch.tensor([1.0, lr0], dtype=torch.float32, device=DEV)
    active = torch.ones(1, dtype=torch.int32, device=DEV)
    improved = torch.zeros(1, dtype=torch.int32, device=DEV)
    got = []
    for it, (loss, q) in enumerate(rows):
        metrics[0], metrics[1], metrics[2], metrics[8], metrics[9] = loss, 10.0 + it, 0.5, 3.0 + it, 20.0 + it
        if ho:      # the selection follows ema_val_loss; ema_loss is a decoy that would select differently
            ema[0], ema[1], ema[8], ema[9] = 5.0 + it, 30.0 + it, q, 40.0 + it
        else:
            ema[0], ema[1], ema[8], ema[9] = q, 30.0 + it, 5.0 - it, 40.0 + it
        _lib.check(L.dpi_loop_control_ema(metrics.data_ptr(), ema.data_ptr(), ho, state.data_ptr(), hist.data_ptr(), len(rows),
                                          step_lr.data_ptr(), active.data_ptr(), improved.data_ptr(), int(plateau is not None),
                                          *(plateau if plateau else (0.9, 1e-5, 100)), 0.0, 1e-8, es[0], es[1], _lib.stream()))
        torch.cuda.synchronize()
        if it < len(ref):
            got.append((int(improved.item()), None, int(state[9].item())))
        if not active.item():
            break
    n = int(state[0].item())
    assert n == len(ref) == len(got), (n, len(ref), len(got))
    assert [g[0] for g in got] == [r[0] for r in ref]
    assert [g[2] for g in got] == [r[2] for r in ref]
    h = hist[:cols * n].view(n, cols).cpu().numpy()
    np.testing.assert_allclose(h[:, 3], [r[1] for r in ref], rtol=1e-7)
    np.testing.assert_array_equal(h[:, 0], [r[0] for r in rows[:n]])
    np.testing.assert_array_equal(h[:, 1], 10.0 + np.arange(n))
    k = 4
    if ho:
        np.testing.assert_array_equal(h[:, 4], 3.0 + np.arange(n))
        np.testing.assert_array_equal(h[:, 5], 20.0 + np.arange(n))
        k = 6
        np.testing.assert_array_equal(h[:, k], 5.0 + np.arange(n))
        np.testing.assert_array_equal(h[:, k + 2], [r[1] for r in rows[:n]])
        np.testing.assert_array_equal(h[:, k + 3], 40.0 + np.arange(n))
        assert state[8].item() == 3.0                       # the raw held-out minimum
    else:
        np.testing.assert_array_equal(h[:, k], [r[1] for r in rows[:n]])
    np.testing.assert_array_equal(h[:, k + 1], 30.0 + np.arange(n))
    finite = [r[1] for r in rows[:n] if r[1] == r[1]]
    assert state[10].item() == min(finite)
    if name in ("rising", "nan"):
        assert active.item() == 0 and n < len(rows)
    if name == "nan_raw":
        assert active.item() == 1 and n == len(rows)
    if name == "plateau":
        assert h[-1, 3] < h[0, 3] and active.item() == 1
    if name == "ties":
        assert [g[2] for g in got] == [0, 1, 2, 3, 3, 5]


# ---------------------------------------------------------------- the loop --------------------------------------------------------------
def _golden_interp(g, epochs, holdout, ema=BETA, seed=7):
    from deep_prior_interpolation_amd.main import Interpolator
    a = Namespace(**jstr(g["args"]))
    a.epochs, a.gpu, a.holdout, a.out_ema = epochs, 0, holdout, ema
    T = Interpolator(a, "/tmp")
    T.load_data({"image": g["image"], "mask": g["mask"], "name": "0"})
    T.begin_patch(seed)
    T.build_model()
    T.build_input()
    return T, a


def _interp3d(extra, epochs, shape=(16, 16, 16), index=0):
    from deep_prior_interpolation_amd.main import Interpolator
    from deep_prior_interpolation_amd.parameter import parse_arguments
    from deep_prior_interpolation_amd import utils as u
    a = parse_arguments(["--imgdir", "x", "--datadim", "3d", "--filters", "4", "8", "16", "--skip", "4", "8", "--inputdepth", "8",
                         "--upsample", "linear", "--epochs", str(epochs), "--gpu", "0"] + extra)
    vol = u.hyperbolic_volume(shape, seed=3)[..., None].astype(np.float64) * 10.0
    mask = u.random_trace_mask(shape, 0.5, seed=4)[..., None].astype(np.float64)
    T = Interpolator(a, "/tmp")
    T.load_data({"image": vol, "mask": np.broadcast_to(mask, vol.shape).copy(), "name": str(index)})
    T.begin_patch(index)
    T.build_model()
    T.build_input()
    return T


def _columns(h):
    names = ["loss", "snr", "pcorr", "lr"] + [c for c in ("val_loss", "val_snr", "ema_loss", "ema_snr", "ema_val_loss", "ema_val_snr")
                                              if hasattr(h, c)]
    return names, [np.array(getattr(h, c)) for c in names]


def _result(T):
    names, cols = _columns(T.history)
    assert "ema_loss" in names and len(T.history) == len(cols[0])
    return (cols, T.out_best.copy(), T.best_iter, {k: v.detach().cpu().numpy().copy() for k, v in T.net.state_dict().items()}, names)


def _same(r1, r2, params_only=False):
    """params_only: after an early stop the captured graph may still be replayed up to check_every times before the host polls `active`:
    Adam is gated on the device, the BatchNorm running statistics (buffers, unused in the training-mode forward) are not."""
    assert r1[4] == r2[4]
    for name, c1, c2 in zip(r1[4], r1[0], r2[0]):
        if name == "lr":      # the eager loop logs the Python float, the device history the fp32 value the kernels use
            np.testing.assert_allclose(c2, c1, rtol=1e-6)
        else:
            np.testing.assert_array_equal(c1, c2, err_msg=name)
    np.testing.assert_array_equal(r1[1], r2[1])
    assert r1[2] == r2[2] and r1[2] is not None
    for k, v in r1[3].items():
        if params_only and ("running_" in k or "num_batches_tracked" in k):
            continue
        np.testing.assert_array_equal(r2[3][k], v, err_msg=k)


@pytest.mark.parametrize("holdout", [0.0, 0.25])
def test_graph_equals_eager(golden, holdout):
    from deep_prior_interpolation_amd import utils as u
    g = golden("net_mulresunet3d_tiny_trilinear_mae")
    res = {}
    for mode in ("eager", "graph"):
        T, a = _golden_interp(g, 12, holdout)
        T.optimize(verbose=False, mode=mode, check_every=5)
        assert type(T.history) is (u.HistoryHoldoutEma if holdout else u.HistoryEma)
        res[mode] = _result(T)
    assert len(res["graph"][0][0]) == 12 and len(res["graph"][4]) == (10 if holdout else 6)
    _same(res["eager"], res["graph"])
    e = res["eager"]
    q = e[0][e[4].index("ema_val_loss" if holdout else "ema_loss")]
    assert e[2] == len(q) - 1 - int(np.argmin(q[::-1]))
    assert not np.array_equal(e[0][e[4].index("ema_snr")][1:], e[0][1][1:])        # an average, not the iterate


def test_graph_equals_eager_early_stop_and_plateau(golden):
    g = golden("net_mulresunet3d_tiny_nearest_mse")
    res = {}
    for mode in ("eager", "graph"):
        T, a = _golden_interp(g, 40, 0.3, seed=3)
        a.reduce_lr, a.lr_patience, a.lr_factor, a.lr_thresh = True, 1, 0.5, 0.9
        a.earlystop_patience, a.earlystop_min_delta = 6, 20.0
        T.optimize(verbose=False, mode=mode, check_every=4)
        res[mode] = _result(T)
    n = len(res["eager"][0][0])
    assert len(res["graph"][0][0]) == n < 40
    _same(res["eager"], res["graph"], params_only=True)
    assert res["eager"][0][3][-1] < res["eager"][0][3][0]


def test_concurrent_slots():
    from deep_prior_interpolation_amd.main import optimize_concurrently
    solo = []
    for i in range(2):
        T = _interp3d(["--out_ema", str(BETA)], 6, index=i)
        T.optimize(verbose=False, mode="graph", check_every=2)
        solo.append(_result(T))
    Ts = [_interp3d(["--out_ema", str(BETA)], 6, index=i) for i in range(2)]
    optimize_concurrently(Ts, check_every=2)
    for T, r in zip(Ts, solo):
        _same(r, _result(T))


def test_trajectory_is_untouched_and_run_file_keys(tmp_path):
    """The average only watches: with default patience (no early stop) loss, snr, lr and the final weights of a run with the flag are bit
    for bit those of a run without it, and without the flag the run file has today's keys."""
    runs = {}
    for key, extra in (("off", []), ("ema", ["--out_ema", str(BETA)])):
        T = _interp3d(extra, 12)
        T.outpath = str(tmp_path)
        T.image_name = key
        T.optimize(verbose=False, mode="eager")
        T.save_result()
        runs[key] = (T.history, {k: v.detach().cpu().numpy().copy() for k, v in T.net.state_dict().items()}, T.out_best.copy(),
                     np.load(os.path.join(str(tmp_path), key + "_run.npy"), allow_pickle=True).item())
    h0, h1 = runs["off"][0], runs["ema"][0]
    for c in ("loss", "snr", "pcorr", "lr"):
        np.testing.assert_array_equal(np.array(getattr(h0, c)), np.array(getattr(h1, c)), err_msg=c)
    for k, v in runs["off"][1].items():
        np.testing.assert_array_equal(runs["ema"][1][k], v, err_msg=k)
    assert not np.array_equal(runs["off"][2], runs["ema"][2])
    r0, r1 = runs["off"][3], runs["ema"][3]
    assert sorted(r0) == ["device", "elapsed", "history", "image", "mask", "noise", "outpath", "output"]
    assert sorted(set(r1) - set(r0)) == ["best_iter", "out_ema"]
    assert r1["out_ema"] == BETA and r1["best_iter"] == len(h1.ema_loss) - 1 - int(np.argmin(np.array(h1.ema_loss)[::-1]))
    np.testing.assert_array_equal(r1["output"], runs["ema"][2])
    assert not hasattr(r0["history"], "ema_loss") and r1["history"].ema_snr == h1.ema_snr


def test_selection_follows_the_average_and_snapshots_it():
    """best_iter is the last argmin of ema_loss, and out_best is the average AS IT WAS at best_iter: its SNR against the image, computed on
    the host, is ema_snr[best_iter] — the next iterations overwrote the average itself.  Patches are tried in index order until one
    selects an iteration before the last.  beta 0.5: a window of two iterations keeps about half of the iterates' jitter, so the
    average's misfit is not monotone over the run; with 0.9 it falls until the last of these 100 iterations on every patch tried, and
    a snapshot could not be told from the live buffer."""
    from deep_prior_interpolation_amd import utils as u
    epochs, seen = 100, []
    for index in range(6):
        T = _interp3d(["--out_ema", "0.5", "--lr", "3e-3"], epochs, index=index)
        T.optimize(verbose=False, mode="eager")
        q = np.array(T.history.ema_loss)
        assert len(q) == epochs and T.best_iter == len(q) - 1 - int(np.argmin(q[::-1]))
        seen.append((index, T.best_iter))
        if T.best_iter < epochs - 1:
            break
    assert T.best_iter < epochs - 1, seen
    host = float(u.snr(T.out_best.astype(np.float64), T.img[..., 0].astype(np.float32).astype(np.float64)))
    print("patch %d: best_iter %d, host SNR %.6f, ema_snr[best] %.6f, ema_snr[-1] %.6f"
          % (index, T.best_iter, host, T.history.ema_snr[T.best_iter], T.history.ema_snr[-1]))
    assert abs(host - T.history.ema_snr[T.best_iter]) <= 1e-4
    assert abs(host - T.history.ema_snr[-1]) > 1e-4
    assert T.ema_snr() == T.history.ema_snr[T.best_iter]


def test_recursion_end_to_end(tmp_path):
    """out_0 from a one-iteration run, out_1.. from --save_every 1 (which keeps saving the raw iterate): the float64 recursion over them is
    out_best at best_iter, within the bar of test_recursion_against_float64."""
    T0 = _interp3d([], 1)
    T0.optimize(verbose=False, mode="eager")
    out0 = T0.out_best.astype(np.float64)
    N = 10
    T = _interp3d(["--out_ema", str(BETA), "--save_every", "1"], N)
    T.outpath = str(tmp_path)
    T.optimize(verbose=False)
    assert len(T.history.ema_loss) == N and T.best_iter is not None
    w = float(np.float32(1.0 - float(np.float32(BETA))))
    ref, top = out0, float(np.abs(out0).max())
    for k in range(1, T.best_iter + 1):
        o = np.load(os.path.join(str(tmp_path), "0_output%s.npy" % str(k).zfill(T.zfill))).astype(np.float64)
        top = max(top, float(np.abs(o).max()))
        ref = ref + w * (o - ref)
    err, bar = float(np.abs(T.out_best.astype(np.float64) - ref).max()), (T.best_iter + 1) * 2.0 ** -21 * top
    print("best_iter %d: max err %.3e, bar %.3e" % (T.best_iter, err, bar))
    assert err <= bar
    if T.best_iter > 0:
        assert float(np.abs(T.out_best - o).max()) > 1e3 * bar         # not the raw iterate
