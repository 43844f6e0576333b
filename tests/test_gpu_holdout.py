"""GPU tests of --holdout (self-validation on held-out traces): the fused loss pass against dpi_masked_loss and float64 numpy, the
device loop control against a host model, graph against eager, the selection rule, concurrent slots and the CLI end to end."""
import os
from argparse import Namespace

import numpy as np
import pytest
import torch

import iteration_cases as I
from conftest import jstr

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _loss_pair(shape, sel_p, kind, seed=0):
    """(out, img, mask, sel) on the device; mask: random traces with a few dropped samples, sel: random 0/1 per (c, s)."""
    rng = np.random.RandomState(seed)
    C_, S_ = shape[1], shape[3:]
    out = torch.from_numpy(rng.randn(*shape).astype(np.float32)).to(DEV)
    img = torch.from_numpy(rng.randn(*shape).astype(np.float32)).to(DEV)
    tr = (rng.rand(1, C_, 1, *S_) > 0.4).astype(np.float32)
    m = np.broadcast_to(tr, shape) * (rng.rand(*shape) > 0.05)
    sel = ((rng.rand(C_, *S_) < sel_p) & (tr[0, :, 0] > 0)).astype(np.float32)
    return out, img, torch.from_numpy(np.ascontiguousarray(m, dtype=np.float32)).to(DEV), torch.from_numpy(sel).to(DEV)


def _raw(out, img, mask, kind, sel=None):
    """dout and result doubles of one raw call of dpi_masked_loss (sel None) or dpi_masked_loss_holdout."""
    from deep_prior_interpolation_amd import _lib
    L = _lib.load()
    n = out.numel()
    dout = torch.full_like(out, 7.0)
    ws = torch.empty(2 * L.dpi_loss_ws_doubles(n), dtype=torch.float64, device=DEV)
    if sel is None:
        res = torch.empty(8, dtype=torch.float64, device=DEV)
        _lib.check(L.dpi_masked_loss(out.data_ptr(), img.data_ptr(), mask.data_ptr(), n, kind, 1.0, dout.data_ptr(), ws.data_ptr(),
                                     res.data_ptr(), _lib.stream()))
    else:
        C_, T_ = out.shape[1], out.shape[2]
        res = torch.empty(11, dtype=torch.float64, device=DEV)
        _lib.check(L.dpi_masked_loss_holdout(out.data_ptr(), img.data_ptr(), mask.data_ptr(), sel.data_ptr(), C_, T_, n // (C_ * T_), kind,
                                             1.0, dout.data_ptr(), ws.data_ptr(), res.data_ptr(), _lib.stream()))
    torch.cuda.synchronize()
    return dout.cpu().numpy(), res.cpu().numpy()


SHAPES = [(1, 1, 17, 13, 11), (1, 3, 19, 23), (1, 2, 48, 96, 260)]       # odd 3-D, 2-D [C][T][X], multi-block grid with several channels


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("kind", [0, 1])
def test_loss_pass_is_masked_loss_on_the_training_mask(shape, kind):
    out, img, mask, sel = _loss_pair(shape, 0.3, kind)
    zero = torch.zeros_like(sel)
    d0, r0 = _raw(out, img, mask, kind)
    d1, r1 = _raw(out, img, mask, kind, zero)
    np.testing.assert_array_equal(d1.view(np.uint32), d0.view(np.uint32))
    np.testing.assert_array_equal(r1[:8].view(np.uint64), r0[:8].view(np.uint64))
    h = sel.reshape((1, shape[1], 1) + tuple(shape[3:]))
    m_tr = mask * (1 - h)
    d2, r2 = _raw(out, img, m_tr.contiguous(), kind)
    d3, r3 = _raw(out, img, mask, kind, sel)
    np.testing.assert_array_equal(d3.view(np.uint32), d2.view(np.uint32))
    np.testing.assert_array_equal(r3[:8].view(np.uint64), r2[:8].view(np.uint64))
    held = np.broadcast_to((mask * h).cpu().numpy() != 0, shape)
    assert held.sum() > 0 and np.all(d3[held] == 0)


@pytest.mark.parametrize("shape", SHAPES[:2])
@pytest.mark.parametrize("kind", [0, 1])
def test_validation_numbers_against_float64(shape, kind):
    out, img, mask, sel = _loss_pair(shape, 0.4, kind, seed=3)
    _, r = _raw(out, img, mask, kind, sel)
    o, t = out.cpu().numpy().astype(np.float64), img.cpu().numpy().astype(np.float64)
    mh = mask.cpu().numpy().astype(np.float64) * sel.cpu().numpy().reshape((1, shape[1], 1) + tuple(shape[3:]))
    e = (o - t) * mh
    n_ho = int((mh != 0).sum())
    val = (np.square(e) if kind == 1 else np.abs(e)).sum() / n_ho
    vsnr = 10 * np.log10(np.square(t * mh).sum() / np.square(e).sum())
    assert r[10] == n_ho
    assert abs(r[8] - val) <= 1e-6 * val
    assert abs(r[9] - vsnr) <= 1e-6 * abs(vsnr) + 1e-9


# ---------------------------------------------------------------- loop control ----------------------------------------------------------
SCRIPTS = I.HOLDOUT_SCRIPTS          # shared with the host tests (tests/iteration_cases.py), as is the model of the eager rules


@pytest.mark.parametrize("name", sorted(SCRIPTS))
def test_loop_control_against_host_model(name):
    from deep_prior_interpolation_amd import _lib
    L = _lib.load()
    rows, plateau, es = SCRIPTS[name]
    lr0 = 1e-3
    ref = I.eager_loop_model(rows, lr0, plateau, es)
    metrics = torch.zeros(11, dtype=torch.float64, device=DEV)
    state = torch.zeros(10, dtype=torch.float64, device=DEV)
    state[2] = float("inf")
    hist = torch.zeros(6 * len(rows), dtype=torch.float64, device=DEV)
    step_lr = torch.tensor([1.0, lr0], dtype=torch.float32, device=DEV)
    active = torch.ones(1, dtype=torch.int32, device=DEV)
    improved = torch.zeros(1, dtype=torch.int32, device=DEV)
    got = []
    for it, (loss, val) in enumerate(rows):
        metrics[0], metrics[1], metrics[2], metrics[8], metrics[9] = loss, 10.0 + it, 0.5, val, 20.0 + it
        _lib.check(L.dpi_loop_control_holdout(metrics.data_ptr(), state.data_ptr(), hist.data_ptr(), len(rows), step_lr.data_ptr(),
                                              active.data_ptr(), improved.data_ptr(), int(plateau is not None),
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
    h = hist[:6 * n].view(n, 6).cpu().numpy()
    np.testing.assert_allclose(h[:, 3], [r[1] for r in ref], rtol=1e-7)
    np.testing.assert_array_equal(h[:, 0], [r[0] for r in rows[:n]])
    np.testing.assert_array_equal(h[:, 4], [r[1] for r in rows[:n]])
    np.testing.assert_array_equal(h[:, 5], 20.0 + np.arange(n))
    if name in ("rising", "nan"):
        assert active.item() == 0 and n < len(rows)
    if name == "plateau":
        assert h[-1, 3] < h[0, 3]
    if name == "ties":
        assert [g[2] for g in got] == [0, 1, 2, 3, 3, 5]


# ---------------------------------------------------------------- the loop --------------------------------------------------------------
def _golden_interp(g, epochs, holdout, seed=7):
    from deep_prior_interpolation_amd.main import Interpolator
    a = Namespace(**jstr(g["args"]))
    a.epochs, a.gpu, a.holdout = epochs, 0, holdout
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


def _result(T):
    h = T.history
    return ([np.array(c) for c in (h.loss, h.snr, h.pcorr, h.lr, h.val_loss, h.val_snr)], T.out_best.copy(), T.best_iter,
            {k: v.detach().cpu().numpy().copy() for k, v in T.net.state_dict().items()})


def _same(r1, r2, params_only=False):
    """params_only: after an early stop the captured graph may still be replayed up to check_every times before the host polls `active`:
    Adam is gated on the device, the BatchNorm running statistics (buffers, unused in the training-mode forward) are not."""
    for k, (c1, c2) in enumerate(zip(r1[0], r2[0])):
        if k == 3:      # lr: the eager loop logs the Python float, the device history the fp32 value the kernels use
            np.testing.assert_allclose(c2, c1, rtol=1e-6)
        else:
            np.testing.assert_array_equal(c1, c2)
    np.testing.assert_array_equal(r1[1], r2[1])
    assert r1[2] == r2[2]
    for k, v in r1[3].items():
        if params_only and ("running_" in k or "num_batches_tracked" in k):
            continue
        np.testing.assert_array_equal(r2[3][k], v, err_msg=k)


def test_graph_equals_eager_with_holdout(golden):
    from deep_prior_interpolation_amd import utils as u
    g = golden("net_mulresunet3d_tiny_trilinear_mae")
    res = {}
    for mode in ("eager", "graph"):
        T, a = _golden_interp(g, 12, 0.25)
        T.optimize(verbose=False, mode=mode, check_every=5)
        assert type(T.history) is u.HistoryHoldout and T.holdout_sel.sum() > 0
        res[mode] = _result(T)
    assert len(res["graph"][0][0]) == 12
    _same(res["eager"], res["graph"])


def test_graph_equals_eager_early_stop_and_plateau_with_holdout(golden):
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


def test_graph_equals_eager_bf16_multires3d_with_holdout():
    res = {}
    for mode in ("eager", "graph"):
        T = _interp3d(["--holdout", "0.2", "--precision", "bf16"], 8)
        T.optimize(verbose=False, mode=mode, check_every=3)
        res[mode] = _result(T)
    _same(res["eager"], res["graph"])


def test_selection_follows_the_held_out_misfit(tmp_path):
    """Eager with --save_every 1: best_iter is the last argmin of val_loss and out_best is the output saved at best_iter.  Patches are
    tried in index order until one has best_iter > 0 (iteration 0's output is never saved) and one selects another iteration than the
    training-loss argmin would (so the test tells the two rules apart)."""
    checked, differs, seen = False, False, []
    for index in range(6):
        T = _interp3d(["--holdout", "0.15", "--save_every", "1", "--lr", "3e-3"], 100, index=index)
        T.outpath = str(tmp_path)
        T.optimize(verbose=False)
        v, l = np.array(T.history.val_loss), np.array(T.history.loss)
        last_argmin = len(v) - 1 - int(np.argmin(v[::-1]))
        assert T.best_iter == last_argmin
        assert T.holdout_snr() == T.history.val_snr[T.best_iter]
        if T.best_iter > 0:
            saved = np.load(os.path.join(str(tmp_path), "%d_output%s.npy" % (index, str(T.best_iter).zfill(T.zfill))))
            np.testing.assert_array_equal(T.out_best, saved)
            checked = True
        loss_argmin = len(l) - 1 - int(np.argmin(l[::-1]))
        differs |= loss_argmin != T.best_iter
        seen.append((index, T.best_iter, loss_argmin))
        if checked and differs:
            break
    assert checked and differs, seen


def test_concurrent_slots_with_holdout():
    from deep_prior_interpolation_amd.main import optimize_concurrently
    solo = []
    for i in range(2):
        T = _interp3d(["--holdout", "0.2"], 6, index=i)
        T.optimize(verbose=False, mode="graph", check_every=2)
        solo.append(_result(T))
    Ts = [_interp3d(["--holdout", "0.2"], 6, index=i) for i in range(2)]
    optimize_concurrently(Ts, check_every=2)
    for T, r in zip(Ts, solo):
        _same(r, _result(T))


def test_cli_end_to_end_3d_with_aa(tmp_path, monkeypatch, capsys):
    from deep_prior_interpolation_amd import main as M, utils as u
    from deep_prior_interpolation_amd.data import reconstruct_patches
    from deep_prior_interpolation_amd.parameter import parse_arguments
    monkeypatch.chdir(tmp_path)
    shape = (16, 16, 32)
    vol = u.hyperbolic_volume(shape, seed=1).astype(np.float32)
    mask = np.broadcast_to(u.random_trace_mask(shape, 0.5, seed=2), shape).astype(np.float32)
    np.save("vol.npy", vol)
    np.save("mask.npy", mask)
    argv = ["--imgdir", str(tmp_path), "--imgname", "vol.npy", "--maskname", "mask.npy", "--datadim", "3d", "--patch_shape", "16", "16", "16",
            "--filters", "4", "8", "--skip", "4", "--inputdepth", "4", "--upsample", "linear", "--epochs", "6", "--gpu", "0", "--gain", "10",
            "--aa_weight", "0.25", "--holdout", "0.1", "--outdir", "ho"]
    M.main(argv)
    assert "held-out SNR" in capsys.readouterr().out
    for name in ("0", "1"):
        r = np.load(os.path.join("results", "ho", name + "_run.npy"), allow_pickle=True).item()
        h = r["history"]
        assert isinstance(h, u.HistoryRegHoldout) and len(h) == 6 and np.isfinite(h.val_loss).all()
        assert r["holdout"].shape == (1, 16, 16, 1) and r["holdout"].sum() > 0
        assert np.all(r["mask"][:, r["holdout"][0, ..., 0] > 0] != 0)             # held-out traces are known traces
        assert r["best_iter"] == len(h.val_loss) - 1 - int(np.argmin(np.array(h.val_loss)[::-1]))
        assert r["output"].shape == (16, 16, 16) and np.isfinite(r["output"]).all()
    rec = reconstruct_patches(parse_arguments(argv))
    assert np.asarray(rec).squeeze().shape == shape and np.isfinite(rec).all()


def test_rolling_driver_with_holdout(tmp_path, monkeypatch, capsys):
    """parallel.main with two concurrency slots (the rolling driver: captured graphs replayed side by side) takes the flag through, writes the
    new keys and prints the held-out SNR summary."""
    from deep_prior_interpolation_amd import parallel as P, utils as u
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("DPI_CONCURRENT_PATCHES", "2")
    shape = (16, 16, 32)
    np.save("vol.npy", u.hyperbolic_volume(shape, seed=1).astype(np.float32))
    np.save("mask.npy", np.broadcast_to(u.random_trace_mask(shape, 0.5, seed=2), shape).astype(np.float32))
    P.main(["--imgdir", str(tmp_path), "--imgname", "vol.npy", "--maskname", "mask.npy", "--datadim", "3d", "--patch_shape", "16", "16", "16",
            "--filters", "4", "8", "--skip", "4", "--inputdepth", "4", "--upsample", "linear", "--epochs", "6", "--gpu", "0", "--gain", "10",
            "--holdout", "0.2", "--outdir", "roll"])
    assert "held-out SNR of the selected outputs over 2 patches" in capsys.readouterr().out
    for name in ("0", "1"):
        r = np.load(os.path.join("results", "roll", name + "_run.npy"), allow_pickle=True).item()
        h = r["history"]
        assert isinstance(h, u.HistoryHoldout) and len(h) == 6 and r["holdout"].sum() > 0
        assert r["best_iter"] == len(h.val_loss) - 1 - int(np.argmin(np.array(h.val_loss)[::-1]))
    assert np.isfinite(np.load(os.path.join("results", "roll", "reconstructed.npy"))).all()


@pytest.mark.parametrize("datadim", ["3d", "2d"])
def test_dips_come_from_the_training_traces(datadim):
    """--aa_weight with --holdout: the dip field is estimated from img * m_tr, so no slope of a held-out trace enters the training loss."""
    from deep_prior_interpolation_amd.main import Interpolator
    from deep_prior_interpolation_amd.parameter import parse_arguments
    from deep_prior_interpolation_amd import utils as u
    shape = (16, 16, 16) if datadim == "3d" else (32, 24, 1)
    a = parse_arguments(["--imgdir", "x", "--datadim", datadim, "--filters", "4", "8", "--skip", "4", "--inputdepth", "4", "--epochs", "3",
                         "--gpu", "0", "--aa_weight", "0.5", "--holdout", "0.3"])
    vol = u.hyperbolic_volume(shape, seed=3).astype(np.float64) * 10.0       # 2-D: (T, X, 1) = a (T, X) section with one channel
    mask = u.random_trace_mask(shape, 0.4, seed=4).astype(np.float64)
    if datadim == "3d":
        vol, mask = vol[..., None], mask[..., None]
    T = Interpolator(a, "/tmp")
    T.load_data({"image": vol, "mask": mask.copy(), "name": "0"})
    T.begin_patch(2)
    T.build_model()
    T.build_input()
    T.build_regularizer()
    m_tr = T.training_mask()
    assert float((T.mask_ - m_tr).abs().sum()) > 0
    if datadim == "3d":
        ref, full = (torch.stack(u.structure_tensor_dips_sections(T.img_ * mm, smooth=float(a.aa_smooth))) for mm in (m_tr, T.mask_))
    else:
        ref, full = (u.structure_tensor_dips(T.img_ * mm, smooth=float(a.aa_smooth))[0] for mm in (m_tr, T.mask_))
    got = T._aa_op.dips
    got = torch.stack(list(got)) if isinstance(got, (tuple, list)) else got
    np.testing.assert_array_equal(got.reshape(ref.shape).cpu().numpy(), ref.cpu().numpy())
    assert not torch.equal(ref, full)
    T.optimize(verbose=False)
    assert np.isfinite(T.history.val_snr).all() and T.best_iter is not None


def test_data_forgetting_with_holdout_runs():
    T = _interp3d(["--holdout", "0.2", "--data_forgetting_factor", "3"], 5)
    held = torch.from_numpy(np.moveaxis(T.holdout_sel, -1, 0)[0] > 0).to(DEV)          # (X, Y); the term is (1, inputdepth, T, X, Y)
    assert float(T.add_data_[0][:, :, held].abs().sum()) == 0.0
    T.optimize(verbose=False)
    assert len(T.history.val_loss) == 5 and np.isfinite(T.history.val_loss).all()
