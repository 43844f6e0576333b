"""GPU tests of the Langevin samplers (--optimizer sgld | psgld): dpi_langevin_multi against the recorded reference trajectories and a
float32 numpy restatement, its Philox stream, dpi_moments_update against float64, graph against eager, concurrent slots, the CLI end to
end, and the untouched default run."""
import os
from argparse import Namespace

import numpy as np
import pytest
import torch

from conftest import GOLDEN, jstr

pytestmark = pytest.mark.gpu
DEV = "cuda"
F = np.float32
SENTINEL = -777.25
PAD = 8


# ---------------------------------------------------------------- helpers ----------------------------------------------------------------
def _guarded(values, misalign):
    """A device buffer filled with SENTINEL holding `values` at element offset 4 (16-byte aligned) or 5 (one element off); returns
    (buffer, view).  torch's allocations are aligned to at least 256 bytes."""
    v = np.asarray(values, dtype=F).ravel()
    buf = torch.full((v.size + 2 * PAD,), SENTINEL, dtype=torch.float32, device=DEV)
    off = 5 if misalign else 4
    view = buf[off:off + v.size]
    view.copy_(torch.from_numpy(v))
    assert view.data_ptr() % 16 == (4 if misalign else 0)
    return buf, view


def _guards_intact(buf, view):
    b = buf.cpu().numpy()
    off = (view.data_ptr() - buf.data_ptr()) // 4
    return bool(np.all(b[:off] == F(SENTINEL)) and np.all(b[off + view.numel():] == F(SENTINEL)))


def _launch(rows, kind, step, lr, wd=0.0, beta=0.99, lam=1e-8, ns=0.1, temp=1.0, seed=0, xi=None, active=None):
    """One raw dpi_langevin_multi call; rows = [(p, g, m, v)] device tensors."""
    from deep_prior_interpolation_amd import _lib
    table = torch.tensor([t.data_ptr() for r in rows for t in r], dtype=torch.int64).to(DEV)
    sizes = torch.tensor([r[0].numel() for r in rows], dtype=torch.int64).to(DEV)
    step_lr = torch.tensor([float(step), lr], dtype=torch.float32).to(DEV)
    xp = None if xi is None else torch.tensor([x.data_ptr() for x in xi], dtype=torch.int64).to(DEV)
    _lib.check(_lib.load().dpi_langevin_multi(table.data_ptr(), sizes.data_ptr(), len(rows), step_lr.data_ptr(), kind, wd, beta, lam, ns, temp,
                                              seed, _lib.ptr(xp), _lib.ptr(active), _lib.stream()), "dpi_langevin_multi")
    torch.cuda.synchronize()


def _fma(a, b, c):
    """fp32 fused multiply-add: the product of two fp32 numbers is exact in float64."""
    return (np.asarray(a, dtype=np.float64) * np.asarray(b, dtype=np.float64) + np.asarray(c, dtype=np.float64)).astype(F)


def _rule(kind, p, g, V, lr, wd, beta=0.99, lam=1e-8):
    """The two rules without noise, in float32 with the rounding points of the torch calls the reference makes (csrc/loss_optim.hip)."""
    d = _fma(p, F(wd), g) if wd != 0 else g
    if kind == 0:
        return _fma(d, F(-lr), p), V
    V = _fma((F(1.0 - beta) * d).astype(F), d, (V * F(beta)).astype(F))
    G = (np.sqrt(V) + F(lam)).astype(F)
    return (p + ((F(-lr) * d).astype(F) / G).astype(F)).astype(F), V


def _fill_normal(n, seed, stream_id):
    from deep_prior_interpolation_amd import _lib
    out = torch.empty(n, dtype=torch.float32, device=DEV)
    _lib.check(_lib.load().dpi_fill_normal(out.data_ptr(), n, 0.0, 1.0, seed, stream_id, _lib.stream()), "dpi_fill_normal")
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(GOLDEN, "langevin.npz"))


# ---------------------------------------------------------------- parity with the reference ----------------------------------------------
@pytest.mark.parametrize("case", ["sgld", "sgld_wd", "psgld", "psgld_wd"])
def test_parity_with_the_reference(fixture, case):
    """FusedLangevin(noise="torch_cpu") on the recorded gradients, torch's CPU generator seeded as the recorder seeded it, one step at a
    time from the recorded state before the step (so each figure is the error of ONE step).

    SGLD, V of pSGLD and the pSGLD rows of 1 and 3 elements are bit-equal to the recording.  pSGLD rows of 1025 and 405 elements are not:
    torch's vectorised CPU sqrt (V.sqrt() and noise_std.sqrt(), rows of at least one SIMD width) is off by one ulp on ~0.5 % of its inputs
    where sqrtf on the device is correctly rounded.  Each sqrt feeds one addend of the update (G into the drift, G and the second sqrt into
    the noise); measured against the fixture with an IEEE float32 restatement on the host and on the device: at most 4 ulp of
    max(|p|, |update|) per step, on 1 % of the elements.  The bound is twice that, the ceiling of 8 ulp per step."""
    from deep_prior_interpolation_amd.optim import FusedLangevin
    f = fixture
    h = jstr(f[case + "/hyper"])
    shapes = [tuple(s) for s in jstr(f["shapes"])]
    bufs, params = [], []
    for i, s in enumerate(shapes):
        buf, view = _guarded(f["%s/p%d_init" % (case, i)], misalign=(i == 2))
        bufs.append((buf, view))
        params.append(view.view(s).requires_grad_())
    kw = dict(noise_scale=h["noise_scale"]) if h["kind"] == "sgld" else dict(beta=h["beta"], Lambda=h["Lambda"])
    opt = FusedLangevin(params, h["kind"], lr=h["lr"], weight_decay=h["weight_decay"], temperature=1.0, noise="torch_cpu", **kw)
    vbufs = [_guarded(np.zeros(int(np.prod(s))), misalign=(i in (1, 2))) for i, s in enumerate(shapes)]
    opt._v = [v for _, v in vbufs]                      # the state slices inside guarded buffers (row 2: every pointer one element off)
    worst = 0.0
    for step in range(4):
        before = [p.detach().cpu().numpy().copy() for p in params]
        for i, p in enumerate(params):
            p.grad = torch.from_numpy(f["%s/g%d_%d" % (case, step, i)]).to(DEV)
        torch.manual_seed(int(f[case + "/seeds"][step]))
        opt.step()
        torch.cuda.synchronize()
        for i, p in enumerate(params):
            np.testing.assert_array_equal(opt._xi[i].cpu().numpy(), f["%s/xi%d_%d" % (case, step, i)])
            want = f["%s/p%d_%d" % (case, step, i)]
            got = p.detach().cpu().numpy()
            if h["kind"] == "psgld":
                Vw = f["%s/V%d_%d" % (case, step, i)]
                np.testing.assert_array_equal(opt._v[i].cpu().numpy().view(np.uint32), Vw.ravel().view(np.uint32), err_msg="V row %d step %d" % (i, step))
            if h["kind"] == "sgld" or want.size < 8:
                np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32), err_msg="row %d step %d" % (i, step))
            else:
                ulp = np.spacing(np.maximum(np.abs(want), np.abs(want - before[i])).astype(F))
                err = float((np.abs(got.astype(np.float64) - want) / ulp).max())
                worst = max(worst, err)
                print("%s row %d step %d: %.2f ulp, %d of %d elements differ" % (case, i, step, err, int((got != want).sum()), want.size))
                assert err <= 8.0, (i, step, err)
            with torch.no_grad():                        # the next step starts from the recorded state
                p.copy_(torch.from_numpy(want).to(DEV))
                if h["kind"] == "psgld":
                    opt._v[i].copy_(torch.from_numpy(f["%s/V%d_%d" % (case, step, i)].ravel()).to(DEV))
    print("%s: worst %.2f ulp" % (case, worst))
    assert float(opt.step_lr[0].item()) == 4.0
    for buf, view in bufs + vbufs:
        assert _guards_intact(buf, view)
    if h["kind"] == "sgld":
        assert all(float(v.abs().sum()) == 0.0 for v in opt._v)          # SGLD has no state
    assert float(opt.exp_avg.abs().sum()) == 0.0                            # the m slot is unused


def test_a_row_without_gradient_is_skipped():
    from deep_prior_interpolation_amd.optim import FusedLangevin
    rng = np.random.RandomState(0)
    init = [rng.randn(n).astype(F) for n in (5, 7, 9)]
    grads = [rng.randn(n).astype(F) for n in (5, 7, 9)]
    for kind in ("sgld", "psgld"):
        params = [torch.from_numpy(a.copy()).to(DEV).requires_grad_() for a in init]
        opt = FusedLangevin(params, kind, lr=0.01, temperature=0.0, seed=1)
        params[0].grad, params[2].grad = torch.from_numpy(grads[0]).to(DEV), torch.from_numpy(grads[2]).to(DEV)
        opt.step()
        torch.cuda.synchronize()
        np.testing.assert_array_equal(params[1].detach().cpu().numpy(), init[1])
        assert float(opt._v[1].abs().sum()) == 0.0
        for i in (0, 2):
            want, _ = _rule(opt.KINDS[kind], init[i], grads[i], np.zeros_like(init[i]), 0.01, 0.0)
            np.testing.assert_array_equal(params[i].detach().cpu().numpy().view(np.uint32), want.view(np.uint32))


# ---------------------------------------------------------------- sizes ------------------------------------------------------------------
SIZES = [1, 3, 4, 1023, 1025, 262149]        # the last: one grid-stride pass of 256 blocks x 1024 elements plus a tail


@pytest.mark.parametrize("misalign", [False, True])
@pytest.mark.parametrize("kind", [0, 1])
def test_sizes_against_numpy(kind, misalign):
    """All six sizes as the rows of ONE launch, temperature 0 (no noise), against the float32 numpy restatement: bit-equal — every
    operation is an IEEE one (-ffp-contract=off, correctly rounded division and square root)."""
    rng = np.random.RandomState(10 * kind + misalign)
    lr, wd = 0.01, 0.05
    host, dev = [], []
    for n in SIZES:
        p, g, V = (0.1 * rng.randn(n)).astype(F), (0.02 * rng.randn(n)).astype(F), (1e-4 * (0.1 + rng.rand(n))).astype(F)
        host.append((p, g, V))
        dev.append([_guarded(a, misalign) for a in (p, g, np.zeros(n), V)])
    _launch([tuple(view for _, view in row) for row in dev], kind, step=3, lr=lr, wd=wd, temp=0.0, seed=5)
    for n, (p, g, V), row in zip(SIZES, host, dev):
        wp, wV = _rule(kind, p, g, V, lr, wd)
        np.testing.assert_array_equal(row[0][1].cpu().numpy().view(np.uint32), wp.view(np.uint32), err_msg="p, n = %d" % n)
        np.testing.assert_array_equal(row[3][1].cpu().numpy().view(np.uint32), wV.view(np.uint32), err_msg="V, n = %d" % n)
        np.testing.assert_array_equal(row[1][1].cpu().numpy(), g)
        assert float(row[2][1].abs().sum()) == 0.0
        assert not np.array_equal(wp, p) and (kind == 0 or not np.array_equal(wV, V))
        assert all(_guards_intact(buf, view) for buf, view in row), n


# ---------------------------------------------------------------- the Philox stream ------------------------------------------------------
def _noise_only(ns, seed, step, misalign=False):
    """SGLD on p = 0, g = 0 without weight decay, noise_scale 1, temperature 1: the parameters after the step ARE the normals."""
    rows = [[_guarded(np.zeros(n), misalign) for _ in range(4)] for n in ns]
    _launch([tuple(v for _, v in r) for r in rows], 0, step=step, lr=0.01, ns=1.0, temp=1.0, seed=seed)
    assert all(_guards_intact(b, v) for r in rows for b, v in r)
    return [r[0][1].cpu().numpy() for r in rows]


@pytest.mark.parametrize("n", [1025, 4096])
def test_philox_stream_is_the_documented_one(n):
    seed = 1234567
    for step in (1, 2, 7):
        for misalign in (False, True):
            got = _noise_only([n], seed, step, misalign)[0]
            want = _fill_normal(n, seed, (0xFFFFFFFE << 32) | step)
            np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))
    assert not np.array_equal(_noise_only([n], seed, 1)[0], _noise_only([n], seed + 1, 1)[0])


def test_philox_rows_and_steps_are_independent_standard_normals():
    """Five-sigma bounds of the estimators for N independent N(0,1) samples: the mean has std 1/sqrt(N), the variance sqrt(2/N), a
    sample correlation 1/sqrt(N).  The seed is fixed: the test is deterministic."""
    N = 65536
    x = [_noise_only([N, N, N], 99, step) for step in (1, 2)]
    vecs = {(s, r): x[s][r].astype(np.float64) for s in range(2) for r in range(3)}
    for v in vecs.values():
        assert abs(v.mean()) < 5 / np.sqrt(N)
        assert abs(v.var() - 1.0) < 5 * np.sqrt(2.0 / N)
    corr = lambda a, b: float(np.corrcoef(a, b)[0, 1])
    for s in range(2):
        for r1 in range(3):
            for r2 in range(r1 + 1, 3):
                assert abs(corr(vecs[(s, r1)], vecs[(s, r2)])) < 5 / np.sqrt(N)
    for r in range(3):
        assert abs(corr(vecs[(0, r)], vecs[(1, r)])) < 5 / np.sqrt(N)


@pytest.mark.parametrize("kind", [0, 1])
def test_temperature_zero_leaves_no_noise(kind):
    rng = np.random.RandomState(3)
    p, g, V = (0.1 * rng.randn(1025)).astype(F), (0.02 * rng.randn(1025)).astype(F), (1e-4 * (0.1 + rng.rand(1025))).astype(F)
    res = []
    for seed, temp in ((1, 0.0), (2, 0.0), (1, 1.0)):
        row = [torch.from_numpy(a.copy()).to(DEV) for a in (p, g, np.zeros_like(p), V)]
        _launch([tuple(row)], kind, step=1, lr=0.01, temp=temp, seed=seed)
        res.append(row[0].cpu().numpy())
    np.testing.assert_array_equal(res[0].view(np.uint32), res[1].view(np.uint32))
    assert not np.array_equal(res[0], res[2])


def test_bad_arguments_are_refused():
    from deep_prior_interpolation_amd import _lib
    L = _lib.load()
    t = torch.zeros(8, dtype=torch.float32, device=DEV)
    table = torch.tensor([t.data_ptr()] * 4, dtype=torch.int64).to(DEV)
    sizes = torch.tensor([8], dtype=torch.int64).to(DEV)
    sl = torch.tensor([1.0, 0.01], dtype=torch.float32).to(DEV)
    ok = [table.data_ptr(), sizes.data_ptr(), 1, sl.data_ptr(), 0, 0.0, 0.99, 1e-8, 0.1, 0.0, 0, None, None, _lib.stream()]
    for pos, bad in ((0, None), (1, None), (3, None), (2, 0), (2, 65536), (4, 2), (5, -1.0), (7, -1e-8), (8, -0.1), (9, -1.0)):
        args = list(ok)
        args[pos] = bad
        assert L.dpi_langevin_multi(*args) != 0, pos
    okm = [t.data_ptr(), t.data_ptr(), t.data_ptr(), 8, sl.data_ptr(), 0, 1, None, _lib.stream()]
    for pos, bad in ((0, None), (1, None), (2, None), (4, None), (3, 0), (5, -1), (6, 0)):
        args = list(okm)
        args[pos] = bad
        assert L.dpi_moments_update(*args) != 0, pos
    torch.cuda.synchronize()
    assert float(t.abs().sum()) == 0.0


# ---------------------------------------------------------------- the active gate --------------------------------------------------------
def test_active_gate():
    from deep_prior_interpolation_amd import _lib
    rng = np.random.RandomState(4)
    off = torch.zeros(1, dtype=torch.int32, device=DEV)
    for kind in (0, 1):
        host = [(0.1 * rng.randn(1025)).astype(F) for _ in range(4)]
        row = [torch.from_numpy(a.copy()).to(DEV) for a in host]
        _launch([tuple(row)], kind, step=1, lr=0.01, active=off)
        for a, t in zip(host, row):
            np.testing.assert_array_equal(t.cpu().numpy(), a)
    out, mean, m2 = (torch.from_numpy(rng.randn(1025).astype(F)).to(DEV) for _ in range(3))
    m0, q0 = mean.cpu().numpy().copy(), m2.cpu().numpy().copy()
    sl = torch.tensor([0.0, 0.01], dtype=torch.float32).to(DEV)
    _lib.check(_lib.load().dpi_moments_update(out.data_ptr(), mean.data_ptr(), m2.data_ptr(), 1025, sl.data_ptr(), 0, 1, off.data_ptr(),
                                              _lib.stream()))
    torch.cuda.synchronize()
    np.testing.assert_array_equal(mean.cpu().numpy(), m0)
    np.testing.assert_array_equal(m2.cpu().numpy(), q0)
    off.fill_(1)
    _lib.check(_lib.load().dpi_moments_update(out.data_ptr(), mean.data_ptr(), m2.data_ptr(), 1025, sl.data_ptr(), 0, 1, off.data_ptr(),
                                              _lib.stream()))
    torch.cuda.synchronize()
    assert not np.array_equal(mean.cpu().numpy(), m0)


# ---------------------------------------------------------------- moments ----------------------------------------------------------------
@pytest.mark.parametrize("n, misalign", [(1, False), (1025, False), (17 * 13 * 11, False), (1028, True), (1028, False)])
def test_moments_against_float64(n, misalign):
    """K = 64 samples, burn-in 3, thin 2: iterations 0..129, the step counter advanced by hand.  Skipped iterations leave both buffers
    bit-identical.  Bounds: an update rounds three quantities of the magnitude of the running mean or of delta (<= 2 max|x|) — delta,
    delta / k, the new mean — so the mean drifts by at most 4 * 2^-24 * max|x| per update, 4 K 2^-24 max|x| after K; m2 adds a product
    delta * (x - mean) <= 4 max|x|^2 to a running sum <= 4 K max|x|^2 with two roundings of that magnitude per update, so K updates
    give at most 8 K 2^-24 max|x|^2 K."""
    from deep_prior_interpolation_amd import _lib
    L = _lib.load()
    K, burn, thin = 64, 3, 2
    rng = np.random.RandomState(n)
    xs = rng.randn(burn + thin * (K - 1) + 1, n).astype(F)
    (ob, out), (mb, mean), (qb, m2) = (_guarded(np.zeros(n), misalign) for _ in range(3))
    sl = torch.zeros(2, dtype=torch.float32, device=DEV)
    sampled = []
    for it in range(xs.shape[0]):
        out.copy_(torch.from_numpy(xs[it]))
        sl[0] = float(it)
        prev = (mean.cpu().numpy().copy(), m2.cpu().numpy().copy())
        _lib.check(L.dpi_moments_update(out.data_ptr(), mean.data_ptr(), m2.data_ptr(), n, sl.data_ptr(), burn, thin, None, _lib.stream()))
        if it >= burn and (it - burn) % thin == 0:
            sampled.append(it)
        else:
            np.testing.assert_array_equal(mean.cpu().numpy().view(np.uint32), prev[0].view(np.uint32))
            np.testing.assert_array_equal(m2.cpu().numpy().view(np.uint32), prev[1].view(np.uint32))
    torch.cuda.synchronize()
    assert len(sampled) == K
    x64 = xs[sampled].astype(np.float64)
    amax = float(np.abs(x64).max())
    ref_mean = x64.mean(axis=0)
    ref_m2 = ((x64 - ref_mean) ** 2).sum(axis=0)
    em = float(np.abs(mean.cpu().numpy() - ref_mean).max())
    eq = float(np.abs(m2.cpu().numpy() - ref_m2).max())
    print("n %d: mean error %.3g (bound %.3g), m2 error %.3g (bound %.3g)" % (n, em, 4 * K * 2.0 ** -24 * amax, eq, 8 * K * 2.0 ** -24 * amax ** 2 * K))
    assert em <= 4 * K * 2.0 ** -24 * amax
    assert eq <= 8 * K * 2.0 ** -24 * amax ** 2 * K
    assert all(_guards_intact(b, v) for b, v in ((ob, out), (mb, mean), (qb, m2)))


def test_moments_non_temporal_path():
    """n >= 32 << 20 takes the non-temporal vector accesses: two samples against torch float64 on the device."""
    from deep_prior_interpolation_amd import _lib
    L = _lib.load()
    n = (32 << 20) + 4
    g = torch.Generator(device=DEV).manual_seed(0)
    mean, m2 = torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    sl = torch.zeros(2, dtype=torch.float32, device=DEV)
    xs = [torch.randn(n, device=DEV, generator=g) for _ in range(2)]
    for it, x in enumerate(xs):
        sl[0] = float(it)
        _lib.check(L.dpi_moments_update(x.data_ptr(), mean.data_ptr(), m2.data_ptr(), n, sl.data_ptr(), 0, 1, None, _lib.stream()))
    a, b = xs[0].double(), xs[1].double()
    amax = float(torch.maximum(a.abs().max(), b.abs().max()))
    assert float((mean.double() - (a + b) / 2).abs().max()) <= 4 * 2 * 2.0 ** -24 * amax
    assert float((m2.double() - (a - b) ** 2 / 2).abs().max()) <= 8 * 2 * 2.0 ** -24 * amax ** 2 * 2


# ---------------------------------------------------------------- the loop ---------------------------------------------------------------
def _golden_interp(g, epochs, optimizer, holdout=0.0, seed=7, burnin=4, thin=2):
    from deep_prior_interpolation_amd.main import Interpolator
    a = Namespace(**jstr(g["args"]))
    a.epochs, a.gpu, a.holdout = epochs, 0, holdout
    a.optimizer, a.posterior_burnin, a.posterior_thin = optimizer, burnin, thin
    a.earlystop_patience = epochs              # the parser's default: no early stop (pSGLD's first steps, with V still near 0, raise the loss)
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
    cols = [h.loss, h.snr, h.pcorr, h.lr] + ([h.val_loss, h.val_snr] if hasattr(h, "val_loss") else [])
    return dict(hist=[np.array(c) for c in cols], out=T.out_best.copy(), std=None if T.posterior_std is None else T.posterior_std.copy(),
                sel=T.output_selected.copy(), K=T.posterior_samples, best_iter=T.best_iter, snr=T.posterior_snr, vsnr=T.posterior_val_snr,
                state={k: v.detach().cpu().numpy().copy() for k, v in T.net.state_dict().items()})


def _same(r1, r2, params_only=False):
    for k, (c1, c2) in enumerate(zip(r1["hist"], r2["hist"])):
        if k == 3:      # lr: the eager loop logs the Python float, the device history the fp32 value the kernels use
            np.testing.assert_allclose(c2, c1, rtol=1e-6)
        else:
            np.testing.assert_array_equal(c1, c2)
    np.testing.assert_array_equal(r1["out"], r2["out"])
    np.testing.assert_array_equal(r1["sel"], r2["sel"])
    assert (r1["std"] is None) == (r2["std"] is None)
    if r1["std"] is not None:
        np.testing.assert_array_equal(r1["std"], r2["std"])
    assert (r1["K"], r1["best_iter"], r1["snr"], r1["vsnr"]) == (r2["K"], r2["best_iter"], r2["snr"], r2["vsnr"])
    for k, v in r1["state"].items():
        if params_only and ("running_" in k or "num_batches_tracked" in k):
            continue
        np.testing.assert_array_equal(r2["state"][k], v, err_msg=k)


@pytest.mark.parametrize("holdout", [0.0, 0.25])
@pytest.mark.parametrize("optimizer", ["psgld", "sgld"])
def test_graph_equals_eager(golden, optimizer, holdout):
    g = golden("net_mulresunet3d_tiny_trilinear_mae")
    res = {}
    for mode in ("eager", "graph"):
        T, a = _golden_interp(g, 12, optimizer, holdout)
        T.optimize(verbose=False, mode=mode, check_every=5)
        res[mode] = _result(T)
    r = res["graph"]
    assert len(r["hist"][0]) == 12 and r["K"] == 4 and np.isfinite(r["hist"][0]).all()
    assert r["std"].shape == r["out"].shape and np.isfinite(r["std"]).all() and (r["std"] >= 0).all() and r["std"].max() > 0
    assert not np.array_equal(r["out"], r["sel"])
    assert np.isfinite(r["snr"]) and ((r["vsnr"] is None) if holdout == 0.0 else np.isfinite(r["vsnr"]))
    _same(res["eager"], res["graph"])


def test_early_stop_before_the_burn_in(golden):
    g = golden("net_mulresunet3d_tiny_nearest_mse")
    res = {}
    for mode in ("eager", "graph"):
        T, a = _golden_interp(g, 60, "psgld", 0.3, seed=3, burnin=55, thin=1)
        a.earlystop_patience, a.earlystop_min_delta = 3, 50.0
        T.optimize(verbose=False, mode=mode, check_every=4)
        res[mode] = _result(T)
        assert T.iiter <= 55 and T.posterior_samples is None and T.posterior_std is None and T.posterior_snr is None
        np.testing.assert_array_equal(T.out_best, T.output_selected)
        assert float(T._post_mean.abs().sum()) == 0.0 and float(T._post_m2.abs().sum()) == 0.0
    _same(res["eager"], res["graph"], params_only=True)


def test_the_mean_is_the_mean(tmp_path):
    """Eager with --save_every 1: the outputs saved from the burn-in on, averaged in float64, against out_best and posterior_std (bounds
    of test_moments_against_float64 with K = 4; the std through m2 = std^2 (K - 1), whose square root and square add three roundings)."""
    burn, thin, K = 3, 2, 4
    T = _interp3d(["--optimizer", "psgld", "--save_every", "1", "--posterior_burnin", str(burn), "--posterior_thin", str(thin)], 10)
    T.outpath = str(tmp_path)
    T.optimize(verbose=False)
    assert T.posterior_samples == K and len(T.history) == 10
    xs = np.stack([np.load(os.path.join(str(tmp_path), "0_output%s.npy" % str(it).zfill(T.zfill))) for it in (3, 5, 7, 9)]).astype(np.float64)
    amax = float(np.abs(xs).max())
    ref_mean = xs.mean(axis=0)
    ref_m2 = ((xs - ref_mean) ** 2).sum(axis=0)
    assert ref_m2.max() > 0
    assert np.abs(T.out_best - ref_mean).max() <= 4 * K * 2.0 ** -24 * amax
    got_m2 = T.posterior_std.astype(np.float64) ** 2 * (K - 1)
    assert np.abs(got_m2 - ref_m2).max() <= 8 * K * 2.0 ** -24 * amax ** 2 * K + 3 * 2.0 ** -24 * ref_m2.max()
    l = np.array(T.history.loss)
    best = len(l) - 1 - int(np.argmin(l[::-1]))         # the loss-selected iterate is still tracked (iteration 0 is never saved)
    if best > 0:
        np.testing.assert_array_equal(T.output_selected, np.load(os.path.join(str(tmp_path), "0_output%s.npy" % str(best).zfill(T.zfill))))


def test_concurrent_slots():
    from deep_prior_interpolation_amd.main import optimize_concurrently
    extra = ["--optimizer", "psgld", "--holdout", "0.2"]
    solo = []
    for i in range(2):
        T = _interp3d(extra, 6, index=i)
        T.optimize(verbose=False, mode="graph", check_every=2)
        solo.append(_result(T))
    assert solo[0]["K"] == 3 and not np.array_equal(solo[0]["out"], solo[1]["out"])
    Ts = [_interp3d(extra, 6, index=i) for i in range(2)]
    optimize_concurrently(Ts, check_every=2)
    for T, r in zip(Ts, solo):
        _same(r, _result(T))
        np.testing.assert_array_equal(T._to_numpy_out(T._out_best_dev), T.out_best)      # what the re-assembly blends is the mean


def test_default_temperature_and_seed_follow_the_patch():
    T = _interp3d(["--optimizer", "sgld", "--holdout", "0.2"], 4, index=5)
    opt = T.make_optimizer()
    n = int(torch.count_nonzero(T.training_mask()).item())
    assert 0 < n < T.mask_.numel() and opt.temperature == 1.0 / n and opt.seed == T.noise_seed == 5 and opt.noise == "philox"
    T = _interp3d(["--optimizer", "psgld", "--langevin_temperature", "1", "--noise_source", "torch_cpu", "--weight_decay", "0.5"], 4)
    opt = T.make_optimizer()
    assert opt.temperature == 1.0 and opt.noise == "torch_cpu" and opt.kind == "psgld" and opt.param_groups[0]["weight_decay"] == 0.5
    with pytest.raises(ValueError, match="cannot be captured"):
        T.optimize(verbose=False, mode="graph")
    T.optimize(verbose=False)
    assert T.posterior_samples == 2 and np.isfinite(T.out_best).all()


# ---------------------------------------------------------------- the CLI ----------------------------------------------------------------
def _cli(tmp_path, monkeypatch, extra, outdir):
    from deep_prior_interpolation_amd import main as M, utils as u
    monkeypatch.chdir(tmp_path)
    shape = (16, 16, 16)
    np.save("vol.npy", u.hyperbolic_volume(shape, seed=1).astype(np.float32))
    np.save("mask.npy", np.broadcast_to(u.random_trace_mask(shape, 0.5, seed=2), shape).astype(np.float32))
    M.main(["--imgdir", str(tmp_path), "--imgname", "vol.npy", "--maskname", "mask.npy", "--datadim", "3d", "--patch_shape", "16", "16", "16",
            "--filters", "4", "8", "--skip", "4", "--inputdepth", "4", "--upsample", "linear", "--epochs", "6", "--gpu", "0", "--gain", "10",
            "--outdir", outdir] + extra)
    return np.load(os.path.join("results", outdir, "0_run.npy"), allow_pickle=True).item()


def test_cli_end_to_end(tmp_path, monkeypatch, capsys):
    r = _cli(tmp_path, monkeypatch, ["--optimizer", "psgld", "--holdout", "0.2"], "lang")
    log = capsys.readouterr().out
    assert "posterior mean over 3 samples" in log and "held-out SNR" in log
    assert r["posterior_samples"] == 3
    for k in ("output", "posterior_std", "output_selected"):
        assert r[k].shape == (16, 16, 16) and np.isfinite(r[k]).all(), k
    assert (r["posterior_std"] >= 0).all() and r["posterior_std"].max() > 0
    assert isinstance(r["posterior_val_snr"], float) and isinstance(r["posterior_snr"], float)
    assert len(r["history"]) == 6 and r["holdout"].sum() > 0


def test_default_run_is_untouched(tmp_path, monkeypatch):
    from deep_prior_interpolation_amd.optim import FusedAdam
    r = _cli(tmp_path, monkeypatch, ["--optimizer", "adam"], "adam")
    assert sorted(r) == sorted(["device", "elapsed", "outpath", "history", "mask", "image", "output", "noise"])
    T = _interp3d([], 6)
    T.optimize(verbose=False, mode="eager")
    assert type(T.optimizer) is FusedAdam and T.posterior_std is None and T.output_selected is None and T._post_mean is None
    T2 = _interp3d([], 6)
    T2.optimizer = FusedAdam(T2.net.parameters(), lr=T2.args.lr)
    for _ in range(6):
        T2.optimizer.zero_grad()
        T2.optimization_loop()
        T2.optimizer.step()
    torch.cuda.synchronize()
    np.testing.assert_array_equal(np.array(T.history.loss), np.array(T2.history.loss))
    np.testing.assert_array_equal(T.out_best, T2._to_numpy_out(T2._out_best_dev))
    for (k, v), (_, v2) in zip(T.net.state_dict().items(), T2.net.state_dict().items()):
        np.testing.assert_array_equal(v.cpu().numpy(), v2.cpu().numpy(), err_msg=k)
