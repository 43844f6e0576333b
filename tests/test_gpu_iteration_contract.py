"""What the per-iteration launches of csrc/loss_optim.hip compute and may touch, at the sizes where their code paths change: the rows of
tests/iteration_cases.py through the C ABI, every buffer owned by the test.  Buffers a launch may write sit inside guard bands
(gpu_guard.guard): pure outputs NaN-filled, in-place buffers filled with their data; inputs sit inside bands too; ws, result, state and
hist have exactly the documented size.  After every launch: _launch, _check_guards (both end the session on a launch error or a device
fault, as in test_gpu_conv_contract.py), every declared output element finite, and the result against the numpy restatement of
iteration_cases.py (held against torch, the Random123 vectors and the recorded traces by tests/test_iteration_refs_host.py, which also
shows that each check function used here fails on a mutated restatement).  Kernels are a reference for each other only where bit
equality between two entry points is the documented contract (holdout / EMA against the plain loss pass, regen against noise_add).

Bars: bit equality for Adam (p, m, v), the loss gradient, the running average, copies, overlap-add and its normalisation, and the loop
control's state; (k 2^-24 + n 2^-53) sum|term| for the loss sums with k counted in iteration_cases.loss_k / check_holdout; 1e-6 dB and
1e-8 for SNR and PCORR (the propagated bounds lie below them: check_loss_result asserts it); 1e-3 std + half an ulp for the Philox
normals (a discrimination threshold, see test_fill_normal).

Precondition (include/dpi_hip.h): the noise kernels choose the float4 path from n % 4 alone, so every buffer here with n % 4 == 0 is
16-byte aligned (bf16: 8-byte) — _aligned asserts it — and offset = 1 appears only with n % 4 != 0.  dpi_adam_multi uses scalar
accesses only: its rows sit at any element offset."""
import functools

import numpy as np
import pytest
import torch

import iteration_cases as I
from gpu_guard import guard
from test_gpu_conv_contract import _check_guards, _launch

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
F = np.float32
E_ARG = -1
SEED = 11


@pytest.fixture(scope="module")
def lib():
    from deep_prior_interpolation_amd import _lib
    return _lib


# ---- buffers -----------------------------------------------------------------------------------------------------------------------------
def _aligned(g, n):
    if n % 4 == 0:
        assert g.payload.data_ptr() % (4 * g.payload.element_size()) == 0, "test buffer off the alignment the vector path needs"
    return g


def gin(a, dtype=F32, offset=0):
    """Host data inside guard bands, at a 256-byte-aligned address (+ offset elements)."""
    a = np.ascontiguousarray(a)
    return _aligned(guard(a.size, dtype, DEV, fill=torch.from_numpy(a.reshape(-1)), offset=offset), 1 if offset else a.size)


def gout(n, dtype=F32, offset=0):
    """A NaN-filled output inside guard bands."""
    return _aligned(guard(n, dtype, DEV, offset=offset), 1 if offset else n)


def gints(values, int_dtype=torch.int64):
    """Integers (pointers, sizes, flags, a step counter) inside guard bands: a float buffer of the same width, written through an integer view."""
    values = [int(v) for v in values]
    g = guard(len(values), F64 if int_dtype == torch.int64 else F32, DEV, fill=torch.zeros(len(values)))
    g.payload.view(int_dtype).copy_(torch.tensor(values, dtype=int_dtype))
    return g


def ints(g, int_dtype=torch.int32):
    return g.payload.view(int_dtype).cpu().numpy()


def ptr(g):
    return None if g is None else (g.payload if hasattr(g, "payload") else g).data_ptr()


def host(g):
    t = g.payload if hasattr(g, "payload") else g
    return (t.float() if t.dtype == BF else t).cpu().numpy()


def written(g, what):
    t = g.payload if hasattr(g, "payload") else g
    bad = int((~torch.isfinite(t.float())).sum())
    assert bad == 0, "%s: %d elements were not written (NaN pre-fill left)" % (what, bad)


# ---- 1. Adam -----------------------------------------------------------------------------------------------------------------------------
def adam_launch(lib, rows, sizes, step_lr, hyper, active, what):
    """rows: [(p, g, m, v)] of Guarded buffers or device tensors; returns after _launch and _check_guards of everything handed over."""
    table, sz = gints([ptr(b) for r in rows for b in r]), gints(sizes)
    rc = lib.load().dpi_adam_multi(ptr(table), ptr(sz), len(rows), ptr(step_lr), *hyper, ptr(active), lib.stream())
    _launch(lib, rc, what)
    named = [("table", table), ("sizes", sz), ("step_lr", step_lr), ("active", active)]
    named += [("%s of row %d" % (k, i), b) for i, r in enumerate(rows) for k, b in zip("pgmv", r) if hasattr(b, "check")]
    _check_guards(named, what)


def adam_rows(sizes, seed, zero_row=None):
    rng = np.random.RandomState(seed)
    data = [I.adam_row(n, rng, zero_state=(i == zero_row)) for i, n in enumerate(sizes)]
    dev = [tuple(gin(a, offset=1 if n in I.ADAM_OFFSET1 else 0) for a in row) for n, row in zip(sizes, data)]
    return data, dev


@pytest.mark.parametrize("launch", [0, 1], ids=["default-step1-active-null", "other-betas-step10-active-set"])
def test_adam_sizes(lib, launch):
    """All ten sizes as the rows of ONE launch: p, m and v bit-equal to adam_np, g unchanged.  262149 is the first row to take the
    grid-stride loop (and its cut group), 524293 runs two full passes; the rows of ADAM_OFFSET1 have all four pointers one element off a
    256-byte boundary.  Launch 0: step 1 with one row of zero moments, active == NULL (the update happens); launch 1: betas 0.8 / 0.99,
    eps 1e-6, step 10, *active == 1."""
    hyper, step, lr = I.ADAM_LAUNCHES[launch]
    data, dev = adam_rows(I.ADAM_SIZES, 100 + launch, zero_row=4 if launch == 0 else None)
    for n, r in zip(I.ADAM_SIZES, dev):
        assert all((ptr(b) % 256 == 4) == (n in I.ADAM_OFFSET1) for b in r)
    active = gints([1], torch.int32) if launch else None
    adam_launch(lib, dev, I.ADAM_SIZES, gin(np.array([step, lr], dtype=F)), hyper, active, "adam_multi sizes")
    for n, (p, g, m, v), (pg, gg, mg, vg) in zip(I.ADAM_SIZES, data, dev):
        for b in (pg, mg, vg):
            written(b, "adam n=%d" % n)
        want = I.adam_np(p, g, m, v, step, lr, *hyper)
        I.check_adam((host(pg), host(mg), host(vg)), want, "adam n=%d" % n)
        I.check_bits(host(gg), g, "adam n=%d: g" % n)
        assert not np.array_equal(want[0], p)


def test_adam_many_rows(lib):
    """300 rows of 1 .. 7 elements in one launch (blockIdx.y), consecutive slices of four flat buffers: any element offset."""
    hyper, step, lr = I.ADAM_LAUNCHES[2]
    rng = np.random.RandomState(7)
    sizes = list(I.ADAM_MANY)
    offs = np.concatenate([[0], np.cumsum(sizes)])
    p, g, m, v = I.adam_row(int(offs[-1]), rng)
    flat = [gin(a) for a in (p, g, m, v)]
    rows = [tuple(b.payload[offs[i]:offs[i + 1]] for b in flat) for i in range(len(sizes))]
    adam_launch(lib, rows, sizes, gin(np.array([step, lr], dtype=F)), hyper, None, "adam_multi 300 rows")
    _check_guards(list(zip("pgmv", flat)), "adam_multi 300 rows")
    want = [np.concatenate(x) for x in zip(*[I.adam_np(p[a:b], g[a:b], m[a:b], v[a:b], step, lr, *hyper) for a, b in zip(offs[:-1], offs[1:])])]
    I.check_adam((host(flat[0]), host(flat[2]), host(flat[3])), want, "adam 300 rows")
    I.check_bits(host(flat[1]), g, "adam 300 rows: g")


def test_adam_three_consecutive_steps(lib):
    """Steps 1, 2, 3 on the device state (fresh gradients each step) against adam_np iterated on the host: bit-equal after every step."""
    hyper, lr = I.ADAM_DEFAULT, 1e-3
    sizes = (5, 1025, 262149)
    data, dev = adam_rows(sizes, 21, zero_row=0)
    state = [(p, m, v) for p, _, m, v in data]
    step_lr = gin(np.array([0.0, lr], dtype=F))
    for step in (1, 2, 3):
        assert (hyper, step, lr) in I.ADAM_LAUNCHES
        rng = np.random.RandomState(30 + step)
        grads = [I.adam_row(n, rng)[1] for n in sizes]
        for r, g in zip(dev, grads):
            r[1].payload.copy_(torch.from_numpy(g))
        step_lr.payload[0] = float(step)
        adam_launch(lib, dev, sizes, step_lr, hyper, None, "adam_multi step %d" % step)
        state = [I.adam_np(p, g, m, v, step, lr, *hyper) for (p, m, v), g in zip(state, grads)]
        for n, want, (pg, gg, mg, vg) in zip(sizes, state, dev):
            I.check_adam((host(pg), host(mg), host(vg)), want, "adam step %d n=%d" % (step, n))


def test_adam_gate_and_refusals(lib):
    """*active == 0: p, m and v keep their bits.  ntensors 0 and 65536 and a NULL table: DPI_E_ARG, nothing written."""
    hyper, step, lr = I.ADAM_LAUNCHES[0]
    sizes = (5, 1025)
    data, dev = adam_rows(sizes, 40)
    before = [[b.bits() for b in r] for r in dev]
    step_lr = gin(np.array([step, lr], dtype=F))
    off = gints([0], torch.int32)
    adam_launch(lib, dev, sizes, step_lr, hyper, off, "adam_multi gated")
    assert all(b.untouched(x) for r, rb in zip(dev, before) for b, x in zip(r, rb)), "a gated launch wrote"
    L = lib.load()
    table, sz = gints([ptr(b) for r in dev for b in r]), gints(sizes)
    for args in ((ptr(table), ptr(sz), 0), (ptr(table), ptr(sz), 65536), (None, ptr(sz), 2)):
        rc = L.dpi_adam_multi(*args, ptr(step_lr), *hyper, None, lib.stream())
        assert rc == E_ARG and L.dpi_last_error().decode().startswith("adam_multi:"), (args[2], rc)
    _check_guards([("table", table), ("sizes", sz)] + [("row", b) for r in dev for b in r], "adam_multi refusals")
    assert all(b.untouched(x) for r, rb in zip(dev, before) for b, x in zip(r, rb)), "a refused launch wrote"


def test_fused_adam_skips_a_row_without_gradient(lib):
    """The FusedAdam twin of test_gpu_langevin.test_a_row_without_gradient_is_skipped: the parameter without a gradient and its state
    slices are untouched, the others bit-equal to adam_np."""
    from deep_prior_interpolation_amd.optim import FusedAdam
    hyper, step, lr = I.ADAM_LAUNCHES[0]
    rng = np.random.RandomState(0)
    rows = [I.adam_row(n, rng) for n in (5, 7, 9)]
    params = [torch.from_numpy(r[0].copy()).to(DEV).requires_grad_() for r in rows]
    opt = FusedAdam(params, lr=lr, betas=hyper[:2], eps=hyper[2])
    params[0].grad, params[2].grad = torch.from_numpy(rows[0][1]).to(DEV), torch.from_numpy(rows[2][1]).to(DEV)
    opt.step()
    torch.cuda.synchronize()
    I.check_bits(params[1].detach().cpu().numpy(), rows[1][0], "the parameter without a gradient")
    assert float(opt._m[1].abs().sum()) == 0.0 and float(opt._v[1].abs().sum()) == 0.0
    for i in (0, 2):
        z = np.zeros_like(rows[i][0])
        want = I.adam_np(rows[i][0], rows[i][1], z, z, step, lr, *hyper)
        I.check_adam((params[i].detach().cpu().numpy(), opt._m[i].cpu().numpy(), opt._v[i].cpu().numpy()), want, "FusedAdam row %d" % i)


# ---- 2. masked loss, held-out part, EMA --------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def loss_problem(n, fractional=False):
    """Host operands and their device copies inside bands, shared by the tests of one n and never modified."""
    o, t, m = I.loss_inputs(n, n % 1000 + (500 if fractional else 0), fractional)
    return (o, t, m), tuple(gin(a) for a in (o, t, m))


def loss_call(lib, dev, n, kind, gscale, with_dout, what, sel=None, shape=None):
    """One dpi_masked_loss (sel None) or dpi_masked_loss_holdout launch on guarded ws / result / dout of exactly the documented sizes;
    returns (dout or None, result) on the host."""
    L = lib.load()
    og, tg, mg = dev
    ho = sel is not None
    ws = gout((2 if ho else 1) * L.dpi_loss_ws_doubles(n), F64)
    res = gout(11 if ho else 8, F64)
    dout = gout(n) if with_dout else None
    if ho:
        rc = L.dpi_masked_loss_holdout(ptr(og), ptr(tg), ptr(mg), ptr(sel), shape[0], shape[1], shape[2], kind, gscale, ptr(dout), ptr(ws), ptr(res), lib.stream())
    else:
        rc = L.dpi_masked_loss(ptr(og), ptr(tg), ptr(mg), n, kind, gscale, ptr(dout), ptr(ws), ptr(res), lib.stream())
    _launch(lib, rc, what)
    _check_guards([("out", og), ("img", tg), ("mask", mg), ("sel", sel), ("ws", ws), ("result", res), ("dout", dout)], what)
    if dout is not None:
        written(dout, what + " dout")
    return (None if dout is None else host(dout)), host(res)


def result_written(res, n, what):
    ok = np.isfinite(res)
    if n == 1:
        ok[2] = True                                   # PCORR of one sample is 0 / 0
    assert ok.all(), "%s: result %s not written" % (what, np.flatnonzero(~ok))


@pytest.mark.parametrize("kind", [0, 1], ids=["l1", "mse"])
@pytest.mark.parametrize("n", I.LOSS_N)
def test_masked_loss(lib, n, kind):
    """dout bit-equal to loss_grad_np for grad_scale 1 and 0.37; the eight doubles against float64 (iteration_cases.check_loss_result:
    k = 1 (L1) / 2 (MSE) for the misfit with this 0/1 mask, 2 for sum (t-o)^2, 0 for the other sums; SNR at 1e-6 dB and PCORR at 1e-8,
    the existing bars, the propagated bounds being smaller); identical bits from a second launch and from one with dout == NULL.
    n = 2097152 reaches the 1024-block cap exactly, n = 2359299 is the first row whose grid the cap cuts (9 passes and a tail)."""
    (o, t, m), dev = loss_problem(n)
    what = "masked_loss n=%d kind=%d" % (n, kind)
    dout, res = loss_call(lib, dev, n, kind, 1.0, True, what)
    result_written(res, n, what)
    I.check_bits(dout, I.loss_grad_np(o, t, m, kind, 1.0), what + " dout")
    worst = I.check_loss_result(res, o, t, m, kind, False, what)
    print("%s: sums at %.3g of their bound" % (what, worst))
    dout2, res2 = loss_call(lib, dev, n, kind, 1.0, True, what + " again")
    I.check_bits(dout2, dout, what + ": dout of a second launch"), I.check_bits(res2, res, what + ": result of a second launch")
    dout3, _ = loss_call(lib, dev, n, kind, 0.37, True, what + " gscale 0.37")
    I.check_bits(dout3, I.loss_grad_np(o, t, m, kind, 0.37), what + " dout, grad_scale 0.37")
    _, res4 = loss_call(lib, dev, n, kind, 1.0, False, what + " dout NULL")
    I.check_bits(res4, res, what + ": result without dout")


@pytest.mark.parametrize("kind", [0, 1], ids=["l1", "mse"])
def test_masked_loss_fractional_mask(lib, kind):
    """A mask in [0, 1): o m and t m round, so the misfit's terms are held against |o m| + |t m| with k = 2 (L1: two products and the
    difference, less the higher-order terms) and its square with k = 4 (MSE) — iteration_cases.loss_k."""
    n = I.LOSS_FRACTIONAL_N
    (o, t, m), dev = loss_problem(n, True)
    assert 0.0 <= m.min() and m.max() < 1.0 and (m * 4 % 1 != 0).any()
    what = "masked_loss fractional mask kind=%d" % kind
    dout, res = loss_call(lib, dev, n, kind, 0.37, True, what)
    result_written(res, n, what)
    I.check_bits(dout, I.loss_grad_np(o, t, m, kind, 0.37), what + " dout")
    I.check_loss_result(res, o, t, m, kind, True, what)


@functools.lru_cache(maxsize=None)
def holdout_problem(shape):
    o, t, m, sel = I.holdout_inputs(shape, 7)
    h = np.broadcast_to(sel[:, None, :], shape)
    m_tr = (m * (F(1.0) - h)).astype(F)
    return (o, t, m, sel, h, m_tr), tuple(gin(a) for a in (o, t, m, sel, m_tr))


@pytest.mark.parametrize("kind", [0, 1], ids=["l1", "mse"])
@pytest.mark.parametrize("shape", I.HOLDOUT_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_masked_loss_holdout(lib, shape, kind):
    """result[10] exactly, result[8] and result[9] against float64 (check_holdout: k = 1 / 2 for the misfit, 0 and 2 for the two sums of
    val_snr), dout and result[0..7] bit for bit dpi_masked_loss on a materialised m_tr — the documented contract — and that training part
    against float64 as well.  (3, 37, 2311) is the first shape where both carries of the index walk occur."""
    (o, t, m, sel, h, m_tr), (og, tg, mg, sg, mtg) = holdout_problem(shape)
    n = o.size
    what = "masked_loss_holdout %s kind=%d" % (shape, kind)
    dout, res = loss_call(lib, (og, tg, mg), n, kind, 0.37, True, what, sel=sg, shape=shape)
    assert np.isfinite(res).all(), (what, res)
    dout_tr, res_tr = loss_call(lib, (og, tg, mtg), n, kind, 0.37, True, what + " materialised")
    I.check_bits(dout, dout_tr, what + ": dout against the plain pass"), I.check_bits(res[:8], res_tr, what + ": result[0..7] against the plain pass")
    I.check_bits(dout, I.loss_grad_np(o.ravel(), t.ravel(), m_tr.ravel(), kind, 0.37), what + " dout")
    I.check_loss_result(res[:8], o.ravel(), t.ravel(), m_tr.ravel(), kind, False, what)
    I.check_holdout(res, o, t, m, h, kind, what)
    assert res[10] > 0 and (dout.reshape(shape)[(m * h) != 0] == 0).all()


EMA_CASES = {"3x37x2311-sel": ((3, 37, 2311), True), "2359299-no-sel": ((1, 3, 786433), False)}


@pytest.mark.parametrize("kind", [0, 1], ids=["l1", "mse"])
@pytest.mark.parametrize("case", sorted(EMA_CASES))
def test_ema_loss(lib, case, kind):
    """Iteration 0, then iteration 1: avg bit-equal to ema_np (a NaN-filled avg is not read at iteration 0); the metrics bit for bit
    those of the loss pass run on the stored avg (the documented contract) and within the float64 bounds of the loss tests; without sel
    result[8..10] are not written."""
    L = lib.load()
    shape, with_sel = EMA_CASES[case]
    n = shape[0] * shape[1] * shape[2]
    assert n == 2359299 or with_sel
    beta = 0.99
    if with_sel:
        (o, t, m, sel, h, m_tr), (og, tg, mg, sg, _) = holdout_problem(shape)
    else:
        (o, t, m), (og, tg, mg) = loss_problem(n)
        sg, h, m_tr = None, None, m
    x1 = (o.ravel() + 0.5 * np.random.RandomState(3).randn(n)).astype(F)
    x1g = gin(x1)
    avg = gout(n)
    step_lr = gin(np.array([0.0, 1e-3], dtype=F))
    want = None
    for it, (xg, x) in enumerate(((og, o.ravel()), (x1g, x1))):
        what = "ema_loss %s kind=%d it=%d" % (case, kind, it)
        step_lr.payload[0] = float(it)
        ws, res = gout(2 * L.dpi_loss_ws_doubles(n), F64), gout(11, F64)
        _launch(lib, L.dpi_ema_loss(ptr(xg), ptr(avg), ptr(tg), ptr(mg), ptr(sg), shape[0], shape[1], shape[2], kind, beta, ptr(step_lr), None,
                                    ptr(ws), ptr(res), lib.stream()), what)
        _check_guards([("out", xg), ("avg", avg), ("img", tg), ("mask", mg), ("sel", sg), ("step_lr", step_lr), ("ws", ws), ("result", res)], what)
        written(avg, what + " avg")
        want = I.ema_np(want, x, beta, it == 0)
        I.check_bits(host(avg), want, what + " avg")
        r = host(res)
        _, r_pass = loss_call(lib, (avg, tg, mg), n, kind, 1.0, False, what + " loss pass on avg", sel=sg, shape=shape if with_sel else None)
        I.check_bits(r[:r_pass.size], r_pass, what + ": metrics against the loss pass on the stored avg")
        I.check_loss_result(r[:8], want, t.ravel(), np.asarray(m_tr).ravel(), kind, False, what)
        if with_sel:
            I.check_holdout(r, want.reshape(shape), t, m, h, kind, what)
        else:
            assert np.isnan(r[8:]).all(), (what, "result[8..10] written without sel", r[8:])
    assert not np.array_equal(want, x1) and not np.array_equal(want, o.ravel())


# ---- 3. Philox input noise ---------------------------------------------------------------------------------------------------------------
MAX_Q = -(-max(I.NOISE_N) // 4)


@functools.lru_cache(maxsize=None)
def z_ref(stream_id):
    """The float64 normals of counters 0 .. MAX_Q - 1 for key SEED, computed once per stream and never modified."""
    return I.normals64(0, MAX_Q, stream_id, SEED)


def off1(n):
    return 1 if n % 4 else 0


def fill_call(lib, n, mean, std, stream_id, what, offset=None):
    out = gout(n, offset=off1(n) if offset is None else offset)
    _launch(lib, lib.load().dpi_fill_normal(ptr(out), n, mean, std, SEED, stream_id, lib.stream()), what)
    _check_guards([("out", out)], what)
    return out


@pytest.mark.parametrize("n", I.NOISE_N)
def test_fill_normal(lib, n):
    """dpi_fill_normal(mean 2, std 0.5) on a stream id with a non-zero high word against the host Philox4x32-10 + float64 Box-Muller:
    |out - (mean + std z64)| <= 1e-3 std + half an fp32 ulp.  The error of __logf / __sincosf has not been characterised; a wrong
    counter, key, stream word or lane order moves a sample by O(std), so 1e-3 std is a discrimination threshold, not an accuracy claim.
    Observed on an MI355X: at most 1.98e-6 std over these sizes (the fp32 rounding of the stored value included), printed per row.
    4198403 is the first row to take the element path in a second grid-stride pass, 4198404 the vector path."""
    what = "fill_normal n=%d" % n
    out = fill_call(lib, n, 2.0, 0.5, I.FILL_STREAM, what)
    worst = I.check_normals(host(out), 2.0, z_ref(I.FILL_STREAM)[:n], 0.5, False, what)
    print("%s: max |out - ref| = %.3g std" % (what, worst))


@pytest.mark.parametrize("step", [None, I.STEP_STREAM], ids=["step-null", "step-set"])
@pytest.mark.parametrize("io", [0, 1], ids=["fp32", "bf16"])
@pytest.mark.parametrize("n", I.NOISE_N)
def test_noise_add(lib, n, io, step):
    """out = z + std N(0, 1) with the stream id *step_ptr (0 when NULL); z inside bands and untouched; a bf16 out gets half a bf16 ulp
    on top of the bar of test_fill_normal.  Observed on an MI355X: at most 1.91e-6 std with an fp32 out; 0.065 std with a bf16 out, which
    is that format's rounding of z + noise (half a bf16 ulp of 0.25 .. 0.5 is 0.033 std at std = 0.03)."""
    what = "noise_add n=%d io=%d step=%s" % (n, io, step)
    z = (0.1 * np.random.RandomState(n % 997).randn(n)).astype(F)
    zg = gin(z, offset=off1(n))
    before = zg.bits()
    out = gout(n, BF if io else F32, offset=off1(n))
    sp = None if step is None else gints([step])
    _launch(lib, lib.load().dpi_noise_add_io(ptr(zg), n, 0.03, SEED, ptr(sp), ptr(out), io, lib.stream()), what)
    _check_guards([("z", zg), ("out", out), ("step", sp)], what)
    assert zg.untouched(before), what + ": z was written"
    worst = I.check_normals(host(out), z, z_ref(0 if step is None else step)[:n], 0.03, bool(io), what)
    print("%s: max |out - ref| = %.3g std" % (what, worst))


@pytest.mark.parametrize("io", [0, 1], ids=["fp32", "bf16"])
@pytest.mark.parametrize("n", [1027, 4198403])
def test_noise_add_regen_is_noise_add_on_the_fill(lib, n, io):
    """dpi_noise_add_regen_io against dpi_noise_add_io on z = dpi_fill_normal(0, z_std, z_seed, z_stream): the same bits (the documented
    contract), on the element path with one block and under grid stride."""
    L = lib.load()
    what = "noise_add_regen n=%d io=%d" % (n, io)
    zg = fill_call(lib, n, 0.0, 0.1, I.FILL_STREAM, what + " fill")
    written(zg, what + " z")
    sp = gints([I.STEP_STREAM])
    a, b = (gout(n, BF if io else F32, offset=off1(n)) for _ in range(2))
    _launch(lib, L.dpi_noise_add_io(ptr(zg), n, 0.03, SEED + 1, ptr(sp), ptr(a), io, lib.stream()), what)
    _launch(lib, L.dpi_noise_add_regen_io(n, 0.1, SEED, I.FILL_STREAM, 0.03, SEED + 1, ptr(sp), ptr(b), io, lib.stream()), what)
    _check_guards([("z", zg), ("step", sp), ("noise_add out", a), ("regen out", b)], what)
    written(a, what), written(b, what)
    assert torch.equal(a.payload.view(torch.int16 if io else torch.int32), b.payload.view(torch.int16 if io else torch.int32))


def test_noise_paths_agree(lib):
    """The first 1024 elements of the n = 1027 launch (element path) are bit-equal to the n = 1024 launch (vector path)."""
    a = fill_call(lib, 1027, 2.0, 0.5, I.FILL_STREAM, "fill_normal 1027")
    b = fill_call(lib, 1024, 2.0, 0.5, I.FILL_STREAM, "fill_normal 1024")
    written(a, "1027"), written(b, "1024")
    I.check_bits(host(a)[:1024], host(b), "element path against vector path")


def test_noise_non_temporal_path(lib):
    """One fill at n = 33554432 (n >= 32 Mi: non-temporal stores, 8 grid-stride passes): every element written, the first 4194304
    bit-equal to the n = 4194304 fill, the last 4096 within the bar of the restatement evaluated on that counter range only."""
    n = I.NOISE_NT
    big = fill_call(lib, n, 2.0, 0.5, I.FILL_STREAM, "fill_normal 32 Mi")
    written(big, "fill_normal 32 Mi")
    small = fill_call(lib, I.NOISE_PASS, 2.0, 0.5, I.FILL_STREAM, "fill_normal one pass")
    assert torch.equal(big.payload[:I.NOISE_PASS].view(torch.int32), small.payload.view(torch.int32))
    tail = big.payload[n - 4096:].cpu().numpy()
    worst = I.check_normals(tail, 2.0, I.normals64(n // 4 - 1024, n // 4, I.FILL_STREAM, SEED), 0.5, False, "fill_normal 32 Mi, last 4096")
    print("fill_normal 32 Mi tail: max |out - ref| = %.3g std" % worst)


# ---- 4. loop control and dpi_copy_if -----------------------------------------------------------------------------------------------------
def loop_run_device(lib, losses, lr0, max_iters, cfg, extra_gated_calls=0, variant="plain", qs=None):
    """dpi_loop_control (or the entry point of `variant`) over a loss sequence on guarded buffers of exactly the documented sizes —
    metrics and ema of 8 doubles, 11 with a held-out part; state and hist as iteration_cases.loop_layout says; the log and history in the
    form of iteration_cases.loop_control_run.  After the sequence (or the stop) `extra_gated_calls` more calls are made with *active == 0."""
    L = lib.load()
    ho, has_ema = I.LOOP_VARIANTS[variant]
    n_state, cols = I.loop_layout(variant)
    inputs = lambda it, loss: [None if x is None else x[:11 if ho else 8] for x in I.loop_inputs(variant, it, loss, None if qs is None else qs[min(it, len(qs) - 1)])]
    metrics, ema = (None if x is None else gin(x, F64) for x in inputs(0, 0.0))
    state = gin(I.new_loop_state(variant), F64)
    assert state.payload.numel() == n_state
    hist = gout(cols * max_iters, F64)
    step_lr = gin(np.array([1.0, lr0], dtype=F))
    active, improved = gints([1], torch.int32), gints([7], torch.int32)
    guards = [("metrics", metrics), ("state", state), ("hist", hist), ("step_lr", step_lr), ("active", active), ("improved", improved)]
    guards += [("ema", ema)] if has_ema else []
    args = (cfg["use_plateau"], cfg["factor"], cfg["threshold"], cfg["patience"], cfg["min_lr"], cfg["lr_eps"], cfg["es_patience"], cfg["es_min_delta"])
    entry = L.dpi_loop_control_ema if has_ema else (L.dpi_loop_control_holdout if ho else L.dpi_loop_control)
    head = (ptr(metrics), ptr(ema), ho) if has_ema else (ptr(metrics),)

    def call(it, loss):
        for g, x in zip((metrics, ema), inputs(it, loss)):
            if g is not None:
                g.payload.copy_(torch.from_numpy(x))
        improved.payload.view(torch.int32).fill_(7)
        _launch(lib, entry(*head, ptr(state), ptr(hist), max_iters, ptr(step_lr), ptr(active), ptr(improved), *args, lib.stream()),
                "loop_control call %d" % it)
        _check_guards(guards, "loop_control call %d" % it)
    log = []
    for it, loss in enumerate(losses):
        call(it, loss)
        log.append((int(ints(improved)[0]), int(ints(active)[0]), float(host(step_lr)[1]), host(state).copy()))
        if not log[-1][1]:
            break
    if extra_gated_calls:
        active.payload.view(torch.int32).fill_(0)
        frozen = state.bits(), hist.bits(), step_lr.bits()
        for k in range(extra_gated_calls):
            call(len(log) + k, 0.01)
            assert int(ints(improved)[0]) == 0, "a gated call raised *improved"
            assert state.untouched(frozen[0]) and hist.untouched(frozen[1]) and step_lr.untouched(frozen[2]), "a gated call wrote"
    return log, host(hist)


LOOP_CASES = [pytest.param(v, k, id=k if v == "plain" else v + "-" + k) for v in I.LOOP_VARIANTS for k in sorted(I.variant_scripts(v))]


@pytest.mark.parametrize("variant, name", LOOP_CASES)
def test_loop_control_scripts(lib, variant, name):
    """dpi_loop_control, dpi_loop_control_holdout and dpi_loop_control_ema (with and without a held-out part) against the host model,
    call by call: *improved, *active, step_lr[1] and every state double (8 / 10 / 12) bit-equal, the history rows equal and NaN where no
    row was written.  `past-max-iters` has hist of three rows and six calls: the later ones leave hist alone and still advance state[0]."""
    losses, qs, cfg, max_iters = I.variant_scripts(variant)[name]
    want, want_hist = I.loop_control_run(losses, 1e-3, max_iters, cfg, variant=variant, qs=qs)
    got, got_hist = loop_run_device(lib, losses, 1e-3, max_iters, cfg, extra_gated_calls=2, variant=variant, qs=qs)
    I.check_loop_log(got, want, "loop_control %s %s" % (variant, name))
    np.testing.assert_array_equal(got_hist, want_hist)
    if name == "past-max-iters":
        assert got[-1][3][0] == len(losses) > max_iters and np.isfinite(got_hist).all()


def test_loop_control_recorded_sequences(lib, golden):
    """The recorded loss curve of host.npz with the recorded ReduceLROnPlateau configuration and EarlyStopping(patience 40, 1 %)."""
    h = golden("host")
    losses = h["earlystop"]["losses"]
    lr0, factor, thr, pat = (float(x) for x in h["plateau"]["cfg"])
    for es in (0, 40):
        cfg = I.loop_cfg(use_plateau=1, factor=factor, threshold=thr, patience=int(pat), es_patience=es, es_min_delta=1.0)
        want, want_hist = I.loop_control_run(losses, lr0, len(losses), cfg)
        got, got_hist = loop_run_device(lib, losses, lr0, len(losses), cfg, extra_gated_calls=1 if es else 0)
        I.check_loop_log(got, want, "loop_control recorded es=%d" % es)
        np.testing.assert_array_equal(got_hist, want_hist)
        assert (len(got) < len(losses)) == bool(es) and got[-1][2] < lr0


@pytest.mark.parametrize("n", I.COPY_N)
def test_copy_if(lib, n):
    """Flag 0 leaves the dst bits untouched; flags 1 and -5 copy bit for bit (n = 1048579: past the 4096-block cap, second pass)."""
    L = lib.load()
    rng = np.random.RandomState(n % 1000)
    src = rng.randn(n).astype(F)
    src[::7] = -0.0
    src[n // 2] = F(1e-41)                                                    # a subnormal travels as it is
    sg = gin(src, offset=off1(n))
    old = gin(rng.randn(n).astype(F), offset=off1(n))
    before = old.bits()
    flag = gints([0], torch.int32)
    _launch(lib, L.dpi_copy_if(ptr(flag), ptr(sg), ptr(old), n, lib.stream()), "copy_if flag 0")
    _check_guards([("flag", flag), ("src", sg), ("dst", old)], "copy_if flag 0 n=%d" % n)
    assert old.untouched(before), "copy_if with flag 0 wrote dst"
    for f in (1, -5):
        flag, dst = gints([f], torch.int32), gout(n, offset=off1(n))
        _launch(lib, L.dpi_copy_if(ptr(flag), ptr(sg), ptr(dst), n, lib.stream()), "copy_if flag %d" % f)
        _check_guards([("flag", flag), ("src", sg), ("dst", dst)], "copy_if flag %d n=%d" % (f, n))
        written(dst, "copy_if dst")
        I.check_bits(host(dst), src, "copy_if flag %d n=%d" % (f, n))


# ---- 5. plain overlap-add ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(I.OVERLAP_CASES))
def test_overlap_add_and_normalize(lib, name):
    """acc bit-equal to the fp32 restatement after the adds (launch order), then to acc / (fp32(count) * gain) after
    dpi_overlap_normalize.  The 65 x 128 x 130 patch (1081600 elements) is the first to run the grid-stride loop past 4096 blocks; in
    the (66, 130, 133) volume it also sits flush with the far corner, and the normalisation's own grid is capped there too."""
    L = lib.load()
    volume, patch, stride, _ = I.OVERLAP_CASES[name]
    patches, origins = I.overlap_patches(name)
    acc = gin(np.zeros(volume, dtype=F))
    pgs = [gin(p) for p in patches]
    for pg, org in zip(pgs, origins):
        _launch(lib, L.dpi_overlap_add(ptr(pg), *patch, *org, ptr(acc), *volume, lib.stream()), "overlap_add " + name)
    _check_guards([("acc", acc)] + [("patch", pg) for pg in pgs], "overlap_add " + name)
    written(acc, "acc")
    want = I.overlap_add_np(volume, patch, patches, origins)
    I.check_bits(host(acc).reshape(volume), want, "overlap_add " + name)
    _launch(lib, L.dpi_overlap_normalize(ptr(acc), *volume, *patch, *stride, 40.0, lib.stream()), "overlap_normalize " + name)
    _check_guards([("acc", acc)], "overlap_normalize " + name)
    written(acc, "acc")
    I.check_bits(host(acc).reshape(volume), I.overlap_normalize_np(want, patch, stride, 40.0), "overlap_normalize " + name)


def test_overlap_refusals(lib):
    """A patch reaching outside the volume, gain == 0 and a stride of 0: DPI_E_ARG with acc untouched."""
    L = lib.load()
    volume, patch = (20, 18, 22), (8, 6, 10)
    acc = gin(np.random.RandomState(0).randn(*volume).astype(F))
    pg = gin(np.ones(patch, dtype=F))
    before = acc.bits()
    calls = [("overlap_add", lambda org=org: L.dpi_overlap_add(ptr(pg), *patch, *org, ptr(acc), *volume, lib.stream()))
             for org in ((13, 0, 0), (0, 13, 0), (0, 0, 13), (-1, 0, 0))]
    calls += [("overlap_normalize", lambda: L.dpi_overlap_normalize(ptr(acc), *volume, *patch, 4, 4, 6, 0.0, lib.stream())),
              ("overlap_normalize", lambda: L.dpi_overlap_normalize(ptr(acc), *volume, *patch, 0, 4, 6, 40.0, lib.stream())),
              ("overlap_normalize", lambda: L.dpi_overlap_normalize(ptr(acc), *volume, *patch, 4, 4, 0, 40.0, lib.stream()))]
    for name, call in calls:
        rc = call()
        assert rc == E_ARG and L.dpi_last_error().decode().startswith(name + ":"), (name, rc, L.dpi_last_error().decode())
    _check_guards([("acc", acc), ("patch", pg)], "overlap refusals")
    assert acc.untouched(before), "a refused launch wrote acc"
