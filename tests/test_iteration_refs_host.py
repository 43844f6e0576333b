"""The restatements of tests/iteration_cases.py against independent code — torch.optim.Adam, the Random123 known answers of Philox4x32-10,
the recorded ReduceLROnPlateau / EarlyStopping traces of tests/golden/host.npz, utils.EarlyStopping, plain division for the index walk,
a brute-force window count — the size facts every row is named for, and, restatement against restatement, that the check functions of
tests/test_gpu_iteration_contract.py fail on a kernel with one of the defects they exist for.  No GPU: the library is only asked for
dpi_loss_ws_doubles."""
import math

import numpy as np
import pytest
import torch

import iteration_cases as I

F = np.float32


def _fails(fn):
    try:
        fn()
    except AssertionError:
        return True
    return False


# ---- size facts --------------------------------------------------------------------------------------------------------------------------
def test_rows_reach_the_paths_they_are_named_for():
    P = I.ADAM_PASS
    assert P == 262144 and I.ADAM_SIZES == (1, 3, 4, 5, 1023, 1024, 1025, 262144, 262149, 524293)
    assert 262149 == P + 5 and 524293 == 2 * P + 5 and len(I.ADAM_MANY) == 300 and set(I.ADAM_MANY) == set(range(1, 8))
    assert all(n % 4 for n in I.ADAM_OFFSET1) and set(I.ADAM_OFFSET1) <= set(I.ADAM_SIZES)
    assert [I.loss_blocks(n) for n in I.LOSS_N] == [1, 1, 1, 2, 129, 1024, 1024]
    assert 2097152 == 1024 * 2048 and 2359299 == 9 * 1024 * 256 + 3 and -(-2359299 // 2048) > 1024
    assert I.NOISE_PASS == 4194304 and [I.noise_blocks(n) for n in I.NOISE_N] == [1] * 7 + [2, 4096, 4096, 4096]
    assert 4198404 % 4 == 0 and 4198403 % 4 == 3 and 4198403 > I.NOISE_PASS and -(-4198403 // 1024) > 4096
    assert I.NOISE_NT == 33554432 and I.NOISE_NT % 4 == 0
    assert I.COPY_N[2] == 1048579 and -(-I.COPY_N[2] // 256) > 4096
    assert 65 * 128 * 130 == 1081600 > 4096 * 256 and 66 * 130 * 133 > 4096 * 256
    for volume, patch, stride, origins in I.OVERLAP_CASES.values():
        assert all((N - p) % s == 0 for N, p, s in zip(volume, patch, stride))
        for o in origins or ():
            assert o in I.window_origins(volume, patch, stride)
    v, p, _, o = I.OVERLAP_CASES["65x128x130-far-corner"]
    assert tuple(a + b for a, b in zip(o[1], p)) == v and all(a > 0 for a in o[1])


def test_workspace_extent():
    from deep_prior_interpolation_amd import _lib
    L = _lib.load()
    for n in I.LOSS_N:
        assert L.dpi_loss_ws_doubles(n) == 8 * I.LOSS_BLOCKS >= 8 * I.loss_blocks(n)


# ---- Adam --------------------------------------------------------------------------------------------------------------------------------
def test_adam_scalars_are_away_from_rounding_ties():
    """step_size and bc2s in double lie at least 2^-40 (relative) from a midpoint between two fp32 values for every launch of the device
    test: a last-bit difference of the device's double pow (2^-52) cannot change the rounded scalar."""
    assert {s for _, s, _ in I.ADAM_LAUNCHES} == {1, 2, 3, 10, 1000}        # 1, 2, 3: the three consecutive steps
    for (b1, b2, eps), step, lr in I.ADAM_LAUNCHES:
        _, (step_size, bc2s) = I.adam_scalars(step, lr, b1, b2, eps)
        assert I.midpoint_margin(step_size) >= 2.0 ** -40 and I.midpoint_margin(bc2s) >= 2.0 ** -40, (b1, b2, step, lr)
    assert I.midpoint_margin(1.0 + 2.0 ** -24) == 0.0 and I.midpoint_margin(1.0 + 2.0 ** -24 + 2.0 ** -50) < 2.0 ** -40


def _ulp_err(got, want, before):
    """max |got - want| in fp32 spacings of max(|want|, |want - before|)."""
    ulp = np.spacing(np.maximum(np.abs(want), np.abs(want - before)).astype(F))
    return float((np.abs(got.astype(np.float64) - want) / ulp).max())


def test_adam_restatement_against_torch(golden):
    """adam_np against torch.optim.Adam(foreach=False) on the CPU over 5 steps, one step at a time from torch's state before the step (so
    each figure is the error of ONE step): the 37-element fixture of host.npz, whose recorded trajectory torch reproduces bit for bit
    here, and a 4099-element row with the default and the other betas.

    Bit equality does not hold.  The scalars agree; the element-wise operations do not: torch's CPU kernels evaluate exp_avg.lerp_ and
    exp_avg_sq.addcmul_ with a fused multiply-add (one rounding where adam_kernel, built with -ffp-contract=off, has two), and
    param.addcdiv_ as (value * exp_avg) / denom where adam_kernel forms step_size * (exp_avg / denom).  Measured here: exp_avg and
    exp_avg_sq at most 1 ulp of max(|new|, |old|) (bit-equal at step 1, where the old state is 0), p at most 5 ulp of
    max(|p|, |update|).  The bars are twice that: 2 ulp for the moments, 10 ulp for p, per step."""
    a = golden("host")["adam"]
    rng = np.random.RandomState(1)
    cases = [(a["p0"].astype(F), a["grads"].astype(F), 1e-3, I.ADAM_DEFAULT)]
    for hyper in (I.ADAM_DEFAULT, I.ADAM_OTHER):
        rows = [I.adam_row(4099, rng) for _ in range(5)]
        cases.append((rows[0][0], np.stack([r[1] for r in rows]), 1e-3, hyper))
    worst = np.zeros(3)
    for ci, (p0, grads, lr, (b1, b2, eps)) in enumerate(cases):
        pt = torch.nn.Parameter(torch.from_numpy(p0.copy()))
        opt = torch.optim.Adam([pt], lr=lr, betas=(b1, b2), eps=eps, foreach=False)
        p, m, v = p0.copy(), np.zeros_like(p0), np.zeros_like(p0)
        for k, g in enumerate(grads):
            pt.grad = torch.from_numpy(g.copy())
            opt.step()
            want = [pt.detach().numpy().copy(), opt.state[pt]["exp_avg"].numpy().copy(), opt.state[pt]["exp_avg_sq"].numpy().copy()]
            if ci == 0:
                np.testing.assert_array_equal(want[0], a["traj"][k])
            got = I.adam_np(p, g, m, v, k + 1, lr, b1, b2, eps)
            err = np.array([_ulp_err(x, w, b) for x, w, b in zip(got, want, (p, m, v))])
            worst = np.maximum(worst, err)
            assert err[0] <= 10.0 and err[1] <= 2.0 and err[2] <= 2.0, (ci, k, err)
            if k == 0:
                I.check_bits(got[1], want[1], "exp_avg after step 1"), I.check_bits(got[2], want[2], "exp_avg_sq after step 1")
            p, m, v = want
    print("adam_np against torch.optim.Adam, one step: p %.2f ulp, exp_avg %.2f ulp, exp_avg_sq %.2f ulp" % tuple(worst))


def test_adam_rows_hold_the_values_they_are_named_for():
    rng = np.random.RandomState(0)
    for n in (1, 5, 1023, 4099):
        p, g, m0, v0 = I.adam_row(n, rng)
        assert (g == 0).any() and ((g == 0) & (v0 == 0)).any() and (m0 != 0).all()
        assert (v0[g != 0] != 0).all()
        if n > 1000:
            a = np.abs(g[g != 0])
            assert a.min() < 1e-8 and a.max() > 0.1
            assert (g < 0).any() and (g > 0).any()
            z = (g == 0) & (v0 == 0)                                        # there denom == eps: the update is step_size * m / eps
            p1, m1, v1 = I.adam_np(p, g, m0, v0, 1, 1e-3)
            assert (v1[z] == 0).all() and np.isfinite(p1).all() and (p1[z] != p[z]).all()
    p, g, m0, v0 = I.adam_row(7, rng, zero_state=True)
    assert not m0.any() and not v0.any()


# ---- loss --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [0, 1])
def test_loss_restatement_against_torch(kind):
    n = 2049
    o, t, m = I.loss_inputs(n, 3)
    ot = torch.from_numpy(o).double().requires_grad_()
    d = ot * torch.from_numpy(m).double() - torch.from_numpy(t).double() * torch.from_numpy(m).double()
    loss = (d * d).mean() if kind == 1 else d.abs().mean()
    (loss * 0.37).backward()
    res = I.loss_result64(o, t, m, kind)
    assert abs(res[0] - loss.item()) <= 1e-14 * loss.item()
    g = I.loss_grad_np(o, t, m, kind, 0.37)
    assert g.dtype == F and np.abs(g - ot.grad.numpy()).max() <= 4 * I.U * np.abs(ot.grad.numpy()).max()
    e = torch.from_numpy(t).double() - torch.from_numpy(o).double()
    assert abs(res[1] - 10 * math.log10(float((torch.from_numpy(t).double() ** 2).sum() / (e ** 2).sum()))) < 1e-12
    assert abs(res[2] - np.corrcoef(o.astype(np.float64), t.astype(np.float64))[0, 1]) < 1e-12
    I.check_loss_result(res, o, t, m, kind, False, "float64 against itself")
    # an fp32 evaluation of the terms, summed in double, passes: the bound has room for the kernel's arithmetic
    for frac in (False, True):
        o, t, m = I.loss_inputs(n, 4, fractional=frac)
        d32 = (o * m - t * m).astype(np.float64)
        res = I.loss_result64(o, t, m, kind)
        res[0] = ((d32 * d32).sum() if kind == 1 else np.abs(d32).sum()) / n
        res[4] = ((t - o).astype(np.float64) ** 2).sum()
        I.check_loss_result(res, o, t, m, kind, frac, "fp32 terms")


def test_holdout_walk_is_division():
    """The incremental walk equals i // TS, i % S for every thread and pass of the four shapes, which sit where they are named for."""
    facts = {}
    for shape in I.HOLDOUT_SHAPES:
        C, T, S = shape
        n, TS = C * T * S, T * S
        c, s, carries = I.holdout_walk(shape)
        i = np.arange(n)
        np.testing.assert_array_equal(c, i // TS)
        np.testing.assert_array_equal(s, i % S)
        facts[shape] = (256 * I.loss_blocks(n), TS, carries)
    G, TS, carries = facts[(3, 37, 2311)]
    assert G < TS and carries["r"] > 0 and carries["s"] > 0
    G, TS, _ = facts[(40, 5, 1301)]
    assert G > TS and G // TS == 5
    assert facts[(2, 48, 24960)][0] == 262144 and I.loss_blocks(2 * 48 * 24960) == I.LOSS_BLOCKS


def test_ema_restatement():
    rng = np.random.RandomState(2)
    a, x = rng.randn(100).astype(F), rng.randn(100).astype(F)
    I.check_bits(I.ema_np(np.full(100, np.nan, dtype=F), x, 0.99, True), x, "first")
    got = I.ema_np(a, x, 0.99, False)
    assert got.dtype == F and np.abs(got - (0.99 * a.astype(np.float64) + 0.01 * x)).max() < 1e-6


# ---- Philox ------------------------------------------------------------------------------------------------------------------------------
def test_philox_known_answers():
    """The three Random123 known-answer vectors of philox4x32-10."""
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for c, k, want in kat:
        ctr, sid, seed = c[0] | (c[1] << 32), c[2] | (c[3] << 32), k[0] | (k[1] << 32)
        got = I.philox4x32_10(np.array([ctr], dtype=np.uint64), sid, seed)[0]
        assert tuple(int(w) for w in got) == want, [hex(int(w)) for w in got]


def test_normals_are_standard_and_ordered():
    z = I.normals64(0, 1 << 16, I.FILL_STREAM, 11)
    assert z.shape == (1 << 18,) and abs(z.mean()) < 5 / 512 and abs(z.var() - 1) < 5 * math.sqrt(2.0 / (1 << 18))
    w = I.philox4x32_10(np.array([5], dtype=np.uint64), I.FILL_STREAM, 11)[0] >> np.uint64(8)
    r = math.sqrt(-2 * math.log((int(w[0]) + 1) / 2 ** 24))
    a = 2 * math.pi * int(w[1]) / 2 ** 24
    np.testing.assert_allclose(z[20:22], [r * math.cos(a), r * math.sin(a)], rtol=1e-12)
    np.testing.assert_array_equal(I.normals64(3, 9, 7, 11), I.normals64(0, 9, 7, 11)[12:])


# ---- loop control ------------------------------------------------------------------------------------------------------------------------
def test_loop_model_against_the_recorded_plateau_trace(golden):
    """plateau/lr of host.npz is the lr after each scheduler step, in double; the model keeps step_lr[1] in fp32, so every cut adds one
    rounding: rtol (cuts + 1) 2^-24."""
    h = golden("host")
    losses, rec = h["earlystop"]["losses"], h["plateau"]["lr"]
    lr0, factor, thr, pat = (float(x) for x in h["plateau"]["cfg"])
    log, hist = I.loop_control_run(losses, lr0, len(losses), I.loop_cfg(use_plateau=1, factor=factor, threshold=thr, patience=int(pat)))
    lrs = np.array([r[2] for r in log])
    cuts = int((np.diff(rec) != 0).sum())
    assert cuts >= 3 and len(log) == len(losses)
    np.testing.assert_allclose(lrs, rec, rtol=(cuts + 1) * 2.0 ** -24)
    np.testing.assert_array_equal(np.diff(lrs) != 0, np.diff(rec) != 0)
    hist = hist.reshape(-1, 4)
    np.testing.assert_array_equal(hist[:, 0], losses)
    np.testing.assert_array_equal(hist[1:, 3], lrs[:-1])                      # the row holds the lr the iteration used
    best = [i for i, r in enumerate(log) if r[0]]
    assert best == [i for i in range(len(losses)) if losses[i] <= losses[:i + 1].min()]


def test_loop_model_against_the_recorded_early_stop_and_the_host_class(golden):
    from deep_prior_interpolation_amd import utils as u
    h = golden("host")
    losses, stop = h["earlystop"]["losses"], h["earlystop"]["stop"]
    log, _ = I.loop_control_run(losses, 1e-3, len(losses), I.loop_cfg(es_patience=40, es_min_delta=1.0))
    first = int(np.flatnonzero(stop)[0])
    assert len(log) == first + 1 and log[-1][1] == 0 and all(r[1] == 1 for r in log[:-1])
    for name, (seq, cfg, _) in I.LOOP_SCRIPTS.items():
        log, _ = I.loop_control_run(seq, 1e-3, len(seq), cfg)
        st = u.EarlyStopping(patience=cfg["es_patience"], min_delta=cfg["es_min_delta"], percentage=True)
        want = []
        for loss in seq:
            want.append(bool(st.step(loss)))
            if want[-1]:
                break
        assert [r[1] == 0 for r in log] == want, name


def test_loop_scripts_reach_the_branches_they_are_named_for():
    run = lambda name: I.loop_control_run(I.LOOP_SCRIPTS[name][0], 1e-3, I.LOOP_SCRIPTS[name][2] or len(I.LOOP_SCRIPTS[name][0]), I.LOOP_SCRIPTS[name][1])
    assert [r[0] for r in run("ties")[0]] == [1, 1, 1, 0, 1, 1, 1]
    log, _ = run("nan-first")
    assert len(log) == 4 and log[-1][1] == 0 and [r[0] for r in log] == [1, 0, 0, 0]
    assert [r[0] for r in run("nan-first-no-es")[0]] == [1, 0, 0]
    log, _ = run("nan-later")
    assert len(log) == 3 and log[-1][1] == 0
    log, _ = run("nan-later-no-es")
    assert len(log) == 5 and [r[0] for r in log] == [1, 1, 0, 1, 1]
    assert len(run("rising")[0]) == 5
    assert all(r[2] == float(F(1e-3)) for r in run("lr-eps")[0]) and all(r[2] == float(F(1e-3)) for r in run("no-plateau")[0])
    lrs = [r[2] for r in run("min-lr")[0]]
    assert lrs[-1] == float(F(3e-4)) and float(F(5e-4)) in lrs and min(lrs) == float(F(3e-4))
    log, hist = run("past-max-iters")
    assert len(log) == 6 and log[-1][3][0] == 6.0 and np.isfinite(hist).all() and hist[8] == 0.8 and log[-1][2] < float(F(1e-3))


# ---- overlap-add -------------------------------------------------------------------------------------------------------------------------
def test_hits_against_a_brute_force_count():
    for N, p, s in ((20, 8, 4), (22, 10, 6), (27, 9, 9), (5, 3, 1), (8, 4, 2), (133, 130, 3), (65, 65, 1), (23, 10, 6)):
        want = np.zeros(N, dtype=np.int64)
        for k in range(0, N - p + 1, s):
            want[k:k + p] += 1
        np.testing.assert_array_equal(I.hits(N, p, s), want)
    assert (I.hits(23, 10, 6)[-1:] == 0).all()                                # an uncovered tail: count 0


@pytest.mark.parametrize("name", [k for k in I.OVERLAP_CASES if not k.startswith("65")])
def test_overlap_restatement_against_float64(name):
    volume, patch, stride, _ = I.OVERLAP_CASES[name]
    patches, origins = I.overlap_patches(name)
    acc = I.overlap_add_np(volume, patch, patches, origins)
    ref, cnt = np.zeros(volume), np.zeros(volume)
    for p, (a, b, c) in zip(patches, origins):
        ref[a:a + patch[0], b:b + patch[1], c:c + patch[2]] += p
        cnt[a:a + patch[0], b:b + patch[1], c:c + patch[2]] += 1
    assert cnt.min() >= 1
    out = I.overlap_normalize_np(acc, patch, stride, 40.0)
    assert out.dtype == F
    np.testing.assert_allclose(out, ref / cnt / 40.0, rtol=1e-5, atol=1e-6)


# ---- a wrong kernel is caught: the device test's check functions on mutated restatements -------------------------------------------------
def test_adam_without_the_tail_fails_the_check():
    rng = np.random.RandomState(5)
    for n in I.ADAM_SIZES[:7] + (4099,):
        p, g, m, v = I.adam_row(n, rng)
        want = I.adam_np(p, g, m, v, 10, 1e-3)
        I.check_adam(I.adam_np(p, g, m, v, 10, 1e-3), want, "unmutated")
        assert _fails(lambda: I.check_adam(I.adam_np(p, g, m, v, 10, 1e-3, mutation="no_tail"), want, "no tail")) == (n % 4 != 0), n


def test_adam_with_the_bias_correction_inside_the_root_fails_the_check():
    rng = np.random.RandomState(6)
    for hyper, step, lr in I.ADAM_LAUNCHES:
        p, g, m, v = I.adam_row(1023, rng)
        want = I.adam_np(p, g, m, v, step, lr, *hyper)
        assert _fails(lambda: I.check_adam(I.adam_np(p, g, m, v, step, lr, *hyper, mutation="bc2s_before_sqrt"), want, "bc2s"))


@pytest.mark.parametrize("kind", [0, 1])
def test_a_loss_sum_without_its_last_pass_fails_the_check(kind):
    for n in (255, 2048, 2049, 262147, 2359299):
        o, t, m = I.loss_inputs(n, n)
        I.check_loss_result(I.loss_result64(o, t, m, kind), o, t, m, kind, False, "unmutated")
        bad = I.loss_result64(o, t, m, kind, keep=I.loss_walk_keep(n, "drop_last_pass"))
        assert _fails(lambda: I.check_loss_result(bad, o, t, m, kind, False, "last pass dropped")), n


@pytest.mark.parametrize("shape", I.HOLDOUT_SHAPES)
def test_a_holdout_walk_without_the_carry_fails_the_check(shape):
    C, T, S = shape
    o, t, m, sel = I.holdout_inputs(shape, 7)
    h = I.holdout_h(shape, sel)
    np.testing.assert_array_equal(h, np.broadcast_to(sel[:, None, :], shape))
    ref, _, count = I.holdout_ref(o, t, m, h, 1)
    good = np.array([0] * 8 + [ref[0] / count, 10 * math.log10(ref[1] / ref[2]), count], dtype=np.float64)
    I.check_holdout(good, o, t, m, h, 1, "unmutated")
    hb = I.holdout_h(shape, sel, "no_r_carry")
    rb, _, cb = I.holdout_ref(o, t, m, hb, 1)
    bad = np.array([0] * 8 + [rb[0] / max(cb, 1), 10 * math.log10(rb[1] / rb[2]) if cb else 0.0, cb], dtype=np.float64)
    carried = I.holdout_walk(shape)[2]["r"] > 0
    assert _fails(lambda: I.check_holdout(bad, o, t, m, h, 1, "no carry")) == carried, shape
    # the training part would differ too: m_tr = m (1 - h) is what dout and result[0..7] are compared on, bit for bit
    assert (not np.array_equal(m * (1 - hb), m * (1 - h))) == carried


def test_philox_with_counter_and_stream_swapped_fails_the_check():
    for q0, q1 in ((0, 257), (I.NOISE_NT // 4 - 1024, I.NOISE_NT // 4)):
        z = I.normals64(q0, q1, I.FILL_STREAM, 11)
        got = (2.0 + 0.5 * z).astype(F)                                       # an fp32 evaluation passes
        assert I.check_normals(got, 2.0, z, 0.5, False, "unmutated") < 1e-3
        bad = (2.0 + 0.5 * I.normals64(q0, q1, I.FILL_STREAM, 11, mutation="swap_ctr_stream")).astype(F)
        assert _fails(lambda: I.check_normals(bad, 2.0, z, 0.5, False, "swapped"))
        lanes = (2.0 + 0.5 * z.reshape(-1, 4)[:, [1, 0, 2, 3]].reshape(-1)).astype(F)
        assert _fails(lambda: I.check_normals(lanes, 2.0, z, 0.5, False, "sin before cos"))
    zb = torch.from_numpy((0.03 * z).astype(F)).to(torch.bfloat16).float().numpy()
    I.check_normals(zb, 0.0, z, 0.03, True, "bf16 storage")
    assert _fails(lambda: I.check_normals(zb, 0.0, z, 0.03, False, "bf16 held to the fp32 bar"))


def test_loop_control_with_a_strict_comparison_fails_the_check():
    seq, cfg, _ = I.LOOP_SCRIPTS["ties"]
    want, _ = I.loop_control_run(seq, 1e-3, len(seq), cfg)
    got, _ = I.loop_control_run(seq, 1e-3, len(seq), cfg, mutation="improved<")
    I.check_loop_log(want, want, "unmutated")
    assert _fails(lambda: I.check_loop_log(got, want, "strict"))


def test_loop_control_holdout_with_a_strict_comparison_fails_the_check():
    seq, qs, cfg, n = I.variant_scripts("holdout")["ties"]
    want, _ = I.loop_control_run(seq, 1e-3, n, cfg, variant="holdout", qs=qs)
    got, _ = I.loop_control_run(seq, 1e-3, n, cfg, mutation="improved<", variant="holdout", qs=qs)
    I.check_loop_log(want, want, "unmutated")
    assert _fails(lambda: I.check_loop_log(got, want, "strict"))


MOVED = [(v, k) for v, table in (("holdout", I.HOLDOUT_SCRIPTS), ("ema", I.EMA_SCRIPTS), ("ema-holdout", I.EMA_SCRIPTS)) for k in sorted(table)]


@pytest.mark.parametrize("variant, name", MOVED, ids=["%s-%s" % c for c in MOVED])
def test_loop_model_variants_against_the_eager_rules(variant, name):
    """The extended model against utils.select_latest_min + utils.EarlyStopping + the plateau arithmetic (iteration_cases.eager_loop_model)
    on every script of the two shared tables: improved, best_iter, the lr each iteration used (bit-equal: both cut in fp32) and the
    stopping iteration."""
    rows, plateau, es = (I.HOLDOUT_SCRIPTS if variant == "holdout" else I.EMA_SCRIPTS)[name]
    losses, qs, cfg, n = I.variant_scripts(variant)[name]
    assert cfg == I.script_cfg(plateau, es) and n == len(rows)
    ref = I.eager_loop_model(rows, 1e-3, plateau, es)
    log, hist = I.loop_control_run(losses, 1e-3, n, cfg, variant=variant, qs=qs)
    assert len(log) == len(ref)                                                # the stopping iteration
    assert (log[-1][1] == 0) == (len(ref) < len(rows))
    assert [r[0] for r in log] == [r[0] for r in ref]
    assert [int(r[3][9]) for r in log] == [r[2] for r in ref]
    lr_used = hist.reshape(n, -1)[:len(log), 3]
    np.testing.assert_array_equal(lr_used, [r[1] for r in ref])
    assert log[-1][3][0] == len(log) and np.isnan(hist.reshape(n, -1)[len(log):]).all()


# ---- csrc/loop_rule.h as a stand-alone program -----------------------------------------------------------------------------------------
def _hex64(x):
    return "%016x" % int(np.float64(x).view(np.uint64))


def test_loop_rule_header_as_plain_cpp_against_the_model(tmp_path):
    """csrc/loop_rule.h, the one body behind the three dpi_loop_control* kernels, compiled as plain C++ with tests/host_loop_rule/main.cpp
    under the address and undefined-behaviour sanitizers and run on the CPU over every script of every variant (variant_scripts: the
    past-the-end case has six calls on a history of three rows), on heap buffers of exactly the documented sizes.  *improved, *active,
    the bits of step_lr[1], every state double and the whole history must equal the numpy model's bit for bit, a NaN equal to a NaN.
    The sanitizers instrument host code only: nothing here is compiled for, or run on, a device."""
    import os
    import shutil
    import subprocess
    from conftest import ROOT
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    csrc = os.path.join(ROOT, "deep_prior_interpolation_amd", "csrc")
    exe = str(tmp_path / "host_loop_rule")
    flags = ("-x c++ -O1 -g -std=c++17 -ffp-contract=off -Wall -Xarch_host -fsanitize=address,undefined -fno-sanitize-recover=undefined "
             "-fno-omit-frame-pointer")
    subprocess.check_call([hipcc] + flags.split() + ["-I", csrc, os.path.join(ROOT, "tests", "host_loop_rule", "main.cpp"), "-o", exe], timeout=300)
    cases, lines = [], []
    for variant, (ho, ema) in I.LOOP_VARIANTS.items():
        for name, (losses, qs, cfg, n) in sorted(I.variant_scripts(variant).items()):
            cases.append((variant, name, I.loop_control_run(losses, 1e-3, n, cfg, variant=variant, qs=qs)))
            n_in = 11 if ho else 8
            lines.append("run %d %d %d %d %d %08x %d %s %s %d %s %s %d %s" % (
                ho, ema, n, len(losses), n_in, int(F(1e-3).view(np.uint32)), cfg["use_plateau"], _hex64(cfg["factor"]), _hex64(cfg["threshold"]),
                cfg["patience"], _hex64(cfg["min_lr"]), _hex64(cfg["lr_eps"]), cfg["es_patience"], _hex64(cfg["es_min_delta"])))
            for it, loss in enumerate(losses):
                for x in I.loop_inputs(variant, it, loss, None if qs is None else qs[it]):
                    if x is not None:
                        lines.append(" ".join(_hex64(v) for v in x[:n_in]))
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1"))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    out = r.stdout.split("\n")
    assert out[-2] == "%d runs" % len(cases) and len(cases) == 10 + (4 + 1) + 2 * (5 + 1)
    doubles = lambda words: np.array([int(w, 16) for w in words], dtype=np.uint64).view(np.float64)
    k = 0
    for variant, name, (want, want_hist) in cases:
        got = []
        while out[k].startswith("C "):
            w = out[k].split()
            got.append((int(w[1]), int(w[2]), float(np.array([int(w[3], 16)], dtype=np.uint32).view(F)[0]), doubles(w[4:])))
            k += 1
        assert out[k].startswith("H")
        got_hist = doubles(out[k].split()[1:])
        k += 1
        what = "loop_rule.h %s %s" % (variant, name)
        I.check_loop_log(got, want, what)
        for g, w in zip(got, want):                                             # bit patterns, beyond check_loop_log's values
            same = (g[3].view(np.uint64) == w[3].view(np.uint64)) | (np.isnan(g[3]) & np.isnan(w[3]))
            assert same.all(), (what, g[3], w[3])
        assert got_hist.shape == want_hist.shape, what
        same = (got_hist.view(np.uint64) == want_hist.view(np.uint64)) | (np.isnan(got_hist) & np.isnan(want_hist))
        assert same.all(), (what, got_hist, want_hist)


@pytest.mark.parametrize("name", [k for k in I.OVERLAP_CASES if not k.startswith("65")])
def test_a_window_count_with_kmax_off_by_one_fails_the_check(name):
    volume, patch, stride, _ = I.OVERLAP_CASES[name]
    patches, origins = I.overlap_patches(name)
    acc = I.overlap_add_np(volume, patch, patches, origins)
    want = I.overlap_normalize_np(acc, patch, stride, 40.0)
    I.check_bits(I.overlap_normalize_np(acc, patch, stride, 40.0), want, "unmutated")
    assert _fails(lambda: I.check_bits(I.overlap_normalize_np(acc, patch, stride, 40.0, mutation="kmax-1"), want, "kmax - 1"))
