"""What a launch of csrc/elementwise.hip computes and may touch, kernel by kernel, at the sizes where the kernels change behaviour: the rows
of tests/elementwise_cases.py through the C ABI, every buffer owned by the test.  Tensors a launch may write are NaN-filled channel slices
of a larger buffer (guard_slice) or NaN-filled buffers inside guard bands (guard), inputs sit inside bands too, partial rows and
workspaces have exactly the queried size.  After every launch: _launch, _check_guards (both end the session on a launch error or a device
fault, as in test_gpu_conv_contract.py), every declared element finite, and the result against the float64 restatement of
elementwise_cases.py (held against torch by tests/test_elementwise_refs_host.py).  Kernels are never a reference for each other.

Bars (none is new): 5e-6 norm-wise for fp32 elementwise results of one expression (test_bn_large_offset), 2e-5 on dx tensors and 2e-4 on
per-channel gradients (test_join_bwd_two_pass...), 1e-6 up-sampling forward and 2e-6 adjoint, bit equality for copies, add, lrelu_bwd,
nearest up-sampling and crop, half a bf16 ulp (half_ulp_ok, slack 0.503) for a bf16 tensor stored once from bf16-representable operands.
Partial sums are bounded absolutely, partial by partial: |got - float64| <= (k 2^-24 + n 2^-53) sum|term| (elementwise_cases.
check_partials), with k counted from the kernel's arithmetic at each call site below.

Precondition (include/dpi_hip.h): the vector paths are chosen from V % 4 alone, so every buffer here is 16-byte aligned (bf16: 8-byte)
whenever V % 4 == 0 — _aligned asserts it — and element-aligned bases appear only with V % 4 != 0."""
import functools

import numpy as np
import pytest
import torch

import elementwise_cases as E
from gpu_guard import guard, guard_slice
from test_gpu_bf16_storage import half_ulp_ok
from test_gpu_conv_contract import _check_guards, _launch, rel

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
S02 = float(np.float32(0.2))                       # the slope as the kernels receive it
IO_IDS = {0: "fp32", 1: "fwd-bf16", 2: "grad-bf16", 3: "bf16"}
vid = lambda r: "V%d" % r.V
upid = lambda r: "%dx%dx%d-%dx%dx%d" % (r.inp + r.out)
V_IO = [(r, 0) for r in E.V_ROWS] + [(r, 3) for r in E.V_ROWS_BF16]
v_io = pytest.mark.parametrize("row,io", V_IO, ids=["%s-%s" % (vid(r), IO_IDS[io]) for r, io in V_IO])


@pytest.fixture(scope="module")
def lib():
    from deep_prior_interpolation_amd import _lib
    return _lib


# ---- buffers -----------------------------------------------------------------------------------------------------------------------------
def _aligned(g, V):
    """The precondition of the vector paths: V % 4 == 0 comes with a 16-byte-aligned base (8 bytes for bf16)."""
    if V % 4 == 0:
        assert g.payload.data_ptr() % (4 * g.payload.element_size()) == 0, "test buffer off the alignment a channel slice has"
    return g


def gin(t, dtype=F32, offset=0):
    """An input inside guard bands, [C][V...] at a 256-byte-aligned address (+ offset elements)."""
    return _aligned(guard(t.numel(), dtype, DEV, fill=t, offset=offset, shape=tuple(t.shape)), 1 if offset else t.shape[-1])


def gout(C_, V, dtype=F32, c0=None):
    """An output: NaN-filled channels [c0, c0 + C) of a larger channel-planar buffer."""
    return _aligned(guard_slice(C_, V, dtype, DEV, c0=c0), V)


def gvec(n, dtype=F32, fill=None):
    return guard(n, dtype, DEV, fill=fill)


def ptr(g):
    return None if g is None else (g.payload if hasattr(g, "payload") else g).data_ptr()


def written(t, what):
    assert bool(torch.isfinite(t.float()).all()), "%s: %d elements were not written (NaN pre-fill left)" % (what, int((~torch.isfinite(t.float())).sum()))


def stored_ok(got, ref64, what, bar):
    """A stored tensor against the float64 restatement: `bar` norm-wise for fp32, half a bf16 ulp for a bf16 tensor stored once."""
    written(got, what)
    if got.dtype == BF:
        half_ulp_ok(got, ref64.reshape(got.shape), what)
    else:
        assert rel(got, ref64) < bar, (what, rel(got, ref64))


@functools.lru_cache(maxsize=None)
def v_problem(V, bf16):
    """Operands of one V row (C = 3), shared by its tests and never modified: per-channel offset and scale, chain tables whose channel 1
    is the identity (a NULL chain is what chain_b and dpi_channel_sum use), bf16-representable tensors for the bf16 rows."""
    gen = torch.Generator().manual_seed(1000 + V)
    p = {k: E.channel_data(3, V, gen, bf16) for k in ("x", "a", "b")}
    p["dy"] = torch.randn((3, V), generator=gen)
    p["dy"] = p["dy"].to(BF).float() if bf16 else p["dy"]
    p["chain"], p["chain_out"] = E.chain_table(3, gen), E.chain_table(3, gen, identity=(2,))
    p["gamma"], p["beta"] = torch.rand(3, generator=gen) + 0.5, torch.randn(3, generator=gen) * 0.3
    p["chain_d"], p["chain_out_d"] = p["chain"].to(DEV), p["chain_out"].to(DEV)          # held here: a temporary would be freed before the launch
    p["chain_b"] = E.chain_table(3, gen, identity=(0,))                                    # drawn last: the operands above keep their values
    p["chain_b_d"] = p["chain_b"].to(DEV)
    return p


def dt(io, bit):
    return BF if io & bit else F32


def stat_mags(m):
    return torch.stack([E.span_sums(m), E.span_sums(m * m)], 2)


# ---- the span kernels at every V row -----------------------------------------------------------------------------------------------------
@v_io
def test_channel_stats_partial_rows(lib, row, io):
    """partials[nblk][C][2] = {sum T(x), sum T(x)^2} span by span.  k = 6 for both: T(x) = fma, slope product, fma is three roundings, each
    at most 2^-24 of |qs act(ps x + pb)| + |qb| (the term's magnitude); the four-element fp32 pre-sum `ls += y` adds three more of at most
    2^-24 sum|y|; squares are formed and summed in double from the fp32 y: (y + e)^2 - y^2 <= 2 x 3 x 2^-24 term^2."""
    L, p = lib.load(), v_problem(row.V, bool(io))
    C_, V = 3, row.V
    xg, pg = gin(p["x"], dt(io, 1)), gvec(row.nblk * C_ * 2, F64)
    _launch(lib, L.dpi_channel_stats_io(ptr(xg), ptr(p["chain_d"]), C_, V, ptr(pg), io & 1, lib.stream()), "dpi_channel_stats_io")
    _check_guards([("x", xg), ("partials", pg)], "channel_stats " + vid(row))
    E.check_partials(pg.payload.view(row.nblk, C_, 2), E.partials64(E.chain64(p["x"], p["chain"])), stat_mags(E.chain_mag64(p["x"], p["chain"])),
                     6, "channel_stats " + vid(row))


@pytest.mark.parametrize("row", E.V_ROWS, ids=vid)
def test_channel_sum(lib, row):
    """ws = the partial rows of the identity chain (k = 3: only the fp32 pre-sum rounds), out[c] = float(total): one more rounding of the
    total on top of the partials' bound."""
    L, p = lib.load(), v_problem(row.V, False)
    C_, V = 3, row.V
    xg, wg, og = gin(p["x"]), gvec(row.nblk * C_ * 2, F64), gvec(C_)
    _launch(lib, L.dpi_channel_sum(ptr(xg), C_, V, ptr(wg), ptr(og), lib.stream()), "dpi_channel_sum")
    _check_guards([("x", xg), ("ws", wg), ("out", og)], "channel_sum " + vid(row))
    x64 = p["x"].double()
    E.check_partials(wg.payload.view(row.nblk, C_, 2), E.partials64(x64), stat_mags(x64.abs()), 3, "channel_sum ws " + vid(row))
    written(og.payload, "out")
    tot, mag = x64.sum(1), x64.abs().sum(1)
    assert bool(((og.payload.cpu().double() - tot).abs() <= (3 * E.U + V * 2.0 ** -53) * mag + E.U * tot.abs()).all())


@v_io
def test_chain_apply(lib, row, io):
    L, p = lib.load(), v_problem(row.V, bool(io))
    xg, yg = gin(p["x"], dt(io, 1)), gout(3, row.V, dt(io, 1))
    _launch(lib, L.dpi_chain_apply_io(ptr(xg), ptr(p["chain_d"]), 3, row.V, ptr(yg), io & 1, lib.stream()), "dpi_chain_apply_io")
    _check_guards([("x", xg), ("y", yg)], "chain_apply " + vid(row))
    stored_ok(yg.payload, E.chain64(p["x"], p["chain"]), "chain_apply y", 5e-6)


@pytest.mark.parametrize("form", ["pre-post", "in_chain-post"])
@v_io
def test_bn_bwd_reduce_and_apply(lib, row, io, form):
    """Phase 1 partial rows {sum g, sum g xhat} span by span, then phase 2 driven by them: dgamma, dbeta and every element of dx against
    float64 autograd of act_post(BN(act_pre(x))) (or BN(T_in(x)), gradient with respect to T_in(x)).
    k for sum g: 4 = the product dy * post_slope + three pre-sum additions, terms |g|.  k for sum g xhat: 10 with terms
    |g| invstd (mag(u) + |mean|) >= |g xhat|: g rounds once; u rounds up to three times (a chain), u - mean and the product with invstd
    once each, together at most 5 x 2^-24 invstd (mag(u) + |mean|); the four fmas of the pre-sum round four times.
    V = 1 has dx = dgamma = 0 exactly (every term cancels): there the error is held against the terms that cancel, |gamma invstd dy|.
    Elements within 1e-5 of the jump of act_post' get dy = 0 (elementwise_cases.post_edge64: a handful per row at most)."""
    L, p = lib.load(), v_problem(row.V, bool(io))
    C_, V = 3, row.V
    chain = p["chain"] if form.startswith("in_chain") else None
    pre, post = (1.0 if chain is not None else S02), S02
    u = E.chain64(p["x"], chain) if chain is not None else E.lrelu(p["x"].double(), pre)
    mi = E.mean_invstd_of(u)
    edge = E.post_edge64(p["x"], mi, p["gamma"], p["beta"], chain, pre)
    assert int(edge.sum()) <= 8, int(edge.sum())
    p = dict(p, dy=torch.where(edge, torch.zeros(()), p["dy"]))
    dev = lambda t: None if t is None else t.to(DEV)
    mi_d, ga, be, ch = dev(mi), dev(p["gamma"]), dev(p["beta"]), dev(chain)
    xg, dyg, pg = gin(p["x"], dt(io, 1)), gin(p["dy"], dt(io, 2)), gvec(row.nblk * C_ * 2, F64)
    _launch(lib, L.dpi_bn_bwd_reduce_io(ptr(dyg), ptr(xg), ptr(mi_d), ptr(ga), ptr(be), ptr(ch), pre, post, C_, V, ptr(pg), io, lib.stream()),
            "dpi_bn_bwd_reduce_io")
    _check_guards([("x", xg), ("dy", dyg), ("partials", pg)], "bn_bwd_reduce " + vid(row))
    ref, mag = E.bn_bwd_partials64(p["dy"], p["x"], mi, p["gamma"], p["beta"], chain, pre, post)
    E.check_partials(pg.payload.view(row.nblk, C_, 2), ref, mag, torch.tensor([4.0, 10.0], dtype=F64), "bn_bwd_reduce " + vid(row))
    dxg, dgg, dbg = gout(C_, V, dt(io, 2)), gvec(C_), gvec(C_)
    _launch(lib, L.dpi_bn_bwd_apply_io(ptr(dyg), ptr(xg), ptr(mi_d), ptr(ga), ptr(be), ptr(ch), pre, post, ptr(pg), row.nblk, C_, V, ptr(dxg), ptr(dgg),
                                       ptr(dbg), io, lib.stream()), "dpi_bn_bwd_apply_io")
    _check_guards([("x", xg), ("dy", dyg), ("partials", pg), ("dx", dxg), ("dgamma", dgg), ("dbeta", dbg)], "bn_bwd_apply " + vid(row))
    dx, dg, db = E.bn_bwd_autograd64(p["dy"], p["x"], p["gamma"], p["beta"], chain, pre, post)
    for t_, w in ((dxg.payload, "dx"), (dgg.payload, "dgamma"), (dbg.payload, "dbeta")):
        written(t_, w)
    if V == 1:
        scale = float((p["gamma"].double() * mi[1].double() * p["dy"][:, 0].double()).norm())
        assert float(dxg.payload.double().norm()) <= 2e-5 * scale
        assert bool((dgg.payload.cpu().double().abs() <= 11 * E.U * mag[0, :, 1]).all())          # the partial's own bound + the rounding to float
        assert rel(dbg.payload, db) < 2e-4
        return
    stored_ok(dxg.payload, dx, "dx", 2e-5)
    assert rel(dgg.payload, dg) < 2e-4 and rel(dbg.payload, db) < 2e-4, (rel(dgg.payload, dg), rel(dbg.payload, db))


def _chain_add_stats(lib, row, io, store_t, with_chain_b):
    L, p = lib.load(), v_problem(row.V, bool(io))
    C_, V = 3, row.V
    chain_b, chain_b_d = (p["chain_b"], p["chain_b_d"]) if with_chain_b else (None, None)
    ag, bg = gin(p["a"], dt(io, 1)), gin(p["b"], dt(io, 1))
    tg, pg = (gout(C_, V, dt(io, 1)) if store_t else None), gvec(row.nblk * C_ * 2, F64)
    _launch(lib, L.dpi_chain_add_stats_io(ptr(ag), ptr(p["chain_d"]), ptr(bg), ptr(chain_b_d), C_, V, S02, ptr(tg), ptr(pg), io & 1, lib.stream()),
            "dpi_chain_add_stats_io")
    _check_guards([("a", ag), ("b", bg), ("t", tg), ("partials", pg)], "chain_add_stats " + vid(row))
    t64 = E.chain_add64(p["a"], p["chain"], p["b"], chain_b)
    got = pg.payload.view(row.nblk, C_, 2)
    if store_t:
        stored_ok(tg.payload, t64, "t", 5e-6)
    if store_t and io:
        y = E.lrelu(tg.payload.float().cpu().double(), S02)
        E.check_partials(got, E.partials64(y), stat_mags(y.abs()), torch.tensor([4.0, 2.0], dtype=F64), "chain_add_stats (stored t) " + vid(row))
    else:
        mag = E.chain_mag64(p["a"], p["chain"]) + E.chain_mag64(p["b"], chain_b)
        E.check_partials(got, E.partials64(E.lrelu(t64, S02)), stat_mags(mag), torch.tensor([8.0, 10.0], dtype=F64), "chain_add_stats " + vid(row))


@pytest.mark.parametrize("store_t", [True, False], ids=["t", "stats-only"])
@v_io
def test_chain_add_stats(lib, row, io, store_t):
    """t = T_a(a) + b (chain_b NULL) and the partial rows of act(t).  k = 8 for the sums, 10 for the squares, terms mag(T_a(a)) + |b|: three
    roundings in T_a, one in the sum, one in the slope product (5), three pre-sum additions; squares 2 x 5, summed in double.  With t stored
    as bf16 the statistics describe the STORED t: they are held against float64 sums of act(what the launch stored) — k = 4 and 2: the slope
    product and the pre-sum."""
    _chain_add_stats(lib, row, io, store_t, False)


@pytest.mark.parametrize("store_t", [True, False], ids=["t", "stats-only"])
@v_io
def test_chain_add_stats_with_chain_b(lib, row, io, store_t):
    """t = T_a(a) + T_b(b), what side B of a Block3d join carries (channel 0 of chain_b is the identity).  The same k: T_b's three roundings
    are at most 3 x 2^-24 of mag(T_b(b)) as T_a's are of mag(T_a(a)), so the terms mag(T_a(a)) + mag(T_b(b)) keep k = 8 and 10."""
    _chain_add_stats(lib, row, io, store_t, True)


def _chain_add_apply(lib, row, io, with_chain_b):
    L, p = lib.load(), v_problem(row.V, bool(io))
    chain_b, chain_b_d = (p["chain_b"], p["chain_b_d"]) if with_chain_b else (None, None)
    ag, bg, yg = gin(p["a"], dt(io, 1)), gin(p["b"], dt(io, 1)), gout(3, row.V, dt(io, 1))
    _launch(lib, L.dpi_chain_add_apply(ptr(ag), ptr(p["chain_d"]), ptr(bg), ptr(chain_b_d), ptr(p["chain_out_d"]), 3, row.V, ptr(yg), io & 1, lib.stream()),
            "dpi_chain_add_apply")
    _check_guards([("a", ag), ("b", bg), ("y", yg)], "chain_add_apply " + vid(row))
    stored_ok(yg.payload, E.chain64(E.chain_add64(p["a"], p["chain"], p["b"], chain_b), p["chain_out"]), "chain_add_apply y", 5e-6)


@v_io
def test_chain_add_apply(lib, row, io):
    _chain_add_apply(lib, row, io, False)


@v_io
def test_chain_add_apply_with_chain_b(lib, row, io):
    """chain_b != NULL: y = T_out(T_a(a) + T_b(b)), the same 5e-6."""
    _chain_add_apply(lib, row, io, True)


# ---- partial-row counts ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["plain", "act_first", "in_chain"])
@pytest.mark.parametrize("nblk", E.FINALIZE_NBLK)
def test_bn_finalize_row_counts(lib, nblk, form):
    """Synthetic partial rows (every row moves the statistics by far more than the bar, elementwise_cases.synthetic_partials) around the
    bounds of the two-loads loop; C in {1, 5}, with and without running statistics; mean, invstd, running statistics and chain_out at the
    5e-6 of an fp32 result of one expression, num_batches_tracked exactly."""
    L = lib.load()
    count = 4096
    for C_ in (1, 5):
        for running in (False, True):
            gen = torch.Generator().manual_seed(nblk * 10 + C_)
            part = E.synthetic_partials(nblk, C_, seed=C_)
            gamma, beta = torch.rand(C_, generator=gen) + 0.5, torch.randn(C_, generator=gen) * 0.3
            rm, rv = torch.randn(C_, generator=gen), torch.rand(C_, generator=gen) + 0.5
            in_chain = E.chain_table(C_, gen, identity=()) if form == "in_chain" else None
            slope = 1.0 if form == "in_chain" else S02
            pg, mg, cg = gin(part, F64), gvec(2 * C_), gvec(5 * C_)
            rmg, rvg = (gvec(C_, fill=rm), gvec(C_, fill=rv)) if running else (None, None)
            nbt = torch.tensor([7], dtype=torch.int64, device=DEV) if running else None
            dev = lambda t: None if t is None else t.to(DEV)
            ga, be, ic = dev(gamma), dev(beta), dev(in_chain)
            _launch(lib, L.dpi_bn_finalize(ptr(pg), nblk, C_, count, ptr(ga), ptr(be), E.EPS, E.MOMENTUM, slope, int(form == "act_first"), ptr(ic), ptr(rmg),
                                           ptr(rvg), ptr(nbt), ptr(mg), ptr(cg), lib.stream()), "dpi_bn_finalize")
            what = "bn_finalize nblk=%d C=%d %s" % (nblk, C_, form)
            _check_guards([("partials", pg), ("mean_invstd", mg), ("chain_out", cg), ("running_mean", rmg), ("running_var", rvg)], what)
            ref = E.finalize64(part, count, gamma, beta, slope=slope, act_first=int(form == "act_first"), in_chain=in_chain,
                               running_mean=rm if running else None, running_var=rv if running else None, nbt=7 if running else None)
            stored_ok(mg.payload, ref["mean_invstd"], what + " mean_invstd", 5e-6)
            stored_ok(cg.payload, ref["chain_out"], what + " chain_out", 5e-6)
            if running:
                stored_ok(rmg.payload, ref["running_mean"], what + " running_mean", 5e-6)
                stored_ok(rvg.payload, ref["running_var"], what + " running_var", 5e-6)
                assert int(nbt) == ref["nbt"] == 8


@pytest.mark.parametrize("nblk", E.APPLY_NBLK)
def test_bn_bwd_apply_row_counts(lib, nblk):
    """dpi_bn_bwd_apply with a caller-given number of partial rows (what a convolution's fused statistics hand over), V = 1287: the one-wave
    prologue strides by 64.  The rows are synthetic, so the totals are not the sums of these tensors: dx is held against the header's
    formula with the float64 totals of the rows; one dropped row would move sum_g / V by about 0.3 where |g| is about 1."""
    L, p = lib.load(), v_problem(1287, False)
    C_, V = 3, 1287
    part = E.synthetic_partials(nblk, C_, seed=3) * (0.2 * V)
    mi = E.mean_invstd_of(E.lrelu(p["x"].double(), S02))
    dev = lambda t: t.to(DEV)
    mi_d, ga, be = dev(mi), dev(p["gamma"]), dev(p["beta"])
    xg, dyg, pg = gin(p["x"]), gin(p["dy"]), gin(part, F64)
    dxg, dgg, dbg = gout(C_, V), gvec(C_), gvec(C_)
    _launch(lib, L.dpi_bn_bwd_apply(ptr(dyg), ptr(xg), ptr(mi_d), ptr(ga), ptr(be), None, S02, S02, ptr(pg), nblk, C_, V, ptr(dxg), ptr(dgg), ptr(dbg),
                                    lib.stream()), "dpi_bn_bwd_apply")
    _check_guards([("x", xg), ("dy", dyg), ("partials", pg), ("dx", dxg), ("dgamma", dgg), ("dbeta", dbg)], "bn_bwd_apply nblk=%d" % nblk)
    dx, dg, db = E.bn_bwd_apply64(p["dy"], p["x"], mi, p["gamma"], p["beta"], None, S02, S02, part.sum(0))
    stored_ok(dxg.payload, dx, "dx", 2e-5)
    written(dgg.payload, "dgamma"), written(dbg.payload, "dbeta")
    assert rel(dgg.payload, dg) < 2e-4 and rel(dbg.payload, db) < 2e-4


# ---- one large row per streaming kernel ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def large():
    """C = 1, V = LARGE_V + 1 floats drawn on the device from a seeded generator (the vector rows use the first LARGE_V of them; that view
    is 256-byte aligned), inside guard bands, shared by the large tests and never modified.  The float64 restatements are evaluated by torch
    on the device copies: 33.5 M doubles per intermediate would take the host seconds per test."""
    gen = torch.Generator(device=DEV).manual_seed(77)
    n = E.LARGE_V + 1
    x = torch.randn(n, generator=gen, device=DEV) * 1.3 + 0.7
    dy = torch.randn(n, generator=gen, device=DEV)
    x[:8] = torch.tensor([0.0, -0.0, 1.0, -1.0, 0.0, -0.0, 2.0, -2.0], device=DEV)          # zeros of both signs for lrelu_bwd
    gen_h = torch.Generator().manual_seed(78)
    chain = E.chain_table(1, gen_h, identity=())
    return {"x": guard(n, F32, DEV, fill=x), "dy": guard(n, F32, DEV, fill=dy), "chain": chain, "chain_d": chain.to(DEV),
            "gamma": torch.tensor([1.3]), "beta": torch.tensor([-0.2])}


def rel_dev(a, b):
    """`rel` without the trip to the host."""
    a, b = a.detach().double().reshape(-1), b.detach().double().reshape(-1)
    return float((a - b).norm() / (b.norm() + 1e-300))


@pytest.mark.parametrize("extra", [0, 1], ids=["V", "V+1"])
def test_large_channel_stats(lib, extra):
    """Non-temporal loads, 2048 capped blocks with spans of 16396 voxels (17 trips per thread); V + 1: the same on the scalar path.
    k = 6 as in test_channel_stats_partial_rows."""
    L, p = lib.load(), large()
    V = E.LARGE_V + extra
    x = p["x"].payload[:V].view(1, V)
    pg = gvec(E.MAX_STAT_BLOCKS * 2, F64)
    _launch(lib, L.dpi_channel_stats(x.data_ptr(), ptr(p["chain_d"]), 1, V, ptr(pg), lib.stream()), "dpi_channel_stats")
    _check_guards([("x", p["x"]), ("partials", pg)], "channel_stats large")
    y, m = E.chain64(x, p["chain"]), E.chain_mag64(x, p["chain"])
    E.check_partials(pg.payload.view(-1, 1, 2), E.partials64(y), stat_mags(m), 6, "channel_stats large", span_len=E.stat_span(V, E.MAX_STAT_BLOCKS))


def test_large_chain_apply(lib):
    """Non-temporal loads and stores, grid capped at 4096 blocks: the grid-stride loop."""
    L, p = lib.load(), large()
    V = E.LARGE_V
    x = p["x"].payload[:V].view(1, V)
    yg = _aligned(guard(V, F32, DEV), V)
    _launch(lib, L.dpi_chain_apply(x.data_ptr(), ptr(p["chain_d"]), 1, V, ptr(yg), lib.stream()), "dpi_chain_apply")
    _check_guards([("x", p["x"]), ("y", yg)], "chain_apply large")
    written(yg.payload, "y")
    assert rel_dev(yg.payload, E.chain64(x, p["chain"])) < 5e-6


@pytest.mark.parametrize("extra", [0, 1], ids=["V", "V+1"])
def test_large_bn_bwd(lib, extra):
    """dpi_bn_bwd_reduce at the capped block count (V + 1: scalar path, reduce only) and, at V, dpi_bn_bwd_apply with its grid-stride loop:
    dgamma, dbeta and every element of dx.  No activation masks (pre = post = 1): one element of 33.5 M whose mask flips in fp32 would be a
    difference of the operands, not of the kernel.  k = 3 for sum g (g = dy is exact: the pre-sum only) and 6 for sum g xhat (u = x is exact,
    u - mean and the product with invstd round once each, the four fmas of the pre-sum four times)."""
    L, p = lib.load(), large()
    V = E.LARGE_V + extra
    x, dy = p["x"].payload[:V].view(1, V), p["dy"].payload[:V].view(1, V)
    mi = E.mean_invstd_of(x.double()).cpu()
    mi_d, ga, be = mi.to(DEV), p["gamma"].to(DEV), p["beta"].to(DEV)
    nblk = E.MAX_STAT_BLOCKS
    pg = gvec(nblk * 2, F64)
    _launch(lib, L.dpi_bn_bwd_reduce(dy.data_ptr(), x.data_ptr(), ptr(mi_d), ptr(ga), ptr(be), None, 1.0, 1.0, 1, V, ptr(pg), lib.stream()), "dpi_bn_bwd_reduce")
    _check_guards([("x", p["x"]), ("dy", p["dy"]), ("partials", pg)], "bn_bwd_reduce large")
    ref, mag = E.bn_bwd_partials64(dy, x, mi, p["gamma"], p["beta"], None, 1.0, 1.0)
    E.check_partials(pg.payload.view(-1, 1, 2), ref, mag, torch.tensor([3.0, 6.0], dtype=F64), "bn_bwd_reduce large", span_len=E.stat_span(V, nblk))
    if extra:
        return
    dxg, dgg, dbg = _aligned(guard(V, F32, DEV), V), gvec(1), gvec(1)
    _launch(lib, L.dpi_bn_bwd_apply(dy.data_ptr(), x.data_ptr(), ptr(mi_d), ptr(ga), ptr(be), None, 1.0, 1.0, ptr(pg), nblk, 1, V, ptr(dxg), ptr(dgg), ptr(dbg),
                                    lib.stream()), "dpi_bn_bwd_apply")
    _check_guards([("x", p["x"]), ("dy", p["dy"]), ("partials", pg), ("dx", dxg), ("dgamma", dgg), ("dbeta", dbg)], "bn_bwd_apply large")
    dx, dg, db = E.bn_bwd_apply64(dy, x, mi, p["gamma"], p["beta"], None, 1.0, 1.0, ref.sum(0))
    written(dxg.payload, "dx"), written(dgg.payload, "dgamma"), written(dbg.payload, "dbeta")
    assert rel_dev(dxg.payload, dx) < 2e-5
    assert rel(dgg.payload, dg) < 2e-4 and rel(dbg.payload, db) < 2e-4


def test_large_add_and_lrelu_bwd(lib):
    """Non-temporal path and grid-stride loop of the two flat kernels; one IEEE addition / one product per element: bit equality."""
    L, p = lib.load(), large()
    V = E.LARGE_V
    x, dy = p["x"].payload[:V], p["dy"].payload[:V]
    yg = _aligned(guard(V, F32, DEV), V)
    _launch(lib, L.dpi_add(x.data_ptr(), dy.data_ptr(), V, ptr(yg), lib.stream()), "dpi_add")
    _check_guards([("a", p["x"]), ("b", p["dy"]), ("y", yg)], "add large")
    assert torch.equal(yg.payload, x + dy)
    yg.payload.fill_(float("nan"))
    _launch(lib, L.dpi_lrelu_bwd(dy.data_ptr(), x.data_ptr(), S02, V, ptr(yg), lib.stream()), "dpi_lrelu_bwd")
    _check_guards([("x", p["x"]), ("dy", p["dy"]), ("dx", yg)], "lrelu_bwd large")
    assert torch.equal(yg.payload.view(torch.int32), E.lrelu_bwd_ref(dy, x, S02).view(torch.int32))


# ---- up-sampling -------------------------------------------------------------------------------------------------------------------------
UP_FWD = [(r, 1, 0) for r in E.UPSAMPLE_ROWS] + [(r, 0, 0) for r in E.UPSAMPLE_ROWS if r.nearest] + [(r, 1, 1) for r in E.UPSAMPLE_ROWS if r.bf16]


@pytest.mark.parametrize("row,linear,io", UP_FWD, ids=["%s-%s-%s" % (upid(r), "linear" if l else "nearest", IO_IDS[io]) for r, l, io in UP_FWD])
def test_upsample_forward(lib, row, linear, io):
    """y = up2(T(x)) cropped, against the oracle's up-sampling of the float64 chain: 1e-6 (linear, fp32), half a bf16 ulp (bf16), and for
    nearest mode — launched without a chain, so every output is a copy — bit equality.  A bf16 y is handed over 4-byte aligned (an even
    channel offset into the concat buffer): the packed-pair store of the cube kernel decides from the element offset alone."""
    L = lib.load()
    gen = torch.Generator().manual_seed(21)
    (D, H, W), (Do, Ho, Wo) = row.inp, row.out
    x = torch.randn((row.C,) + row.inp, generator=gen)
    x = x.to(BF).float() if io else x
    chain = E.chain_table(row.C, gen) if linear else None
    chain_d = None if chain is None else chain.to(DEV)
    xg = gin(x.reshape(row.C, -1), dt(io, 1))
    yg = gout(row.C, Do * Ho * Wo, dt(io, 1), c0=4 if io else None)
    assert yg.payload.data_ptr() % 4 == 0
    _launch(lib, L.dpi_upsample2x_fwd_io(ptr(xg), ptr(chain_d), row.C, D, H, W, Do, Ho, Wo, linear, ptr(yg), io, lib.stream()),
            "dpi_upsample2x_fwd_io")
    _check_guards([("x", xg), ("y", yg)], "upsample_fwd " + upid(row))
    ref = E.upsample_fwd64(x, chain, row.out, linear).reshape(row.C, -1)
    if linear:
        stored_ok(yg.payload, ref, "y", 1e-6)
    else:
        assert torch.equal(yg.payload.cpu().view(torch.int32), ref.float().view(torch.int32))


UP_BWD = ([(r, 1, v, 0) for r in E.UPSAMPLE_ROWS for v in ("ws", "gather", "dy+1")] + [(r, 0, "gather", 0) for r in E.UPSAMPLE_ROWS if r.nearest]
          + [(r, 1, v, 2) for r in E.UPSAMPLE_ROWS if r.bf16 for v in ("ws", "gather")])


@pytest.mark.parametrize("row,linear,variant,io", UP_BWD, ids=["%s-%s-%s-%s" % (upid(r), "linear" if l else "nearest", v, IO_IDS[io]) for r, l, v, io in UP_BWD])
def test_upsample_adjoint(lib, row, linear, variant, io):
    """dx = up2^T(dy) three ways: separable passes through a workspace of exactly the queried size (row-pair kernel for the W pass where
    Wo = 2 W, W even, Wo % 4 == 0 and dy, ws are 16-byte aligned), the gather kernel (ws = NULL), and the separable passes with dy moved by
    one float, which hands the W pass to the axis kernel.  Against float64 autograd through the oracle's up-sampling, 2e-6."""
    L = lib.load()
    gen = torch.Generator().manual_seed(22)
    (D, H, W), (Do, Ho, Wo) = row.inp, row.out
    dy = torch.randn((row.C,) + row.out, generator=gen)
    dy = dy.to(BF).float() if io else dy
    dyg = gin(dy.reshape(row.C, -1), dt(io, 2), offset=1 if variant == "dy+1" else 0)
    dxg = gout(row.C, D * H * W, dt(io, 2))
    n_ws = L.dpi_upsample2x_bwd_ws_floats(row.C, D, H, W, Do, Ho, Wo, linear)
    wg = gvec(n_ws) if variant != "gather" else None
    assert (n_ws > 0) == bool(linear)
    _launch(lib, L.dpi_upsample2x_bwd_io(ptr(dyg), row.C, D, H, W, Do, Ho, Wo, linear, ptr(dxg), ptr(wg), io, lib.stream()), "dpi_upsample2x_bwd_io")
    _check_guards([("dy", dyg), ("dx", dxg), ("ws", wg)], "upsample_bwd %s %s" % (upid(row), variant))
    stored_ok(dxg.payload, E.upsample_bwd64(dy, row.inp, linear).reshape(row.C, -1), "dx", 2e-6)


# ---- the small kernels -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("win", E.CROP_WINDOWS, ids=lambda w: "-".join(map(str, w)))
def test_crop_copy_and_its_adjoint(lib, win):
    L = lib.load()
    D, H, W = E.CROP_SHAPE
    od, oh, ow, Do, Ho, Wo = win
    gen = torch.Generator().manual_seed(5)
    x, dy = torch.randn((2, D, H, W), generator=gen), torch.randn((2, Do, Ho, Wo), generator=gen)
    xg, yg = gin(x.reshape(2, -1)), gout(2, Do * Ho * Wo)
    _launch(lib, L.dpi_crop_copy(ptr(xg), 2, D, H, W, od, oh, ow, Do, Ho, Wo, ptr(yg), lib.stream()), "dpi_crop_copy")
    _check_guards([("x", xg), ("y", yg)], "crop_copy")
    assert torch.equal(yg.payload.cpu().view(torch.int32), E.crop64(x, win).reshape(2, -1).view(torch.int32))
    dyg, dxg = gin(dy.reshape(2, -1)), gout(2, D * H * W)
    _launch(lib, L.dpi_crop_copy_bwd(ptr(dyg), 2, D, H, W, od, oh, ow, Do, Ho, Wo, ptr(dxg), lib.stream()), "dpi_crop_copy_bwd")
    _check_guards([("dy", dyg), ("dx", dxg)], "crop_copy_bwd")
    assert torch.equal(dxg.payload.cpu().view(torch.int32), E.crop_bwd64(dy, E.CROP_SHAPE, win).reshape(2, -1).view(torch.int32))


@pytest.mark.parametrize("K", E.FIR_K)
def test_fir_axis0(lib, K):
    """K fmas per output: the 5e-6 of an fp32 result of one expression; every T (K > T included) and S of the case table."""
    L = lib.load()
    gen = torch.Generator().manual_seed(K)
    taps = torch.randn(K, generator=gen)
    tg = gvec(K, fill=taps)
    for T in E.FIR_T:
        for S in E.FIR_S:
            x = torch.randn((2, T, S), generator=gen)
            xg, yg = gin(x.reshape(2, -1)), gout(2, T * S)
            _launch(lib, L.dpi_fir_axis0(ptr(xg), ptr(tg), K, 2, T, S, ptr(yg), lib.stream()), "dpi_fir_axis0")
            _check_guards([("x", xg), ("taps", tg), ("y", yg)], "fir K=%d T=%d S=%d" % (K, T, S))
            stored_ok(yg.payload, E.fir64(x, taps), "fir K=%d T=%d S=%d" % (K, T, S), 5e-6)


# max |y - float64| over the case set in units of the float32 spacing at the float64 value, measured on an MI355X (device expm1f / tanhf /
# expf): see test_activations
ACT_ULP = {E.ACT_ELU: 0.7668, E.ACT_TANH: 1.1544, E.ACT_SIGMOID: 1.9015}


@pytest.mark.parametrize("kind", [E.ACT_ELU, E.ACT_TANH, E.ACT_SIGMOID], ids=["elu", "tanh", "sigmoid"])
def test_activations(lib, kind):
    """dpi_act_fwd over n in ACT_N on inputs spanning [-100, 100], +-0 and values near 0: every element's error in units of the float32
    spacing at the float64 value (below the smallest normal: the subnormal spacing 2^-149), at most twice what was measured on the device
    and never above 4.  Measured on an MI355X: ELU 0.7668, tanh 1.1544, sigmoid 1.9015 (ACT_ULP).  Sigmoid measured 2.05e6 before
    act_fwd_one took e^x below x = -87: for x in (-103.3, -88.73) the value is a subnormal float and 1 / (1 + expf(-x)) = 1 / inf gave 0.
    dpi_act_bwd (plain arithmetic on y) at 5e-6 norm-wise."""
    L = lib.load()
    worst = 0.0
    for n in E.ACT_N:
        x = E.act_inputs(n, torch.Generator().manual_seed(n))
        xg, yg = _aligned(gin(x), n), _aligned(gvec(n), n)
        _launch(lib, L.dpi_act_fwd(ptr(xg), n, kind, ptr(yg), lib.stream()), "dpi_act_fwd")
        _check_guards([("x", xg), ("y", yg)], "act_fwd n=%d" % n)
        written(yg.payload, "y")
        worst = max(worst, E.ulp_error(yg.payload, E.act_fwd64(kind, x)))
        y = E.act_fwd64(kind, x).float()
        dy = torch.randn(n, generator=torch.Generator().manual_seed(n + 1))
        yin, dyg, dxg = gin(y), gin(dy), _aligned(gvec(n), n)
        _launch(lib, L.dpi_act_bwd(ptr(dyg), ptr(yin), n, kind, ptr(dxg), lib.stream()), "dpi_act_bwd")
        _check_guards([("y", yin), ("dy", dyg), ("dx", dxg)], "act_bwd n=%d" % n)
        stored_ok(dxg.payload, E.act_bwd64(kind, y, dy), "act_bwd dx", 5e-6)
    print("act_fwd kind %d: max error %.4f float32 spacings" % (kind, worst))
    assert worst <= 4.0, worst
    assert ACT_ULP[kind] is not None and worst <= 2 * ACT_ULP[kind], (worst, ACT_ULP[kind])


@pytest.mark.parametrize("n", E.ACT_N)
def test_add_axpy_lrelu_bwd(lib, n):
    L = lib.load()
    gen = torch.Generator().manual_seed(n)
    a, b = torch.randn(n, generator=gen), torch.randn(n, generator=gen)
    a[::3] = torch.tensor([0.0, -0.0])[torch.arange(a[::3].numel()) % 2]                    # zeros of both signs where lrelu_bwd decides
    ag, bg, yg = _aligned(gin(a), n), _aligned(gin(b), n), _aligned(gvec(n), n)
    _launch(lib, L.dpi_add(ptr(ag), ptr(bg), n, ptr(yg), lib.stream()), "dpi_add")
    _check_guards([("a", ag), ("b", bg), ("y", yg)], "add n=%d" % n)
    assert torch.equal(yg.payload.cpu().view(torch.int32), (a + b).view(torch.int32))
    dxg = _aligned(gvec(n), n)
    _launch(lib, L.dpi_lrelu_bwd(ptr(bg), ptr(ag), S02, n, ptr(dxg), lib.stream()), "dpi_lrelu_bwd")          # x = a holds zeros of both signs
    _check_guards([("x", ag), ("dy", bg), ("dx", dxg)], "lrelu_bwd n=%d" % n)
    assert torch.equal(dxg.payload.cpu().view(torch.int32), E.lrelu_bwd_ref(b, a, S02).view(torch.int32))
    acc = _aligned(gvec(n, fill=b), n)
    _launch(lib, L.dpi_axpy(-0.37, ptr(ag), n, ptr(acc), lib.stream()), "dpi_axpy")
    _check_guards([("x", ag), ("y", acc)], "axpy n=%d" % n)
    stored_ok(acc.payload, float(np.float32(-0.37)) * a.double() + b.double(), "axpy y", 5e-6)


# ---- rejected arguments ------------------------------------------------------------------------------------------------------------------
def _refusals(L, g):
    """(entry point's name in the message, call) for the arguments each entry point documents as refused; g: dict of device buffers."""
    x, y, d, q, st = g["x"], ptr(g["y"]), ptr(g["d"]), g["q"], g["stream"]
    return [
        ("channel_stats", lambda: L.dpi_channel_stats_io(x, None, 0, 16, d, 0, st)),
        ("channel_stats", lambda: L.dpi_channel_stats_io(x, None, 2, 0, d, 0, st)),
        ("channel_stats", lambda: L.dpi_channel_stats_io(None, None, 2, 16, d, 0, st)),
        ("channel_stats", lambda: L.dpi_channel_stats_io(x, None, 2, 16, d, 4, st)),
        ("bn_finalize", lambda: L.dpi_bn_finalize(g["p"], 0, 2, 16, None, None, 1e-5, 0.1, 1.0, 0, None, None, None, None, y, None, st)),
        ("bn_finalize", lambda: L.dpi_bn_finalize(g["p"], 1, 2, 0, None, None, 1e-5, 0.1, 1.0, 0, None, None, None, None, y, None, st)),
        ("bn_finalize", lambda: L.dpi_bn_finalize(g["p"], 1, 2, 16, None, None, 1e-5, 0.1, 0.2, 0, q, None, None, None, y, y, st)),
        ("bn_finalize", lambda: L.dpi_bn_finalize(g["p"], 1, 2, 16, None, None, 1e-5, 0.1, 1.0, 1, q, None, None, None, y, y, st)),
        ("chain_apply", lambda: L.dpi_chain_apply_io(x, None, 2, 0, y, 0, st)),
        ("chain_apply", lambda: L.dpi_chain_apply_io(x, None, 2, 16, y, 4, st)),
        ("bn_bwd_reduce", lambda: L.dpi_bn_bwd_reduce_io(x, x, None, None, None, None, 1.0, 1.0, 2, 16, d, 0, st)),
        ("bn_bwd_reduce", lambda: L.dpi_bn_bwd_reduce_io(x, x, q, None, None, q, 0.2, 1.0, 2, 16, d, 0, st)),
        ("bn_bwd_reduce", lambda: L.dpi_bn_bwd_reduce_io(x, x, q, None, None, None, 1.0, 1.0, 2, 16, d, 8, st)),
        ("bn_bwd_apply", lambda: L.dpi_bn_bwd_apply_io(x, x, q, None, None, None, 1.0, 1.0, g["p"], 0, 2, 16, y, None, None, 0, st)),
        ("bn_bwd_apply", lambda: L.dpi_bn_bwd_apply_io(x, x, q, None, None, q, 0.2, 1.0, g["p"], 1, 2, 16, y, None, None, 0, st)),
        ("bn_bwd_apply", lambda: L.dpi_bn_bwd_apply_io(x, x, q, None, None, None, 1.0, 1.0, g["p"], 1, 2, 16, y, None, None, 4, st)),
        ("chain_add_stats", lambda: L.dpi_chain_add_stats_io(x, None, None, None, 2, 16, 0.2, y, d, 0, st)),
        ("chain_add_stats", lambda: L.dpi_chain_add_stats_io(x, None, x, None, 2, 16, 0.2, y, d, 4, st)),
        ("chain_add_apply", lambda: L.dpi_chain_add_apply(x, None, x, None, None, 2, 0, y, 0, st)),
        ("chain_add_apply", lambda: L.dpi_chain_add_apply(x, None, x, None, None, 2, 16, y, 4, st)),
        ("lrelu_bwd", lambda: L.dpi_lrelu_bwd(x, x, 0.2, 0, y, st)),
        ("act_fwd", lambda: L.dpi_act_fwd(x, 32, 0, y, st)),
        ("act_fwd", lambda: L.dpi_act_fwd(x, 32, 4, y, st)),
        ("act_bwd", lambda: L.dpi_act_bwd(x, x, 32, 4, y, st)),
        ("act_bwd", lambda: L.dpi_act_bwd(x, x, 0, 1, y, st)),
        ("add", lambda: L.dpi_add(x, None, 32, y, st)),
        ("channel_sum", lambda: L.dpi_channel_sum(x, 2, 0, d, y, st)),
        ("upsample_fwd", lambda: L.dpi_upsample2x_fwd_io(x, None, 2, 1, 2, 2, 3, 4, 4, 1, y, 0, st)),          # Do = 3 > 2 D
        ("upsample_fwd", lambda: L.dpi_upsample2x_fwd_io(x, None, 2, 1, 2, 2, 1, 4, 5, 1, y, 0, st)),          # Wo = 5 > 2 W
        ("upsample_fwd", lambda: L.dpi_upsample2x_fwd_io(x, None, 2, 1, 2, 2, 1, 0, 4, 1, y, 0, st)),          # Ho = 0
        ("upsample_fwd", lambda: L.dpi_upsample2x_fwd_io(x, None, 2, 1, 2, 2, 1, 4, 4, 1, y, 4, st)),
        ("upsample_bwd", lambda: L.dpi_upsample2x_bwd_io(x, 2, 0, 2, 2, 1, 4, 4, 1, y, None, 0, st)),
        ("upsample_bwd", lambda: L.dpi_upsample2x_bwd_io(x, 2, 1, 2, 2, 1, 4, 4, 1, y, None, 4, st)),
        ("crop_copy", lambda: L.dpi_crop_copy(x, 2, 1, 4, 4, 0, 2, 0, 1, 3, 4, y, st)),                         # oh + Ho > H
        ("crop_copy", lambda: L.dpi_crop_copy(x, 2, 1, 4, 4, 0, 0, -1, 1, 4, 4, y, st)),
        ("crop_copy_bwd", lambda: L.dpi_crop_copy_bwd(x, 2, 1, 4, 4, 0, 0, 1, 1, 4, 4, y, st)),                 # ow + Wo > W
        ("fir_axis0", lambda: L.dpi_fir_axis0(x, q, 2, 2, 4, 4, y, st)),                                        # even tap count
        ("fir_axis0", lambda: L.dpi_fir_axis0(x, q, 3, 2, 0, 4, y, st)),
        ("axpy", lambda: L.dpi_axpy(1.0, x, 0, y, st)),
    ]


def test_rejected_arguments_launch_nothing(lib):
    """Every documented DPI_REQUIRE: DPI_E_ARG, a message that names the entry point, and the NaN outputs (a float tensor, a double partial
    buffer) bit for bit as they were, bands included."""
    L = lib.load()
    g = {"y": gout(2, 32), "d": gvec(8, F64), "stream": lib.stream()}
    xg, qg, pg = gin(torch.randn(2, 32)), gin(torch.rand(2, 5) + 0.5), gin(torch.rand(4), F64)
    g.update(x=ptr(xg), q=ptr(qg), p=ptr(pg))
    before = g["y"].bits(), g["d"].bits()
    for name, call in _refusals(L, g):
        rc = call()
        msg = L.dpi_last_error().decode()
        assert rc == -1, (name, rc, msg)                                 # DPI_E_ARG
        assert msg.startswith(name + ":"), (name, msg)
    _check_guards([("x", xg), ("q", qg), ("p", pg), ("y", g["y"]), ("d", g["d"])], "rejected arguments")
    assert g["y"].untouched(before[0]) and g["d"].untouched(before[1]), "a refused launch wrote an output"
