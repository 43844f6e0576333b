"""The float64 restatements of tests/elementwise_cases.py against independent torch float64 code (torch.nn.functional.batch_norm, interpolate,
elu, conv1d, pad, with autograd), the size facts every row is named for (straight from dpi_stat_blocks and the span formula: a row that
stops exercising its edge fails here), and — restatement against restatement — that the checks of the device test catch a wrong kernel.
No GPU: dpi_stat_blocks and the workspace queries are host functions of the library."""
import pytest
import torch
import torch.nn.functional as F

import elementwise_cases as E

F64 = torch.float64
SMALL_V = [r for r in E.V_ROWS if r.V <= 1287]


@pytest.fixture(scope="module")
def L():
    from deep_prior_interpolation_amd import _lib
    return _lib.load()


def close(a, b, tol=1e-12):
    assert E.rel(a, b) < tol, E.rel(a, b)


# ---- size facts --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", E.V_ROWS, ids=lambda r: "V%d" % r.V)
def test_v_rows_reach_the_blocks_and_tails_they_are_named_for(L, row):
    nblk = L.dpi_stat_blocks(3, row.V)
    assert nblk == row.nblk == E.stat_blocks(3, row.V)
    assert E.stat_span(row.V, nblk) == row.span and row.span % 4 == 0
    sp = E.spans(row.V, nblk)
    assert all(e > b for b, e in sp) and sp[0][0] == 0 and sp[-1][1] == row.V and all(sp[i][1] == sp[i + 1][0] for i in range(nblk - 1))
    assert sp[-1][1] - sp[-1][0] == row.last
    assert (row.V % 4 == 0) == row.vec
    assert 3 * row.V < E.NT_MIN_FLOATS and E.ew_blocks(-(-row.V // 4)) < E.EW_MAX_BLOCKS


def test_named_rows_have_the_sizes_they_are_named_for():
    by = {r.V: r for r in E.V_ROWS}
    assert [r.V for r in E.V_ROWS] == [1, 3, 4, 5, 1023, 1287, 16384, 16385, 16388, 32772, 49153]
    assert by[16384].nblk == 1 and by[16384].last == by[16384].span == 16384                          # exactly one block
    assert by[16385].nblk == 2 and by[16385].span == 8196 and not by[16385].vec and by[16385].last < 8196
    assert by[16388].nblk == 2 and by[16388].vec
    assert by[32772].nblk == 3 and by[49153].nblk == 4 and 49153 % 2 == 1
    assert 1023 % 4 == 3 and 1287 > 1024 and 1287 % 4 == 3                                              # a partial group in the loop's second trip
    assert [r.V for r in E.V_ROWS_BF16] == [1287, 16385, 16388]


def test_large_row_crosses_the_thresholds_it_exists_for(L):
    V = E.LARGE_V
    assert V == 33570820 and V % 4 == 0 and (V + 1) % 4 != 0
    for v in (V, V + 1):
        assert 1 * v >= E.NT_MIN_FLOATS                                                                 # non-temporal path
        assert L.dpi_stat_blocks(1, v) == E.MAX_STAT_BLOCKS == E.stat_blocks(1, v) and -(-v // E.STAT_SPAN) > E.MAX_STAT_BLOCKS
        span = E.stat_span(v, E.MAX_STAT_BLOCKS)
        assert span > E.STAT_SPAN and -(-span // 1024) == 17                                            # spans over 16384: 17 trips per thread
        sp = E.spans(v, E.MAX_STAT_BLOCKS)
        assert 0 < sp[-1][1] - sp[-1][0] < span and sp[-1][1] == v
    assert -(-(-(-V // 4)) // 256) > E.EW_MAX_BLOCKS                                                  # chain_apply, add, lrelu_bwd: grid-stride loop
    assert -(-(-(-V // 32)) // 256) > E.EW_MAX_BLOCKS                                                 # bn_bwd_apply (8 float4 per thread) too


def test_join_rows_have_two_blocks(L):
    for shape, vec in (((4, 17, 241), True), ((5, 29, 113), False)):
        V = shape[0] * shape[1] * shape[2]
        assert V == (16388 if vec else 16385) and L.dpi_stat_blocks(6, V) == 2
        assert L.dpi_join_bwd_ws_doubles(6, V) == 2 * 6 * 24


def test_partial_row_counts_sit_around_the_loop_bounds():
    assert set(E.FINALIZE_NBLK) >= {n + d for n in (64, 256, 512) for d in (-1, 0, 1)} | {1, 2, 768, 769, 2048, 8192}
    # the remainder statement of bn_finalize adds at least one row unless nblk is a multiple of 512
    for nblk in E.FINALIZE_NBLK:
        p = E.synthetic_partials(nblk, 1)
        dropped = not torch.equal(E.finalize_totals(p, "finalize_no_remainder"), E.finalize_totals(p))
        assert dropped == (nblk % 512 != 0), nblk
    assert set(E.APPLY_NBLK) == {1, 63, 64, 65, 2048}


@pytest.mark.parametrize("row", E.UPSAMPLE_ROWS, ids=lambda r: "%dx%dx%d-%dx%dx%d" % (r.inp + r.out))
def test_upsample_rows_reach_the_kernels_they_are_named_for(L, row):
    (D, H, W), (Do, Ho, Wo) = row.inp, row.out
    scale_d = not (D == 1 and Do == 1)
    assert 1 <= Do <= (2 * D if scale_d else 1) and 1 <= Ho <= 2 * H and 1 <= Wo <= 2 * W
    ws = L.dpi_upsample2x_bwd_ws_floats(row.C, D, H, W, Do, Ho, Wo, 1)
    assert ws == row.C * Do * Ho * W + (row.C * Do * H * W if scale_d else 0)
    assert L.dpi_upsample2x_bwd_ws_floats(row.C, D, H, W, Do, Ho, Wo, 0) == 0
    cube = H > 1 and W > 1 and (not scale_d or D > 1)
    row_pair = Wo == 2 * W and W % 2 == 0 and Wo % 4 == 0
    if "cube" in row.why:
        assert cube
    if "generic forward" in row.why:
        assert not cube
    if "crop along W only" in row.why:
        assert (Do, Ho, Wo) == (2 * D, 2 * H, 2 * W - 1)
    if "every axis cropped" in row.why:
        assert (Do, Ho, Wo) == (2 * D - 1, 2 * H - 1, 2 * W - 1)
    if "row-pair" in row.why:
        assert row_pair and W == 2
    if "odd Wo" in row.why:
        assert Wo % 2 == 1 and not scale_d
    if "slab of 260" in row.why:
        assert W >= 256 and H * W >= 256 and row_pair        # H pass: slab = H W; W pass: slab = W, in the axis kernel once dy is moved by one float
    if "gy halving" in row.why:
        assert row.C * Do * Ho > 16384 and row_pair                                                    # aligned dy: row-pair kernel; dy + 1: axis kernel, gy halved
    assert [r.nearest for r in E.UPSAMPLE_ROWS][:4] == [True, True, False, True]


# ---- chains, statistics, finalise against F.batch_norm -----------------------------------------------------------------------------------
@pytest.mark.parametrize("row", SMALL_V, ids=lambda r: "V%d" % r.V)
@pytest.mark.parametrize("form", ["plain", "act_first", "in_chain"])
def test_statistics_and_finalise_against_torch_batch_norm(row, form):
    C, V = 3, row.V
    gen = torch.Generator().manual_seed(V)
    x = E.channel_data(C, V, gen)
    chain = E.chain_table(C, gen)
    gamma, beta = torch.rand(C, generator=gen) + 0.5, torch.randn(C, generator=gen) * 0.3
    rm, rv = torch.randn(C, generator=gen).double(), torch.rand(C, generator=gen).double() + 0.5
    slope = 0.2
    # the tensor the BatchNorm normalises, and the chain that hands the partials' kernel that tensor
    if form == "plain":
        stat_chain, u = None, x.double()
    elif form == "act_first":
        stat_chain = torch.tensor([[1.0, 0.0, slope, 1.0, 0.0]] * C, dtype=F64)
        u = F.leaky_relu(x.double(), slope)
    else:
        stat_chain = chain
        ch = chain.double()
        v = ch[:, 0:1] * x.double() + ch[:, 1:2]
        u = ch[:, 3:4] * torch.maximum(v, torch.zeros_like(v)) + ch[:, 3:4] * ch[:, 2:3] * torch.minimum(v, torch.zeros_like(v)) + ch[:, 4:5]
    y = E.chain64(x, stat_chain)
    close(y, u)
    part = E.partials64(y)
    assert part.shape == (row.nblk, C, 2)
    close(part.sum(0)[:, 0], u.sum(1)), close(part.sum(0)[:, 1], (u * u).sum(1))
    out = E.finalize64(part, V, gamma, beta, slope=1.0 if form == "in_chain" else slope, act_first=int(form == "act_first"),
                       in_chain=chain if form == "in_chain" else None, running_mean=rm, running_var=rv, nbt=4)
    assert out["nbt"] == 5
    if V == 1:                                        # torch refuses one value per channel: mean = x, biased = unbiased variance = 0
        close(out["mean_invstd"][0], u[:, 0]), close(out["mean_invstd"][1], torch.full((C,), E.EPS ** -0.5, dtype=F64), 1e-9)
        close(out["running_var"], 0.9 * rv)
        return
    rm_t, rv_t = rm.clone(), rv.clone()
    bn = F.batch_norm(u[None], rm_t, rv_t, gamma.double(), beta.double(), True, E.MOMENTUM, E.EPS)[0]
    close(out["running_mean"], rm_t, 1e-10), close(out["running_var"], rv_t, 1e-9)
    close(out["mean_invstd"][0], u.mean(1), 1e-10), close(out["mean_invstd"][1], 1 / torch.sqrt(u.var(1, unbiased=False) + E.EPS), 1e-9)
    want = bn if form != "plain" else F.leaky_relu(bn, slope)
    close(E.chain64(x, out["chain_out"]), want, 1e-9)


@pytest.mark.parametrize("row", SMALL_V[1:], ids=lambda r: "V%d" % r.V)
@pytest.mark.parametrize("form", ["plain", "pre", "post", "in_chain"])
def test_batchnorm_backward_against_torch_autograd(row, form):
    C, V = 3, row.V
    gen = torch.Generator().manual_seed(100 + V)
    x, dy = E.channel_data(C, V, gen), torch.randn((C, V), generator=gen)
    gamma, beta = torch.rand(C, generator=gen) + 0.5, torch.randn(C, generator=gen) * 0.3
    pre, post = (0.2 if form == "pre" else 1.0), (0.2 if form == "post" else 1.0)
    chain = E.chain_table(C, gen) if form == "in_chain" else None
    # torch: BatchNorm in training mode on u, gradient with respect to u (in_chain) or x
    leaf = (E.chain64(x, chain) if chain is not None else x.double()).detach().requires_grad_()
    u = leaf if chain is not None else F.leaky_relu(leaf, pre)
    g64, b64 = gamma.double().requires_grad_(), beta.double().requires_grad_()
    y = F.leaky_relu(F.batch_norm(u[None], None, None, g64, b64, True, 0.0, E.EPS)[0], post)
    (y * dy.double()).sum().backward()
    dx, dg, db = E.bn_bwd_autograd64(dy, x, gamma, beta, chain, pre, post)
    close(dx, leaf.grad, 1e-10), close(dg, g64.grad, 1e-10), close(db, b64.grad, 1e-10)
    # the two-phase form of the header with the float32 statistics the kernels are handed
    mi = E.mean_invstd_of(u.detach())
    part, mag = E.bn_bwd_partials64(dy, x, mi, gamma, beta, chain, pre, post)
    assert part.shape == (row.nblk, C, 2) and bool((mag >= part.abs() * (1 - 1e-12)).all())
    dx2, dg2, db2 = E.bn_bwd_apply64(dy, x, mi, gamma, beta, chain, pre, post, part.sum(0))
    close(dx2, leaf.grad, 2e-6), close(dg2, g64.grad, 2e-6), close(db2, b64.grad, 2e-6)


def test_edge_mask_names_the_elements_at_the_jump_of_the_post_activation():
    """post_edge64: exactly the elements whose BatchNorm output is (relatively) within the margin of 0; with dy = 0 there, the mask of
    act_post no longer matters — the gradient is the same whichever side they take."""
    gen = torch.Generator().manual_seed(9)
    x, dy = E.channel_data(3, 1287, gen), torch.randn((3, 1287), generator=gen)
    gamma, beta = torch.rand(3, generator=gen) + 0.5, torch.randn(3, generator=gen) * 0.3
    mi = E.mean_invstd_of(x.double())
    a = (gamma * mi[1]).double()[:, None]
    pb = (beta - mi[0] * gamma * mi[1]).double()[:, None]
    x[:, 5] = (-pb / a)[:, 0].float()                                     # BatchNorm output ~ 0 (to float32 rounding) in every channel
    edge = E.post_edge64(x, mi, gamma, beta, None, 1.0)
    assert bool(edge[:, 5].all()) and int(edge.sum()) <= 5
    dy0 = torch.where(edge, torch.zeros(()), dy)
    for flip in (1.0, -1.0):                                              # push the edge elements to either side
        xs = x.clone()
        xs[:, 5] += flip * 1e-4
        _, _, g, _ = E.bn_bwd_terms64(dy0, xs, mi, gamma, beta, None, 1.0, 0.2)
        assert bool((g[:, 5] == 0).all())


def test_join_sum_is_the_sum_of_the_two_chains():
    gen = torch.Generator().manual_seed(5)
    a, b = E.channel_data(3, 37, gen), E.channel_data(3, 37, gen)
    cha = E.chain_table(3, gen)
    ch = cha.double()
    v = ch[:, 0:1] * a.double() + ch[:, 1:2]
    want = ch[:, 3:4] * (torch.relu(v) - ch[:, 2:3] * torch.relu(-v)) + ch[:, 4:5] + b.double()
    close(E.chain_add64(a, cha, b, None), want)
    assert bool((E.chain_mag64(a, cha) >= E.chain64(a, cha).abs() * (1 - 1e-12)).all())


# ---- up-sampling, crop, FIR, activations -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("linear", [1, 0])
@pytest.mark.parametrize("row", E.UPSAMPLE_ROWS, ids=lambda r: "%dx%dx%d-%dx%dx%d" % (r.inp + r.out))
def test_upsampling_and_its_adjoint_against_interpolate(row, linear):
    gen = torch.Generator().manual_seed(3)
    (D, H, W), (Do, Ho, Wo) = row.inp, row.out
    x = torch.randn((row.C,) + row.inp, generator=gen, dtype=F64).requires_grad_()
    if D == 1 and Do == 1:
        full = F.interpolate(x[None, :, 0], scale_factor=2, mode="bilinear" if linear else "nearest", **({"align_corners": False} if linear else {}))[0][:, None]
    else:
        full = F.interpolate(x[None], scale_factor=2, mode="trilinear" if linear else "nearest", **({"align_corners": False} if linear else {}))[0]
    want = full[:, :Do, :Ho, :Wo]
    close(E.upsample_fwd64(x.detach(), None, row.out, linear), want)
    dy = torch.randn(want.shape, generator=gen, dtype=F64)
    (want * dy).sum().backward()
    close(E.upsample_bwd64(dy, row.inp, linear), x.grad)
    chain = E.chain_table(row.C, gen)
    close(E.upsample_fwd64(x.detach(), chain, row.out, linear), E.upsample_fwd64(E.chain64(x.detach(), chain), None, row.out, linear))


@pytest.mark.parametrize("win", E.CROP_WINDOWS, ids=lambda w: "-".join(map(str, w)))
def test_crop_against_slicing_and_padding(win):
    D, H, W = E.CROP_SHAPE
    od, oh, ow, Do, Ho, Wo = win
    assert od + Do <= D and oh + Ho <= H and ow + Wo <= W
    x = torch.randn((2, D, H, W), generator=torch.Generator().manual_seed(1))
    y = E.crop64(x, win)
    assert torch.equal(y, x.narrow(1, od, Do).narrow(2, oh, Ho).narrow(3, ow, Wo))
    assert torch.equal(E.crop_bwd64(y, E.CROP_SHAPE, win), F.pad(y, (ow, W - ow - Wo, oh, H - oh - Ho, od, D - od - Do)))


def test_crop_windows_touch_every_face_and_the_interior():
    D, H, W = E.CROP_SHAPE
    faces = set()
    for od, oh, ow, Do, Ho, Wo in E.CROP_WINDOWS:
        touch = (od == 0, od + Do == D, oh == 0, oh + Ho == H, ow == 0, ow + Wo == W)
        faces |= {i for i, t in enumerate(touch) if t and sum(touch) == 1}
        faces |= {"interior"} if not any(touch) and Do * Ho * Wo > 1 else set()
        faces |= {"full"} if all(touch) else set()
        faces |= {"voxel"} if Do * Ho * Wo == 1 else set()
    assert faces == {0, 1, 2, 3, 4, 5, "interior", "full", "voxel"}


@pytest.mark.parametrize("K", E.FIR_K)
def test_fir_against_conv1d(K):
    gen = torch.Generator().manual_seed(K)
    taps = torch.randn(K, generator=gen)
    assert any(K > T for T in E.FIR_T) or K == 1
    for T in E.FIR_T:
        for S in E.FIR_S:
            x = torch.randn((2, T, S), generator=gen)
            want = F.conv1d(x.double().permute(0, 2, 1).reshape(2 * S, 1, T), taps.double().flip(0).reshape(1, 1, K), padding=K // 2)
            close(E.fir64(x, taps), want.reshape(2, S, T).permute(0, 2, 1))


@pytest.mark.parametrize("kind,fn", [(E.ACT_ELU, F.elu), (E.ACT_TANH, torch.tanh), (E.ACT_SIGMOID, torch.sigmoid)])
def test_activations_and_their_output_based_derivatives(kind, fn):
    for n in E.ACT_N:
        x = E.act_inputs(n, torch.Generator().manual_seed(n)).double().requires_grad_()
        assert x.numel() == n
        y = fn(x)
        close(E.act_fwd64(kind, x.detach()), y, 1e-14)
        dy = torch.randn(n, generator=torch.Generator().manual_seed(n + 1), dtype=F64)
        (y * dy).sum().backward()
        close(E.act_bwd64(kind, y.detach(), dy), x.grad, 1e-12)
    big = E.act_inputs(4096, torch.Generator().manual_seed(4096))
    assert float(big.min()) == -100.0 and float(big.max()) == 100.0 and bool((big == 0).any()) and bool((big.abs() < 1e-3).sum() > 100)
    assert E.ulp_error(torch.tensor([1.0 + 2.0 ** -23]), torch.tensor([1.0], dtype=F64)) == 1.0


# ---- a wrong kernel is caught: the device test's checks on mutated restatements ------------------------------------------------------------
def _stats_case(V):
    gen = torch.Generator().manual_seed(V)
    x, chain = E.channel_data(3, V, gen), E.chain_table(3, gen)
    y = E.chain64(x, chain)
    return y, E.partials64(y), torch.stack([E.span_sums(E.chain_mag64(x, chain)), E.span_sums(E.chain_mag64(x, chain) ** 2)], 2)


def _fails(fn):
    try:
        fn()
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize("row", [r for r in E.V_ROWS if r.V <= 16388], ids=lambda r: "V%d" % r.V)
def test_mutated_spans_and_tails_fail_the_partial_row_check(row):
    y, ref, mag = _stats_case(row.V)
    E.check_partials(ref.clone(), ref, mag, 6, "unmutated")                                           # the check itself passes
    E.check_partials(E.partials64(y.float().double()), ref, mag, 6, "fp32-rounded terms")            # ... and has room for an fp32 evaluation
    moved = E.partials64(y, mutation="span_start+4")
    assert _fails(lambda: E.check_partials(moved, ref, mag, 6, "span start + 4")) == (row.nblk > 1)
    if row.nblk > 1:                                # the totals alone would also differ here, but a shifted boundary cancels in them:
        shifted = ref.clone()
        four = y[:, row.span:row.span + 4]
        shifted[0] += torch.stack([four.sum(1), (four ** 2).sum(1)], 1)
        shifted[1] -= torch.stack([four.sum(1), (four ** 2).sum(1)], 1)
        close(shifted.sum(0), ref.sum(0), 1e-12)
        assert _fails(lambda: E.check_partials(shifted, ref, mag, 6, "boundary moved by 4"))
    beyond = torch.cat([y[1:, 0], y.new_zeros(1)])
    tail = E.partials64(y, mutation="tail<=", beyond=beyond)
    assert _fails(lambda: E.check_partials(tail, ref, mag, 6, "tail <=")) == (not row.vec)


@pytest.mark.parametrize("nblk", E.FINALIZE_NBLK)
def test_a_dropped_remainder_row_fails_the_finalise_check(nblk):
    p = E.synthetic_partials(nblk, 5)
    gamma, beta = torch.linspace(0.5, 1.5, 5), torch.linspace(-0.3, 0.3, 5)
    ref = E.finalize64(p, 4096, gamma, beta, slope=0.2)
    bad = E.finalize64(p, 4096, gamma, beta, slope=0.2, mutation="finalize_no_remainder")
    assert E.rel(ref["mean_invstd"].float(), ref["mean_invstd"]) < 5e-6
    assert (E.rel(bad["mean_invstd"], ref["mean_invstd"]) >= 5e-6) == (nblk % 512 != 0)
    # every single row matters: dropping or doubling any one moves mean / invstd by far more than the bar
    for b in sorted({0, nblk // 2, nblk - 1}):
        for f in (0.0, 2.0):
            q = p.clone()
            q[b] *= f
            assert E.rel(E.finalize64(q, 4096, gamma, beta)["mean_invstd"], ref["mean_invstd"]) > 1e-3, (nblk, b, f)


@pytest.mark.parametrize("row", E.UPSAMPLE_ROWS[:9], ids=lambda r: "%dx%dx%d-%dx%dx%d" % (r.inp + r.out))
def test_a_missing_w_crop_predicate_fails_the_forward_check(row):
    gen = torch.Generator().manual_seed(3)
    x = torch.randn((row.C,) + row.inp, generator=gen)
    ref = E.upsample_fwd64(x, None, row.out, 1)
    got, behind = E.upsample_fwd64(x, None, row.out, 1, mutation="no_w_crop")
    caught = E.rel(got, ref) >= 1e-6 or behind is not None
    assert caught == (row.out[2] < 2 * row.inp[2])
    assert E.rel(ref.float(), ref) < 1e-6


@pytest.mark.parametrize("K", E.FIR_K)
def test_a_fir_centred_one_tap_early_fails_the_check(K):
    gen = torch.Generator().manual_seed(K)
    taps = torch.randn(K, generator=gen)
    for T in E.FIR_T:
        for S in E.FIR_S:
            x = torch.randn((2, T, S), generator=gen)
            ref = E.fir64(x, taps)
            assert E.rel(ref.float(), ref) < 5e-6 <= E.rel(E.fir64(x, taps, mutation="fir_centre-1"), ref), (K, T, S)
