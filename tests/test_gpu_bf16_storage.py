"""bf16 STORAGE of activations (BASELINE configs[4]: "bf16 activations + fp32 Adam master weights"; ABI 400: dpi_conv_desc.io, the *_io
entry points).  The reference is fp32-only (main.py:112 `.type(dtype)`), so the oracle statement is: a kernel given bf16 tensors computes,
in fp32, what the fp64 oracle computes on the WIDENED bf16 values, and what it stores is that result rounded to nearest-even.

 (1) every convolution family (forward, backward-data, backward-weight; fp32-MFMA, bf16-MFMA, 1x1x1, stride 2, VALU fall-backs) on operands
     that are bf16-representable — products are then exact in every arithmetic mode, so a stored element may differ from the fp64 oracle by
     half a bf16 ulp (+ the fp32 accumulation error), and weight gradients (fp32 outputs) keep the fp32 kernels' own 5e-6;
 (2) every elementwise kernel bit-for-bit against round_bf16(fp32 entry point on the widened tensors) — the fp32 entry points are the ones
     tests/test_gpu_ops.py holds against the reference's golden vectors and the oracle;
 (3) the fused nodes and the whole loop: storage mode against fp32 storage on the same seed, and a field-scale patch.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import dpi_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16


@pytest.fixture(scope="module")
def ops():
    from deep_prior_interpolation_amd import ops as _ops
    return _ops


@pytest.fixture(autouse=True)
def _modes_restored(ops):
    yield
    ops.set_precision("fp32")
    ops.set_storage("fp32")


def bf16_values(shape, gen, scale=1.0):
    """fp32 tensor whose values are exactly bf16-representable."""
    return (torch.randn(shape, generator=gen) * scale).to(BF).float()


def half_ulp_ok(got, ref64, what, slack=0.503):
    """|got - ref| <= half a bf16 ulp of ref (+ a little for the fp32 accumulation error moving a value across a rounding boundary)."""
    got = got.detach().float().cpu().double()
    ref = ref64.detach().cpu().double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    # ulp of a bf16 value v: 2^(floor(log2|v|) - 7); a tiny absolute term covers results that cancel to ~0 (their fp32 error is absolute)
    bound = slack * 2.0 ** (torch.floor(torch.log2(ref.abs().clamp_min(1e-30))) - 7) + 2e-6 * ref.abs().max()
    bad = (got - ref).abs() > bound
    assert not bad.any(), "%s: %d of %d elements off by more than half a bf16 ulp (worst %.3g vs bound %.3g)" % (
        what, int(bad.sum()), bad.numel(), float(((got - ref).abs() / bound).max()), 1.0)


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-300))


# ---------------------------------------------------------------------------------------------------------------------------------------
# (1) convolutions
# cin, cout, shape, k, stride — each row names the kernel the shape reaches with bf16 tensors
CONV_IO = [
    (8, 13, (64, 64, 64), 3, 1),      # >= 512 big tiles: conv_bf16_kernel<3,4,2> in bf16 mode, conv_mfma IOB variants in fp32 mode; bf16 bww
    (25, 16, (32, 64, 64), 3, 1),     # 4m + 1 channels (tap-packed tail variants)
    (64, 4, (64, 64, 64), 3, 1),      # few output channels: no 4x4x1 / fewco kernel with bf16 tensors -> bf16 kernel / VALU kernel
    (4, 8, (64, 64, 64), 3, 1),
    (25, 1, (32, 32, 64), 3, 1),      # the output layer's shape (y fp32 in the net; here bf16 as well)
    (35, 53, (8, 16, 16), 3, 1),      # coarse level: small-tile conv_mfma, input-channel split off / on below
    (212, 71, (4, 8, 8), 3, 1),       # input-channel split (workspace) + splitk_reduce_kernel storing bf16
    (25, 25, (16, 32, 32), 3, 2),     # stride 2: conv_mfma<..,S=2>, conv_bwd_data_s2_mfma; backward-weight: conv_bf16_bww_s2_kernel<2> in bf16 mode (W % 16 == 0)
    (40, 13, (7, 9, 48), 3, 2),       # ... odd depth / height (rows past the end of x), one output tile, three 16-channel input tiles, ragged last octet chunk
    (1, 20, (4, 6, 16), 3, 2),        # stride-2 bf16 kernels (forward / backward-data / backward-weight): one input channel, W = 16 (a single 16-column output tile, 8 octets per row)
    (33, 7, (5, 8, 64), 3, 2),        # ... 33 = 4 groups + 1 channel, 7 output channels (one ragged 16-row tile), W = 64
    (16, 64, (2, 2, 32), 3, 2),       # ... four output tiles per workgroup (forward MT = 4), D = H = 2 (one output slice / row)
    (70, 70, (3, 5, 24), 3, 2),       # ... W = 24: forward and backward-data (W % 8 == 0) on the bf16 MFMA, backward-weight (needs W % 16 == 0) on the fp32 kernel
    (51, 51, (9, 11, 13), 3, 2),      # stride 2, odd sizes
    (3, 5, (6, 6, 6), 3, 2),          # VALU stride-2 kernels (few channels)
    (64, 25, (16, 16, 32), 1, 1),     # 1x1x1 MFMA forward / backward-data / backward-weight
    (137, 51, (5, 7, 9), 1, 1),       # 1x1x1, V not a multiple of 4 (scalar paths)
    (6, 3, (5, 7, 9), 1, 1),          # 1x1x1 VALU kernels
    (13, 9, (7, 9, 11), 3, 1),        # odd row lengths: element-wise staging everywhere, dY rows not 8-byte aligned
    (7, 3, (9, 10, 12), 3, 1),        # VALU forward / backward-weight
    (13, 4, (32, 32, 40), 3, 1),      # few-output-channel backward-weight kernels (swapped MFMA orientation / smallco)
    (16, 25, (16, 16, 34), 3, 1),     # W % 4 != 0: the bf16 kernel's 4-element staging pieces do not apply -> conv_mfma IOB in every mode
    (40, 40, (4, 16, 32), 3, 1),      # row-band tiles, two 16-channel output tiles per workgroup (conv_bf16_kernel<..., MT = 2>), third tile ragged
    (105, 64, (16, 16, 32), 3, 1),    # row-band tiles, one output tile per workgroup (plenty of workgroups), 13 channel groups + ragged last
]


def _conv_case(ops, cin, cout, shape, k, stride, seed):
    gen = torch.Generator().manual_seed(seed)
    x = bf16_values((1, cin) + shape, gen)
    w = bf16_values((cout, cin, k, k, k), gen, 1.0 / np.sqrt(cin * k ** 3))
    b = bf16_values((cout,), gen)
    xr, wr, br = (t.double().requires_grad_(True) for t in (x, w, b))
    yr = O.conv_nd(xr, wr, br, stride)
    dy = bf16_values(tuple(yr.shape), gen)
    yr.backward(dy.double())
    return x, w, b, dy, yr.detach(), xr.grad, wr.grad


@pytest.mark.parametrize("prec", ["fp32", "bf16mm"])
@pytest.mark.parametrize("cin,cout,shape,k,stride", CONV_IO)
def test_conv_kernels_with_bf16_tensors_vs_oracle(ops, cin, cout, shape, k, stride, prec):
    """forward x(bf16) -> y(bf16) with BatchNorm partials of the STORED y, backward-data dy(bf16) -> dx(bf16), backward-data with
    accumulate (read-modify-write of a bf16 dx), backward-weight (x bf16, dy bf16) -> dw fp32."""
    ops.set_precision(prec)
    L = ops._lib.load()
    x, w, b, dy, yr, dxr, dwr = _conv_case(ops, cin, cout, shape, k, stride, cin * 131 + cout)
    xg, wg, bg, dyg = x.to(DEV).to(BF), w.to(DEV), b.to(DEV), dy.to(DEV).to(BF)
    d = ops.make_desc(xg, wg, stride, BF)
    assert d.io == 15
    y = torch.empty(yr.shape, dtype=BF, device=DEV)
    nblk = L.dpi_conv_fwd_stat_blocks(C.byref(d))
    part = torch.zeros(nblk * cout * 2, dtype=torch.float64, device=DEV)
    ops.raw_conv_fwd(d, xg, None, wg, bg, y, part)
    half_ulp_ok(y, yr, "y")
    # the partials are {sum, sum^2} of what was stored
    p = part.view(nblk, cout, 2).sum(0).cpu()
    ys = y.float().double().cpu().reshape(cout, -1)
    np.testing.assert_allclose(p[:, 0].numpy(), ys.sum(1).numpy(), rtol=1e-9, atol=1e-7 * float(ys.abs().sum(1).max()))
    np.testing.assert_allclose(p[:, 1].numpy(), (ys * ys).sum(1).numpy(), rtol=1e-9)
    # backward-data, plain and accumulating into a bf16 destination
    dx = torch.empty(x.shape, dtype=BF, device=DEV)
    ops.raw_conv_bwd_data(d, dyg, wg, dx)
    half_ulp_ok(dx, dxr, "dx")
    base = bf16_values(tuple(x.shape), torch.Generator().manual_seed(5))
    dx2 = base.to(DEV).to(BF)
    ops.raw_conv_bwd_data(d, dyg, wg, dx2, accumulate=True)
    half_ulp_ok(dx2, dxr + base.double(), "dx (accumulate)")
    # backward-weight: fp32 output, exact products -> the fp32 kernels' own tolerance
    dw = torch.empty_like(wg)
    ops.raw_conv_bwd_weight(d, xg, None, dyg, dw)
    assert rel(dw, dwr) < 5e-6, rel(dw, dwr)


@pytest.mark.parametrize("store", ["bf16", "fp32"])
def test_packed_weights_follow_in_place_updates(ops, store):
    """conv_bf16_kernel reads the weights from a per-layer packed copy that every launch rewrites (conv_bf16_pack_kernel): an optimiser
    step that changes the weight tensor IN PLACE (same pointer, same slot) must show in the next launch, in both directions, eagerly
    and when the launches are replayed from a captured graph."""
    ops.set_precision("bf16mm")
    adt = BF if store == "bf16" else torch.float32
    x, w, b, dy, yr, dxr, _ = _conv_case(ops, 25, 16, (16, 32, 32), 3, 1, 77)
    xg, wg, bg, dyg = x.to(DEV).to(adt), w.to(DEV).clone(), b.to(DEV), dy.to(DEV).to(adt)
    d = ops.make_desc(xg, wg, 1, adt)
    y, dx = torch.empty(yr.shape, dtype=adt, device=DEV), torch.empty(x.shape, dtype=adt, device=DEV)

    def run():
        ops.raw_conv_fwd(d, xg, None, wg, bg, y)
        ops.raw_conv_bwd_data(d, dyg, wg, dx)

    def check(wnow, what):
        xr, wr = x.double(), wnow.double().cpu()
        yref, dxref = O.conv_nd(xr, wr, b.double(), 1), torch.nn.grad.conv3d_input(x.shape, wr, dy.double(), padding=1)
        if store == "bf16":
            half_ulp_ok(y, yref, "y " + what)
            half_ulp_ok(dx, dxref, "dx " + what)
        else:                                        # fp32 tensors: the bf16 products are exact, fp32 accumulation
            assert rel(y, yref) < 1e-5 and rel(dx, dxref) < 1e-5, (what, rel(y, yref), rel(dx, dxref))

    run()
    check(wg, "first launch")
    wg.mul_(-0.5).add_(bf16_values(tuple(wg.shape), torch.Generator().manual_seed(3), 0.02).to(DEV))     # in place: same pointer
    wg.copy_(wg.to(BF).float())                                                                           # keep the products exact
    run()
    check(wg, "after an in-place update")
    g = torch.cuda.CUDAGraph()
    s_ = torch.cuda.Stream()
    with torch.cuda.stream(s_):
        with torch.cuda.graph(g, stream=s_):
            run()
    wg.copy_((wg * 1.5 + 0.01).to(BF).float())
    y.zero_(); dx.zero_()
    g.replay()
    torch.cuda.synchronize()
    check(wg, "graph replay after another update")


@pytest.mark.parametrize("cin,cout,shape", [(64, 25, (16, 16, 32)), (67, 25, (8, 16, 24)), (137, 51, (4, 8, 16)), (7, 3, (2, 4, 8))])
def test_pointwise_backward_weight_on_the_bf16_mfma(ops, cin, cout, shape):
    """conv_pw_bwd_weight_bf16_kernel (1x1x1, x and dy bf16, bf16 arithmetic, V % 8 == 0): operands go from memory straight into the bf16
    MFMA.  Without a chain the products are exact (the fp32 kernels' tolerance); with the producer's chain T(x) is rounded to bf16 as
    an operand (2^-9 relative per element, uncorrelated), and the result must agree with the oracle fed that rounded T(x) tightly."""
    ops.set_precision("bf16mm")
    gen = torch.Generator().manual_seed(cin + cout)
    x = bf16_values((1, cin) + shape, gen)
    w = bf16_values((cout, cin, 1, 1, 1), gen, 0.1)
    dy = bf16_values((1, cout) + shape, gen)
    xg, dyg, wg = x.to(DEV).to(BF), dy.to(DEV).to(BF), w.to(DEV)
    d = ops.make_desc(xg, wg, 1, BF)
    assert d.io == 15 and d.precision == 1
    dw = torch.empty_like(wg)
    ops.raw_conv_bwd_weight(d, xg, None, dyg, dw)
    ref = torch.einsum("ov,iv->oi", dy.double().reshape(cout, -1), x.double().reshape(cin, -1)).reshape(wg.shape)
    assert rel(dw, ref) < 5e-6, rel(dw, ref)
    chain = torch.stack([torch.rand(cin, generator=gen) + 0.5, torch.randn(cin, generator=gen) * 0.3, torch.full((cin,), 0.2),
                         torch.rand(cin, generator=gen) + 0.5, torch.randn(cin, generator=gen) * 0.1], 1).contiguous()
    ps, pb, sl, qs, qb = (chain[:, i].view(1, cin, 1, 1, 1) for i in range(5))
    v = ps * x + pb                                       # fp32, the kernel's own arithmetic (apply_chain: no contraction)
    tx = qs * torch.where(v > 0, v, v * sl) + qb
    ops.raw_conv_bwd_weight(d, xg, chain.to(DEV), dyg, dw)
    ref_r = torch.einsum("ov,iv->oi", dy.double().reshape(cout, -1), tx.to(BF).double().reshape(cin, -1)).reshape(wg.shape)
    ref_x = torch.einsum("ov,iv->oi", dy.double().reshape(cout, -1), tx.double().reshape(cin, -1)).reshape(wg.shape)
    assert rel(dw, ref_x) < 4e-3, rel(dw, ref_x)
    # the MFMA kernel rounds T(x) (a few values may round the other way: fp32 association of the chain); the VALU kernel that serves the
    # few-channel layer keeps T(x) in fp32
    assert rel(dw, ref_r) < 2e-4 or rel(dw, ref_x) < 5e-6, (rel(dw, ref_r), rel(dw, ref_x))


def test_pack_scratch_release_and_regrow(ops):
    """ABI 401: dpi_pack_release() hands the packed-weight scratch back; the next launch allocates a fresh slot and is still right."""
    ops.set_precision("bf16mm")
    L = ops._lib.load()
    x, w, b, dy, yr, dxr, _ = _conv_case(ops, 16, 16, (8, 16, 32), 3, 1, 5)
    xg, wg, bg = x.to(DEV).to(BF), w.to(DEV), b.to(DEV)
    d = ops.make_desc(xg, wg, 1, BF)
    y = torch.empty(yr.shape, dtype=BF, device=DEV)
    ops.raw_conv_fwd(d, xg, None, wg, bg, y)
    held = L.dpi_pack_scratch_bytes()
    assert held >= (64 << 20) and held % (64 << 20) == 0
    assert L.dpi_pack_release() == 0 and L.dpi_pack_scratch_bytes() == 0
    y.zero_()
    ops.raw_conv_fwd(d, xg, None, wg, bg, y)
    assert L.dpi_pack_scratch_bytes() == (64 << 20)
    half_ulp_ok(y, yr, "y after dpi_pack_release")


@pytest.mark.parametrize("xbf,ybf", [(True, False), (False, True)])
@pytest.mark.parametrize("cin,cout,shape,k,stride", [(25, 1, (32, 32, 64), 3, 1), (8, 13, (64, 64, 64), 3, 1), (35, 53, (8, 16, 16), 3, 1),
                                                     (25, 25, (16, 32, 32), 3, 2), (64, 25, (16, 16, 32), 1, 1), (7, 3, (9, 10, 12), 3, 1)])
def test_conv_mixed_storage_types(ops, cin, cout, shape, k, stride, xbf, ybf):
    """One side bf16, the other fp32: the network's first layers (fp32 z when the perturbation is off, bf16 outputs) and its output layer
    (bf16 input, fp32 output / fp32 incoming gradient, bf16 input gradient)."""
    ops.set_precision("bf16mm")
    x, w, b, dy, yr, dxr, dwr = _conv_case(ops, cin, cout, shape, k, stride, cin * 7 + cout)
    xg = x.to(DEV).to(BF) if xbf else x.to(DEV)
    dyg = dy.to(DEV).to(BF) if ybf else dy.to(DEV)
    wg, bg = w.to(DEV), b.to(DEV)
    d = ops.make_desc(xg, wg, stride, BF if ybf else torch.float32)
    assert d.io == (9 if xbf else 0) + (6 if ybf else 0)
    y = torch.empty(yr.shape, dtype=BF if ybf else torch.float32, device=DEV)
    ops.raw_conv_fwd(d, xg, None, wg, bg, y)
    if ybf:
        half_ulp_ok(y, yr, "y")
    else:
        assert rel(y, yr) < 2e-6
    dx = torch.empty(x.shape, dtype=xg.dtype, device=DEV)
    ops.raw_conv_bwd_data(d, dyg, wg, dx)
    if xbf:
        half_ulp_ok(dx, dxr, "dx")
    else:
        assert rel(dx, dxr) < 2e-6
    dw = torch.empty_like(wg)
    ops.raw_conv_bwd_weight(d, xg, None, dyg, dw)
    assert rel(dw, dwr) < 5e-6


def test_conv_chain_on_bf16_input_and_dual_backward(ops):
    """The producer's BatchNorm + LeakyReLU chain applied while a bf16 tensor is staged (forward and backward-weight), and the fused
    input gradient of a 3x3x3 + 1x1x1 pair (dpi_conv_bwd_data_dual: two launches with bf16 tensors, the second accumulating)."""
    ops.set_precision("bf16mm")
    gen = torch.Generator().manual_seed(3)
    cin, c3, c1, shape = 25, 16, 25, (16, 32, 64)
    x = bf16_values((1, cin) + shape, gen)
    chain = torch.stack([torch.rand(cin, generator=gen) + 0.5, torch.randn(cin, generator=gen) * 0.3, torch.full((cin,), 0.2),
                         torch.rand(cin, generator=gen) + 0.5, torch.randn(cin, generator=gen) * 0.1], 1).contiguous()
    w3 = bf16_values((c3, cin, 3, 3, 3), gen, 0.05)
    w1 = bf16_values((c1, cin, 1, 1, 1), gen, 0.2)
    xd = x.double()
    ps, pb, sl, qs, qb = (chain[:, i].double().view(1, cin, 1, 1, 1) for i in range(5))
    v = ps * xd + pb
    tx = (qs * torch.where(v > 0, v, v * sl) + qb)
    # T(x) is NOT bf16-representable: the bf16 arithmetic mode rounds it while staging, so compare the fp32 arithmetic mode tightly ...
    ops.set_precision("fp32")
    xg, wg = x.to(DEV).to(BF), w3.to(DEV)
    d3 = ops.make_desc(xg, wg, 1, BF)
    y = torch.empty((1, c3) + shape, dtype=BF, device=DEV)
    ops.raw_conv_fwd(d3, xg, chain.to(DEV), wg, None, y)
    yr = O.conv_nd(tx, w3.double(), None, 1)
    half_ulp_ok(y, yr, "y (chain)")
    dy3 = bf16_values(tuple(yr.shape), gen)
    dw = torch.empty_like(wg)
    ops.raw_conv_bwd_weight(d3, xg, chain.to(DEV), dy3.to(DEV).to(BF), dw)
    txr = tx.clone().requires_grad_(False)
    wr = w3.double().requires_grad_(True)
    O.conv_nd(txr, wr, None, 1).backward(dy3.double())
    assert rel(dw, wr.grad) < 5e-6
    # ... and the bf16 arithmetic mode at its operand rounding (2^-9 per staged element)
    ops.set_precision("bf16mm")
    d3b = ops.make_desc(xg, wg, 1, BF)
    ops.raw_conv_fwd(d3b, xg, chain.to(DEV), wg, None, y)
    assert rel(y.float(), yr) < 4e-3
    # dual backward-data
    dy1 = bf16_values((1, c1) + shape, gen)
    d1 = ops.make_desc(xg, w1.to(DEV), 1, BF)
    dx = torch.empty((1, cin) + shape, dtype=BF, device=DEV)
    ops.raw_conv_bwd_data_dual(d3b, dy3.to(DEV).to(BF), wg, d1, dy1.to(DEV).to(BF), w1.to(DEV), dx)
    xr = x.double().requires_grad_(True)
    (O.conv_nd(xr, w3.double(), None, 1) * dy3.double()).sum().backward()
    g3 = xr.grad.clone()
    xr.grad = None
    (O.conv_nd(xr, w1.double(), None, 1) * dy1.double()).sum().backward()
    # two stores (the 1x1x1 launch rounds, the 3x3x3 launch adds and rounds again): one bf16 ulp
    half_ulp_ok(dx, g3 + xr.grad, "dx (dual)", slack=1.01)


@pytest.mark.parametrize("store", ["bf16", "fp32"])
@pytest.mark.parametrize("cin,c3,c1,shape,acc", [(67, 4, 25, (32, 64, 64), False), (25, 16, 25, (64, 64, 64), True), (21, 8, 16, (32, 64, 64), False),
                                                 (40, 32, 35, (32, 32, 64), True)])
def test_dual_backward_fused_into_the_bf16_kernel(ops, cin, c3, c1, shape, acc, store):
    """dpi_conv_bwd_data_dual in the bf16 arithmetic mode on big-tile shapes: the 1x1x1 layer's term runs as extra K blocks of
    conv_bf16_kernel (one pass over dx) — bf16 and fp32 tensors, with and without gradient fan-in, C2 = 16 (one step), 25 / 35 (ragged steps).
    Operands are bf16-representable, so the single rounding of the fused pass keeps a bf16 result within half an ulp of the fp64 oracle."""
    ops.set_precision("bf16mm")
    gen = torch.Generator().manual_seed(cin + c1)
    adt = BF if store == "bf16" else torch.float32
    w3 = bf16_values((c3, cin, 3, 3, 3), gen, 0.05)
    w1 = bf16_values((c1, cin, 1, 1, 1), gen, 0.2)
    dy3 = bf16_values((1, c3) + shape, gen)
    dy1 = bf16_values((1, c1) + shape, gen)
    base = bf16_values((1, cin) + shape, gen)
    xr = torch.zeros((1, cin) + shape, dtype=torch.float64, requires_grad=True)
    ((O.conv_nd(xr, w3.double(), None, 1) * dy3.double()).sum() + (O.conv_nd(xr, w1.double(), None, 1) * dy1.double()).sum()).backward()
    ref = xr.grad + (base.double() if acc else 0.0)
    xproto = torch.empty((1, cin) + shape, dtype=adt, device=DEV)
    d3 = ops.make_desc(xproto, w3.to(DEV), 1, adt)
    d1 = ops.make_desc(xproto, w1.to(DEV), 1, adt)
    dx = base.to(DEV).to(adt) if acc else torch.empty_like(xproto)
    ops.raw_conv_bwd_data_dual(d3, dy3.to(DEV).to(adt), w3.to(DEV), d1, dy1.to(DEV).to(adt), w1.to(DEV), dx, accumulate=acc)
    if store == "bf16":
        half_ulp_ok(dx, ref, "dx (fused dual)")
    else:
        assert rel(dx, ref) < 2e-6, rel(dx, ref)
    # the library really took one launch: with the fusion switched off the same call must give the two-launch result (two roundings in bf16)
    L = ops._lib.load()
    L.set_option("dual_bwd_data", 0)
    try:
        dx2 = base.to(DEV).to(adt) if acc else torch.empty_like(xproto)
        ops.raw_conv_bwd_data_dual(d3, dy3.to(DEV).to(adt), w3.to(DEV), d1, dy1.to(DEV).to(adt), w1.to(DEV), dx2, accumulate=acc)
    finally:
        L.set_option("dual_bwd_data", 1)
    assert rel(dx2.float(), ref) < (6e-3 if store == "bf16" else 2e-6)


def test_unknown_io_bits_are_rejected(ops):
    L = ops._lib.load()
    x = torch.zeros((1, 4, 4, 4, 4), device=DEV)
    w = torch.zeros((4, 4, 3, 3, 3), device=DEV)
    d = ops.make_desc(x, w, 1)
    d.io = 16
    assert L.dpi_conv_fwd(C.byref(d), x.data_ptr(), None, w.data_ptr(), None, x.data_ptr(), None, None) < 0
    assert L.dpi_chain_apply_io(x.data_ptr(), None, 4, 64, x.data_ptr(), 4, None) < 0


# ---------------------------------------------------------------------------------------------------------------------------------------
# (2) elementwise kernels: bf16 entry == round_bf16(fp32 entry on the widened tensors), bit for bit
def _chain(C_, gen):
    return torch.stack([torch.rand(C_, generator=gen) + 0.5, torch.randn(C_, generator=gen) * 0.3, torch.full((C_,), 0.2),
                        torch.rand(C_, generator=gen) + 0.5, torch.randn(C_, generator=gen) * 0.1], 1).contiguous().to(DEV)


def _bits_equal(a_bf16, b_f32, what):
    """a (bf16 tensor) == round-to-nearest-even(b) exactly."""
    assert a_bf16.dtype == BF
    exp = b_f32.to(BF)
    same = a_bf16.view(torch.int16) == exp.view(torch.int16)
    assert bool(same.all()), "%s: %d of %d elements differ from round_bf16(fp32 path)" % (what, int((~same).sum()), same.numel())


@pytest.mark.parametrize("C_,shape", [(5, (6, 8, 12)), (3, (5, 7, 9)), (13, (16, 16, 32))])
def test_chain_apply_add_stats_and_channel_stats_bf16(ops, C_, shape):
    from deep_prior_interpolation_amd._lib import check, load, ptr, stream
    L = load()
    gen = torch.Generator().manual_seed(C_)
    V = int(np.prod(shape))
    a, b = (bf16_values((1, C_) + shape, gen).to(DEV) for _ in range(2))
    cha, chb = _chain(C_, gen), _chain(C_, gen)
    ab, bb = a.to(BF), b.to(BF)
    # chain_apply
    y32 = torch.empty_like(a)
    ops.raw_chain_apply(a, cha, C_, V, y32)
    y16 = torch.empty_like(ab)
    ops.raw_chain_apply(ab, cha, C_, V, y16)
    _bits_equal(y16, y32, "chain_apply")
    # channel statistics of T(x) read from a bf16 tensor == read from its widened copy
    nblk = L.dpi_stat_blocks(C_, V)
    p32 = torch.zeros(nblk * C_ * 2, dtype=torch.float64, device=DEV)
    p16 = torch.zeros_like(p32)
    check(L.dpi_channel_stats_io(ptr(a), ptr(cha), C_, V, ptr(p32), 0, stream()))
    check(L.dpi_channel_stats_io(ptr(ab), ptr(cha), C_, V, ptr(p16), 1, stream()))
    assert torch.equal(p32, p16)
    # residual join: t stored as bf16, statistics of act(stored t)
    t32, t16 = torch.empty_like(a), torch.empty_like(ab)
    q32, q16 = torch.zeros_like(p32), torch.zeros_like(p32)
    check(L.dpi_chain_add_stats_io(ptr(a), ptr(cha), ptr(b), ptr(chb), C_, V, 0.2, ptr(t32), ptr(q32), 0, stream()))
    check(L.dpi_chain_add_stats_io(ptr(ab), ptr(cha), ptr(bb), ptr(chb), C_, V, 0.2, ptr(t16), ptr(q16), 1, stream()))
    _bits_equal(t16, t32, "chain_add_stats t")
    ts = t16.float().double()
    act = torch.where(ts > 0, ts, ts * 0.2).reshape(C_, -1)
    got = q16.view(nblk, C_, 2).sum(0)
    np.testing.assert_allclose(got[:, 0].cpu().numpy(), act.sum(1).cpu().numpy(), rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(got[:, 1].cpu().numpy(), (act * act).sum(1).cpu().numpy(), rtol=1e-6)


@pytest.mark.parametrize("C_,shape", [(6, (6, 8, 12)), (3, (5, 7, 9)), (25, (8, 16, 32)), (6, (4, 17, 241)), (6, (5, 29, 113))])      # the last two: two reduction blocks
def test_batchnorm_backward_kernels_bf16(ops, C_, shape):
    """reduce / apply / apply_fork / apply_dual with bf16 forward tensors and bf16 gradients: same partials, dx == round(fp32 dx), and the
    follow-up partials a fork / dual emits describe the STORED (rounded) dx."""
    from deep_prior_interpolation_amd._lib import load
    L = load()
    gen = torch.Generator().manual_seed(C_ + 100)
    x, xa, xb_, dy = (bf16_values((1, C_) + shape, gen).to(DEV) for _ in range(4))
    f32 = dict(dtype=torch.float32, device=DEV)
    gam, bet = torch.rand(C_, generator=gen).to(DEV) + 0.5, torch.randn(C_, generator=gen).to(DEV) * 0.2

    def mi_of(t):
        m = t.double().reshape(C_, -1).mean(1)
        v = t.double().reshape(C_, -1).var(1, unbiased=False)
        return torch.cat([m, 1.0 / torch.sqrt(v + 1e-5)]).float().to(DEV)
    mi, mia, mib = mi_of(x), mi_of(xa), mi_of(xb_)
    b16 = lambda t: t.to(BF)
    # plain two-phase backward
    dx32, dg32, db32 = ops._bn_backward(dy, x, mi, gam, bet, 1.0, 0.2)
    dx16, dg16, db16 = ops._bn_backward(b16(dy), b16(x), mi, gam, bet, 1.0, 0.2)
    _bits_equal(dx16, dx32, "bn_bwd_apply dx")
    assert torch.equal(dg32, dg16) and torch.equal(db32, db16)
    # fork: dx feeds two more BatchNorms; their partials must equal a reduce pass over the stored dx
    forks32 = [(xa, mia, gam, bet, None, 0.2), (xb_, mib, gam, bet, None, 1.0)]
    forks16 = [(b16(xa), mia, gam, bet, None, 0.2), (b16(xb_), mib, gam, bet, None, 1.0)]
    dt32, _, _, reds32 = ops._bn_backward_fork(dy, x, mi, gam, bet, 0.2, 1.0, forks32)
    dt16, _, _, reds16 = ops._bn_backward_fork(b16(dy), b16(x), mi, gam, bet, 0.2, 1.0, forks16)
    _bits_equal(dt16, dt32, "bn_bwd_apply_fork dx")
    for (xk, mik, gk, ek, _, postk), (nblk, got) in zip(forks16, reds16):
        # phase-2 driven by those partials == phase-2 after an explicit reduce over the stored gradient
        a1 = ops._bn_backward_apply(dt16, xk, mik, gk, ek, 1.0, postk, (nblk, got))
        a2 = ops._bn_backward(dt16, xk, mik, gk, ek, 1.0, postk)
        assert torch.equal(a1[0].view(torch.int16), a2[0].view(torch.int16))
        np.testing.assert_allclose(a1[1].cpu().numpy(), a2[1].cpu().numpy(), rtol=2e-5, atol=1e-5)
    # dual: two sides share the incoming gradient, third BatchNorm forked off side b on a channel range
    lo, hi = 1, C_ - 1
    xs = xb_[:, lo:hi].double().reshape(hi - lo, -1)
    mif = torch.cat([xs.mean(1), 1.0 / torch.sqrt(xs.var(1, unbiased=False) + 1e-5)]).float().to(DEV)
    (da32, _, _), (db32_, _, _), _ = ops._bn_backward_apply_dual(dt32, (xa, mia, gam, bet, None, 0.2, reds32[0]), (xb_, mib, gam, bet, None, 1.0, reds32[1]),
                                                                fork=(lo, hi, mif, gam[lo:hi].contiguous(), bet[lo:hi].contiguous(), 0.2))
    (da16, _, _), (db16_, _, _), redf = ops._bn_backward_apply_dual(dt16, (b16(xa), mia, gam, bet, None, 0.2, reds16[0]), (b16(xb_), mib, gam, bet, None, 1.0, reds16[1]),
                                                                   fork=(lo, hi, mif, gam[lo:hi].contiguous(), bet[lo:hi].contiguous(), 0.2))
    # (the dual's inputs differ between the two runs by the rounding of dt and of the fork partials: compare against the fp32 entry point
    #  fed with the widened bf16 inputs of the bf16 run instead)
    (da_w, _, _), (db_w, _, _), _ = ops._bn_backward_apply_dual(dt16.float(), (xa, mia, gam, bet, None, 0.2, reds16[0]), (xb_, mib, gam, bet, None, 1.0, reds16[1]))
    _bits_equal(da16, da_w, "bn_bwd_apply_dual dxa")
    _bits_equal(db16_, db_w, "bn_bwd_apply_dual dxb")
    g1 = ops._bn_backward_apply(db16_[:, lo:hi], b16(xb_)[:, lo:hi], mif, gam[lo:hi].contiguous(), bet[lo:hi].contiguous(), 1.0, 0.2, redf)
    g2 = ops._bn_backward(db16_[:, lo:hi].contiguous(), b16(xb_)[:, lo:hi].contiguous(), mif, gam[lo:hi].contiguous(), bet[lo:hi].contiguous(), 1.0, 0.2)
    assert torch.equal(g1[0].view(torch.int16), g2[0].view(torch.int16))
    del L, f32


@pytest.mark.parametrize("linear", [0, 1])
@pytest.mark.parametrize("C_,shape,crop", [(3, (4, 6, 8), (0, 0, 0)), (5, (3, 5, 7), (1, 1, 1)), (2, (8, 8, 16), (0, 1, 0))])
def test_upsample_forward_and_adjoint_bf16(ops, C_, shape, crop, linear):
    from deep_prior_interpolation_amd._lib import check, load, ptr, stream
    L = load()
    gen = torch.Generator().manual_seed(11)
    D, H, W = shape
    Do, Ho, Wo = 2 * D - crop[0], 2 * H - crop[1], 2 * W - crop[2]
    x = bf16_values((1, C_) + shape, gen).to(DEV)
    y32 = torch.empty((1, C_, Do, Ho, Wo), device=DEV)
    y16 = torch.empty_like(y32, dtype=BF)
    check(L.dpi_upsample2x_fwd_io(ptr(x), None, C_, D, H, W, Do, Ho, Wo, linear, ptr(y32), 0, stream()))
    check(L.dpi_upsample2x_fwd_io(ptr(x.to(BF)), None, C_, D, H, W, Do, Ho, Wo, linear, ptr(y16), 1, stream()))
    _bits_equal(y16, y32, "upsample fwd")
    dy = bf16_values(tuple(y32.shape), gen).to(DEV)
    dx32 = torch.empty_like(x)
    dx16 = torch.empty_like(x, dtype=BF)
    ops.raw_upsample2x_bwd(dy, C_, D, H, W, Do, Ho, Wo, linear, dx32)
    ops.raw_upsample2x_bwd(dy.to(BF), C_, D, H, W, Do, Ho, Wo, linear, dx16)
    _bits_equal(dx16, dx32, "upsample bwd")
    # and without the workspace (gather kernels)
    dx16b = torch.empty_like(dx16)
    check(L.dpi_upsample2x_bwd_io(ptr(dy.to(BF)), C_, D, H, W, Do, Ho, Wo, linear, ptr(dx16b), None, 2, stream()))
    dx32b = torch.empty_like(dx32)
    check(L.dpi_upsample2x_bwd_io(ptr(dy), C_, D, H, W, Do, Ho, Wo, linear, ptr(dx32b), None, 0, stream()))
    _bits_equal(dx16b, dx32b, "upsample bwd (gather)")


def test_noise_add_writes_the_same_stream_as_bf16():
    from deep_prior_interpolation_amd._lib import check, load, ptr, stream
    L = load()
    for n in (4096, 4099):
        z = torch.randn(n, device=DEV)
        step = torch.tensor([7], dtype=torch.int64, device=DEV)
        o32 = torch.empty(n, device=DEV)
        o16 = torch.empty(n, dtype=BF, device=DEV)
        check(L.dpi_noise_add_io(ptr(z), n, 0.03, 5, ptr(step), ptr(o32), 0, stream()))
        check(L.dpi_noise_add_io(ptr(z), n, 0.03, 5, ptr(step), ptr(o16), 1, stream()))
        _bits_equal(o16, o32, "noise_add")


# ---------------------------------------------------------------------------------------------------------------------------------------
# (3) fused nodes and the loop
def _net_run(shape, precision, epochs, seed=3, inputdepth=16, extra=()):
    from deep_prior_interpolation_amd import utils as u
    from deep_prior_interpolation_amd.main import Interpolator
    from deep_prior_interpolation_amd.parameter import parse_arguments
    vol = u.hyperbolic_volume(shape, seed=seed)
    mask = u.random_trace_mask(shape, 0.5, seed=seed + 1)
    args = parse_arguments(["--imgdir", "synthetic", "--datadim", "3d", "--net", "multiunet", "--inputdepth", str(inputdepth), "--upsample", "linear",
                            "--loss", "mae", "--lr", "1e-3", "--gain", "40", "--epochs", str(epochs), "--gpu", "0", "--precision", precision] + list(extra))
    u.set_seed(7)
    T = Interpolator(args, "/tmp", seed=7)
    T.load_data({"image": (vol.astype(np.float64) * 40)[..., None], "mask": mask.astype(np.float64)[..., None], "name": "0"})
    T.build_model()
    T.build_input()
    return T


@pytest.mark.parametrize("C,shape,fork", [(25, (8, 16, 32), (12, 25)), (16, (6, 10, 12), None), (6, (5, 7, 9), (4, 6)),
                                          (6, (4, 17, 241), (4, 6)), (6, (5, 29, 113), None)])      # V = 16388, 16385: two reduction blocks
def test_join_kernels_with_bf16_tensors_equal_the_rounded_fp32_call(ops, C, shape, fork):
    """Round 5: dpi_join_bwd / dpi_chain_add_apply / dpi_chain_add_stats(t = NULL) with bf16 tensors: a bf16 element is widened exactly on load,
    arithmetic and the nested per-channel sums are fp32 / double, results are rounded to nearest-even on store — so every stored tensor must be
    BIT-EQUAL to round_bf16 of what the fp32 call computes on the widened operands, and the per-channel outputs (statistics, dgamma / dbeta)
    equal to it (they never pass through bf16)."""
    L = ops._lib.load()
    g = torch.Generator().manual_seed(31)
    slope = 0.2
    V = int(np.prod(shape))
    lo, hi = fork if fork else (0, 0)
    mk = lambda scale=1.0: bf16_values((1, C) + shape, g, scale).to(DEV)
    xa, xb, dy = mk(2.0), mk(1.5), mk(1.0)
    stat = lambda n: torch.cat([torch.randn(n, generator=g) * 0.2, torch.rand(n, generator=g) + 0.5]).to(DEV)      # {mean, invstd}
    vec = lambda n: (torch.rand(n, generator=g) * 2 + 0.5).to(DEV)
    chain = lambda n: torch.stack([torch.rand(n, generator=g) + 0.5, torch.randn(n, generator=g) * 0.2, torch.full((n,), slope),
                                   torch.rand(n, generator=g) + 0.5, torch.randn(n, generator=g) * 0.2], dim=1).contiguous().to(DEV)
    mi, mia, mib = stat(C), stat(C), stat(C)
    ga, ea, gb, eb, gt, et = (vec(C) for _ in range(6))
    fwa, fwb, inb, cho = chain(C), chain(C), chain(C), chain(C)
    mif, gf, ef = stat(hi - lo), vec(hi - lo), vec(hi - lo)

    def run(dt):
        xa_, xb_, dy_ = xa.to(dt), xb.to(dt), dy.to(dt)
        cv = {id(xa): xa_, id(xb): xb_, id(dy): dy_}.__getitem__
        cv = (lambda f: (lambda t: f(id(t))))(cv)
        # forward half: statistics of act(T_a(a) + T_b(b)) without storing the sum, then y = T_out(sum)
        nblk = L.dpi_stat_blocks(C, V)
        part = torch.zeros(nblk * C * 2, dtype=torch.float64, device=DEV)
        io_f = ops._io(cv(xa))
        ops.check(L.dpi_chain_add_stats_io(ops.ptr(cv(xa)), ops.ptr(fwa), ops.ptr(cv(xb)), ops.ptr(fwb), C, V, slope, None, ops.ptr(part), io_f,
                                           ops.stream()), "stats")
        y = torch.empty((1, C) + shape, dtype=dt, device=DEV)
        ops.check(L.dpi_chain_add_apply(ops.ptr(cv(xa)), ops.ptr(fwa), ops.ptr(cv(xb)), ops.ptr(fwb), ops.ptr(cho), C, V, ops.ptr(y), io_f,
                                        ops.stream()), "apply")
        dxf = torch.empty((1, hi - lo) + shape, dtype=dt, device=DEV) if hi > lo else None
        fk = (lo, hi, mif, gf, ef, slope, dxf) if hi > lo else None
        out = ops._join_backward(cv(dy), None, mi, gt, et, slope, (cv(xa), mia, ga, ea, None, slope), (cv(xb), mib, gb, eb, inb, 1.0), fk,
                                 fwd_chains=(fwa, fwb))
        torch.cuda.synchronize()
        return part, y, out, dxf
    p32, y32, ((dxa32, dga32, dea32), (dxb32, dgb32, deb32), (dgt32, det32), f32_), dxf32 = run(torch.float32)
    p16, y16, ((dxa16, dga16, dea16), (dxb16, dgb16, deb16), (dgt16, det16), f16_), dxf16 = run(BF)
    assert y16.dtype == BF and dxa16.dtype == BF
    assert torch.equal(p16, p32)
    rnd = lambda t: t.to(BF)
    assert torch.equal(y16, rnd(y32)) and torch.equal(dxa16, rnd(dxa32))
    keep = [c for c in range(C) if not (lo <= c < hi)]
    if keep:
        assert torch.equal(dxb16[:, keep], rnd(dxb32[:, keep]))
    if hi > lo:
        assert torch.equal(dxf16, rnd(dxf32)) and torch.equal(f16_[0], f32_[0]) and torch.equal(f16_[1], f32_[1])
    for a_, b_ in ((dga16, dga32), (dea16, dea32), (dgb16, dgb32), (deb16, deb32), (dgt16, dgt32), (det16, det32)):
        assert torch.equal(a_, b_)


def test_a_long_multi_patch_job_recycles_the_packed_weight_scratch(ops):
    """every patch builds a new network (reference main.py:286) and the bf16 stencil kernel keeps one scratch slot per
    (weight tensor, shape) — 343 patches per configs[2] volume used to add 343 networks' worth of slots until the 4 GB cap failed every launch.
    Interpolator.build_model() now hands the old network's slots back (dpi_pack_forget, ABI 402) and the new network's layers take them from
    the free list.  Here: 220 patches through ONE Interpolator, every 3x3x3 layer forced through the bf16 kernel, two Adam iterations each:
    the live slot count stays at one network's worth, the scratch at its first chunk, and the last patch still computes what a fresh
    process computes for it."""
    from deep_prior_interpolation_amd import utils as u
    from deep_prior_interpolation_amd.main import Interpolator
    from deep_prior_interpolation_amd.parameter import parse_arguments
    L = ops._lib.load()
    assert L.dpi_pack_release() == 0
    shape = (16, 16, 32)
    args = parse_arguments(["--imgdir", "synthetic", "--datadim", "3d", "--net", "multiunet", "--filters", "8", "16", "--skip", "8", "--inputdepth", "8",
                            "--upsample", "linear", "--loss", "mae", "--epochs", "2", "--gpu", "0", "--precision", "bf16"])
    vol = (u.hyperbolic_volume(shape, seed=2).astype(np.float64) * 40)[..., None]
    mask = u.random_trace_mask(shape, 0.5, seed=3).astype(np.float64)[..., None]
    L.set_option("bf16_debug", 8)
    try:
        T = Interpolator(args, "/tmp")
        per_net, last = None, None
        for i in range(220):
            T.load_data({"image": vol, "mask": mask, "name": str(i)})
            T.begin_patch(i % 7)
            T.build_model()
            T.build_input()
            T.optimize(verbose=False, mode="eager")
            n = int(L.dpi_pack_slot_count())
            if per_net is None:
                per_net = n
                assert per_net >= 8, per_net                       # the mode really packs (forward + backward-data slots of the stride-1 layers)
            assert n == per_net, (i, n, per_net)                   # recycled, not grown
            last = (np.array(T.history.loss), T.out_best.copy())
            T.clean()
        assert int(L.dpi_pack_scratch_bytes()) == (64 << 20)
        assert T.release_packed_weights() == per_net and int(L.dpi_pack_slot_count()) == 0
        # the recycled slots hold what their new owner packed: patch 219 (seed 219 % 7 = 2) from a fresh scratch gives the same numbers
        assert L.dpi_pack_release() == 0
        T2 = Interpolator(args, "/tmp")
        T2.load_data({"image": vol, "mask": mask, "name": "x"})
        T2.begin_patch(219 % 7)
        T2.build_model()
        T2.build_input()
        T2.optimize(verbose=False, mode="eager")
        np.testing.assert_array_equal(last[0], np.array(T2.history.loss))
        np.testing.assert_array_equal(last[1], T2.out_best)
    finally:
        L.set_option("bf16_debug", 0)
        ops.set_precision("fp32")
        ops.set_storage("fp32")


@pytest.mark.parametrize("shape", [(32, 32, 64), (20, 18, 36), (17, 19, 22)])
def test_one_iteration_in_storage_mode_against_fp32_storage(ops, shape):
    """Same weights, same perturbed input: forward output, loss and the convolution weight gradients of the default MulResUnet3D with bf16
    activations against fp32 storage.  The freshly initialised net is sensitive to rounding — its gradients are small correlated residuals of
    large sums — so the bar is CALIBRATED in the test itself: the fp32 kernels with nothing but the ten block outputs rounded to bf16 by hand
    (forward hooks) move the output by ~1.3 % and the conv weight gradients by ~12 % (median); the storage mode rounds ~6 tensors per block
    plus every gradient tensor and must stay within 8 x / 4 x of that, with the loss within 0.1 % and every conv-weight gradient at
    cosine > 0.85.  (tools/diag_storage.py prints the error block by block: it grows smoothly, ~0.5 % per block, no jump at any kernel.)
    Also checks that the storage mode really is on: bf16 tensors between the nodes, fp32 network output."""
    seen = []
    T32 = _net_run(shape, "fp32", 1)
    T16 = _net_run(shape, "bf16", 1)
    T16.net.load_state_dict(T32.net.state_dict())
    z = T32.input_.clone()
    out = {}

    def run(name, T, hook):
        hooks = [m.register_forward_hook(hook) for m in T.net.modules() if type(m).__name__ == "MultiResBlock"]
        T.net.zero_grad()
        with T.precision_scope():                                          # this Interpolator's mode, on this thread, for the nodes built inside
            stored.append(ops.storage_bf16())
            o = T.net(z.to(BF) if ops.storage_bf16() else z)
            loss, _ = ops.masked_loss(o, T.img_, T.mask_, "mae")
        assert not ops.storage_bf16()                                      # ... and nothing of it outlives the scope
        loss.backward()
        for h in hooks:
            h.remove()
        out[name] = (o.detach().clone(), float(loss), {k: p.grad.detach().clone() for k, p in T.net.named_parameters() if p.grad is not None and p.ndim == 5})
    stored = []
    run("fp32", T32, lambda mod, i, o: seen.append(("fp32", o.dtype)))
    assert stored == [False]
    run("hand", T32, lambda mod, i, o: o.to(BF).float())                    # calibration: block outputs rounded, everything else fp32
    run("bf16", T16, lambda mod, i, o: seen.append(("bf16", o.dtype)))
    assert stored == [False, False, True]
    assert {d for n, d in seen if n == "bf16"} == {BF} and {d for n, d in seen if n == "fp32"} == {torch.float32}
    o32, l32, g32 = out["fp32"]
    oh, lh, gh = out["hand"]
    o16, l16, g16 = out["bf16"]
    assert o16.dtype == torch.float32
    cal_o = rel(oh, o32)
    cal_g = float(np.median([rel(gh[k], g32[k]) for k in g32]))
    got_o = rel(o16, o32)
    got_g = float(np.median([rel(g16[k], g32[k]) for k in g32]))
    cos = {k: float((g16[k].double().flatten() @ g32[k].double().flatten()) / (g16[k].double().norm() * g32[k].double().norm())) for k in g32}
    print(shape, "output rel %.3e (block outputs rounded by hand: %.3e), loss %.6f / %.6f, conv-weight gradient rel median %.3e (hand: %.3e), min cos %.3f"
          % (got_o, cal_o, l32, l16, got_g, cal_g, min(cos.values())))
    assert got_o < 8 * cal_o and got_o < 0.15
    assert abs(l16 - l32) < 1e-3 * abs(l32)
    assert got_g < 4 * cal_g
    assert min(cos.values()) > 0.85, min(cos.items(), key=lambda kv: kv[1])


def test_loop_in_storage_mode_eager_and_graph_agree_and_converge(ops):
    """Interpolator.optimize with --precision bf16 (storage mode): the captured-graph loop reproduces the eager loop bit for bit, both
    stay finite and reach the fp32 run's loss level."""
    shape = (32, 32, 32)
    runs = {}
    for prec, mode in (("fp32", "eager"), ("bf16", "eager"), ("bf16", "graph")):
        T = _net_run(shape, prec, 120)
        T.optimize(verbose=False, mode=mode)
        runs[(prec, mode)] = np.array(T.history.loss)
        assert np.isfinite(runs[(prec, mode)]).all() and np.isfinite(np.asarray(T.out_best)).all()
    np.testing.assert_array_equal(runs[("bf16", "eager")], runs[("bf16", "graph")])
    ref, got = runs[("fp32", "eager")], runs[("bf16", "eager")]
    # (the first ~60 iterations are chaotic — the loss leaves its initial plateau somewhere between iteration 20 and 50, and runs that differ
    #  in their last bit are 30-80 % apart at iteration 40 (round 5, two seeds x two kernel variants: 0.89 .. 1.37 in fp32, 1.14 .. 1.88 with
    #  bf16 storage) and back within 30 % by iteration 120 — so the comparison is made at 120 iterations with loose bars: same start, a clear
    #  decrease, the fp32 run's level within a factor; the SNR protocols of tests/test_gpu_snr_parity.py are the statement)
    assert abs(got[0] - ref[0]) < 1e-2 * ref[0]
    assert got[-1] < 0.5 * got[0] and got[-1] < 1.6 * ref[-1], (ref[-1], got[-1])


def test_nets_without_fused_3d_nodes_keep_fp32_storage(ops):
    """--precision bf16 on a net the storage mode is not built for (2-D MulResUnet, ELU activation): operand rounding only, fp32 tensors."""
    from deep_prior_interpolation_amd import utils as u
    from deep_prior_interpolation_amd.main import Interpolator
    from deep_prior_interpolation_amd.parameter import parse_arguments
    T = _net_run((16, 16, 16), "bf16", 2, extra=["--activation", "ELU"])
    assert not T.storage_bf16_ok()
    T.optimize(verbose=False)
    with T.precision_scope():
        assert not ops.storage_bf16() and ops.precision() == 1
    assert np.isfinite(T.history.loss).all()
    args = parse_arguments(["--imgdir", "x", "--datadim", "2d", "--filters", "4", "8", "--skip", "4", "--inputdepth", "4", "--epochs", "2", "--gpu", "0",
                            "--precision", "bf16"])
    u.set_seed(0)
    T = Interpolator(args, "/tmp")
    rng = np.random.RandomState(0)
    T.load_data({"image": rng.randn(24, 20, 1), "mask": (rng.rand(24, 20, 1) > 0.5).astype(np.float64), "name": "0"})
    T.build_model()
    T.build_input()
    assert not T.storage_bf16_ok()
    T.optimize(verbose=False)
    assert np.isfinite(T.history.loss).all()


def test_configs4_field_scale_job_end_to_end(ops, monkeypatch):
    """BASELINE configs[4] as written, on one GPU: a 512 x 512 x 1024 synthetic volume (notebook-like events, mirror-tiled), 70 % irregular
    trace decimation, cut into 512 x 256 x 256 patches with stride 256 x 128 x 128 (reference data.py:44-84 / utils/patch_extractor.py:299-368:
    21 windows, up to 4 hits per voxel), every patch pulled from parallel.PatchQueue and optimised with bf16 activations / gradients + fp32
    master weights (two Adam iterations each: the job's plumbing and residency, not its convergence), overlap-added on the device
    (dpi_overlap_add), normalised by the analytic hit count (dpi_overlap_normalize; reference patch_extractor.py:370-428).
    Asserted: every patch finite and bf16-stored, the allocator's peak below what fp32 storage of ONE such patch needs (~160 GB), and the
    re-assembled volume equal to the reference's host arithmetic (float64 accumulate + counted hits, parallel.HostOverlapAccumulator) on
    the very patch outputs the device path accumulated."""
    from deep_prior_interpolation_amd import parallel, utils as u
    from deep_prior_interpolation_amd.data import patch_extractor_for
    from deep_prior_interpolation_amd.parameter import parse_arguments
    vshape, missing = (512, 512, 1024), 0.70
    args = parse_arguments(["--imgdir", "synthetic", "--datadim", "3d", "--net", "multiunet", "--inputdepth", "64", "--upsample", "linear",
                            "--loss", "mae", "--lr", "1e-3", "--gain", "40", "--epochs", "2", "--gpu", "0", "--precision", "bf16",
                            "--patch_shape", "512", "256", "256", "--patch_stride", "256", "128", "128"])
    vol = u.tiled_hyperbolic_volume(vshape, seed=0)
    mask = u.random_trace_mask(vshape, missing, seed=1)
    assert abs(1.0 - float(mask[0].mean()) - missing) < 1e-3
    pe = patch_extractor_for(vshape, args.patch_shape, args.patch_stride, "3d")
    origins = u.window_origins(vshape, pe.dim, pe.stride)
    assert len(origins) == 21 and tuple(pe.dim) == (512, 256, 256)

    class Patches:                        # the patch list of reference data.py:44-84, cut on demand (21 x 2 x 134 MB otherwise)
        def __len__(self):
            return len(origins)

        def __getitem__(self, i):
            sl = tuple(slice(int(o), int(o) + d) for o, d in zip(origins[i], pe.dim))
            return {"image": (vol[sl] * args.gain)[..., None], "mask": mask[sl][..., None], "name": str(i).zfill(3)}
    seen, dtypes = {}, set()

    class Recording(parallel.DeviceOverlapAccumulator):
        def add(self, patch, origin):
            seen[tuple(int(o) for o in origin)] = patch.detach().float().cpu().numpy()
            super().add(patch, origin)
    monkeypatch.setattr(parallel, "DeviceOverlapAccumulator", Recording)
    real_conv = ops.raw_conv_fwd

    def spy(d, x, chain, w, bias, y, partials=None):
        dtypes.add((x.dtype, y.dtype))
        return real_conv(d, x, chain, w, bias, y, partials)
    monkeypatch.setattr(ops, "raw_conv_fwd", spy)
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    timings = {}
    rec, mine = parallel.optimise_volume(args, Patches(), origins, vshape, pe, torch.device("cuda", 0), "/tmp", 1,
                                         parallel.PatchQueue(len(origins)), save=False, timings=timings)
    peak = torch.cuda.max_memory_allocated() / 2 ** 30
    print("configs[4] job: %d patches, set-up %.1f s, loops %.1f s, peak %.1f GiB" % (len(mine), timings["setup_s"], timings["loop_s"], peak))
    assert sorted(mine) == list(range(21)) and len(seen) == 21
    assert (torch.bfloat16, torch.bfloat16) in dtypes and (torch.bfloat16, torch.float32) in dtypes      # bf16 between the nodes, fp32 network output
    assert peak < 130.0
    assert rec.shape == vshape and np.isfinite(rec).all()
    host = parallel.HostOverlapAccumulator(vshape, pe.dim, pe.stride)
    for org, p in seen.items():
        assert np.isfinite(p).all()
        host.add(p, org)
    ref = host.finalize(args.gain)
    err = float(np.abs(rec - ref).max())
    print("device overlap-add + analytic hit count vs host float64 accumulate + counted hits: max |difference| %.3g (max |value| %.3g)"
          % (err, float(np.abs(ref).max())))
    assert err <= 2e-6 * float(np.abs(ref).max())        # fp32 sums of <= 4 patch values against float64
    torch.cuda.empty_cache()


def test_whole_net_in_storage_mode_against_the_fp64_oracle_with_the_same_rounding_points(ops, monkeypatch):
    """the net-level bf16 tests compared HIP with HIP.  Here the ORACLE (fp64 arithmetic) is given the rounding points of the
    storage mode and the HIP net is compared with it.  Rounding points of `--precision bf16` on the 3-D MultiRes-UNet:
      * every tensor a fused node STORES is bf16: raw conv outputs (bias added), the stride-2 layer's activation, block / ResPath outputs, the up-sampled
        deep branch (both halves of a level's concat buffer), the network input; the output layer writes fp32;
      * a 3x3x3 layer (stride 1 or 2) rounds BOTH matrix operands to bf16 — the chained input T(stored) and the weights; a 1x1x1 layer multiplies the
        stored (bf16) input with fp32 weights on the fp32 MFMA (tools/diag_bf16_weights.py shows each of these on single launches);
      * BatchNorm statistics are those of the stored values; chains, joins, sums, loss: fp32 (the oracle: fp64).
    What can and cannot be asserted (tests/diag/diag_bf16_emulation.py prints every stage): where fp32 accumulation lands a value on the other side of a bf16
    rounding boundary than fp64 does, ONE element differs by a bf16 ulp, and every conv + BatchNorm stage that follows roughly doubles such a difference
    (2.5e-5 after the first layer, 1e-4 after the first block, 1e-2 at the output ten stages later) — the net is as chaotic forward as the loop is over
    iterations.  So the rounding points are pinned where they are first used, against the WRONG alternatives: at the first block the emulation must be
    >= 5 x closer to the HIP tensors than each variant with one rounding point moved (1x1x1 weights rounded too; 3x3x3 weights not rounded; chained
    operands not re-rounded; block outputs not rounded), the first stride-2 layer, the first ResPath and the output have absolute bars, and the whole
    net must be closer to the emulated oracle than to the exact one."""
    from oracle import dpi_oracle as O
    shape = (32, 32, 64)
    T = _net_run(shape, "bf16", 1, extra=["--filters", "16", "32", "64", "--skip", "16", "32"], inputdepth=16)
    assert T.storage_bf16_ok()
    init = {k: v.detach().cpu().clone() for k, v in T.net.state_dict().items()}
    gen = torch.Generator().manual_seed(11)
    x = (0.1 * torch.randn((1, 16) + shape, generator=gen)).to(BF).float()               # the stored network input
    cfg = {"ndim": 3, "filters": T.args.filters, "skip": T.args.skip, "upsample": "trilinear"}
    img, msk = T.img_.cpu().double(), T.mask_.cpu().double()
    rb = lambda t: t.to(BF).to(t.dtype)                                                   # round to nearest-even, identity gradient
    nrm = lambda a, b: float((a.double() - b.double()).norm() / b.double().norm())
    # ---- the HIP net, with its block outputs, stride-2 layer outputs and raw conv outputs recorded
    blocks, s2_out, raw = [], [], {}
    hooks = [m.register_forward_hook(lambda mod, i, o: blocks.append(o.detach().float().cpu())) for m in T.net.modules() if type(m).__name__ == "MultiResBlock"]
    name_of = {p.data_ptr(): n for n, p in T.net.named_parameters()}
    orig_cba, orig_raw = ops.conv_bn_act, ops._cba_raw
    monkeypatch.setattr(ops, "conv_bn_act", lambda *a, **k: (lambda y: (s2_out.append(y.detach().float().cpu()), y)[1])(orig_cba(*a, **k)))

    def rec_raw(d, xx, in_chain, w, b, bn, slope, r_out, mi_out, chain_out):
        orig_raw(d, xx, in_chain, w, b, bn, slope, r_out, mi_out, chain_out)
        raw[name_of[w.data_ptr()][:-len(".weight")]] = r_out.detach().float().cpu()
    monkeypatch.setattr(ops, "_cba_raw", rec_raw)
    T.net.zero_grad()
    with T.precision_scope():
        out_dev = T.net(x.to(DEV).to(BF))
        loss, _ = ops.masked_loss(out_dev, T.img_, T.mask_, "mae")
    loss.backward()
    for h in hooks:
        h.remove()
    out = out_dev.detach().float().cpu()
    # ---- the oracle with movable rounding points
    orig_fn = {n: getattr(O, n) for n in ("block3d", "respath3d", "upsample2x", "activation")}

    def emulate(round_w3=True, round_w1=False, round_x=True, round_blocks=True, exact=False, grad=False):
        rec = {"raw": {}, "acts": []}

        class St(O.NetState):
            def conv(self, key, xin, stride=1):
                w, b = self.P[key + ".weight"], self.P.get(key + ".bias")
                if exact:
                    return O.conv_nd(xin, w, b, stride)
                xin = rb(xin) if round_x else xin                                         # a stored tensor (no-op) or the bf16 MFMA operand T(stored)
                if (w.shape[-1] == 3 and round_w3) or (w.shape[-1] == 1 and round_w1):
                    w = rb(w)
                y = O.conv_nd(xin, w, b, stride)
                y = y if key == "4.0" else rb(y)                                          # the output layer writes fp32
                rec["raw"][key] = y.detach()
                return y
        for n in ("block3d", "respath3d", "upsample2x"):
            monkeypatch.setattr(O, n, (lambda f: (lambda *a, **k: rb(f(*a, **k))))(orig_fn[n]) if (round_blocks and not exact) else orig_fn[n])
        monkeypatch.setattr(O, "activation", lambda name, t: (lambda r: (rec["acts"].append(r.detach()), r)[1])(orig_fn["activation"](name, t)))
        taps = {}
        S = St(init, dtype=torch.float64, requires_grad=grad)
        o = O.net_forward(S, x.double(), cfg, taps=taps)
        return S, o, [taps[k].detach() for k in ("enc0", "enc1", "enc2", "dec2", "dec1") if k in taps], rec
    _, o_exact, t_exact, _ = emulate(exact=True)
    o_exact = o_exact.detach()
    wrong = {"1x1x1 weights rounded too": dict(round_w1=True), "3x3x3 weights not rounded": dict(round_w3=False),
             "chained operands not re-rounded": dict(round_x=False), "block outputs not rounded": dict(round_blocks=False)}
    first_block_wrong = {name: nrm(blocks[0], emulate(**kw)[2][0]) for name, kw in wrong.items()}
    emu, o_emu, t_emu, rec = emulate(grad=True)
    l_emu = O.masked_loss(o_emu, img, msk, "mae")
    l_emu.backward()
    o_emu = o_emu.detach()
    per_block = [nrm(h, e) for h, e in zip(blocks, t_emu)]
    effect = [nrm(e, x_) for e, x_ in zip(t_emu, t_exact)]
    print("per block, HIP vs emulated oracle: %s   (the storage mode's effect, emulated vs exact: %s)" % (" ".join("%.2e" % v for v in per_block), " ".join("%.2e" % v for v in effect)))
    print("first block against the wrong emulations: %s" % ", ".join("%s %.2e" % kv for kv in first_block_wrong.items()))
    assert len(blocks) == len(t_emu) == 5
    assert per_block[0] < 3e-4 and effect[0] > 3e-3
    for name, v in first_block_wrong.items():
        assert v > 5.0 * per_block[0], (name, v, per_block[0])
    # the first stride-2 layer (stored activation) and the first ResPath (its two raw conv outputs), fed by the first block
    s2_e = [a for a in rec["acts"] if tuple(a.shape) == tuple(s2_out[0].shape)]
    assert len(s2_e) == 1 and nrm(s2_out[0], rb(s2_e[0])) < 1.5e-3
    for key in ("2.0.1.conv3x3.0.0", "2.0.1.conv1x1.0.0"):
        assert nrm(raw[key], rec["raw"][key]) < 1.5e-3, key
    # the whole net: closer to the emulated oracle than to the exact one; the loss to 1e-4
    e_emu, e_exact = nrm(out, o_emu), nrm(out, o_exact)
    print("output: HIP vs emulated %.3e, HIP vs exact %.3e, emulated vs exact %.3e; loss HIP %.6f emulated %.6f" % (e_emu, e_exact, nrm(o_emu, o_exact), loss.item(), l_emu.item()))
    assert e_emu < 0.75 * e_exact and e_exact > 5e-3
    assert abs(loss.item() - l_emu.item()) < 2e-4 * abs(l_emu.item())
    # weight gradients: the HIP path also STORES activation gradients as bf16 (the emulation passes gradients through unrounded): same direction
    cos = []
    for k, p in T.net.named_parameters():
        if p.ndim == 5 and p.grad is not None and emu.P[k].grad is not None and emu.P[k].grad.norm() > 0:
            g, ge = p.grad.detach().cpu().double().flatten(), emu.P[k].grad.flatten()
            cos.append(float(torch.dot(g, ge) / (g.norm() * ge.norm() + 1e-300)))
    print("conv-weight gradients vs the emulated oracle: cosine min %.4f median %.4f over %d tensors" % (min(cos), float(np.median(cos)), len(cos)))
    assert np.median(cos) > 0.95 and min(cos) > 0.7
