"""What the 16 entry points of csrc/operators.hip and csrc/unet_ops.hip compute and may touch, at the sizes where their code paths change:
the rows of tests/operator_cases.py through the C ABI, every buffer owned by the test.  Inputs and outputs sit inside guard bands
(gpu_guard.guard), outputs NaN-filled; `ws` and `out` of dpi_scaled_max have exactly the queried / documented size.  After every launch:
_launch, _check_guards (both end the session on a launch error or a device fault, as in test_gpu_conv_contract.py), the inputs' bits
unchanged, every declared output element finite (NaN exactly where the restatement of dpi_dips is NaN), and the result against the numpy
restatement of operator_cases.py (held against the oracle, torch and the recorded vectors by tests/test_operator_refs_host.py, which also
shows that each check function used here fails on a mutated restatement).

Bars: bit equality (as int32) for dpi_diff_axis, dpi_structure_tensor[_sections], dpi_threshold, dpi_pocs_project, dpi_scaled_max, the
pool and the anisotropy of dpi_dips; (k 2^-24 + n 2^-53) S against float64 for dpi_hale2d, dpi_hale_sections and the transposed
convolution, k stated at each call; phi of dpi_dips within ATANF_BAR_ULP of float64 atan of the exactly restated ratio (test_dips).
dpi_hale_sections at element offsets 1 and 2 is bit-identical to the aligned call: the per-sample arithmetic is shared by both widths."""
import functools

import numpy as np
import pytest
import torch

import operator_cases as P
from gpu_guard import guard
from test_gpu_conv_contract import _check_guards, _launch

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = torch.float32
F = np.float32
E_ARG = -1
ATANF_MEASURED_ULP = 2.053458  # the device's atanf against float64 atan, see test_dips
ATANF_BAR_ULP = 2 * ATANF_MEASURED_ULP


@pytest.fixture(scope="module")
def lib():
    from deep_prior_interpolation_amd import _lib
    return _lib


# ---- buffers -----------------------------------------------------------------------------------------------------------------------------
def gin(a, offset=0):
    """Host data inside guard bands, `offset` elements behind a 256-byte boundary."""
    a = np.ascontiguousarray(a, dtype=F)
    return guard(a.size, F32, DEV, fill=torch.from_numpy(a.reshape(-1)), offset=offset)


def gout(n, offset=0):
    """A NaN-filled output inside guard bands."""
    return guard(int(n), F32, DEV, offset=offset)


def ptr(g):
    return None if g is None else g.payload.data_ptr()


def host(g, shape=None):
    a = g.payload.cpu().numpy()
    return a if shape is None else a.reshape(shape)


def run(lib, what, call, ins, outs):
    """One launch: it succeeds, no band changed, no input changed."""
    ins = [(k, g) for k, g in ins if g is not None]
    before = [g.bits() for _, g in ins]
    _launch(lib, call(), what)
    _check_guards(ins + list(outs), what)
    for (k, g), b in zip(ins, before):
        assert g.untouched(b), "%s: the input %s was written" % (what, k)


# ---- 1. the flat kernels -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", P.FLAT_N)
def test_threshold(lib, n):
    """y = x * ((x > th) + (x < -th)) bit for bit at th = 0.5, 0 and -0.25 (both flags true: the factor 2), with +th, -th and -0.0 planted
    at the front and in the tail (strict inequalities give 0); n = 2097409 is the first size with a second, partial grid-stride pass."""
    L = lib.load()
    for th in P.THRESHOLDS:
        what = "threshold n=%d th=%g" % (n, th)
        x = P.threshold_inputs(n, th, n % 1000)
        xg, tg, yg = gin(x), gin([th]), gout(n)
        run(lib, what, lambda: L.dpi_threshold(ptr(xg), n, ptr(tg), ptr(yg), lib.stream()), [("x", xg), ("thresh", tg)], [("y", yg)])
        got = host(yg)
        P.check_written(got, what)
        P.check_bits(got, P.threshold_np(x, th), what)


@pytest.mark.parametrize("n", P.FLAT_N)
def test_pocs_project(lib, n):
    """y = wdata + wmask * x bit for bit: a product and a sum, not contracted."""
    L = lib.load()
    what = "pocs_project n=%d" % n
    rng = np.random.default_rng(n % 1000)
    x, d, m = (rng.standard_normal(n, dtype=F) for _ in range(3))
    xg, dg, mg, yg = gin(x), gin(d), gin(m), gout(n)
    run(lib, what, lambda: L.dpi_pocs_project(ptr(xg), ptr(dg), ptr(mg), n, ptr(yg), lib.stream()), [("x", xg), ("wdata", dg), ("wmask", mg)], [("y", yg)])
    got = host(yg)
    P.check_written(got, what)
    P.check_bits(got, P.pocs_project_np(x, d, m), what)


@pytest.mark.parametrize("n", P.FLAT_N)
def test_dips(lib, n):
    """The anisotropy 1 - l2 / l1 bit for bit (NaN where the restatement is NaN: the zero tensor), phi against float64 atan of the fp32
    ratio (l1 - gvv) / gvh, which the restatement reproduces exactly; NaN -> 0 (0 / 0 where the tensor is diagonal), +pi/2 through +inf.
    Every row starts with operator_cases.DIPS_SPECIAL.

    The only unknown is the device's atanf.  Measured on an MI355X over the ratios of these eight rows (4.3 M arguments) against float64
    atan: at most 2.053458 fp32 spacings of the result (ATANF_MEASURED_ULP; at ratio -1.5453186 of the n = 2097152 row; 1.10, 1.78, 1.40,
    1.71, 1.97, 2.05, 2.03 for n = 63 .. 2097409, and torch.atan on the device gives the same figures, so this is the library function
    and not dips_kernel).  The bar is twice that, ATANF_BAR_ULP = 4.106916 ulp, the margin covering arguments the sample misses.  Each
    row prints its own figure."""
    L = lib.load()
    what = "dips n=%d" % n
    vv, vh, hh = P.dips_inputs(n, n % 1000)
    ratio, aniso = P.dips_np(vv, vh, hh)
    gs = [gin(t) for t in (vv, vh, hh)]
    pg, ag = gout(n), gout(n)
    run(lib, what, lambda: L.dpi_dips(ptr(gs[0]), ptr(gs[1]), ptr(gs[2]), n, ptr(pg), ptr(ag), lib.stream()),
        list(zip(("gvv", "gvh", "ghh"), gs)), [("phi", pg), ("anisotropy", ag)])
    got_a, got_p = host(ag), host(pg)
    P.check_written(got_a, what + " anisotropy", nan_expected=np.isnan(aniso))
    P.check_bits(got_a, aniso, what + " anisotropy", nan_equal=True)
    print("%s: phi at most %.4f ulp from float64 atan of the ratio" % (what, float(P.ulps(got_p, P.phi_ref(ratio)).max())))
    P.check_phi(got_p, ratio, ATANF_BAR_ULP, what)
    assert got_p[0] == 0 and not np.signbit(got_p[0]) and (n < 3 or (got_p[1] == F(np.pi / 2) and got_p[2] == 0))


@pytest.mark.parametrize("n", P.MAX_N)
def test_scaled_max(lib, n):
    """out = fp32(max x) * fp32(scale) with the unique maximum at index 0, 63, 64, n - 1 and (n = 2097409) 2097152 in turn; an
    all-negative tensor (the -inf start value), one holding -inf, one with scale 0.05, one holding NaN (ignored).  ws has exactly dpi_max_ws_floats(n) floats
    (= the number of blocks: 1, 1, 1, 2, 255, 256, 257, 8192, 8192), out is one float."""
    L = lib.load()
    nws = L.dpi_max_ws_floats(n)
    assert nws == max(1, min(-(-n // 256), 8192))
    base = np.random.default_rng(n % 1000).uniform(-1.0, 1.0, n).astype(F)
    cases = []
    for pos in P.max_positions(n):
        x = base.copy()
        x[pos] = 10.0
        cases.append(("max at %d" % pos, x, 0.5))
    neg = -np.abs(base) - F(0.125)
    cases.append(("all negative", neg, 0.5))
    inf = base.copy()
    inf[::3] = -np.inf
    if n == 1:
        inf[0] = 0.25
    cases.append(("with -inf", inf, 0.5))
    cases.append(("scale 0.05", base, 0.05))
    if n > 1:
        nan = base.copy()
        nan[::5] = np.nan                              # ignored, as fmaxf ignores it (include/dpi_hip.h); torch.max would return it
        cases.append(("with NaN", nan, 0.5))
    for name, x, scale in cases:
        what = "scaled_max n=%d %s" % (n, name)
        xg, ws, out = gin(x), gout(nws), gout(1)
        run(lib, what, lambda: L.dpi_scaled_max(ptr(xg), n, scale, ptr(ws), ptr(out), lib.stream()), [("x", xg)], [("ws", ws), ("out", out)])
        got = host(out)
        P.check_written(got, what)
        P.check_written(host(ws), what + " ws")
        P.check_bits(got, P.scaled_max_np(x, scale), what)


# ---- 2. derivatives ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", P.DIFF_SHAPES, ids=P.case_id)
def test_diff_axis(lib, shape):
    """All four stencils, forward and transposed, spacing 0.7, bit for bit (differences, then one division; the second derivative
    divides by the fp32 square of the fp32 spacing).  n = 1, 2, 3 leave no, one or both neighbours; the two largest shapes (stencils 0
    and 3) run the grid-stride loop."""
    L = lib.load()
    outer, n, inner = shape
    x = np.random.default_rng(sum(shape)).standard_normal(shape, dtype=F)
    xg = gin(x)
    for stencil in ((0, 3) if shape in P.DIFF_LARGE else (0, 1, 2, 3)):
        for adjoint in (0, 1):
            what = "diff_axis %s stencil %d adjoint %d" % (shape, stencil, adjoint)
            yg = gout(x.size)
            run(lib, what, lambda: L.dpi_diff_axis(ptr(xg), outer, n, inner, stencil, P.DIFF_SPACING, adjoint, ptr(yg), lib.stream()), [("x", xg)], [("y", yg)])
            got = host(yg, shape)
            P.check_written(got, what)
            P.check_bits(got, P.diff_axis_np(x, stencil, P.DIFF_SPACING, adjoint), what)


# ---- 3. Hale2D and the structure tensor on planes ----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def plane_problem(shape):
    """Host operands shared by the tests of one shape and never modified: x (also the adjoint's g), the coefficient planes, and the
    float64 restatements (value, S) of both directions."""
    rng = np.random.default_rng(sum(shape))
    x, coef = rng.standard_normal(shape, dtype=F), P.hale_coef(shape, rng)
    refs = {adj: (P.hale2d_np(x, *coef, adjoint=bool(adj)), P.hale2d_np(x, *coef, adjoint=bool(adj), absolute=True)) for adj in (0, 1)}
    return x, coef, refs


@pytest.mark.parametrize("adjoint", [0, 1])
@pytest.mark.parametrize("shape", P.PLANE_SHAPES, ids=P.case_id)
def test_hale2d(lib, shape, adjoint):
    """y = -(Dh(a Dv x + b Dh x) + Dv(b Dv x + c Dh x)) and its transpose against float64 with k = operator_cases.HALE_K = 5 (the inner
    difference, the product, the sum of two products, the outer difference, the sum of the two outer differences) over 16 terms.
    (3, 701, 999): 2100897 samples, the planes straddle the grid-stride pass boundary."""
    L = lib.load()
    N, H, W = shape
    x, coef, refs = plane_problem(shape)
    what = "hale2d %s adjoint %d" % (shape, adjoint)
    xg, cg, yg = gin(x), [gin(c) for c in coef], gout(x.size)
    run(lib, what, lambda: L.dpi_hale2d(ptr(xg), ptr(cg[0]), ptr(cg[1]), ptr(cg[2]), N, H, W, adjoint, ptr(yg), lib.stream()),
        [("x", xg)] + list(zip("abc", cg)), [("y", yg)])
    ref, S = refs[adjoint]
    print("%s: at %.3g of its bound" % (what, P.check_bound(host(yg, shape), ref, S, P.HALE_K, P.HALE_TERMS, what)))


@pytest.mark.parametrize("shape", P.PLANE_SHAPES, ids=P.case_id)
def test_structure_tensor(lib, shape):
    """gvv, gvh, ghh bit for bit at dv = 0.5, dh = 2: a difference, a division, a product each."""
    L = lib.load()
    N, H, W = shape
    x = plane_problem(shape)[0]
    what = "structure_tensor %s" % (shape,)
    xg, outs = gin(x), [gout(x.size) for _ in range(3)]
    run(lib, what, lambda: L.dpi_structure_tensor(ptr(xg), N, H, W, P.TENSOR_DV, P.TENSOR_DH, *(ptr(o) for o in outs), lib.stream()),
        [("x", xg)], list(zip(("gvv", "gvh", "ghh"), outs)))
    for name, o, want in zip(("gvv", "gvh", "ghh"), outs, P.structure_tensor_np(x, P.TENSOR_DV, P.TENSOR_DH)):
        P.check_written(host(o), what + " " + name)
        P.check_bits(host(o, shape), want, what + " " + name)


# ---- 4. the same on the sections of a patch ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def sections_problem(shape):
    rng = np.random.default_rng(sum(shape))
    return rng.standard_normal(shape, dtype=F), P.hale_coef(shape, rng, 2), rng.standard_normal((2,) + shape, dtype=F)


@functools.lru_cache(maxsize=None)
def sections_ref(shape, adjoint):
    """The float64 restatement (value, S), computed once per module (seconds for the 8.4 M-sample row)."""
    x, coef, g = sections_problem(shape)
    src = g if adjoint else x
    return P.hale_sections_np(src, coef, adjoint=bool(adjoint)), P.hale_sections_np(src, coef, adjoint=bool(adjoint), absolute=True)


@pytest.mark.parametrize("adjoint", [0, 1])
@pytest.mark.parametrize("shape", P.SECTION_SHAPES, ids=P.case_id)
def test_hale_sections(lib, shape, adjoint):
    """Forward [2][C][T][X][Y] and the adjoint against float64: k = 5 forward (HALE_K, as dpi_hale2d), 6 for the adjoint
    (SECTIONS_ADJ_K: the two families' results are added).  A row with Y % 4 == 0 runs with x, coef and y 256-byte aligned (the float4
    kernel) and moved by 1 and by 2 elements (its scalar twin, include/dpi_hip.h: "by any number of elements"): each call is held to
    the restatement, and the moved calls give the bits of the aligned one.  T, X in {1, 2, 3} are the sizes at which the
    second-neighbour guards decide; (1, 129, 127, 129) and (1, 130, 128, 508) run a second grid-stride pass on either width."""
    L = lib.load()
    C, T, X, Y = shape
    x, coef, g = sections_problem(shape)
    src = g if adjoint else x
    ref, S = sections_ref(shape, adjoint)
    k, terms = (P.SECTIONS_ADJ_K, P.SECTIONS_ADJ_TERMS) if adjoint else (P.HALE_K, P.HALE_TERMS)
    first = None
    for off in (P.SECTION_OFFSETS if Y % 4 == 0 else (0,)):
        what = "hale_sections %s adjoint %d offset %d" % (shape, adjoint, off)
        xg, cg, yg = gin(src, off), gin(coef, off), gout(ref.size, off)
        assert all((ptr(b) - 4 * off) % 256 == 0 for b in (xg, cg, yg))
        run(lib, what, lambda: L.dpi_hale_sections(ptr(xg), ptr(cg), C, T, X, Y, adjoint, ptr(yg), lib.stream()), [("x", xg), ("coef", cg)], [("y", yg)])
        got = host(yg, ref.shape)
        print("%s: at %.3g of its bound" % (what, P.check_bound(got, ref, S, k, terms, what)))
        if first is None:
            first = got
        else:
            P.check_bits(got, first, what + " against the aligned call")


@pytest.mark.parametrize("shape", P.SECTION_SHAPES, ids=P.case_id)
def test_structure_tensor_sections(lib, shape):
    """gtt, gtx, gxx, gty, gyy bit for bit at dt = 0.5, dx = 2, dy = 0.7."""
    L = lib.load()
    C, T, X, Y = shape
    x = sections_problem(shape)[0]
    what = "structure_tensor_sections %s" % (shape,)
    names = ("gtt", "gtx", "gxx", "gty", "gyy")
    xg, outs = gin(x), [gout(x.size) for _ in names]
    run(lib, what, lambda: L.dpi_structure_tensor_sections(ptr(xg), C, T, X, Y, *P.SECTION_SPACINGS, *(ptr(o) for o in outs), lib.stream()),
        [("x", xg)], list(zip(names, outs)))
    for name, o, want in zip(names, outs, P.structure_tensor_sections_np(x, *P.SECTION_SPACINGS)):
        P.check_written(host(o), what + " " + name)
        P.check_bits(host(o, shape), want, what + " " + name)


# ---- 5. the plain UNet's pool and transposed convolution ---------------------------------------------------------------------------------
@pytest.mark.parametrize("ties", [False, True], ids=["random", "ties"])
@pytest.mark.parametrize("shape", P.POOL_SHAPES, ids=P.case_id)
def test_maxpool(lib, shape, ties):
    """y and dx bit for bit: the first maximum in (kh, kw) order is selected and receives dy, dx is written everywhere (+0 at the other
    taps and in the trailing row / column of an odd H / W).  The tie run draws from {-1, -0.0, 0.0, 1}: ties in about half of the
    windows, an all-equal window, and zeros whose sign tells which tap was taken.  (2, 1451, 1453): both launches past 2048 blocks."""
    L = lib.load()
    C, H, W = shape
    x, dy = P.pool_inputs(shape, ties, sum(shape))
    what = "maxpool %s %s" % (shape, "ties" if ties else "random")
    xg, dyg, yg, dxg = gin(x), gin(dy), gout(dy.size), gout(x.size)
    run(lib, what + " forward", lambda: L.dpi_maxpool2x2_fwd(ptr(xg), C, H, W, ptr(yg), lib.stream()), [("x", xg)], [("y", yg)])
    P.check_written(host(yg), what + " y")
    P.check_bits(host(yg, dy.shape), P.maxpool_fwd_np(x), what + " y")
    run(lib, what + " backward", lambda: L.dpi_maxpool2x2_bwd(ptr(dyg), ptr(xg), C, H, W, ptr(dxg), lib.stream()), [("dy", dyg), ("x", xg)], [("dx", dxg)])
    P.check_written(host(dxg), what + " dx")
    P.check_bits(host(dxg, shape), P.maxpool_bwd_np(dy, x), what + " dx")


@pytest.mark.parametrize("shape", P.DECONV_SHAPES, ids=P.case_id)
def test_deconv(lib, shape):
    """Against float64.  Forward: k = 4 Cin (deconv_fwd_k: one fmaf per (ci, tap) onto the bias, at most 2 x 2 taps reach an output),
    with a bias and, on the rows of DECONV_NULL_BIAS, with bias == NULL.  Backward-data: k = 16 Cout (deconv_bwd_data_k).
    Backward-weight: k = ceil(H W / 256) + 6 + 3 (deconv_bwd_weight_k: the per-thread loop, the wave reduction, the four waves' sums).
    (1, 1, 363, 363) is past the forward launch's block cap, (1, 1, 725, 727) past backward-data's, with a 2059-trip per-thread loop."""
    L = lib.load()
    Cin, Cout, H, W = shape
    x, w, b, dy = P.deconv_inputs(shape, sum(shape))
    xg, wg, bg, dyg = gin(x), gin(w), gin(b), gin(dy)
    for bias, bgd in ((b, bg),) + (((None, None),) if shape in P.DECONV_NULL_BIAS else ()):
        what = "deconv_fwd %s%s" % (shape, "" if bias is not None else " bias NULL")
        yg = gout(dy.size)
        run(lib, what, lambda: L.dpi_deconv4x4s2_fwd(ptr(xg), ptr(wg), ptr(bgd), Cin, Cout, H, W, ptr(yg), lib.stream()),
            [("x", xg), ("w", wg), ("bias", bgd)], [("y", yg)])
        r = P.check_bound(host(yg, dy.shape), P.deconv_fwd_np(x, w, bias), P.deconv_fwd_np(x, w, bias, absolute=True), P.deconv_fwd_k(Cin), 4 * Cin + 1, what)
        print("%s: at %.3g of its bound" % (what, r))
    what = "deconv_bwd_data %s" % (shape,)
    dxg = gout(x.size)
    run(lib, what, lambda: L.dpi_deconv4x4s2_bwd_data(ptr(dyg), ptr(wg), Cin, Cout, H, W, ptr(dxg), lib.stream()), [("dy", dyg), ("w", wg)], [("dx", dxg)])
    r = P.check_bound(host(dxg, x.shape), P.deconv_bwd_data_np(dy, w), P.deconv_bwd_data_np(dy, w, absolute=True), P.deconv_bwd_data_k(Cout), 16 * Cout, what)
    print("%s: at %.3g of its bound" % (what, r))
    what = "deconv_bwd_weight %s" % (shape,)
    dwg = gout(w.size)
    run(lib, what, lambda: L.dpi_deconv4x4s2_bwd_weight(ptr(xg), ptr(dyg), Cin, Cout, H, W, ptr(dwg), lib.stream()), [("x", xg), ("dy", dyg)], [("dw", dwg)])
    r = P.check_bound(host(dwg, w.shape), P.deconv_bwd_weight_np(x, dy), P.deconv_bwd_weight_np(x, dy, absolute=True), P.deconv_bwd_weight_k(H, W), H * W, what)
    print("%s: at %.3g of its bound" % (what, r))


# ---- 6. refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals(lib):
    """Every call returns DPI_E_ARG, sets dpi_last_error to a message of its entry point and leaves the output payloads' bits untouched:
    refused on the host before any launch, with valid 16-float buffers (outputs: 96) behind every non-NULL pointer.  A NULL in every
    pointer position of every entry point (bias excepted: NULL is `no bias`), x == y, stencil 4, spacing 0, dv / dh / dt 0, a zero
    extent, H = 1 or W = 1 for the pool, C T X Y = 2^31 for dpi_hale_sections and Cin Cout = 2^30 for dpi_deconv4x4s2_bwd_weight (by
    the dimensions alone)."""
    L = lib.load()
    s = lib.stream()
    a = [gin(np.arange(1, 97, dtype=F)) for _ in range(4)]
    o = [gout(96) for _ in range(5)]
    A, O_ = [ptr(t) for t in a], [ptr(t) for t in o]
    before = [t.bits() for t in o]
    # (entry point, message prefix, valid argument list without the stream, positions of its pointers)
    table = [
        (L.dpi_diff_axis, "diff_axis", [A[0], 1, 4, 4, 0, 0.7, 0, O_[0]], (0, 7)),
        (L.dpi_hale2d, "hale2d", [A[0], A[1], A[2], A[3], 1, 4, 4, 0, O_[0]], (0, 1, 2, 3, 8)),
        (L.dpi_hale_sections, "hale_sections", [A[0], A[1], 1, 2, 2, 4, 0, O_[0]], (0, 1, 7)),
        (L.dpi_structure_tensor_sections, "structure_tensor_sections", [A[0], 1, 2, 2, 4, 0.5, 2.0, 0.7] + O_, (0, 8, 9, 10, 11, 12)),
        (L.dpi_structure_tensor, "structure_tensor", [A[0], 1, 4, 4, 0.5, 2.0] + O_[:3], (0, 6, 7, 8)),
        (L.dpi_dips, "dips", [A[0], A[1], A[2], 16] + O_[:2], (0, 1, 2, 4, 5)),
        (L.dpi_scaled_max, "scaled_max", [A[0], 16, 0.5] + O_[:2], (0, 3, 4)),
        (L.dpi_threshold, "threshold", [A[0], 16, A[1], O_[0]], (0, 2, 3)),
        (L.dpi_pocs_project, "pocs_project", [A[0], A[1], A[2], 16, O_[0]], (0, 1, 2, 4)),
        (L.dpi_maxpool2x2_fwd, "maxpool_fwd", [A[0], 1, 4, 4, O_[0]], (0, 4)),
        (L.dpi_maxpool2x2_bwd, "maxpool_bwd", [A[0], A[1], 1, 4, 4, O_[0]], (0, 1, 5)),
        (L.dpi_deconv4x4s2_fwd, "deconv_fwd", [A[0], A[1], A[2], 1, 1, 2, 2, O_[0]], (0, 1, 7)),
        (L.dpi_deconv4x4s2_bwd_data, "deconv_bwd_data", [A[0], A[1], 1, 1, 2, 2, O_[0]], (0, 1, 6)),
        (L.dpi_deconv4x4s2_bwd_weight, "deconv_bwd_weight", [A[0], A[1], 1, 1, 2, 2, O_[0]], (0, 1, 6)),
    ]
    calls = []

    def variant(row, changes, why):
        fn, prefix, args, _ = row
        args = list(args)
        for i, v in changes.items():
            args[i] = v
        calls.append((fn, prefix, args, why))
    by = {row[1]: row for row in table}
    for row in table:
        for i in row[3]:
            variant(row, {i: None}, "NULL in position %d" % i)
    variant(by["diff_axis"], {7: A[0]}, "x == y")
    variant(by["hale2d"], {8: A[0]}, "x == y")
    variant(by["hale_sections"], {7: A[0]}, "x == y")
    variant(by["diff_axis"], {4: 4}, "stencil 4")
    variant(by["diff_axis"], {4: -1}, "stencil -1")
    variant(by["diff_axis"], {5: 0.0}, "spacing 0")
    variant(by["structure_tensor"], {4: 0.0}, "dv = 0")
    variant(by["structure_tensor"], {5: 0.0}, "dh = 0")
    variant(by["structure_tensor_sections"], {5: 0.0}, "dt = 0")
    for name, dims in (("diff_axis", (1, 2, 3)), ("hale2d", (4, 5, 6)), ("hale_sections", (2, 3, 4, 5)), ("structure_tensor_sections", (1, 2, 3, 4)),
                       ("structure_tensor", (1, 2, 3)), ("dips", (3,)), ("scaled_max", (1,)), ("threshold", (1,)), ("pocs_project", (3,)),
                       ("maxpool_fwd", (1, 2, 3)), ("maxpool_bwd", (2, 3, 4)), ("deconv_fwd", (3, 4, 5, 6)), ("deconv_bwd_data", (2, 3, 4, 5)),
                       ("deconv_bwd_weight", (2, 3, 4, 5))):
        for i in dims:
            variant(by[name], {i: 0}, "a zero extent in position %d" % i)
    variant(by["maxpool_fwd"], {2: 1}, "H = 1")
    variant(by["maxpool_fwd"], {3: 1}, "W = 1")
    variant(by["maxpool_bwd"], {3: 1}, "H = 1")
    variant(by["hale_sections"], {2: 2048, 3: 1024, 4: 1024, 5: 1}, "C T X Y = 2^31")
    variant(by["deconv_bwd_weight"], {2: 32768, 3: 32768, 4: 1, 5: 1}, "Cin Cout = 2^30")
    for fn, prefix, args, why in calls:
        rc = fn(*args, s)
        msg = L.dpi_last_error().decode()
        assert rc == E_ARG and msg.startswith(prefix + ":"), (prefix, why, rc, msg)
    _check_guards([("input", t) for t in a] + [("output", t) for t in o], "refusals")
    assert all(t.untouched(b) for t, b in zip(o, before)), "a refused call wrote an output"
    assert len(calls) > 90
