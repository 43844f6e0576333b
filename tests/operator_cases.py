"""The 16 entry points of csrc/operators.hip (the anti-aliasing add-on, its dip estimator, the three POCS kernels) and csrc/unet_ops.hip
(max-pool and transposed convolution of --net unet) as tests/test_gpu_operator_contract.py checks them on a device: the case rows, numpy
restatements written from include/dpi_hip.h and the reference's formulas (utils/processing.py, utils/slopes.py, utils/pocs.py, unet.py;
the library is never called), and the check functions.  A plain module: no fixtures, importable without a GPU.
tests/test_operator_refs_host.py holds the restatements against independent code (oracle.dpi_oracle, the section stacking of
tests/test_gpu_antialias3d.py, torch's max_pool2d / conv_transpose2d with autograd, the recorded vectors) and proves, restatement against
restatement, that the checks catch a wrong kernel (the `mutation` arguments).

Two kinds of restatement:
 * fp32, one correctly rounded operation per numpy call, compared bit for bit (the library is built with -ffp-contract=off and the
   compiler's correctly rounded fp32 divide and sqrt): diff_axis, structure_tensor[_sections], threshold, pocs_project, scaled_max, the
   pool, the anisotropy of dips and the ratio that feeds its atanf;
 * float64 with a propagated bound |got - ref| <= (k 2^-24 + n 2^-53) S, S the same expression with every product and difference
   replaced by its absolute value: hale2d, hale_sections, the transposed convolution.  k counts the fp32 roundings a term passes and is
   stated at each call; n = the number of terms + 32 k^2, the second part being the higher orders of (1 + u)^k - 1 <= k u + k^2 u^2
   (k^2 u^2 = 32 k^2 2^-53), so the bound is a bound and not a first-order estimate.

Why each row exists (launches of operators.hip are min(ceil(n / 256), 8192) blocks of 256: OP_PASS = 2097152 elements per grid-stride pass;
those of unet_ops.hip min(ceil(n / 256), 2048) blocks per channel: UNET_PASS = 524288):

 FLAT_N (threshold, pocs_project, dips)
   1, 63, 255    one block, threads without an element;  256   one full block;  257   a second block with one element
   65537         257 blocks;  2097152   the cap reached exactly, one pass;  2097409 = 8192 x 256 + 257   a second, partial pass
 MAX_N (scaled_max; blocks 1, 1, 1, 2, 255, 256, 257, 8192, 8192)
   max_final_kernel loops over the partials only past 256 of them: 65280 / 65536 / 65537 sit around that; the unique maximum is put at
   index 0, 63, 64 (a wave boundary), n - 1 and, for the last size, 2097152 (the first element of the second pass)
 DIFF_SHAPES (outer, n, inner)
   n = 1, 2, 3 are the sizes at which `i >= 1` / `i <= n - 2` leave no, one or both neighbours; (2, 1025, 1031) and (1, 2097409, 1)
   run the grid-stride loop with inner > 1 and inner = 1
 PLANE_SHAPES (N, H, W) (hale2d, structure_tensor)
   H or W of 1 and 2: no forward difference / none of a forward difference; (1, 170, 100) the product's section; (3, 701, 999) has
   2100897 samples, its planes straddle the pass boundary
 SECTION_SHAPES (C, T, X, Y) (hale_sections, structure_tensor_sections)
   T, X in {1, 2, 3}: the only sizes at which the second-neighbour guards (t <= T - 3, xi >= 2) decide;  Y = 4: one quad per row;
   Y = 1, 2, 5, 17, 129: the scalar twin;  (1, 129, 127, 129)   scalar, 2113407 samples, second pass;  (1, 130, 128, 508)   float4,
   2113280 quads, second pass.  Every row with Y % 4 == 0 runs aligned and moved by 1 and 2 elements (SECTION_OFFSETS).
 POOL_SHAPES (C, H, W)
   (1, 2, 2)   one window;  odd H and / or W: the trailing row / column of dx is written as zero;  (2, 1451, 1453)   526350 outputs and
   2108303 inputs per channel, both past UNET_PASS, both axes odd
 DECONV_SHAPES (Cin, Cout, H, W)
   H or W of 1: taps 0 and 3 fall outside;  (1, 1, 17, 16)   a 272-sample plane: two trips of backward-weight's per-thread loop;
   (1, 1, 363, 363)   527076 outputs, past the forward cap;  (1, 1, 725, 727)   527075 inputs, past the backward-data cap, 2059 trips
"""
import numpy as np

F = np.float32
U = 2.0 ** -24                                    # unit round-off of fp32

OP_MAX_BLOCKS, UNET_MAX_BLOCKS = 8192, 2048
OP_PASS, UNET_PASS = OP_MAX_BLOCKS * 256, UNET_MAX_BLOCKS * 256

FLAT_N = (1, 63, 255, 256, 257, 65537, 2097152, 2097409)
MAX_N = (1, 64, 255, 257, 65280, 65536, 65537, 2097152, 2097409)
THRESHOLDS = (0.5, 0.0, -0.25)
DIFF_SHAPES = ((1, 1, 1), (1, 1, 300), (1, 2, 1), (2, 2, 2), (1, 3, 1), (3, 5, 7), (300, 1, 1), (1, 300, 1), (3, 70, 5), (2, 1025, 1031),
               (1, 2097409, 1))
DIFF_LARGE = DIFF_SHAPES[-2:]                     # these run stencils 0 and 3 only
DIFF_SPACING = 0.7
PLANE_SHAPES = ((1, 1, 1), (1, 1, 5), (1, 5, 1), (2, 2, 2), (3, 2, 3), (1, 3, 2), (2, 5, 6), (1, 170, 100), (3, 701, 999))
TENSOR_DV, TENSOR_DH = 0.5, 2.0
SECTION_SHAPES = ((1, 1, 1, 1), (1, 1, 1, 4), (1, 2, 1, 4), (1, 1, 2, 8), (1, 2, 2, 2), (1, 3, 2, 5), (1, 2, 3, 12), (2, 3, 3, 8), (2, 13, 10, 17),
                  (1, 24, 16, 40), (1, 129, 127, 129), (1, 130, 128, 508))
SECTION_OFFSETS = (0, 1, 2)
SECTION_SPACINGS = (0.5, 2.0, 0.7)                # dt, dx, dy of structure_tensor_sections
POOL_SHAPES = ((1, 2, 2), (1, 2, 3), (1, 3, 2), (2, 3, 3), (3, 9, 12), (2, 5, 7), (1, 33, 35), (2, 64, 64), (2, 1451, 1453))
DECONV_SHAPES = ((1, 1, 1, 1), (1, 1, 1, 2), (1, 1, 2, 1), (2, 3, 1, 5), (5, 3, 6, 7), (3, 2, 9, 11), (1, 1, 17, 16), (4, 5, 16, 17),
                 (1, 1, 363, 363), (1, 1, 725, 727))
DECONV_NULL_BIAS = ((1, 1, 1, 1), (5, 3, 6, 7), (1, 1, 363, 363))
# (gvv, gvh, ghh) every dips row starts with: 0/0 -> phi 0; x/0 -> +pi/2; the zero tensor -> phi 0 and NaN anisotropy; three ordinary ones
DIPS_SPECIAL = ((3.0, 0.0, 1.0), (1.0, 0.0, 3.0), (0.0, 0.0, 0.0), (1.0, 0.0, 1.0), (4.0, 2.0, 1.0), (2.0, -2.0, 5.0))


def op_blocks(n):
    return max(1, min(-(-n // 256), OP_MAX_BLOCKS))


def unet_blocks(n):
    return max(1, min(-(-n // 256), UNET_MAX_BLOCKS))


def max_positions(n):
    """Where the unique maximum is put, in turn: the first element, the last lane of wave 0, the first of wave 1, the last element and
    the first element of the second grid-stride pass — those that exist."""
    out = []
    for p in (0, 63, 64, n - 1) + ((OP_PASS,) if n > OP_PASS else ()):
        if 0 <= p < n and p not in out:
            out.append(p)
    return out


def case_id(shape):
    return "x".join(map(str, shape))


# ---- checks ------------------------------------------------------------------------------------------------------------------------------
def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def check_written(got, what, nan_expected=None):
    """Every declared element was written: none keeps the NaN pre-fill (nor is infinite), except where the restatement itself is NaN —
    there the element must BE NaN."""
    got = np.asarray(got)
    bad = ~np.isfinite(got)
    if nan_expected is not None:
        nan_expected = np.asarray(nan_expected, dtype=bool).reshape(got.shape)
        miss = np.flatnonzero((nan_expected & ~np.isnan(got)).ravel())
        assert miss.size == 0, "%s: %d elements should be NaN, first at %d: %r" % (what, miss.size, int(miss[0]), got.ravel()[miss[0]])
        bad &= ~nan_expected
    bad = np.flatnonzero(bad.ravel())
    assert bad.size == 0, "%s: %d of %d elements were not written (or are not finite), first at %d" % (what, bad.size, got.size, int(bad[0]))


def check_bits(got, want, what, nan_equal=False):
    """Bit equality as int32, zeros' signs included; names the first differing element.  nan_equal: a NaN matches a NaN whatever its sign
    and payload (0 / 0 has the sign bit set on x86 and clear on the device)."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype == F, (what, got.shape, want.shape, got.dtype, want.dtype)
    differ = bits(got).ravel() != bits(want).ravel()
    if nan_equal:
        differ &= ~(np.isnan(got).ravel() & np.isnan(want).ravel())
    bad = np.flatnonzero(differ)
    assert bad.size == 0, "%s: %d of %d elements differ, first at %d: got %r, want %r" % (
        what, bad.size, got.size, int(bad[0]), got.ravel()[bad[0]], want.ravel()[bad[0]])


def bound(S, k, nterms):
    return (k * U + (nterms + 32.0 * k * k) * 2.0 ** -53) * np.asarray(S, dtype=np.float64)


def check_bound(got, ref, S, k, nterms, what):
    """|got - ref64| <= (k 2^-24 + n 2^-53) S element by element, n = nterms + 32 k^2 (module docstring).  An element whose S is 0 has no
    non-zero term: it must be 0.  Returns the largest |got - ref| / bound."""
    got, ref, S = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64), np.asarray(S, dtype=np.float64)
    assert got.shape == ref.shape == S.shape, (what, got.shape, ref.shape, S.shape)
    check_written(got, what)
    ratio = np.abs(got - ref) / (bound(S, k, nterms) + 1e-300)
    i = int(ratio.argmax())
    assert ratio.ravel()[i] <= 1.0, "%s: element %d is off by %.3g x its bound (got %.9g, float64 %.17g, S %.3g, k %d)" % (
        what, i, ratio.ravel()[i], got.ravel()[i], ref.ravel()[i], S.ravel()[i], k)
    return float(ratio.ravel()[i])


def phi_ref(ratio32):
    """float64 atan of the fp32 ratio, NaN -> 0."""
    with np.errstate(invalid="ignore"):
        p = np.arctan(np.asarray(ratio32, dtype=F).astype(np.float64))
    p[np.isnan(p)] = 0.0
    return p


def ulps(got, ref64):
    """|got - ref64| in fp32 spacings of ref64."""
    ref64 = np.asarray(ref64, dtype=np.float64)
    return np.abs(np.asarray(got, dtype=np.float64) - ref64) / np.spacing(np.abs(ref64).astype(F)).astype(np.float64)


def check_phi(got, ratio32, bar_ulps, what):
    """phi against float64 atan of the exactly reproduced ratio, within bar_ulps fp32 spacings of the result.  Returns the largest error in ulps."""
    got = np.asarray(got)
    assert got.dtype == F
    check_written(got, what)
    e = ulps(got, phi_ref(ratio32))
    i = int(e.argmax())
    assert e[i] <= bar_ulps, "%s: phi[%d] = %r is %.3g ulp from atan(%r) = %.17g (bar %.3g)" % (what, i, got[i], e[i], ratio32[i], phi_ref(ratio32)[i], bar_ulps)
    return float(e[i])


def drop_second_pass(want, pass_elems=OP_PASS, stale=None):
    """A kernel that forgets its grid-stride loop: elements >= pass_elems keep the NaN pre-fill (or `stale`)."""
    out = np.array(want, copy=True)
    flat = out.reshape(-1)
    flat[pass_elems:] = np.nan if stale is None else stale
    return out


# ---- shifts and differences along one axis (zero outside) --------------------------------------------------------------------------------
def _next(a, axis):
    """a[i + 1], 0 at the last index."""
    out = np.zeros_like(a)
    n = a.shape[axis]
    dst, src = [slice(None)] * a.ndim, [slice(None)] * a.ndim
    dst[axis], src[axis] = slice(0, n - 1), slice(1, n)
    out[tuple(dst)] = a[tuple(src)]
    return out


def _prev(a, axis):
    """a[i - 1], 0 at index 0."""
    out = np.zeros_like(a)
    n = a.shape[axis]
    dst, src = [slice(None)] * a.ndim, [slice(None)] * a.ndim
    dst[axis], src[axis] = slice(1, n), slice(0, n - 1)
    out[tuple(dst)] = a[tuple(src)]
    return out


def _rows(a, axis, lo, hi):
    """a on the rows lo <= i <= hi of `axis`, 0 on the others."""
    i = np.arange(a.shape[axis]).reshape([-1 if d == axis else 1 for d in range(a.ndim)])
    return np.where((i >= lo) & (i <= hi), a, np.zeros((), dtype=a.dtype))


# ---- dpi_diff_axis -----------------------------------------------------------------------------------------------------------------------
def diff_axis_np(x, stencil, spacing, adjoint):
    """[outer][n][inner] fp32.  Forward: the rows of utils/processing.py:139-181 — forward (x[i+1] - x[i]) on i <= n-2, backward
    (x[i] - x[i-1]) on i >= 1, centred (0.5 x[i+1] - 0.5 x[i-1]) and second (x[i+1] - 2 x[i] + x[i-1]) on 1 <= i <= n-2, 0 elsewhere —
    then ONE division by h (h * h in fp32 for the second derivative).  Adjoint: the transpose, i.e. the same coefficients on the shifted
    copies of g restricted to the active rows, summed in the order of the forward expression."""
    x = np.asarray(x, dtype=F)
    n = x.shape[1]
    h = F(spacing) * F(spacing) if stencil == 3 else F(spacing)
    lo, hi = {0: (0, n - 2), 1: (1, n - 1), 2: (1, n - 2), 3: (1, n - 2)}[stencil]
    half, two = F(0.5), F(2.0)
    if not adjoint:
        up, dn = _next(x, 1), _prev(x, 1)
        r = {0: lambda: up - x, 1: lambda: x - dn, 2: lambda: half * up - half * dn, 3: lambda: up - two * x + dn}[stencil]()
        r = _rows(r, 1, lo, hi)
    else:
        g = _rows(x, 1, lo, hi)                                   # row j of the matrix exists for lo <= j <= hi
        up, dn = _next(g, 1), _prev(g, 1)                         # column i meets row i + 1 through its x[i-1] tap, row i - 1 through x[i+1]
        r = {0: lambda: dn - g, 1: lambda: g - up, 2: lambda: half * dn - half * up, 3: lambda: dn - two * g + up}[stencil]()
    y = r / h
    assert y.dtype == F
    return y


# ---- Hale2D: dpi_hale2d, dpi_hale_sections -----------------------------------------------------------------------------------------------
def _D(u, axis, absolute, keep_last=False):
    """Forward difference with a zero last row (u[i+1] - u[i] on i <= n-2); absolute: the sum of the two magnitudes."""
    r = _next(u, axis) + u if absolute else _next(u, axis) - u
    return r if keep_last else _rows(r, axis, 0, u.shape[axis] - 2)


def _DT(u, axis, absolute):
    """Its transpose: u[k-1] on k >= 1 minus u[k] on k <= n-2."""
    a, b = _prev(u, axis), _rows(u, axis, 0, u.shape[axis] - 2)
    return a + b if absolute else a - b


def hale_np(x, a, b, c, v, h, adjoint=False, absolute=False, mutation=None):
    """float64.  Forward (utils/slopes.py:51-105): y = -(Dh(a Dv x + b Dh x) + Dv(b Dv x + c Dh x)), D the forward difference along axis
    v / h with a zero last row.  Adjoint: with r1 = Dh^T g, r2 = Dv^T g, x = -(Dv^T(a r1 + b r2) + Dh^T(b r1 + c r2)).
    absolute: every product and difference replaced by its absolute value (the S of the bound).
    mutation "t_guard": the difference along v is taken on the last row too, against a zero row — what `t <= T - 2` in place of
    `t <= T - 3` makes of the neighbour's p2."""
    x, a, b, c = (np.asarray(t, dtype=np.float64) for t in (x, a, b, c))
    if absolute:
        x, a, b, c = np.abs(x), np.abs(a), np.abs(b), np.abs(c)
    if not adjoint:
        gv, gh = _D(x, v, absolute, keep_last=(mutation == "t_guard")), _D(x, h, absolute)
        s = _D(a * gv + b * gh, h, absolute) + _D(b * gv + c * gh, v, absolute)
    else:
        r1, r2 = _DT(x, h, absolute), _DT(x, v, absolute)
        s = _DT(a * r1 + b * r2, v, absolute) + _DT(b * r1 + c * r2, h, absolute)
    return s if absolute else -s


HALE_K, HALE_TERMS = 5, 16
"""k of one Hale2D output: a term x a passes the difference Dx (1), its product with a (1), the sum of the two products (1), the outer
difference (1) and the sum of the two outer differences (1); the sign is exact.  16 terms: 2 outer differences x 2 points x 2 products x 2."""
SECTIONS_ADJ_K, SECTIONS_ADJ_TERMS = HALE_K + 1, 2 * HALE_TERMS
"""The adjoint on sections adds the two families' results: one more rounding."""


def hale2d_np(x, a, b, c, adjoint=False, absolute=False):
    """[N][H][W]: v = H, h = W."""
    return hale_np(x, a, b, c, 1, 2, adjoint, absolute)


def hale_sections_np(x, coef, adjoint=False, absolute=False, mutation=None):
    """[C][T][X][Y]; coef [6][C][T][X][Y] = a, b, c of the (t,x) family (v = T, h = X), then of the (t,y) family (v = T, h = Y).
    Forward: [2][C][T][X][Y]; adjoint: x is that tensor, the result the sum of the two families' adjoints."""
    if not adjoint:
        return np.stack([hale_np(x, coef[0], coef[1], coef[2], 1, 2, False, absolute, mutation),
                         hale_np(x, coef[3], coef[4], coef[5], 1, 3, False, absolute, mutation)])
    return hale_np(x[0], coef[0], coef[1], coef[2], 1, 2, True, absolute) + hale_np(x[1], coef[3], coef[4], coef[5], 1, 3, True, absolute)


def hale_coef(shape, rng, families=1):
    """a = cos^2, b = -cos sin, c = sin^2 of random dips, in fp32: [3 families] + shape."""
    out = []
    for _ in range(families):
        th = rng.uniform(-np.pi / 2, np.pi / 2, shape)
        out += [(np.cos(th) ** 2).astype(F), (-np.cos(th) * np.sin(th)).astype(F), (np.sin(th) ** 2).astype(F)]
    return np.stack(out)


# ---- structure tensor and dips -----------------------------------------------------------------------------------------------------------
def _grad32(x, axis, spacing):
    """(x[i+1] - x[i]) / spacing on i <= n-2, 0 on the last row: fp32, a difference and a division."""
    x = np.asarray(x, dtype=F)
    return _rows((_next(x, axis) - x) / F(spacing), axis, 0, x.shape[axis] - 2)


def structure_tensor_np(x, dv, dh):
    """[N][H][W] -> gvv, gvh, ghh (utils/slopes.py:19-22)."""
    gv, gh = _grad32(x, 1, dv), _grad32(x, 2, dh)
    return gv * gv, gv * gh, gh * gh


def structure_tensor_sections_np(x, dt, dx, dy):
    """[C][T][X][Y] -> gtt, gtx, gxx, gty, gyy."""
    gt, gx, gy = _grad32(x, 1, dt), _grad32(x, 2, dx), _grad32(x, 3, dy)
    return gt * gt, gt * gx, gx * gx, gt * gy, gy * gy


def dips_np(gvv, gvh, ghh):
    """utils/slopes.py:35-46 in fp32, one rounding per operation: t1 = (gvv + ghh) / 2, t2 = sqrt((gvv - ghh)^2 + 4 gvh^2) / 2,
    l1 = t1 + t2, l2 = t1 - t2.  Returns (ratio, anisotropy) = ((l1 - gvv) / gvh, 1 - l2 / l1) as IEEE gives them; phi = atan(ratio)
    with NaN -> 0 is phi_ref(ratio)."""
    vv, vh, hh = (np.asarray(t, dtype=F) for t in (gvv, gvh, ghh))
    with np.errstate(all="ignore"):
        t1 = F(0.5) * (vv + hh)
        d = vv - hh
        t2 = F(0.5) * np.sqrt(d * d + F(4.0) * (vh * vh))
        l1, l2 = t1 + t2, t1 - t2
        ratio, aniso = (l1 - vv) / vh, F(1.0) - l2 / l1
    assert ratio.dtype == aniso.dtype == F
    return ratio, aniso


def dips_inputs(n, seed):
    """(gvv, gvh, ghh) [n]: DIPS_SPECIAL first, then rank-1 tensors (gv^2, gv gh, gh^2) as the unsmoothed estimator produces them and
    sums of three such (full rank, as after smoothing), alternating."""
    rng = np.random.default_rng(seed)
    gv, gh = rng.standard_normal((3, n), dtype=F), rng.standard_normal((3, n), dtype=F)
    full = (np.arange(n) % 2 == 1)
    vv, vh, hh = gv[0] * gv[0], gv[0] * gh[0], gh[0] * gh[0]
    for k in (1, 2):
        vv, vh, hh = (np.where(full, t + u, t) for t, u in ((vv, gv[k] * gv[k]), (vh, gv[k] * gh[k]), (hh, gh[k] * gh[k])))
    sp = np.array(DIPS_SPECIAL, dtype=F)[:n]
    vv[:len(sp)], vh[:len(sp)], hh[:len(sp)] = sp[:, 0], sp[:, 1], sp[:, 2]
    return vv.astype(F), vh.astype(F), hh.astype(F)


# ---- POCS --------------------------------------------------------------------------------------------------------------------------------
def threshold_np(x, th, mutation=None):
    """utils/pocs.py:5-8: x * ((x > th).float() + (x < -th).float()) — the flags added as floats, so a negative th makes the factor 2.
    mutation "ge": >= and <= in place of the strict inequalities."""
    x, th = np.asarray(x, dtype=F), F(th)
    hi, lo = (x >= th, x <= -th) if mutation == "ge" else (x > th, x < -th)
    return x * (hi.astype(F) + lo.astype(F))


def threshold_inputs(n, th, seed):
    """Random values around the threshold with elements exactly +th, -th and -0.0 planted at the front and in the tail."""
    x = np.random.default_rng(seed).standard_normal(n, dtype=F)
    for k, v in enumerate((F(th), -F(th), F(-0.0))):
        if k < n:
            x[k] = v
        if n - 1 - k > 2:
            x[n - 1 - k] = v
    return x


def pocs_project_np(x, wdata, wmask):
    """utils/pocs.py:80-84: wdata + wmask * x, a product and a sum."""
    return np.asarray(wdata, dtype=F) + np.asarray(wmask, dtype=F) * np.asarray(x, dtype=F)


def scaled_max_np(x, scale, mutation=None):
    """fp32(max x) * fp32(scale); a NaN is ignored as fmaxf ignores it.  Mutations: "first_256_partials" — the maximum over the first
    256 of the op_blocks(n) per-block partials only (block b owns the elements i with (i // 256) % blocks == b); "no_second_pass" —
    elements >= OP_PASS are not read."""
    x = np.asarray(x, dtype=F)
    if mutation == "no_second_pass":
        x = x[:OP_PASS]
    elif mutation == "first_256_partials":
        x = x[(np.arange(x.size) // 256) % op_blocks(x.size) < 256]
    with np.errstate(invalid="ignore"):
        return np.array([np.fmax.reduce(x) * F(scale)], dtype=F)


def max_inputs(n, pos, seed):
    """Values in (-1, 1) and the unique maximum 10 at `pos`."""
    x = np.random.default_rng(seed).uniform(-1.0, 1.0, n).astype(F)
    x[pos] = 10.0
    return x


# ---- MaxPool2d(2, 2) ---------------------------------------------------------------------------------------------------------------------
def _windows(x):
    """The four taps of every 2 x 2 window in (kh, kw) scan order: [4][C][H/2][W/2]."""
    C, H, W = x.shape
    Ho, Wo = H // 2, W // 2
    return np.stack([x[:, kh:2 * Ho:2, kw:2 * Wo:2] for kh in (0, 1) for kw in (0, 1)])


def _argmax_first(taps, mutation=None):
    """Index of the first maximum in scan order (aten's rule: a later tap replaces the running maximum only if it is greater; a NaN in
    taps 1..3 therefore never wins).  mutation "last_tie": the last of equal taps wins."""
    arg, m = np.zeros(taps.shape[1:], dtype=np.int64), taps[0].copy()
    for k in (1, 2, 3):
        better = taps[k] >= m if mutation == "last_tie" else taps[k] > m
        arg, m = np.where(better, k, arg), np.where(better, taps[k], m)
    return arg, m


def maxpool_fwd_np(x, mutation=None):
    """[C][H][W] -> [C][H/2][W/2] (floor): the selected tap itself, so the sign of a zero is that of the first maximum."""
    return _argmax_first(_windows(np.asarray(x, dtype=F)), mutation)[1]


def maxpool_bwd_np(dy, x, mutation=None):
    """dx [C][H][W], written everywhere: dy at the first maximum of each window, +0 at the other taps and in the trailing row / column of
    an odd H / W.  mutation "odd_row_unwritten": the trailing odd row keeps the NaN pre-fill."""
    x, dy = np.asarray(x, dtype=F), np.asarray(dy, dtype=F)
    C, H, W = x.shape
    Ho, Wo = H // 2, W // 2
    arg, _ = _argmax_first(_windows(x), mutation)
    dx = np.zeros_like(x)
    for k, (kh, kw) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        dx[:, kh:2 * Ho:2, kw:2 * Wo:2] = np.where(arg == k, dy, F(0.0))
    if mutation == "odd_row_unwritten" and H % 2:
        dx[:, H - 1, :] = np.nan
    return dx


def pool_inputs(shape, ties, seed):
    """(x, dy): random floats, or values from {-1, -0.0, 0.0, 1} (ties in nearly every window) with window (0, 0) of channel 0 all equal."""
    C, H, W = shape
    rng = np.random.default_rng(seed)
    if ties:
        x = rng.choice(np.array([-1.0, -0.0, 0.0, 1.0], dtype=F), size=shape)
        x[0, 0:2, 0:2] = 1.0
    else:
        x = rng.standard_normal(shape, dtype=F)
    return x, rng.standard_normal((C, H // 2, W // 2), dtype=F)


# ---- ConvTranspose2d(Cin, Cout, 4, stride 2, padding 1) ----------------------------------------------------------------------------------
def _tap(k, n):
    """Input and output index ranges of tap k along an axis of n inputs: o = 2 i - 1 + k inside [0, 2 n)."""
    i0, i1 = (1 if k == 0 else 0), (n - 1 if k == 3 else n)
    return slice(i0, max(i0, i1)), slice(2 * i0 - 1 + k, max(2 * i0 - 1 + k, 2 * (i1 - 1) + k), 2)


def deconv_fwd_np(x, w, bias, absolute=False, mutation=None):
    """float64 y [Cout][2H][2W] = bias + sum over ci and the taps of x[ci][ih][iw] w[ci][co][kh][kw] at oh = 2 ih - 1 + kh,
    ow = 2 iw - 1 + kw (unet.py:59; w in torch's [Cin][Cout][4][4]).  bias None: no bias.  mutation "bias_twice"."""
    x, w = np.asarray(x, dtype=np.float64), np.asarray(w, dtype=np.float64)
    if absolute:
        x, w = np.abs(x), np.abs(w)
    Cin, H, W = x.shape
    Cout = w.shape[1]
    y = np.zeros((Cout, 2 * H, 2 * W))
    if bias is not None:
        b = np.asarray(bias, dtype=np.float64)
        y += (np.abs(b) if absolute else b)[:, None, None] * (2.0 if mutation == "bias_twice" else 1.0)
    for kh in range(4):
        ih, oh = _tap(kh, H)
        for kw in range(4):
            iw, ow = _tap(kw, W)
            y[:, oh, ow] += np.einsum("chw,co->ohw", x[:, ih, iw], w[:, :, kh, kw])
    return y


def deconv_bwd_data_np(dy, w, absolute=False):
    """float64 dx [Cin][H][W] = sum over co and the taps of dy[co][oh][ow] w[ci][co][kh][kw]."""
    dy, w = np.asarray(dy, dtype=np.float64), np.asarray(w, dtype=np.float64)
    if absolute:
        dy, w = np.abs(dy), np.abs(w)
    H, W = dy.shape[1] // 2, dy.shape[2] // 2
    dx = np.zeros((w.shape[0], H, W))
    for kh in range(4):
        ih, oh = _tap(kh, H)
        for kw in range(4):
            iw, ow = _tap(kw, W)
            dx[:, ih, iw] += np.einsum("ohw,co->chw", dy[:, oh, ow], w[:, :, kh, kw])
    return dx


def deconv_bwd_weight_np(x, dy, absolute=False):
    """float64 dw [Cin][Cout][4][4] = sum over the plane of x[ci][ih][iw] dy[co][oh][ow]."""
    x, dy = np.asarray(x, dtype=np.float64), np.asarray(dy, dtype=np.float64)
    if absolute:
        x, dy = np.abs(x), np.abs(dy)
    Cin, H, W = x.shape
    dw = np.zeros((Cin, dy.shape[0], 4, 4))
    for kh in range(4):
        ih, oh = _tap(kh, H)
        for kw in range(4):
            iw, ow = _tap(kw, W)
            dw[:, :, kh, kw] = np.einsum("chw,ohw->co", x[:, ih, iw], dy[:, oh, ow])
    return dw


def deconv_fwd_k(Cin):
    """One fmaf per (ci, tap) onto the bias, at most 2 x 2 taps reach an output: the first term passes 4 Cin roundings."""
    return 4 * Cin


def deconv_bwd_data_k(Cout):
    """One fmaf per (co, tap), 4 x 4 taps."""
    return 16 * Cout


def deconv_bwd_weight_k(H, W):
    """The per-thread loop of ceil(H W / 256) fmafs, 6 additions of the wave reduction, 3 of the four waves' sums."""
    return -(-(H * W) // 256) + 6 + 3


def deconv_inputs(shape, seed):
    """(x [Cin][H][W], w [Cin][Cout][4][4], bias [Cout], dy [Cout][2H][2W]) fp32."""
    Cin, Cout, H, W = shape
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((Cin, H, W), dtype=F), (0.3 * rng.standard_normal((Cin, Cout, 4, 4))).astype(F),
            rng.standard_normal(Cout, dtype=F), rng.standard_normal((Cout, 2 * H, 2 * W), dtype=F))
