"""The restatements of tests/operator_cases.py against code they were not written from — oracle.dpi_oracle (first / second derivative,
Hale2D, the structure-tensor dips), the section-by-section stacking of tests/test_gpu_antialias3d.py, torch's max_pool2d and
conv_transpose2d in float64 with autograd, the recorded vectors of tests/golden/operators.npz and unet.npz —, each adjoint against the
transposed dense matrix of its forward restatement, the size facts every row is named for, and, restatement against restatement, that
the check functions of tests/test_gpu_operator_contract.py fail on a kernel with one of the defects they exist for.  No GPU: the library
is only asked for dpi_max_ws_floats."""
import math

import numpy as np
import pytest
import torch

import operator_cases as P
from oracle import dpi_oracle as O
from test_gpu_antialias3d import sections_np, tx_stack, tx_unstack, ty_stack, ty_unstack

F = np.float32
STENCILS = ("forward", "backward", "centered", "second")


def _fails(fn):
    try:
        fn()
    except AssertionError:
        return True
    return False


def _theta_coef(theta):
    return np.cos(theta) ** 2, -np.cos(theta) * np.sin(theta), np.sin(theta) ** 2


# ---- size facts --------------------------------------------------------------------------------------------------------------------------
def test_rows_reach_the_paths_they_are_named_for():
    assert P.OP_PASS == 2097152 and P.UNET_PASS == 524288
    assert P.FLAT_N == (1, 63, 255, 256, 257, 65537, 2097152, 2097409) and 2097409 == 8192 * 256 + 257
    assert [P.op_blocks(n) for n in P.FLAT_N] == [1, 1, 1, 1, 2, 257, 8192, 8192]
    assert P.MAX_N == (1, 64, 255, 257, 65280, 65536, 65537, 2097152, 2097409)
    assert [P.op_blocks(n) for n in P.MAX_N] == [1, 1, 1, 2, 255, 256, 257, 8192, 8192]
    assert P.max_positions(1) == [0] and P.max_positions(64) == [0, 63] and P.max_positions(255) == [0, 63, 64, 254]
    assert P.max_positions(2097409) == [0, 63, 64, 2097408, 2097152]
    assert P.DIFF_SHAPES == ((1, 1, 1), (1, 1, 300), (1, 2, 1), (2, 2, 2), (1, 3, 1), (3, 5, 7), (300, 1, 1), (1, 300, 1), (3, 70, 5),
                             (2, 1025, 1031), (1, 2097409, 1))
    assert {s[1] for s in P.DIFF_SHAPES} >= {1, 2, 3} and all(o * n * i > P.OP_PASS for o, n, i in P.DIFF_LARGE)
    assert P.PLANE_SHAPES == ((1, 1, 1), (1, 1, 5), (1, 5, 1), (2, 2, 2), (3, 2, 3), (1, 3, 2), (2, 5, 6), (1, 170, 100), (3, 701, 999))
    assert 3 * 701 * 999 == 2100897 > P.OP_PASS and P.OP_PASS % (701 * 999) != 0 and 2 * 701 * 999 < P.OP_PASS
    assert P.SECTION_SHAPES == ((1, 1, 1, 1), (1, 1, 1, 4), (1, 2, 1, 4), (1, 1, 2, 8), (1, 2, 2, 2), (1, 3, 2, 5), (1, 2, 3, 12), (2, 3, 3, 8),
                                (2, 13, 10, 17), (1, 24, 16, 40), (1, 129, 127, 129), (1, 130, 128, 508))
    assert [s for s in P.SECTION_SHAPES if s[3] % 4 == 0] == [(1, 1, 1, 4), (1, 2, 1, 4), (1, 1, 2, 8), (1, 2, 3, 12), (2, 3, 3, 8), (1, 24, 16, 40),
                                                            (1, 130, 128, 508)]
    assert {s[1] for s in P.SECTION_SHAPES} >= {1, 2, 3} and {s[2] for s in P.SECTION_SHAPES} >= {1, 2, 3}
    assert 129 * 127 * 129 == 2113407 > P.OP_PASS and 129 % 4 == 1
    assert 130 * 128 * 508 // 4 == 2113280 > P.OP_PASS and 508 % 4 == 0
    assert all(np.prod(s) < 2 ** 31 for s in P.SECTION_SHAPES)
    assert P.POOL_SHAPES == ((1, 2, 2), (1, 2, 3), (1, 3, 2), (2, 3, 3), (3, 9, 12), (2, 5, 7), (1, 33, 35), (2, 64, 64), (2, 1451, 1453))
    assert (1451 // 2) * (1453 // 2) == 526350 > P.UNET_PASS and 1451 * 1453 == 2108303 > P.UNET_PASS
    assert [P.unet_blocks((h // 2) * (w // 2)) for _, h, w in P.POOL_SHAPES][-2:] == [4, 2048]
    assert P.DECONV_SHAPES == ((1, 1, 1, 1), (1, 1, 1, 2), (1, 1, 2, 1), (2, 3, 1, 5), (5, 3, 6, 7), (3, 2, 9, 11), (1, 1, 17, 16), (4, 5, 16, 17),
                               (1, 1, 363, 363), (1, 1, 725, 727))
    assert 4 * 363 * 363 == 527076 > P.UNET_PASS > 363 * 363 and 725 * 727 == 527075 > P.UNET_PASS
    assert P.deconv_bwd_weight_k(725, 727) == 2059 + 9 and P.deconv_bwd_weight_k(17, 16) == 2 + 9 and P.deconv_bwd_weight_k(16, 16) == 1 + 9
    assert len(P.DECONV_NULL_BIAS) == 3 and set(P.DECONV_NULL_BIAS) <= set(P.DECONV_SHAPES)


def test_max_workspace_extent():
    from deep_prior_interpolation_amd import _lib
    L = _lib.load()
    for n in P.MAX_N + P.FLAT_N:
        assert L.dpi_max_ws_floats(n) == max(1, min(-(-n // 256), 8192)) == P.op_blocks(n)


def test_special_dips_are_what_the_rows_say():
    """In float32: the first three special tensors give NaN, +inf, NaN ratios and 2/3, 2/3, NaN anisotropy; phi 0, +pi/2, 0."""
    vv, vh, hh = P.dips_inputs(63, 0)
    assert [tuple(float(t[i]) for t in (vv, vh, hh)) for i in range(6)] == [tuple(map(float, s)) for s in P.DIPS_SPECIAL]
    ratio, aniso = P.dips_np(vv, vh, hh)
    assert np.isnan(ratio[0]) and ratio[1] == np.inf and np.isnan(ratio[2])
    assert aniso[0] == aniso[1] == F(1.0) - F(1.0) / F(3.0) and np.isnan(aniso[2]) and abs(aniso[0] - 2.0 / 3.0) < 1e-7
    phi = P.phi_ref(ratio)
    assert phi[0] == 0.0 and phi[1] == np.pi / 2 and phi[2] == 0.0 and np.isfinite(phi).all()
    assert np.isnan(P.dips_np(*P.dips_inputs(1, 0))[0][0])
    rank1 = np.arange(63) % 2 == 0
    rank1[:6] = False
    with np.errstate(all="ignore"):
        det = vv.astype(np.float64) * hh - vh.astype(np.float64) ** 2
    assert (np.abs(det[rank1]) <= 1e-6 * vv[rank1] * hh[rank1] + 1e-30).all() and (det[~rank1][6:] > 1e-6).any()


# ---- derivatives -------------------------------------------------------------------------------------------------------------------------
def _oracle_diff(x, stencil, spacing):
    if stencil == 3:
        return O.second_derivative_np(x, spacing, axis=1)
    return O.first_derivative_np(x, spacing, axis=1, stencil=STENCILS[stencil])


@pytest.mark.parametrize("stencil", [0, 1, 2, 3])
def test_diff_axis_against_the_oracle_and_its_transpose(stencil):
    """Forward: within 4 fp32 roundings of the oracle in float64 (difference(s), the product with 2 or 0.5, the division, fp32(0.7)) on
    every small row; adjoint: the transposed dense matrix of the forward restatement, on the tiny rows."""
    for shape in P.DIFF_SHAPES[:9]:
        x = np.random.default_rng(sum(shape)).standard_normal(shape, dtype=F)
        got = P.diff_axis_np(x, stencil, P.DIFF_SPACING, 0)
        ref = _oracle_diff(x.astype(np.float64), stencil, P.DIFF_SPACING)
        scale = 4.0 * np.abs(x).max() / P.DIFF_SPACING ** (2 if stencil == 3 else 1)              # >= the sum of the terms' magnitudes
        assert got.shape == ref.shape and (np.abs(got - ref) <= 4 * P.U * scale).all(), (shape, stencil)
        if x.size <= 105:
            A = O.linear_operator_matrix(lambda e: P.diff_axis_np(e.astype(F), stencil, 1.0, 0), shape)
            g = np.random.default_rng(1).standard_normal(shape, dtype=F)
            adj = P.diff_axis_np(g, stencil, 1.0, 1)
            np.testing.assert_allclose(adj.reshape(-1), A.T @ g.reshape(-1).astype(np.float64), rtol=0, atol=1e-6)
            np.testing.assert_array_equal(P.diff_axis_np(g, stencil, P.DIFF_SPACING, 1),
                                          adj / (F(P.DIFF_SPACING) * F(P.DIFF_SPACING) if stencil == 3 else F(P.DIFF_SPACING)))


def test_diff_axis_recorded_vectors(golden):
    """The reference's own fp32 results (spacing 0.7, every axis of a 4-D tensor): the three first derivatives bit for bit — same
    operations, same roundings.  The second derivative's numerator bit for bit as well, but not its divisor: the reference divides by
    fp32(0.7 ** 2), the double product rounded once, the entry point receives fp32(0.7) and divides by its fp32 square (documented in
    include/dpi_hip.h).  The two divisors are one ulp apart here, the quotients at most 2."""
    d = golden("operators")["deriv"]
    x = d["x"]
    assert F(0.7) * F(0.7) != F(0.7 ** 2) and abs(float(F(0.7) * F(0.7)) - float(F(0.7 ** 2))) == np.spacing(F(0.49))
    for ax in range(4):
        outer, n, inner = int(np.prod(x.shape[:ax], dtype=np.int64)), x.shape[ax], int(np.prod(x.shape[ax + 1:], dtype=np.int64))
        x3 = x.reshape(outer, n, inner)
        for st in range(3):
            P.check_bits(P.diff_axis_np(x3, st, 0.7, 0).reshape(x.shape), d["first"]["ax%d" % ax][STENCILS[st]], "deriv ax%d %s" % (ax, STENCILS[st]))
        want = d["second"]["ax%d" % ax]
        P.check_bits((P.diff_axis_np(x3, 3, 1.0, 0) / F(0.7 ** 2)).reshape(x.shape), want, "second derivative ax%d, the reference's divisor" % ax)
        assert P.ulps(P.diff_axis_np(x3, 3, 0.7, 0).ravel(), want.ravel().astype(np.float64)).max() <= 2.0


# ---- Hale2D ------------------------------------------------------------------------------------------------------------------------------
def test_hale2d_against_the_oracle_the_recorded_vectors_and_its_transpose(golden):
    rng = np.random.default_rng(0)
    for shape in P.PLANE_SHAPES[:8]:
        x, theta = rng.standard_normal(shape), rng.uniform(-1.5, 1.5, shape)
        a, b, c = _theta_coef(theta)
        ref = O.hale2d_np(x[None], theta[None])[0]
        got = P.hale2d_np(x, a, b, c)
        S = P.hale2d_np(x, a, b, c, absolute=True)
        assert np.abs(got - ref).max() <= 1e-13 * (1.0 + S.max()) and (S >= np.abs(got) - 1e-12).all()
        P.check_bound(ref, got, S, 0, P.HALE_TERMS, "hale2d float64 %s" % (shape,))
        if x.size <= 60:
            n = x.size
            A = O.linear_operator_matrix(lambda e: P.hale2d_np(e, a, b, c), shape)
            Aabs = O.linear_operator_matrix(lambda e: P.hale2d_np(e, a, b, c, absolute=True), shape)
            g = rng.standard_normal(shape)
            np.testing.assert_allclose(P.hale2d_np(g, a, b, c, adjoint=True).reshape(n), A.T @ g.reshape(n), rtol=0, atol=1e-13 * (1 + np.abs(A).sum(0).max()))
            np.testing.assert_allclose(P.hale2d_np(g, a, b, c, adjoint=True, absolute=True).reshape(n), Aabs.T @ np.abs(g).reshape(n), rtol=1e-13, atol=1e-300)
            assert (Aabs >= np.abs(A) - 1e-14).all()
    for key in ("hale", "hale_c3"):
        h = golden("operators")[key]
        x, theta = h["x"][0].astype(np.float64), h["theta"][0].astype(np.float64)
        a, b, c = _theta_coef(theta)
        # the recorded result is the reference's fp32 evaluation (its own cos / sin in fp32: 2 more roundings per coefficient product)
        P.check_bound(h["y"][0], P.hale2d_np(x, a, b, c), P.hale2d_np(x, a, b, c, absolute=True), P.HALE_K + 4, P.HALE_TERMS, "recorded " + key)


def test_hale_sections_against_the_section_stacking_and_its_transpose():
    rng = np.random.default_rng(1)
    for shape in P.SECTION_SHAPES[:10]:
        z, ptx, pty = rng.standard_normal(shape), rng.uniform(-1.5, 1.5, shape), rng.uniform(-1.5, 1.5, shape)
        coef = np.stack(_theta_coef(ptx) + _theta_coef(pty))
        got = P.hale_sections_np(z, coef)
        ref = np.stack(sections_np(z, ptx, pty))
        S = P.hale_sections_np(z, coef, absolute=True)
        assert got.shape == ref.shape == (2,) + shape and np.abs(got - ref).max() <= 1e-13 * (1.0 + S.max())
        # S section by section as well: the same stacking applied to the 2-D absolute-value restatement
        S_tx = tx_unstack(P.hale_np(tx_stack(z), *(tx_stack(t) for t in coef[:3]), 2, 3, absolute=True))
        S_ty = ty_unstack(P.hale_np(ty_stack(z), *(ty_stack(t) for t in coef[3:]), 2, 3, absolute=True))
        np.testing.assert_allclose(S, np.stack([S_tx, S_ty]), rtol=1e-13, atol=0)
        n = z.size
        if n <= 40:
            A = O.linear_operator_matrix(lambda e: P.hale_sections_np(e, coef), shape)                      # [2 n][n]
            g = rng.standard_normal((2,) + shape)
            np.testing.assert_allclose(P.hale_sections_np(g, coef, adjoint=True).reshape(n), A.T @ g.reshape(2 * n), rtol=0, atol=1e-12)
            Aabs = O.linear_operator_matrix(lambda e: P.hale_sections_np(e, coef, absolute=True), shape)
            np.testing.assert_allclose(P.hale_sections_np(g, coef, adjoint=True, absolute=True).reshape(n), Aabs.T @ np.abs(g).reshape(2 * n), rtol=1e-13)


# ---- structure tensor and dips -----------------------------------------------------------------------------------------------------------
def test_structure_tensor_and_dips_against_the_oracle(golden):
    """The oracle's fp32 evaluation (the reference's own arithmetic): anisotropy bit for bit, phi within 4 ulp of the float64 atan of the
    restated ratio (numpy's fp32 arctan; phi_ref itself against math.atan); the recorded reference result likewise; the section tensors against the 2-D restatement on
    the section stacks, bit for bit."""
    rng = np.random.default_rng(2)
    for shape in P.PLANE_SHAPES[:8]:
        x = rng.standard_normal(shape, dtype=F)
        gvv, gvh, ghh = P.structure_tensor_np(x, P.TENSOR_DV, P.TENSOR_DH)
        ratio, aniso = P.dips_np(gvv, gvh, ghh)
        phi_o, aniso_o = O.structure_tensor_dips_np(x[None], P.TENSOR_DV, P.TENSOR_DH, dtype=F)
        P.check_bits(aniso, aniso_o[0], "anisotropy %s" % (shape,), nan_equal=True)
        assert P.ulps(phi_o[0].ravel(), P.phi_ref(ratio.ravel())).max() <= 4.0                      # numpy's SIMD fp32 arctan: a few ulp
        fin = np.isfinite(ratio.ravel())
        assert np.array_equal(P.phi_ref(ratio.ravel())[fin][:200], [math.atan(float(r)) for r in ratio.ravel()[fin][:200]]) or np.abs(
            P.phi_ref(ratio.ravel())[fin][:200] - [math.atan(float(r)) for r in ratio.ravel()[fin][:200]]).max() <= 2.3e-16
        phi64, _ = O.structure_tensor_dips_np(x[None].astype(np.float64), P.TENSOR_DV, P.TENSOR_DH)
        assert phi64.shape == (1,) + shape
    d = golden("operators")["dips"]
    ratio, aniso = P.dips_np(*P.structure_tensor_np(d["x"][0], 1.0, 1.0))
    # recorded by torch's vectorised CPU kernels, which do not round this chain like one scalar IEEE operation per step (the same torch
    # calls on a single element give the restatement's bits): l2 = t1 - t2 cancels on these rank-1 tensors, so a last-bit difference in
    # t2 is a few 2^-24 of l1 in l2, and that much in 1 - l2 / l1.  139 of the 140 recorded values agree bit for bit.
    rec = d["aniso0"][0]
    both = ~(np.isnan(aniso) | np.isnan(rec))
    assert np.array_equal(np.isnan(aniso), np.isnan(rec)) and np.abs(aniso[both].astype(np.float64) - rec[both]).max() <= 4 * P.U
    assert (P.bits(aniso)[both] == P.bits(rec)[both]).mean() > 0.99
    assert P.ulps(d["phi0"][0].ravel(), P.phi_ref(ratio.ravel())).max() <= 4.0                         # torch's fp32 atan
    dt, dx, dy = P.SECTION_SPACINGS
    for shape in P.SECTION_SHAPES[:10]:
        x = rng.standard_normal(shape, dtype=F)
        gtt, gtx, gxx, gty, gyy = P.structure_tensor_sections_np(x, dt, dx, dy)
        C, T, X, Y = shape
        a = [tx_unstack(t.reshape(C, Y, T, X)) for t in P.structure_tensor_np(tx_stack(x).reshape(C * Y, T, X), dt, dx)]
        b = [ty_unstack(t.reshape(C, X, T, Y)) for t in P.structure_tensor_np(ty_stack(x).reshape(C * X, T, Y), dt, dy)]
        for got, want, name in ((gtt, a[0], "gtt"), (gtx, a[1], "gtx"), (gxx, a[2], "gxx"), (gtt, b[0], "gtt (t,y)"), (gty, b[1], "gty"), (gyy, b[2], "gyy")):
            P.check_bits(got, np.ascontiguousarray(want), "%s %s" % (name, shape))


# ---- POCS --------------------------------------------------------------------------------------------------------------------------------
def test_pocs_restatements(golden):
    """The recorded reference vectors: the thresholded spectrum bit for bit, the threshold within 2 ulp (the reference rounds
    max * perc and the division by 100, dpi_scaled_max one product); the planted +th, -th and -0.0; a negative th doubles."""
    for tag in ("pocs_2d", "pocs_3d"):
        p = golden("operators")[tag]
        th = F(p["thresh"])
        assert float(th) == float(p["thresh"])
        P.check_bits(P.threshold_np(p["spec"], th), p["thresholded"], tag + " thresholded")
        assert P.ulps(P.scaled_max_np(p["spec"].ravel(), 0.05), [float(th)]).max() <= 2.0
        assert (p["thresholded"] == 0).any() and (p["thresholded"] != 0).any()
    for th in P.THRESHOLDS:
        x = P.threshold_inputs(257, th, 3)
        y = P.threshold_np(x, th)
        assert x[0] == F(th) and x[1] == -F(th) and np.signbit(x[2]) and x[2] == 0 and x[256] == F(th) and x[255] == -F(th)
        if th > 0:
            assert y[0] == 0 and y[1] == 0 and ((y == 0) | (y == x)).all() and (y == x).any()
        if th < 0:
            small = np.abs(x) < -th
            assert (y[small] == 2 * x[small]).all() and small.sum() > 10 and y[0] == x[0] and y[1] == x[1]       # x = |th|: only x > th holds
        if th == 0:
            assert np.array_equal(y[3:250], x[3:250]) and y[2] == 0 and np.signbit(y[2])
    x, d, m = (np.random.default_rng(k).standard_normal(300, dtype=F) for k in range(3))
    y = P.pocs_project_np(x, d, m)
    assert y.dtype == F and np.abs(y - (d.astype(np.float64) + m.astype(np.float64) * x)).max() <= 2 * P.U * (np.abs(d) + np.abs(m * x)).max()
    neg = -np.abs(x) - F(0.1)
    assert P.scaled_max_np(neg, 0.5)[0] == neg.max() * F(0.5) < 0
    neg[7] = -np.inf
    assert np.isfinite(P.scaled_max_np(neg, 0.5)[0])
    neg[9] = np.nan
    assert P.scaled_max_np(neg, 0.5)[0] == np.nanmax(neg) * F(0.5)                                               # fmaxf ignores a NaN


# ---- pool and transposed convolution -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ties", [False, True], ids=["random", "ties"])
def test_maxpool_against_torch(ties, golden):
    """torch.nn.functional.max_pool2d in float64 with autograd on every row but the largest: the value, and the gradient routed to the
    first maximum in scan order (aten's CPU backward); the recorded vector; the backward as the transposed selection matrix."""
    for shape in P.POOL_SHAPES[:8]:
        x, dy = P.pool_inputs(shape, ties, sum(shape))
        xt = torch.from_numpy(x).double().requires_grad_()
        yt = torch.nn.functional.max_pool2d(xt[None], 2, 2)[0]
        yt.backward(torch.from_numpy(dy).double())
        y, dx = P.maxpool_fwd_np(x), P.maxpool_bwd_np(dy, x)
        assert y.dtype == dx.dtype == F and y.shape == dy.shape and dx.shape == x.shape
        np.testing.assert_array_equal(y, yt.detach().numpy())
        np.testing.assert_array_equal(dx, xt.grad.numpy())
        assert not np.signbit(dx[dx == 0]).any()
        if ties:
            w = x[:, :2 * (shape[1] // 2), :2 * (shape[2] // 2)].reshape(shape[0], shape[1] // 2, 2, shape[2] // 2, 2)
            tied = ((w == w.max((2, 4), keepdims=True)).sum((2, 4)) > 1)
            assert tied[0, 0, 0] and (w[0, 0, :, 0, :] == 1).all() and (tied.mean() > 0.3 or tied.size < 50)
        if x.size <= 63:
            A = O.linear_operator_matrix(lambda e: P.maxpool_bwd_np(e.astype(F), x), dy.shape)               # dx = A dy: A^T selects
            np.testing.assert_array_equal(A.T @ x.reshape(-1).astype(np.float64), y.reshape(-1).astype(np.float64))
    g = golden("unet")["op_maxpool"]
    P.check_bits(P.maxpool_fwd_np(g["x"][0]), g["y"][0], "recorded max-pool")
    P.check_bits(P.maxpool_bwd_np(g["dy"][0], g["x"][0]), g["dx"][0], "recorded max-pool backward")


def test_deconv_against_torch(golden):
    """torch.nn.functional.conv_transpose2d(stride 2, padding 1) in float64 with autograd on every row but the two largest, with and
    without a bias; S against the same call on the magnitudes; the recorded vectors; backward-data and backward-weight are the
    transposes of the forward restatement by construction of autograd."""
    f = torch.nn.functional.conv_transpose2d
    for shape in P.DECONV_SHAPES[:8]:
        x, w, b, dy = P.deconv_inputs(shape, sum(shape))
        xt, wt, bt = (torch.from_numpy(t).double().requires_grad_() for t in (x, w, b))
        yt = f(xt[None], wt, bt, stride=2, padding=1)[0]
        yt.backward(torch.from_numpy(dy).double())
        for got, ref in ((P.deconv_fwd_np(x, w, b), yt.detach().numpy()), (P.deconv_bwd_data_np(dy, w), xt.grad.numpy()),
                         (P.deconv_bwd_weight_np(x, dy), wt.grad.numpy()),
                         (P.deconv_fwd_np(x, w, None), f(xt[None], wt, None, stride=2, padding=1)[0].detach().numpy()),
                         (P.deconv_fwd_np(x, w, b, absolute=True), f(xt[None].abs(), wt.abs(), bt.abs(), stride=2, padding=1)[0].detach().numpy())):
            assert got.shape == ref.shape, (shape, got.shape, ref.shape)
            np.testing.assert_allclose(got, ref, rtol=0, atol=1e-13 * (1.0 + np.abs(ref).max()))
        # the magnitudes of the two backward sums: autograd of the forward on magnitudes
        xa, wa = (torch.from_numpy(np.abs(t)).double().requires_grad_() for t in (x, w))
        f(xa[None], wa, None, stride=2, padding=1)[0].backward(torch.from_numpy(np.abs(dy)).double())
        np.testing.assert_allclose(P.deconv_bwd_data_np(dy, w, absolute=True), xa.grad.numpy(), rtol=1e-13, atol=1e-300)
        np.testing.assert_allclose(P.deconv_bwd_weight_np(x, dy, absolute=True), wa.grad.numpy(), rtol=1e-13, atol=1e-300)
    d = golden("unet")["op_deconv"]
    x, w, b, dy = d["x"][0], d["state"]["weight"], d["state"]["bias"], d["dy"][0]
    Cin, Cout, H, W = w.shape[0], w.shape[1], x.shape[1], x.shape[2]
    # recorded in fp32 by torch: the same number of terms, so the device bars apply to it as well
    P.check_bound(d["y"][0], P.deconv_fwd_np(x, w, b), P.deconv_fwd_np(x, w, b, absolute=True), P.deconv_fwd_k(Cin), 4 * Cin + 1, "recorded deconv")
    P.check_bound(d["dx"][0], P.deconv_bwd_data_np(dy, w), P.deconv_bwd_data_np(dy, w, absolute=True), P.deconv_bwd_data_k(Cout), 16 * Cout, "recorded dx")
    P.check_bound(d["grads"]["weight"], P.deconv_bwd_weight_np(x, dy), P.deconv_bwd_weight_np(x, dy, absolute=True), H * W, H * W, "recorded dw")


# ---- the checks catch the defects they exist for -----------------------------------------------------------------------------------------
def test_checks_catch_a_skipped_second_pass():
    """Elements >= 2097152 left NaN or stale: check_bits, check_written, check_bound and the maximum all notice."""
    n = P.FLAT_N[-1]
    x = P.threshold_inputs(n, 0.5, 1)
    want = P.threshold_np(x, 0.5)
    P.check_bits(want.copy(), want, "threshold"), P.check_written(want, "threshold")
    assert _fails(lambda: P.check_bits(P.drop_second_pass(want), want, "threshold"))
    assert _fails(lambda: P.check_written(P.drop_second_pass(want), "threshold"))
    assert _fails(lambda: P.check_bits(P.drop_second_pass(want, stale=x[P.OP_PASS:] + F(1.0)), want, "threshold"))
    ref = want.astype(np.float64)
    P.check_bound(want, ref, np.abs(ref), 1, 1, "as a float64 row")
    assert _fails(lambda: P.check_bound(P.drop_second_pass(want), ref, np.abs(ref), 1, 1, "as a float64 row"))
    assert _fails(lambda: P.check_bound(P.drop_second_pass(want, stale=F(0.0)), ref, np.abs(ref), 1, 1, "as a float64 row"))
    xm = P.max_inputs(n, P.OP_PASS, 2)
    assert P.scaled_max_np(xm, 0.5)[0] == 5.0
    assert _fails(lambda: P.check_bits(P.scaled_max_np(xm, 0.5, "no_second_pass"), P.scaled_max_np(xm, 0.5), "scaled_max"))
    vv, vh, hh = P.dips_inputs(n, 3)
    ratio, aniso = P.dips_np(vv, vh, hh)
    P.check_written(aniso, "anisotropy", nan_expected=np.isnan(aniso))
    assert _fails(lambda: P.check_bits(P.drop_second_pass(aniso), aniso, "anisotropy", nan_equal=True))
    assert _fails(lambda: P.check_written(P.drop_second_pass(aniso), "anisotropy", nan_expected=np.isnan(aniso)))
    assert _fails(lambda: P.check_written(np.where(np.isnan(aniso), F(0.0), aniso), "anisotropy", nan_expected=np.isnan(aniso)))
    phi = P.phi_ref(ratio).astype(F)
    assert P.check_phi(phi, ratio, 0.5, "phi") <= 0.5
    assert _fails(lambda: P.check_phi(P.drop_second_pass(phi), ratio, 4.0, "phi"))
    assert _fails(lambda: P.check_phi(np.nextafter(np.nextafter(phi, F(9.0)), F(9.0)), ratio, 1.4, "phi"))


def test_checks_catch_a_maximum_over_the_first_256_partials():
    caught = {}
    for n in P.MAX_N:
        for pos in P.max_positions(n):
            x = P.max_inputs(n, pos, n % 1000 + pos % 7)
            want = P.scaled_max_np(x, 0.5)
            assert want[0] == 5.0
            caught[(n, pos)] = _fails(lambda: P.check_bits(P.scaled_max_np(x, 0.5, "first_256_partials"), want, "scaled_max"))
    assert not any(v for (n, _), v in caught.items() if P.op_blocks(n) <= 256)
    assert caught[(65537, 65536)] and caught[(2097152, 2097151)] and not caught[(65537, 0)]
    assert not caught[(2097409, 2097408)]          # the second pass lands in block 1: that position is test_checks_catch_a_skipped_second_pass's


def test_checks_catch_the_pool_defects():
    """The last tap wins a tie (forward value through the zeros' signs, backward through the routing); the trailing odd row is left
    unwritten."""
    x, dy = P.pool_inputs((2, 5, 7), True, 5)
    P.check_bits(P.maxpool_fwd_np(x), P.maxpool_fwd_np(x), "pool")
    assert _fails(lambda: P.check_bits(P.maxpool_fwd_np(x, "last_tie"), P.maxpool_fwd_np(x), "pool forward"))
    assert _fails(lambda: P.check_bits(P.maxpool_bwd_np(dy, x, "last_tie"), P.maxpool_bwd_np(dy, x), "pool backward"))
    assert _fails(lambda: P.check_written(P.maxpool_bwd_np(dy, x, "odd_row_unwritten"), "pool backward"))
    assert _fails(lambda: P.check_bits(P.maxpool_bwd_np(dy, x, "odd_row_unwritten"), P.maxpool_bwd_np(dy, x), "pool backward"))
    xr, dyr = P.pool_inputs((2, 5, 7), False, 5)                         # without ties the tie rule cannot show: the tie rows are needed
    assert not _fails(lambda: P.check_bits(P.maxpool_bwd_np(dyr, xr, "last_tie"), P.maxpool_bwd_np(dyr, xr), "pool backward"))


def test_checks_catch_a_wrong_second_neighbour_guard():
    """`t <= T - 2` in place of `t <= T - 3`, on the rows with T = 2 and T = 3 (and, for contrast, not on T = 1 where t1 already excludes
    the neighbour)."""
    rng = np.random.default_rng(4)
    for shape, expect in (((1, 2, 1, 4), True), ((1, 3, 2, 5), True), ((2, 3, 3, 8), True)):
        x = rng.standard_normal(shape, dtype=F)
        coef = P.hale_coef(shape, rng, 2)
        ref, S = P.hale_sections_np(x, coef), P.hale_sections_np(x, coef, absolute=True)
        P.check_bound(ref.astype(F), ref, S, P.HALE_K, P.HALE_TERMS, "hale_sections")
        bad = P.hale_sections_np(x, coef, mutation="t_guard").astype(F)
        assert _fails(lambda: P.check_bound(bad, ref, S, P.HALE_K, P.HALE_TERMS, "hale_sections")) == expect, shape


def test_checks_catch_a_doubled_bias_and_a_weak_inequality():
    x, w, b, _ = P.deconv_inputs((5, 3, 6, 7), 6)
    ref, S = P.deconv_fwd_np(x, w, b), P.deconv_fwd_np(x, w, b, absolute=True)
    P.check_bound(ref.astype(F), ref, S, P.deconv_fwd_k(5), 21, "deconv")
    assert _fails(lambda: P.check_bound(P.deconv_fwd_np(x, w, b, mutation="bias_twice").astype(F), ref, S, P.deconv_fwd_k(5), 21, "deconv"))
    for th in (0.5, 0.0, -0.25):
        t = P.threshold_inputs(257, th, 7)
        differs = _fails(lambda: P.check_bits(P.threshold_np(t, th, "ge"), P.threshold_np(t, th), "threshold"))
        assert differs == (th != 0.0), th                                # at th = 0 both flags of x = +-0 change together: 0 * 2 = 0 * 0
