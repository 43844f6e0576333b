"""The anti-aliasing add-on on 3-D patches: the 2-D add-on (utils/slopes.py Hale2D + structure_tensor_dips) applied to the (t,x)
and the (t,y) sections of a (1,C,T,X,Y) patch (Hale2DSections, structure_tensor_dips_sections, dpi_hale_sections).
 (1) operator against the numpy oracle section by section, adjoint = transpose, dot-test, autograd;
 (2) dips against the oracle's estimator per section family (the acceptance rule of the 2-D dip test);
 (3) the same bits as the HIP 2-D path on the contiguous section stacks, and the two reductions of the regulariser to the 2-D add-on;
 (4-6) the regulariser in the loop (small patch, big patch on the eager side-stream path, bf16) and through the CLI."""
import os

import numpy as np
import pytest
import torch

from oracle import dpi_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"


def G(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float32))).to(DEV)


def N(t):
    return t.detach().cpu().numpy()


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm((a - b).ravel()) / (np.linalg.norm(b.ravel()) + 1e-30))


# (C,T,X,Y) <-> section stacks (C, Y, T, X) of the (t,x) family and (C, X, T, Y) of the (t,y) family, as BCHW with H = v = t
def tx_stack(a):
    return a.transpose(0, 3, 1, 2) if isinstance(a, np.ndarray) else a.permute(0, 3, 1, 2).contiguous()


def tx_unstack(a):
    return a.transpose(0, 2, 3, 1) if isinstance(a, np.ndarray) else a.permute(0, 2, 3, 1).contiguous()


def ty_stack(a):
    return a.transpose(0, 2, 1, 3) if isinstance(a, np.ndarray) else a.permute(0, 2, 1, 3).contiguous()


ty_unstack = ty_stack


def sections_np(z, phi_tx, phi_ty):
    """Oracle of Hale2DSections on (C,T,X,Y) arrays: hale2d_np on every section of both families."""
    return (tx_unstack(O.hale2d_np(tx_stack(z), tx_stack(phi_tx))), ty_unstack(O.hale2d_np(ty_stack(z), ty_stack(phi_ty))))


def _dips_agree(got, ref, aniso_ref, what):
    """tests/test_gpu_operators.py's rule: the angle is ill-conditioned where the tensor is nearly diagonal, so the well-conditioned
    samples agree tightly and nearly all samples agree."""
    d = np.abs(np.asarray(got, np.float64) - np.asarray(ref, np.float64))
    d = np.minimum(d, np.abs(d - np.pi))
    well = (np.abs(ref) > 1e-3) & np.isfinite(aniso_ref) & (np.abs(aniso_ref) > 1e-2)
    assert np.median(d[well]) < 1e-4 and np.percentile(d[well], 95) < 5e-3, what
    assert float(np.mean(d < 5e-3)) > 0.9, what


@pytest.mark.parametrize("shape", [(1, 2, 13, 10, 17), (1, 1, 24, 16, 40)])
def test_hale_sections_forward_adjoint_autograd(shape):
    from deep_prior_interpolation_amd import utils as u
    from deep_prior_interpolation_amd.operators import dottest
    rng = np.random.RandomState(sum(shape))
    z, ptx, pty = rng.randn(*shape), rng.randn(*shape), rng.randn(*shape)
    H = u.Hale2DSections(G(ptx), G(pty))
    assert tuple(H.dips.shape) == (2,) + shape[1:]
    y = N(H(G(z)))
    assert y.shape == (2,) + shape
    r0, r1 = sections_np(z[0], ptx[0], pty[0])
    for got, ref in ((y[0, 0], r0), (y[1, 0], r1)):
        np.testing.assert_allclose(got, ref, rtol=1e-4, atol=1e-5 * np.abs(ref).max())
    err_abs, err_rel = dottest(H, G(z), torch.empty((2,) + shape), verbose=False, generator=torch.Generator().manual_seed(1))
    assert err_rel < 1e-5
    # autograd: the gradient of loss(y0) + loss(y1) is the adjoint applied to the loss gradient
    x = G(z).requires_grad_(True)
    yy = H(x)
    w = torch.randn(yy.shape, device=DEV)
    loss = (w[0] * yy[0]).square().mean() + (w[1] * yy[1]).square().mean()
    loss.backward()
    gy = 2.0 * w * w * yy.detach() / yy[0].numel()
    np.testing.assert_allclose(N(x.grad), N(H.adjoint(gy)), rtol=1e-5, atol=1e-6 * float(x.grad.abs().max()))
    with pytest.raises(Exception):
        H(G(z[..., :-1]))


@pytest.mark.parametrize("shape", [(1, 2, 4, 3, 5), (1, 1, 3, 3, 8)])
def test_hale_sections_adjoint_is_transpose(shape):
    from deep_prior_interpolation_amd import utils as u
    rng = np.random.RandomState(7)
    ptx, pty = rng.randn(*shape), rng.randn(*shape)
    H = u.Hale2DSections(G(ptx), G(pty))
    A = O.linear_operator_matrix(lambda t: N(H.forward(G(t))), shape)
    At = O.linear_operator_matrix(lambda t: N(H.adjoint(G(t))), (2,) + shape)
    ref = O.linear_operator_matrix(lambda t: np.stack(sections_np(t[0], ptx[0], pty[0]))[:, None], shape)
    np.testing.assert_allclose(A, ref, atol=1e-5)
    np.testing.assert_allclose(At, A.T, atol=1e-6)


@pytest.mark.parametrize("smooth", [0.0, 1.5])
@pytest.mark.parametrize("shape", [(1, 2, 14, 10, 20), (1, 1, 13, 10, 17)])
def test_structure_tensor_dips_sections_oracle(shape, smooth):
    from deep_prior_interpolation_amd import utils as u
    rng = np.random.RandomState(5)
    x = rng.randn(*shape).astype(np.float32)
    ptx, pty = u.structure_tensor_dips_sections(G(x), smooth=smooth)
    for got, stack, unstack, fam in ((ptx, tx_stack, tx_unstack, "t-x"), (pty, ty_stack, ty_unstack, "t-y")):
        phi, an = O.structure_tensor_dips_np(stack(x[0]), smooth=smooth, dtype=np.float32)
        _dips_agree(N(got)[0], unstack(phi), unstack(an), "%s %s smooth %g" % (shape, fam, smooth))


@pytest.mark.parametrize("shape", [(1, 2, 14, 10, 20), (1, 1, 14, 10, 18)])
def test_sections_match_the_2d_path_bit_for_bit(shape):
    from deep_prior_interpolation_amd import utils as u
    rng = np.random.RandomState(11)
    z = G(rng.randn(*shape))
    ptx, pty = u.structure_tensor_dips_sections(z, smooth=2.0)
    p2tx, _ = u.structure_tensor_dips(tx_stack(z[0]), smooth=2.0)
    p2ty, _ = u.structure_tensor_dips(ty_stack(z[0]), smooth=2.0)
    assert float((tx_unstack(p2tx) - ptx[0]).abs().max()) <= 1e-6
    assert float((ty_unstack(p2ty) - pty[0]).abs().max()) <= 1e-6
    H = u.Hale2DSections(ptx, pty)
    Htx, Hty = u.Hale2D(p2tx), u.Hale2D(p2ty)
    y = H(z)
    assert rel(N(y[0, 0]), N(tx_unstack(Htx(tx_stack(z[0]))))) <= 1e-6
    assert rel(N(y[1, 0]), N(ty_unstack(Hty(ty_stack(z[0]))))) <= 1e-6
    g = torch.randn((2,) + shape, device=DEV)
    ref = tx_unstack(Htx.adjoint(tx_stack(g[0, 0]))) + ty_unstack(Hty.adjoint(ty_stack(g[1, 0])))
    assert rel(N(H.adjoint(g)[0]), N(ref)) <= 1e-6


def _reg_interpolator(loss="mae"):
    from deep_prior_interpolation_amd.main import Interpolator
    from deep_prior_interpolation_amd.parameter import parse_arguments
    return Interpolator(parse_arguments(["--imgdir", "x", "--datadim", "3d", "--aa_weight", "0.5", "--loss", loss, "--gpu", "0"]), "/tmp")


def _set_op(T, op, shape):
    T._aa_op = op
    T._aa_zero = torch.zeros(shape, device=DEV)
    T._aa_one = torch.ones(shape, device=DEV)


@pytest.mark.parametrize("loss", ["mae", "mse"])
def test_regulariser_reduces_to_the_2d_addon(loss):
    """Output constant along y with phi_ty = 0: L_ty vanishes and the value is the 2-D add-on on the (t,x) stack.  A (T,X,1)
    volume with estimated dips: the 2-D add-on on its one (t,x) section (b_ty is 0 or below 5e-8 there)."""
    from deep_prior_interpolation_amd import utils as u
    rng = np.random.RandomState(2)
    C, T_, X, Y = 2, 12, 10, 9
    out = G(np.broadcast_to(rng.randn(1, C, T_, X, 1), (1, C, T_, X, Y)))
    ptx = G(rng.randn(1, C, T_, X, Y))
    T3, T2 = _reg_interpolator(loss), _reg_interpolator(loss)
    _set_op(T3, u.Hale2DSections(ptx, torch.zeros_like(ptx)), (2, 1, C, T_, X, Y))
    _set_op(T2, u.Hale2D(tx_stack(ptx[0])), (C, Y, T_, X))
    w3, r3 = T3.regularization(out, None)
    w2, r2 = T2.regularization(tx_stack(out[0]), None)
    assert w3 == w2 == 0.5 and abs(r3.item() - r2.item()) <= 1e-6 * abs(r2.item())
    # (T, X, 1): estimated dips, default smoothing (an even kernel along the (t,y) sections)
    vol = G(rng.randn(1, 1, 16, 12, 1))
    ptx, pty = u.structure_tensor_dips_sections(vol, smooth=2.0)
    p2, _ = u.structure_tensor_dips(vol[..., 0], smooth=2.0)
    assert float((ptx[..., 0] - p2).abs().max()) <= 1e-6
    b_ty = (-torch.cos(pty) * torch.sin(pty)).abs()
    assert float(b_ty.max()) < 5e-8
    _set_op(T3, u.Hale2DSections(ptx, pty), (2,) + tuple(vol.shape))
    _set_op(T2, u.Hale2D(p2), tuple(p2.shape))
    r3, r2 = T3.regularization(vol, None)[1], T2.regularization(vol[..., 0].contiguous(), None)[1]
    assert abs(r3.item() - r2.item()) <= 1e-6 * abs(r2.item())


def _interp3d(extra, epochs, shape, precision=None, seed=0):
    from deep_prior_interpolation_amd.main import Interpolator
    from deep_prior_interpolation_amd.parameter import parse_arguments
    from deep_prior_interpolation_amd import utils as u
    argv = ["--imgdir", "x", "--datadim", "3d", "--filters", "4", "8", "16", "--skip", "4", "8", "--inputdepth", "8",
            "--upsample", "linear", "--epochs", str(epochs), "--gpu", "0"] + extra + (["--precision", precision] if precision else [])
    a = parse_arguments(argv)
    vol = u.hyperbolic_volume(shape, seed=3)[..., None].astype(np.float64) * 10.0
    mask = u.random_trace_mask(shape, 0.5, seed=4)[..., None].astype(np.float64)
    u.set_seed(seed)
    T = Interpolator(a, "/tmp")
    T.load_data({"image": vol, "mask": np.broadcast_to(mask, vol.shape).copy(), "name": "0"})
    T.build_model()
    T.build_input()
    T.build_regularizer()
    return T


def _check_iteration0(T, w, loss="mae", rtol=1e-4):
    out0 = np.asarray(T.out_best, dtype=np.float64)[None, None, ..., 0] if np.ndim(T.out_best) == 4 else \
        np.asarray(T.out_best, dtype=np.float64)[None, None]
    d = T._aa_op.dips.cpu().numpy().astype(np.float64)
    r0, r1 = sections_np(out0[0], d[0], d[1])
    f = (lambda v: np.abs(v).mean()) if loss == "mae" else (lambda v: np.square(v).mean())
    reg_ref = f(r0) + f(r1)
    h = T.history
    assert abs(h.reg[0] - reg_ref) < rtol * reg_ref + 1e-9, (h.reg[0], reg_ref)
    assert abs(h.loss[0] - (h.df[0] + w * h.reg[0])) < 1e-6 * abs(h.loss[0])


def test_addon_in_the_loop_small_patch():
    from deep_prior_interpolation_amd import utils as u
    shape = (16, 12, 20)
    T = _interp3d(["--aa_weight", "0.5", "--aa_smooth", "2"], 1, shape)
    assert isinstance(T.history, u.HistoryReg) and not T.graph_capable()
    assert tuple(T._aa_op.dips.shape) == (2, 1) + shape
    T.optimize(verbose=False)
    _check_iteration0(T, 0.5)
    T = _interp3d(["--aa_weight", "0.5", "--aa_smooth", "2", "--loss", "mse"], 1, shape)
    T.optimize(verbose=False)
    _check_iteration0(T, 0.5, loss="mse")
    T = _interp3d(["--aa_weight", "0.5", "--aa_smooth", "2"], 30, shape)
    T.optimize(verbose=False)
    h = T.history
    assert len(h) == 30 and np.isfinite(h.loss).all() and h.loss[-1] < 0.7 * h.loss[0] and h.reg[-1] < h.reg[0]
    T0 = _interp3d([], 30, shape)
    T0.optimize(verbose=False, mode="eager")
    assert abs(T0.history.loss[5] - h.df[5]) > 1e-6 * abs(h.df[5])


@pytest.mark.parametrize("precision", [None, "bf16"])
def test_addon_in_the_loop_big_patch(precision):
    """>= 2^20 voxels: the eager path with the weight-gradient side streams (finish_backward's adoption check runs every step)."""
    from deep_prior_interpolation_amd import ops
    T = _interp3d(["--aa_weight", "0.5", "--aa_smooth", "2"], 3, (128, 128, 64), precision=precision)
    assert T.wants_weight_grad_overlap() and not T.graph_capable()
    T.optimize(verbose=False)
    assert ops.sched.deferred == []
    h = T.history
    assert len(h) == 3 and np.isfinite(h.loss).all() and np.isfinite(h.reg).all()
    # iteration 0 alone again to read its output (optimize keeps the best one)
    T1 = _interp3d(["--aa_weight", "0.5", "--aa_smooth", "2"], 1, (128, 128, 64), precision=precision)
    T1.optimize(verbose=False)
    _check_iteration0(T1, 0.5)


def test_addon_through_the_cli(tmp_path, monkeypatch):
    from deep_prior_interpolation_amd import main as M, utils as u
    monkeypatch.chdir(tmp_path)
    shape = (16, 16, 32)
    np.save("vol.npy", u.hyperbolic_volume(shape, seed=1).astype(np.float32))
    np.save("mask.npy", np.broadcast_to(u.random_trace_mask(shape, 0.5, seed=2), shape).astype(np.float32))
    base = ["--imgdir", str(tmp_path), "--imgname", "vol.npy", "--maskname", "mask.npy", "--datadim", "3d", "--patch_shape", "16", "16", "16",
            "--filters", "4", "8", "--skip", "4", "--inputdepth", "4", "--upsample", "linear", "--epochs", "4", "--gpu", "0", "--gain", "10",
            "--aa_weight", "0.25"]
    M.main(base + ["--outdir", "aa"])
    for name in ("0", "1"):
        r = np.load(os.path.join("results", "aa", name + "_run.npy"), allow_pickle=True).item()
        h = r["history"]
        assert isinstance(h, u.HistoryReg) and len(h) == 4 and np.isfinite(h.reg).all() and r["output"].shape == (16, 16, 16)
    np.save("dips.npy", np.zeros(16 * 16 * 16, np.float32))                # one family only: the wrong size
    with pytest.raises(ValueError, match="2\\*C\\*T\\*X\\*Y"):
        M.main(base + ["--outdir", "aa_bad", "--aa_dips", str(tmp_path / "dips.npy")])
