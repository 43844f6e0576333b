"""The 3-D plain UNet on the GPU: the six entry points of csrc/unet3d_ops.hip through the C ABI (every buffer inside guard bands, outputs
NaN-filled, tensors also as views one element off a 256-byte boundary), UNet3D against a float64 torch restatement of the same tree, and the
Interpolator with `--datadim 3d --net unet --upsample deconv` end to end.  The reference has no 3-D UNet: every expectation here is torch on
the CPU in float64, built in this file.

Bars.  Pool: bit equality.  Transposed convolution: |got - ref| <= 2 n 2^-24 S, with ref the float64 result, S the same sum over absolute
values and n the number of terms behind an element (forward 8 Cin + 1, backward-data 64 Cout, backward-weight D H W): every fp32 summation
order of n terms stays inside (n - 1) 2^-24 S to first order, so the bar holds for the MFMA path, the VALU path and the chunked
backward-weight alike.  Net: the bars of test_gpu_nets.test_unet_golden (output 1e-4, input gradient 2e-4, parameter gradients 5e-4, and
its rule for the analytically-zero biases in front of an instance norm)."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as TF
from torch import nn

from gpu_guard import guard
from test_gpu_conv_contract import _check_guards, _launch

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = torch.float32
E_ARG = -1
EPS = 2.0 ** -24

POOL_SHAPES = [(1, 2, 2, 2), (3, 5, 6, 7), (2, 4, 4, 130)]
# the last row: the MFMA path with two workgroup tiles along H and along W, each a partial tile (1 row, 1 column) behind a full one
DECONV_SHAPES = [(1, 1, 1, 1, 1), (3, 2, 2, 3, 5), (17, 5, 3, 2, 2), (16, 16, 2, 2, 2), (32, 16, 4, 4, 8), (256, 128, 1, 1, 2), (16, 16, 2, 9, 17)]


@pytest.fixture(scope="module")
def lib():
    from deep_prior_interpolation_amd import _lib
    return _lib


def gin(a, offset=0):
    a = np.ascontiguousarray(a, dtype=np.float32)
    return guard(a.size, F32, DEV, fill=torch.from_numpy(a.reshape(-1)), offset=offset)


def gout(n, offset=0):
    return guard(int(n), F32, DEV, offset=offset)


def ptr(g):
    return None if g is None else g.payload.data_ptr()


def host(g, shape):
    return g.payload.cpu().numpy().reshape(shape)


def run(lib, what, call, ins, outs):
    """One launch: it succeeds, no band changed, no input changed."""
    ins = [(k, g) for k, g in ins if g is not None]
    before = [g.bits() for _, g in ins]
    _launch(lib, call(), what)
    _check_guards(ins + list(outs), what)
    for (k, g), b in zip(ins, before):
        assert g.untouched(b), "%s: the input %s was written" % (what, k)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


# ---- the pool ----------------------------------------------------------------------------------------------------------------------------
def pool_np(x, dy=None):
    """The stated rule: scan (kd, kh, kw), a later tap replaces the running maximum only if it is greater.  Returns y, or dx for a dy."""
    C, D, H, W = x.shape
    Do, Ho, Wo = D // 2, H // 2, W // 2
    win = np.stack([x[:, kd:2 * Do:2, kh:2 * Ho:2, kw:2 * Wo:2] for kd in (0, 1) for kh in (0, 1) for kw in (0, 1)])
    m, arg = win[0].copy(), np.zeros(win[0].shape, np.int64)
    for t in range(1, 8):
        take = win[t] > m
        m, arg = np.where(take, win[t], m), np.where(take, t, arg)
    if dy is None:
        return m
    dx = np.zeros_like(x)
    for t in range(8):
        kd, kh, kw = t >> 2, (t >> 1) & 1, t & 1
        dx[:, kd:2 * Do:2, kh:2 * Ho:2, kw:2 * Wo:2] = np.where(arg == t, dy, np.float32(0))
    return dx


def pool_torch(x, dy):
    xt = torch.from_numpy(x)[None].requires_grad_(True)
    y = TF.max_pool3d(xt, 2, 2)
    y.backward(torch.from_numpy(dy)[None])
    return y.detach().numpy()[0], xt.grad.numpy()[0]


def _pool_case(lib, x, dy, what, want):
    L = lib.load()
    C, D, H, W = x.shape
    for off in (0, 1):
        xg, dyg, yg, dxg = gin(x, off), gin(dy, off), gout(dy.size, off), gout(x.size, off)
        run(lib, what + " forward", lambda: L.dpi_maxpool2x2x2_fwd(ptr(xg), C, D, H, W, ptr(yg), lib.stream()), [("x", xg)], [("y", yg)])
        assert np.array_equal(bits(host(yg, dy.shape)), bits(want[0])), what + " y (offset %d)" % off
        run(lib, what + " backward", lambda: L.dpi_maxpool2x2x2_bwd(ptr(dyg), ptr(xg), C, D, H, W, ptr(dxg), lib.stream()),
            [("dy", dyg), ("x", xg)], [("dx", dxg)])
        got = host(dxg, x.shape)                                   # the buffer was NaN: every element must have been written
        assert not np.isnan(got).any() or np.isnan(dy).any(), what + ": dx not fully written"
        assert np.array_equal(bits(got), bits(want[1])), what + " dx (offset %d)" % off


@pytest.mark.parametrize("shape", POOL_SHAPES, ids=str)
def test_pool_matches_torch_bit_for_bit(lib, shape):
    rng = np.random.default_rng(sum(shape))
    C, D, H, W = shape
    dy = rng.standard_normal((C, D // 2, H // 2, W // 2)).astype(np.float32)
    for kind in ("random", "ties", "constant"):
        x = {"random": lambda: rng.standard_normal(shape), "ties": lambda: rng.choice([-1.0, -0.0, 0.0, 1.0], size=shape),
             "constant": lambda: np.full(shape, 0.75)}[kind]().astype(np.float32)
        want = pool_torch(x, dy)
        assert np.array_equal(bits(pool_np(x)), bits(want[0])) and np.array_equal(bits(pool_np(x, dy)), bits(want[1]))    # the restatement is aten's rule
        _pool_case(lib, x, dy, "maxpool3d %s %s" % (shape, kind), want)


def test_pool_signed_zero_and_nan(lib):
    """One window per case.  0.0 / -0.0: equal, so tap (0,0,0) is returned with its own sign and receives dy.  NaN: no comparison with
    it is true, so a NaN at tap (0,0,0) stays the maximum and a NaN elsewhere is never selected (the library's rule, as in 2-D)."""
    dy = np.full((1, 1, 1, 1), 3.0, np.float32)
    z = np.array([-0.0, 0.0, 0.0, -0.0, 0.0, 0.0, -0.0, 0.0], np.float32).reshape(1, 2, 2, 2)
    _pool_case(lib, z, dy, "maxpool3d -0.0 first", pool_torch(z, dy))
    assert np.signbit(pool_np(z)).all() and pool_np(z, dy).reshape(-1)[0] == 3.0
    _pool_case(lib, -z, dy, "maxpool3d 0.0 first", pool_torch(-z, dy))
    base = np.array([0.5, 2.0, -1.0, 1.5, 0.25, -3.0, 1.0, 0.0], np.float32)
    for pos in (0, 5):
        x = base.copy()
        x[pos] = np.nan
        x = x.reshape(1, 2, 2, 2)
        want = (pool_np(x), pool_np(x, dy))
        assert np.isnan(want[0]).all() == (pos == 0) and want[1].reshape(-1)[0 if pos == 0 else 1] == 3.0
        _pool_case(lib, x, dy, "maxpool3d NaN at tap %d" % pos, want)


# ---- the transposed convolution ----------------------------------------------------------------------------------------------------------
def deconv_problem(shape, seed):
    Cin, Cout, D, H, W = shape
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((Cin, D, H, W)).astype(np.float32)
    w = (rng.standard_normal((Cin, Cout, 4, 4, 4)) / np.sqrt(8 * Cin)).astype(np.float32)
    b = rng.standard_normal(Cout).astype(np.float32)
    dy = rng.standard_normal((Cout, 2 * D, 2 * H, 2 * W)).astype(np.float32)
    return x, w, b, dy


def deconv_ref(x, w, b, dy, absolute=False):
    """float64 y, dx, dw of conv_transpose3d (autograd); absolute: the same sums over absolute values."""
    f = (lambda a: torch.from_numpy(a).double().abs()) if absolute else (lambda a: torch.from_numpy(a).double())
    xt, wt = f(x)[None].requires_grad_(True), f(w).requires_grad_(True)
    y = TF.conv_transpose3d(xt, wt, None if b is None else f(b), stride=2, padding=1)
    y.backward(f(dy)[None])
    return y.detach().numpy()[0], xt.grad.numpy()[0], wt.grad.numpy()


def check_bound(got, ref, S, n, what):
    assert got.shape == ref.shape and np.isfinite(got).all(), what + ": shape or unwritten / non-finite elements"
    bound = 2.0 * n * EPS * S
    err = np.abs(got.astype(np.float64) - ref)
    ratio = float(np.max(err / np.maximum(bound, 1e-300)))
    print("%s: worst |err| / (2 n 2^-24 S) = %.3g (n = %d)" % (what, ratio, n))
    assert ratio <= 1.0, "%s: %.3g of its bound" % (what, ratio)
    return ratio


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "offset1"])
@pytest.mark.parametrize("shape", DECONV_SHAPES, ids=str)
def test_deconv_against_float64(lib, shape, offset):
    L = lib.load()
    Cin, Cout, D, H, W = shape
    x, w, b, dy = deconv_problem(shape, sum(shape))
    xg, wg, bg, dyg = gin(x, offset), gin(w, offset), gin(b, offset), gin(dy, offset)
    for bias, bgd in ((b, bg), (None, None)):
        ref, S = deconv_ref(x, w, bias, dy), deconv_ref(x, w, bias, dy, absolute=True)
        what = "deconv3d_fwd %s%s" % (shape, "" if bias is not None else " bias NULL")
        yg = gout(dy.size, offset)
        run(lib, what, lambda: L.dpi_deconv4x4x4s2_fwd(ptr(xg), ptr(wg), ptr(bgd), Cin, Cout, D, H, W, ptr(yg), lib.stream()),
            [("x", xg), ("w", wg), ("bias", bgd)], [("y", yg)])
        check_bound(host(yg, dy.shape), ref[0], S[0], 8 * Cin + 1, what)
    what = "deconv3d_bwd_data %s" % (shape,)
    dxg = gout(x.size, offset)
    run(lib, what, lambda: L.dpi_deconv4x4x4s2_bwd_data(ptr(dyg), ptr(wg), Cin, Cout, D, H, W, ptr(dxg), lib.stream()), [("dy", dyg), ("w", wg)], [("dx", dxg)])
    check_bound(host(dxg, x.shape), ref[1], S[1], 64 * Cout, what)
    what = "deconv3d_bwd_weight %s" % (shape,)
    n_ws = int(L.dpi_deconv4x4x4s2_bwd_weight_ws_floats(Cin, Cout, D, H, W))
    assert n_ws > 0
    twice = []
    for _ in range(2):
        dwg, wsg = gout(w.size, offset), gout(n_ws, offset)
        run(lib, what, lambda: L.dpi_deconv4x4x4s2_bwd_weight(ptr(xg), ptr(dyg), Cin, Cout, D, H, W, ptr(dwg), ptr(wsg), lib.stream()),
            [("x", xg), ("dy", dyg)], [("dw", dwg), ("ws", wsg)])
        twice.append(host(dwg, w.shape))
    check_bound(twice[0], ref[2], S[2], D * H * W, what)
    assert np.array_equal(bits(twice[0]), bits(twice[1])), what + ": two launches differ"


@pytest.mark.parametrize("shape", [(3, 2, 2, 3, 5), (32, 16, 4, 4, 8), (16, 16, 2, 9, 17)], ids=str)
def test_deconv_dot_test(lib, shape):
    """<A x, y> = <x, A^T y> with A the forward without bias and A^T backward-data, both from the device, the products summed in float64;
    the difference relative to the value of the product, 1e-5."""
    L = lib.load()
    Cin, Cout, D, H, W = shape
    x, w, _, y = deconv_problem(shape, 99)
    xg, wg, yg, Axg, Atyg = gin(x), gin(w), gin(y), gout(y.size), gout(x.size)
    run(lib, "dot fwd", lambda: L.dpi_deconv4x4x4s2_fwd(ptr(xg), ptr(wg), None, Cin, Cout, D, H, W, ptr(Axg), lib.stream()), [("x", xg), ("w", wg)], [("Ax", Axg)])
    run(lib, "dot bwd", lambda: L.dpi_deconv4x4x4s2_bwd_data(ptr(yg), ptr(wg), Cin, Cout, D, H, W, ptr(Atyg), lib.stream()), [("y", yg), ("w", wg)], [("Aty", Atyg)])
    lhs = float(np.sum(host(Axg, y.shape).astype(np.float64) * y))
    rhs = float(np.sum(host(Atyg, x.shape).astype(np.float64) * x))
    print("dot test %s: %.9g vs %.9g (relative difference %.2e)" % (shape, lhs, rhs, abs(lhs - rhs) / abs(lhs)))
    assert abs(lhs - rhs) <= 1e-5 * abs(lhs)


def test_refusals(lib):
    """Every call returns DPI_E_ARG and leaves the output payloads' bits alone: refused on the host before any launch, with valid buffers
    behind every non-NULL pointer.  NULL in every pointer position (bias excepted), in == out, a zero and a negative extent, D = 1 for
    the pool, and element counts past the index range by the dimensions alone."""
    L = lib.load()
    s = lib.stream()
    a = [gin(np.arange(1, 513, dtype=np.float32)) for _ in range(3)]
    o = [gout(512) for _ in range(2)]
    A, O_ = [ptr(t) for t in a], [ptr(t) for t in o]
    before = [t.bits() for t in o]
    table = [
        (L.dpi_maxpool2x2x2_fwd, "maxpool3d_fwd", [A[0], 1, 2, 2, 2, O_[0]], (0, 5), (1, 2, 3, 4)),
        (L.dpi_maxpool2x2x2_bwd, "maxpool3d_bwd", [A[0], A[1], 1, 2, 2, 2, O_[0]], (0, 1, 6), (2, 3, 4, 5)),
        (L.dpi_deconv4x4x4s2_fwd, "deconv3d_fwd", [A[0], A[1], A[2], 1, 1, 1, 2, 2, O_[0]], (0, 1, 8), (3, 4, 5, 6, 7)),
        (L.dpi_deconv4x4x4s2_bwd_data, "deconv3d_bwd_data", [A[0], A[1], 1, 1, 1, 2, 2, O_[0]], (0, 1, 7), (2, 3, 4, 5, 6)),
        (L.dpi_deconv4x4x4s2_bwd_weight, "deconv3d_bwd_weight", [A[0], A[1], 1, 1, 1, 2, 2, O_[0], O_[1]], (0, 1, 7, 8), (2, 3, 4, 5, 6)),
    ]
    calls = []
    for fn, prefix, args, ptrs, ints in table:
        for i in ptrs:
            calls.append((fn, prefix, args[:i] + [None] + args[i + 1:], "NULL in position %d" % i))
        out_pos = ptrs[-2] if prefix == "deconv3d_bwd_weight" else ptrs[-1]
        calls.append((fn, prefix, args[:out_pos] + [args[0]] + args[out_pos + 1:], "in == out"))
        for i in ints:
            for v in (0, -3):
                calls.append((fn, prefix, args[:i] + [v] + args[i + 1:], "extent %d in position %d" % (v, i)))
        big = list(args)
        big[ints[-1]], big[ints[-2]], big[ints[-3]] = 1 << 11, 1 << 11, 1 << 10                       # 2^32 voxels
        calls.append((fn, prefix, big, "2^32 voxels"))
    calls.append((L.dpi_maxpool2x2x2_fwd, "maxpool3d_fwd", [A[0], 1, 1, 2, 2, O_[0]], "D = 1"))
    calls.append((L.dpi_deconv4x4x4s2_fwd, "deconv3d_fwd", [A[0], A[1], None, 1, 1 << 12, 1 << 6, 1 << 6, 1 << 6, O_[0]], "Cout * 8 V = 2^33"))
    calls.append((L.dpi_deconv4x4x4s2_bwd_weight, "deconv3d_bwd_weight", [A[0], A[1], 1 << 13, 1 << 13, 1, 1, 1, O_[0], O_[1]], "64 Cin Cout = 2^32"))
    assert L.dpi_deconv4x4x4s2_bwd_weight_ws_floats(0, 1, 1, 1, 1) == 0 and L.dpi_deconv4x4x4s2_bwd_weight_ws_floats(16, 16, 1 << 11, 1 << 11, 1 << 10) == 0
    for fn, prefix, args, why in calls:
        rc = fn(*args, s)
        assert rc == E_ARG, "%s (%s) returned %d" % (prefix, why, rc)
        assert L.dpi_last_error().decode().startswith(prefix), (prefix, why, L.dpi_last_error())
    torch.cuda.synchronize()
    for t, bts in zip(o, before):
        t.check("refusals")
        assert t.untouched(bts)
    for t in a:
        t.check("refusals")


# ---- the net against a float64 restatement -----------------------------------------------------------------------------------------------
class _Conv(nn.Module):
    def __init__(self, cin, cout, norm, act):
        super().__init__()
        self.conv1 = self._block(cin, cout, norm, act)
        self.conv2 = self._block(cout, cout, norm, act)

    @staticmethod
    def _block(a, b, norm, act):
        return nn.Sequential(nn.Sequential(nn.Conv3d(a, b, 3, padding=1)), *([nn.InstanceNorm3d(b)] if norm else []), act)

    def forward(self, x):
        return self.conv2(self.conv1(x))


class _Down(nn.Module):
    def __init__(self, cin, cout, act):
        super().__init__()
        self.conv, self.down = _Conv(cin, cout, True, act), nn.MaxPool3d(2, 2)

    def forward(self, x):
        return self.conv(self.down(x))


class _Up(nn.Module):
    def __init__(self, cin, cout, mode, act):
        super().__init__()
        self.up = (nn.ConvTranspose3d(cin, cout, 4, stride=2, padding=1) if mode == "deconv" else
                   nn.Sequential(nn.Upsample(scale_factor=2, mode=mode), nn.Sequential(nn.Conv3d(cin, cout, 3, padding=1))))
        self.conv = _Conv(2 * cout, cout, False, act)

    def forward(self, deep, skip):
        return self.conv(torch.cat([self.up(deep), skip], 1))


class TorchUNet3D(nn.Module):
    """The tree of architectures/unet.py:UNet3D in plain torch modules with the same child names (ReLU, instance norm, bias everywhere)."""

    def __init__(self, cin, cout, f, mode):
        super().__init__()
        act = nn.ReLU()
        self.start = _Conv(cin, f[0], True, act)
        for i in range(1, 5):
            setattr(self, "down%d" % i, _Down(f[i - 1], f[i], act))
        for i in range(4, 0, -1):
            setattr(self, "up%d" % i, _Up(f[i], f[i - 1], mode, act))
        self.final = nn.Sequential(nn.Conv3d(f[0], cout, 1))

    def forward(self, x):
        s0 = self.start(x)
        d1 = self.down1(s0)
        d2 = self.down2(d1)
        d3 = self.down3(d2)
        d4 = self.down4(d3)
        return self.final(self.up1(self.up2(self.up3(self.up4(d4, d3), d2), d1), s0))


def zero_bias(k):
    """Biases of convolutions that feed an instance norm: their gradient is analytically zero (test_unet_golden's rule)."""
    return k.endswith("bias") and k.split(".")[0] in ("start", "down1", "down2", "down3", "down4")


_REF = {}


def reference_run(cin, f, mode, shape, dtype=torch.float64):
    """State, input, target, output, MSE loss and every gradient of the restatement; computed once per case and shared."""
    key = (cin, tuple(f), mode, tuple(shape), dtype)
    if key not in _REF:
        torch.manual_seed(1234 + len(mode))
        m = TorchUNet3D(cin, 1, f, mode)
        state = {k: v.clone() for k, v in m.state_dict().items()}
        x = torch.randn(shape)
        t = torch.randn((1, 1) + tuple(shape[2:]))
        m = m.to(dtype)
        xd = x.to(dtype).requires_grad_(True)
        y = m(xd)
        loss = TF.mse_loss(y, t.to(dtype))
        loss.backward()
        _REF[key] = dict(state=state, x=x, t=t, y=y.detach(), loss=float(loss.detach()), dx=xd.grad, grads={k: p.grad for k, p in m.named_parameters()})
    return _REF[key]


def rel(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    assert a.shape == b.shape, (a.shape, b.shape)
    return float((a - b).norm() / (b.norm() + 1e-30))


NET_CASES = [(4, [2, 4, 8, 16, 32], "deconv", (1, 4, 32, 16, 16)), (4, [2, 4, 8, 16, 32], "trilinear", (1, 4, 32, 16, 16)),
             (4, [2, 4, 8, 16, 32], "nearest", (1, 4, 32, 16, 16)), (8, [16, 16, 32, 32, 32], "deconv", (1, 8, 32, 16, 16))]


@pytest.mark.parametrize("cin,f,mode,shape", NET_CASES, ids=["narrow-deconv", "narrow-trilinear", "narrow-nearest", "mfma-deconv"])
def test_net_against_float64(cin, f, mode, shape):
    """One forward and backward under an MSE loss.  The last case has widths of multiples of 16: its transposed convolutions run on MFMA."""
    from deep_prior_interpolation_amd.architectures import UNet3D
    g = reference_run(cin, f, mode, shape)
    m = UNet3D(cin, 1, f, mode)
    assert list(m.state_dict()) == list(g["state"])
    m.load_state_dict(g["state"])
    m = m.to(DEV)
    x = g["x"].to(DEV).requires_grad_(True)
    y = m(x)
    loss = TF.mse_loss(y, g["t"].to(DEV))
    loss.backward()
    print("UNet3D %s %s: y %.2e, dx %.2e" % (f, mode, rel(y, g["y"]), rel(x.grad, g["dx"])))
    assert rel(y, g["y"]) < 1e-4
    assert rel(x.grad, g["dx"]) < 2e-4
    worst = 0.0
    for k, p in m.named_parameters():
        if zero_bias(k):
            wg = float(g["grads"][k[:-4] + "weight"].abs().max())
            assert float(p.grad.abs().max()) < 1e-3 * wg + 1e-6, k
        else:
            worst = max(worst, rel(p.grad, g["grads"][k]))
            assert rel(p.grad, g["grads"][k]) < 5e-4, k
    print("UNet3D %s %s: worst parameter gradient %.2e" % (f, mode, worst))


# ---- end to end --------------------------------------------------------------------------------------------------------------------------
def _survey(tmp_path, shape):
    from deep_prior_interpolation_amd import utils as u
    d = tmp_path / "data"
    d.mkdir(exist_ok=True)
    img, mask = u.sparse_hyperbolic_volume(shape, seed=5), u.random_trace_mask(shape, 0.5, seed=6)
    np.save(d / "original.npy", np.asarray(img, np.float32))
    np.save(d / "mask.npy", np.asarray(mask, np.float32))
    return ["--imgdir", str(d), "--imgname", "original.npy", "--maskname", "mask.npy", "--gpu", "0", "--net", "unet", "--upsample", "deconv",
            "--filters", "2", "4", "8", "16", "32", "--inputdepth", "4", "--gain", "2", "--inittype", "kaiming"]


def test_interpolator_3d_deconv_eager_and_graph(tmp_path, monkeypatch):
    """30 iterations on a 32x16x16 stand-in (--inittype kaiming: the up path has no norm, and under the default xavier gain of 0.02 nine
    such layers pass no gradient in 30 iterations — the float64 restatement on the CPU stays at its first loss just the same): the loss falls, the hipGraph-captured loop reproduces the eager loop (the comparison of
    test_gpu_nets.test_graph_mode_matches_eager), <patch>_run.npy is written and --savemodel / --netdir round-trip."""
    from deep_prior_interpolation_amd import main as dmain
    from deep_prior_interpolation_amd.architectures import UNet3D
    from deep_prior_interpolation_amd.main import Interpolator
    from deep_prior_interpolation_amd.parameter import parse_arguments
    common = _survey(tmp_path, (32, 16, 16)) + ["--datadim", "3d", "--patch_shape", "32", "16", "16", "--patch_stride", "32", "16", "16"]
    monkeypatch.chdir(tmp_path)
    a = parse_arguments(common + ["--epochs", "30"])
    img, mask = np.load(tmp_path / "data" / "original.npy"), np.load(tmp_path / "data" / "mask.npy")
    res = {}
    for mode in ("eager", "graph"):
        torch.manual_seed(3)
        T = Interpolator(a, str(tmp_path))
        T.load_data({"image": (img.astype(np.float64) * a.gain)[..., None], "mask": mask.astype(np.float64)[..., None], "name": "0"})
        T.build_model()
        assert type(T.net) is UNet3D and not T.storage_bf16_ok()
        T.build_input()
        T.noise_seed = 7
        T.optimize(verbose=False, mode=mode, check_every=8)
        res[mode] = (np.array(T.history.loss), np.array(T.history.snr), np.array(T.history.lr), T.out_best.copy(),
                     {k: v.detach().cpu().numpy().copy() for k, v in T.net.state_dict().items()})
    loss = res["eager"][0]
    print("UNet3D deconv loss", ["%.4f" % v for v in loss[::5]])
    assert len(loss) == 30 and np.isfinite(loss).all() and loss[-5:].mean() < 0.8 * loss[0]
    assert len(res["graph"][0]) == 30
    np.testing.assert_allclose(res["graph"][0], res["eager"][0], rtol=1e-12)
    np.testing.assert_allclose(res["graph"][1], res["eager"][1], rtol=1e-12)
    np.testing.assert_allclose(res["graph"][2], res["eager"][2], rtol=1e-7)
    np.testing.assert_array_equal(res["graph"][3], res["eager"][3])
    for k, v in res["eager"][4].items():
        np.testing.assert_array_equal(res["graph"][4][k], v, err_msg=k)
    # the command line: results, checkpoint, and a second run that starts from it
    dmain.main(common + ["--epochs", "30", "--outdir", "first", "--savemodel"])
    first = np.load("results/first/0_run.npy", allow_pickle=True).item()
    assert first["output"].shape == (32, 16, 16) and np.isfinite(first["output"]).all() and os.path.exists("results/first/0_model.pth")
    sd = torch.load("results/first/0_model.pth", map_location="cpu")
    assert list(sd) == list(UNet3D(4, 1, [2, 4, 8, 16, 32], "deconv").state_dict())
    # what --netdir loads is what --savemodel wrote, tensor for tensor and bit for bit
    b = parse_arguments(_reload(common) + ["--epochs", "3"])
    T = Interpolator(b, str(tmp_path))
    T.load_data({"image": (img.astype(np.float64) * b.gain)[..., None], "mask": mask.astype(np.float64)[..., None], "name": "0"})
    T.build_model(netpath=b.netdir[0])
    loaded = T.net.state_dict()
    assert type(T.net) is UNet3D and list(loaded) == list(sd)
    for k, v in sd.items():
        np.testing.assert_array_equal(loaded[k].cpu().numpy(), v.numpy(), err_msg=k)
    dmain.main(_reload(common) + ["--epochs", "3", "--outdir", "second"])
    second = np.load("results/second/0_run.npy", allow_pickle=True).item()
    l1, l2 = first["history"].loss, second["history"].loss
    print("first run", ["%.4f" % v for v in l1[::5]], "second run (loaded)", ["%.4f" % v for v in l2])
    assert abs(l2[0] - l1[-1]) < abs(l2[0] - l1[0])               # continues from the optimised weights, not from scratch


def _reload(common):
    """The same command line with `--net load --netdir first/0_model.pth`; --upsample stays (the saved args.txt decides the net)."""
    out = list(common)
    out[out.index("--net") + 1] = "load"
    return out + ["--netdir", "first/0_model.pth"]


def test_interpolator_2d_deconv_on_the_lines_section(golden):
    """`--datadim 2d --net unet --upsample deconv`: the 2-D transposed-convolution path, reachable from the command line with this choice,
    on the 160 x 96 window of the lines section (four pools: multiples of 16)."""
    from deep_prior_interpolation_amd import utils as u
    from deep_prior_interpolation_amd.architectures import UNet
    from deep_prior_interpolation_amd.main import Interpolator
    from deep_prior_interpolation_amd.parameter import parse_arguments
    ln = golden("host")["lines"]
    a = parse_arguments(["--imgdir", "x", "--datadim", "2d", "--net", "unet", "--upsample", "deconv", "--filters", "2", "4", "8", "16", "32",
                         "--inputdepth", "4", "--gain", "1", "--epochs", "8", "--gpu", "0", "--inittype", "kaiming"])
    u.set_seed(0)
    T = Interpolator(a, "/tmp")
    T.load_data({"image": ln["original"][:160, :96].astype(np.float64), "mask": ln["mask"][:160, :96].astype(np.float64), "name": "0"})
    T.build_model()
    assert type(T.net) is UNet and isinstance(T.net.up1.up, nn.ConvTranspose2d)
    T.build_input()
    T.optimize(verbose=False)
    loss = np.array(T.history.loss)
    print("UNet 2-D deconv loss", ["%.5f" % v for v in loss])
    assert len(loss) == 8 and np.isfinite(loss).all() and loss[-1] < loss[0] and np.isfinite(T.out_best).all()
