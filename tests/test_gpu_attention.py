"""GPU tests of --net attmultiunet: the attention-gate kernels against float64, at offset views inside guard bands and for bitwise
reproducibility; the gate block, the 2-D net and a 2.5-D optimisation run against the reference's recordings; the 3-D net against a float64
restatement that is first held against the reference in 2-D; the 3-D net through the Interpolator, eager against captured graph."""
import functools
from argparse import Namespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

from conftest import jstr

pytestmark = pytest.mark.gpu
DEV = "cuda"


def G(a, grad=False):
    t = torch.from_numpy(np.array(a, dtype=np.float32)).to(DEV)
    return t.requires_grad_(True) if grad else t


def rel(a, b):
    a = a.detach().cpu().numpy().astype(np.float64) if torch.is_tensor(a) else np.asarray(a, np.float64)
    b = b.detach().cpu().numpy().astype(np.float64) if torch.is_tensor(b) else np.asarray(b, np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(np.linalg.norm((a - b).ravel()) / (np.linalg.norm(b.ravel()) + 1e-30))


def _load_sd(module, state):
    module.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in state.items()})
    return module.to(DEV)


# ---------------------------------------------------------------- the kernels ---------------------------------------------------------
# (C; coarse D, H, W; scale_d): size-1 axes (both edge clamps meet), odd coarse W (8-byte fine rows), a multiple-of-4 W, the default net's 25
# channels, more than one block (256 threads x 4 voxels)
CASES = [(1, 1, 1, 1, 0), (3, 1, 2, 3, 0), (5, 1, 3, 5, 0), (7, 1, 6, 34, 0), (4, 1, 1, 1, 1), (6, 3, 1, 2, 1), (3, 2, 3, 5, 1), (25, 4, 6, 10, 1),
         (5, 5, 12, 18, 1)]
VIEW_CASES = [(3, 1, 2, 3, 0), (7, 1, 6, 34, 0), (3, 2, 3, 5, 1), (5, 5, 12, 18, 1)]
SENTINEL = 12345.678


def _fine(case):
    C, D, H, W, sd = case
    return (2 * D if sd else D), 2 * H, 2 * W


@functools.lru_cache(maxsize=None)
def _case_data(case):
    """Inputs of one case and the float64 expectation (torch.sigmoid / F.interpolate(align_corners=False) / autograd on the CPU); computed
    once, shared by the tests of the case, never written to."""
    C, D, H, W, sd = case
    Do, Ho, Wo = _fine(case)
    gen = torch.Generator().manual_seed(1000 + sum(p * v for p, v in zip((1, 7, 31, 101, 5), case)))
    x = torch.randn((C, Do, Ho, Wo), generator=gen)
    q = 2.0 * torch.randn((D, H, W), generator=gen)
    dy = torch.randn((C, Do, Ho, Wo), generator=gen)
    x64, q64 = x.double().requires_grad_(True), q.double().requires_grad_(True)
    s = torch.sigmoid(q64)
    if sd:
        a = F.interpolate(s[None, None], scale_factor=2, mode="trilinear", align_corners=False)[0, 0]
    else:
        a = F.interpolate(s[None], scale_factor=2, mode="bilinear", align_corners=False)[0]
    y = x64 * a
    y.backward(dy.double())
    return {"x": x, "q": q, "dy": dy, "y": y.detach(), "dx": x64.grad, "dq": q64.grad}


def _run_gate(case, x, q, dy, y, dx):
    """dpi_attn_gate_fwd + dpi_attn_gate_bwd on the given device tensors / views (y, dx are written); returns (s, dq, ws)."""
    from deep_prior_interpolation_amd import _lib
    from deep_prior_interpolation_amd._lib import check, ptr, stream
    C, D, H, W, sd = case
    Do, Ho, Wo = _fine(case)
    L = _lib.load()
    s = torch.full((D * H * W + 8,), SENTINEL, device=DEV)
    dq = torch.full((D * H * W + 8,), SENTINEL, device=DEV)
    n = L.dpi_attn_gate_bwd_ws_floats(C, D, H, W, sd)
    assert n == Do * Ho * Wo
    ws = torch.full((n + 8,), SENTINEL, device=DEV)
    check(L.dpi_attn_gate_fwd(ptr(x), ptr(q), C, D, H, W, sd, ptr(s), ptr(y), stream()), "dpi_attn_gate_fwd")
    check(L.dpi_attn_gate_bwd(ptr(dy), ptr(x), ptr(s), C, D, H, W, sd, ptr(dx), ptr(dq), ptr(ws), stream()), "dpi_attn_gate_bwd")
    torch.cuda.synchronize()
    for t, m in ((s, D * H * W), (dq, D * H * W), (ws, n)):                     # nothing written past the coarse maps / the workspace
        assert bool((t[m:] == SENTINEL).all())
    return s[:D * H * W], dq[:D * H * W], ws[:n]


def _aligned_run(case):
    d = _case_data(case)
    x, q, dy = d["x"].to(DEV), d["q"].to(DEV), d["dy"].to(DEV)
    y, dx = torch.empty_like(x), torch.empty_like(x)
    s, dq, _ = _run_gate(case, x, q, dy, y, dx)
    return y, dx, dq, s


@pytest.mark.parametrize("case", CASES, ids=lambda c: "C%d_%dx%dx%d_sd%d" % c)
def test_gate_kernels_against_float64(case):
    d = _case_data(case)
    y, dx, dq, s = _aligned_run(case)
    e = (rel(y, d["y"]), rel(dx, d["dx"]), rel(dq.view(d["dq"].shape), d["dq"]), rel(s.view(d["q"].shape), torch.sigmoid(d["q"].double())))
    print("gate %s: y %.2e dx %.2e dq %.2e s %.2e" % ((case,) + e))
    assert e[0] < 2e-5 and e[3] < 2e-5          # the bars of test_gpu_nets.py::test_blocks_golden
    assert e[1] < 1e-4 and e[2] < 1e-4


@pytest.mark.parametrize("off", [1, 2])
@pytest.mark.parametrize("case", VIEW_CASES, ids=lambda c: "C%d_%dx%dx%d_sd%d" % c)
def test_gate_kernels_on_offset_views_inside_guard_bands(case, off):
    """x, dy, y, dx at an element offset of 1 (4-byte aligned: scalar accesses) and 2 (8-byte: pairs) into sentinel-filled buffers, y as a
    channel slice of a wider tensor: bit-identical to the aligned call (16-byte accesses), and not one element outside the tensors touched."""
    d = _case_data(case)
    C = case[0]
    Do, Ho, Wo = _fine(case)
    V = Do * Ho * Wo
    n = C * V
    y0, dx0, dq0, s0 = _aligned_run(case)
    xb, dyb, dxb = (torch.full((n + 16,), SENTINEL, device=DEV) for _ in range(3))
    wide = torch.full(((C + 3) * V + 16,), SENTINEL, device=DEV)                  # y = channels 2 .. 2 + C of a (C + 3)-channel tensor at `off`
    xb[off:off + n] = d["x"].to(DEV).reshape(-1)
    dyb[off:off + n] = d["dy"].to(DEV).reshape(-1)
    y_lo = off + 2 * V
    x, dy, dx, y = xb[off:off + n], dyb[off:off + n], dxb[off:off + n], wide[y_lo:y_lo + n]
    assert x.data_ptr() % 16 == 4 * off and y.data_ptr() % 16 == (4 * y_lo) % 16
    x_before, dy_before = xb.clone(), dyb.clone()
    s, dq, _ = _run_gate(case, x, d["q"].to(DEV), dy, y, dx)
    assert torch.equal(y.view(y0.shape), y0) and torch.equal(dx.view(dx0.shape), dx0)
    assert torch.equal(dq, dq0) and torch.equal(s, s0)
    assert torch.equal(xb, x_before) and torch.equal(dyb, dy_before)              # inputs untouched
    for buf, lo, hi in ((dxb, off, off + n), (wide, y_lo, y_lo + n)):
        assert bool((buf[:lo] == SENTINEL).all()) and bool((buf[hi:] == SENTINEL).all())


def test_gate_backward_is_bitwise_reproducible():
    case = (25, 4, 6, 10, 1)
    d = _case_data(case)
    x, q, dy = d["x"].to(DEV), d["q"].to(DEV), d["dy"].to(DEV)
    outs = []
    for _ in range(2):
        y, dx = torch.empty_like(x), torch.empty_like(x)
        s, dq, ws = _run_gate(case, x, q, dy, y, dx)
        outs.append((dq.clone(), dx.clone(), ws.clone(), y.clone()))
    for a, b in zip(*outs):
        assert torch.equal(a, b)


def test_attention_gate_node_checks_and_concat():
    """ops.attention_gate: [skip * gate || up(g)] equals the two halves computed alone (bit for bit: the same kernels), gradients reach skip, q
    and g, and sizes that are not exactly 2:1 raise ValueError."""
    from deep_prior_interpolation_amd import ops
    gen = torch.Generator().manual_seed(3)
    skip, q, g = (torch.randn(s, generator=gen).to(DEV).requires_grad_(True) for s in ((1, 5, 4, 6, 10), (1, 1, 2, 3, 5), (1, 3, 2, 3, 5)))
    for mode in ("nearest", "trilinear"):
        cat = ops.attention_gate(skip, q, g, mode)
        assert cat.shape == (1, 8, 4, 6, 10)
        assert torch.equal(cat[:, :5], ops.attention_gate(skip, q, None)) and torch.equal(cat[:, 5:], ops.upsample2x(g, mode))
        dcat = torch.randn(cat.shape, generator=gen).to(DEV)
        gs = torch.autograd.grad(cat, (skip, q, g), dcat)
        ga = torch.autograd.grad(ops.attention_gate(skip, q, None), (skip, q), dcat[:, :5].contiguous())
        gu = torch.autograd.grad(ops.upsample2x(g, mode), g, dcat[:, 5:].contiguous())
        assert torch.equal(gs[0], ga[0]) and torch.equal(gs[1], ga[1]) and torch.equal(gs[2], gu[0])
    with pytest.raises(ValueError):
        ops.attention_gate(torch.zeros(1, 5, 4, 6, 9, device=DEV), q, g, "nearest")
    with pytest.raises(ValueError):
        ops.attention_gate(torch.zeros(1, 5, 2, 6, 10, device=DEV), q, g, "nearest")
    with pytest.raises(ValueError):
        ops.attention_gate(skip, torch.zeros(1, 2, 2, 3, 5, device=DEV), g, "nearest")


# ---------------------------------------------------------------- the reference's recordings -------------------------------------------
def _check_param_grads(m, ref_grads, exempt_expected=None):
    """test_blocks_golden's rule: 3e-4 relative, except where the reference's gradient norm is below 1e-3 (analytically zero: the bias of a
    convolution that feeds a BatchNorm) — there None or below 1e-3 in absolute value."""
    exempt = []
    for k, p in m.named_parameters():
        ref = ref_grads[k]
        if np.linalg.norm(ref) < 1e-3:
            exempt.append(k)
            assert p.grad is None or float(p.grad.abs().max()) < 1e-3, k
        else:
            assert p.grad is not None, k
            assert rel(p.grad, ref) < 3e-4, (k, rel(p.grad, ref))
    if exempt_expected is not None:
        assert sorted(exempt) == sorted(exempt_expected)
    return exempt


def _bn_fed_biases(net):
    """Names of the biases of convolutions directly followed by a BatchNorm, from the module tree."""
    out = []
    for name, mod in net.named_modules():
        kids = list(mod.named_children())
        for (ka, a), (_, b) in zip(kids, kids[1:]):
            if "BatchNorm" not in type(b).__name__:
                continue
            if "Conv" in type(a).__name__:
                out.append("%s.%s.bias" % (name, ka))
            elif isinstance(a, nn.Sequential) and len(a) == 1 and "Conv" in type(a[0]).__name__:
                out.append("%s.%s.0.bias" % (name, ka))
    return out


def test_gate_block_golden(golden):
    from deep_prior_interpolation_amd.architectures.attention import GridAttentionBlock
    g = golden("attention")["gate2d"]
    m = _load_sd(GridAttentionBlock(2, 6, 5, 4), g["state"])
    gg, x = G(g["g"], True), G(g["x"], True)
    y = m(gg, x)
    assert rel(y, g["y"]) < 2e-5
    y.backward(G(g["dy"]))
    assert rel(gg.grad, g["dg"]) < 1e-4 and rel(x.grad, g["dx"]) < 1e-4
    assert sorted(_check_param_grads(m, g["grads"])) == ["W_g.0.0.bias", "W_x.0.0.bias"]
    sd = m.state_dict()
    for k, v in g["state_after"].items():
        if "running" in k:
            np.testing.assert_allclose(sd[k].cpu().numpy(), v, rtol=1e-5, atol=1e-6, err_msg=k)
        if "num_batches" in k:
            assert int(sd[k]) == int(v)


@pytest.mark.parametrize("mode", ["bilinear", "nearest"])
def test_net2d_golden(golden, mode):
    """The reference's AttMulResUnet2D(6 -> 2, [4, 4, 8, 8, 8]) on (1, 6, 32, 48).  Of its 202 parameter tensors exactly the biases of
    convolutions that feed a BatchNorm — 4 in each of the 9 MultiRes blocks, 4 stride-2 layers, W_g and W_x of the 4 gates: 48 — have a
    rounding-noise gradient in the reference (norm < 1e-3; every conv weight's gradient norm is above 40)."""
    from deep_prior_interpolation_amd.architectures.attention import AttMulResUnet2D
    g = golden("attention")["net2d_" + mode]
    m = AttMulResUnet2D(num_input_channels=6, num_output_channels=2, num_channels_down=[4, 4, 8, 8, 8], upsample_mode=mode)
    assert [[k, list(v.shape)] for k, v in m.state_dict().items()] == jstr(g["keys"])
    m = _load_sd(m, g["init_state"])
    x = G(g["x"], True)
    y = m(x)
    assert rel(y, g["y"]) < 2e-5
    y.backward(G(g["dy"]))
    assert rel(x.grad, g["dx"]) < 1e-4
    ref = g["grads"]
    assert len(ref) == 202 and min(np.linalg.norm(v) for k, v in ref.items() if v.ndim > 1) >= 40
    exempt = _check_param_grads(m, ref, exempt_expected=_bn_fed_biases(m))
    assert len(exempt) == 48 and all(k.endswith(".bias") for k in exempt)


def _interpolator(g, epochs):
    from deep_prior_interpolation_amd.main import Interpolator
    a = Namespace(**jstr(g["args"]))
    a.epochs = epochs
    a.gpu = 0
    T = Interpolator(a, "/tmp")
    T.load_data({"image": g["image"], "mask": g["mask"], "name": "0"})
    T.build_model()              # get_net is on the path
    _load_sd(T.net, g["init_state"])
    T.input_ = G(g["z"])
    return T, a


def test_net25d_iteration0(golden):
    """The body of test_gpu_nets.py::test_net_iteration0 on the 2.5-D attention fixture."""
    from deep_prior_interpolation_amd.architectures.attention import AttMulResUnet
    g = golden("net_attmultiunet25d_tiny")
    T, a = _interpolator(g, 1)
    assert isinstance(T.net, AttMulResUnet) and T.net.nd == 2
    assert abs(T.load_data({"image": g["image"], "mask": g["mask"], "name": "0"}) - float(g["std"])) < 1e-5 * float(g["std"])
    T.optimize(net_inputs=[G(g["net_inputs"][0])], verbose=False)
    assert abs(T.history.loss[0] - g["loss"][0]) <= 1e-5 * abs(g["loss"][0])
    assert abs(T.history.snr[0] - g["snr"][0]) <= 1e-3
    assert abs(T.history.pcorr[0] - g["pcorr"][0]) <= 1e-4


def test_net25d_trajectory(golden):
    """The body of test_gpu_nets.py::test_net_trajectory on the 2.5-D attention fixture, bars unchanged."""
    g = golden("net_attmultiunet25d_tiny")
    K = len(g["loss"])
    assert K == 6
    T, a = _interpolator(g, K)
    T.optimize(net_inputs=[G(x) for x in g["net_inputs"]], verbose=False)
    np.testing.assert_allclose(T.history.loss, g["loss"], rtol=5e-3)
    np.testing.assert_allclose(T.history.snr, g["snr"], atol=0.1)
    np.testing.assert_allclose(T.history.pcorr, g["pcorr"], atol=1e-2)
    assert np.argmin(T.history.loss) == np.argmin(g["loss"])
    assert T.out_best.shape == g["out_best"].shape
    assert rel(T.out_best, g["out_best"]) < 1e-2
    fin = T.net.state_dict()
    for k, v in g["final_state"].items():
        if k.endswith("weight") and v.ndim > 1:
            assert rel(fin[k], v) < 5e-2, k


# ---------------------------------------------------------------- float64 restatement ---------------------------------------------------
# The net as plain torch.nn.functional calls on the CPU, driven by a module's own state_dict, written from its structure:
#     x_1 = down_mb1(inp);  x_{k+1} = down_mb{k+1}(down{k}(x_k));  g = x_n
#     g = up_mb{i}(cat[x_{n-i} * up2(sigmoid(q_i)), up{i}(g)]),  q_i = psi(relu(W_g(g) + W_x(x_{n-i})))      i = 1 .. n-1
#     out = outconv(g)
SLOPE = 0.2


def _params64(state):
    """state_dict -> float64 leaves that require grad; running statistics are left out (train-mode BatchNorm does not read them)."""
    return {k: torch.as_tensor(np.array(v)).to(torch.float64).requires_grad_(True) for k, v in state.items()
            if "running_" not in k and "num_batches" not in k}


def _r_conv(P, key, t, stride=1):
    w = P[key + ".weight"]
    return (F.conv3d if w.ndim == 5 else F.conv2d)(t, w, P[key + ".bias"], stride=stride, padding=(w.shape[-1] - 1) // 2)


def _r_bn(P, key, t):
    return F.batch_norm(t, None, None, P[key + ".weight"], P[key + ".bias"], training=True, eps=1e-5)


def _r_cba(P, key, t, nd):
    """conv -> BatchNorm -> LeakyReLU: children (0.0, 1) in 3-D, (0, 2) in 2-D."""
    if nd == 3:
        return F.leaky_relu(_r_bn(P, key + ".1", _r_conv(P, key + ".0.0", t)), SLOPE)
    return F.leaky_relu(_r_bn(P, key + ".2", _r_conv(P, key + ".0", t)), SLOPE)


def _r_block(P, key, t, nd):
    o1 = _r_cba(P, key + ".conv3x3", t, nd)
    o2 = _r_cba(P, key + ".conv5x5", o1, nd)
    o3 = _r_cba(P, key + ".conv7x7", o2, nd)
    out = torch.cat([o1, o2, o3], 1)
    if nd == 3:
        out = _r_bn(P, key + ".bn1", out)
    out = F.leaky_relu(_r_cba(P, key + ".shortcut", t, nd) + out, SLOPE)
    return _r_bn(P, key + ".bn2", out) if nd == 3 else out


def _r_up(t, mode, nd):
    if mode == "nearest":
        return F.interpolate(t, scale_factor=2, mode="nearest")
    return F.interpolate(t, scale_factor=2, mode="trilinear" if nd == 3 else "bilinear", align_corners=False)


def restated_forward(P, inp, nd, n_scales, mode):
    xs = [_r_block(P, "down_mb1", inp, nd)]
    for k in range(1, n_scales):
        t = F.leaky_relu(_r_bn(P, "down%d.1" % k, _r_conv(P, "down%d.0.0" % k, xs[-1], stride=2)), SLOPE)
        xs.append(_r_block(P, "down_mb%d" % (k + 1), t, nd))
    g = xs[-1]
    for i in range(1, n_scales):
        skip, a = xs[n_scales - 1 - i], "att%d" % i
        g1 = _r_bn(P, a + ".W_g.1", _r_conv(P, a + ".W_g.0.0", g))
        x1 = _r_bn(P, a + ".W_x.1", _r_conv(P, a + ".W_x.0.0", skip, stride=2))
        q = _r_conv(P, a + ".psi.0.0", F.relu(g1 + x1))
        gated = skip * _r_up(torch.sigmoid(q), "linear", nd)
        g = _r_block(P, "up_mb%d" % i, torch.cat([gated, _r_up(g, mode, nd)], 1), nd)
    return _r_conv(P, "outconv.0", g)


def test_restatement_reproduces_the_reference_in_2d(golden):
    """Ties the restatement to the reference before it is trusted in 3-D: float64 against the fp32 recording, to the recording's own
    precision (the bars of the fixture tests: y 2e-5, gradients 1e-4)."""
    g = golden("attention")["net2d_bilinear"]
    P = _params64(g["init_state"])
    x = torch.from_numpy(np.array(g["x"])).double().requires_grad_(True)
    y = restated_forward(P, x, 2, 5, "bilinear")
    assert rel(y, g["y"]) < 2e-5
    y.backward(torch.from_numpy(np.array(g["dy"])).double())
    assert rel(x.grad, g["dx"]) < 1e-4
    for k, v in g["grads"].items():
        if v.ndim > 1:
            assert rel(P[k].grad, v) < 1e-4, k


@pytest.mark.parametrize("mode", ["trilinear", "nearest"])
def test_net3d_against_float64_restatement(mode):
    """AttMulResUnet3D(4 -> 1, [4, 8, 8]) on 16^3: one forward and backward under an MSE loss against the float64 restatement."""
    from deep_prior_interpolation_amd import utils as u
    from deep_prior_interpolation_amd.architectures.attention import AttMulResUnet3D
    u.set_seed(5)
    m = AttMulResUnet3D(num_input_channels=4, num_output_channels=1, num_channels_down=[4, 8, 8], upsample_mode=mode)
    u.init_weights(m, "xavier", 0.02)
    gen = torch.Generator().manual_seed(17)
    x = torch.randn((1, 4, 16, 16, 16), generator=gen)
    tgt = torch.randn((1, 1, 16, 16, 16), generator=gen)
    P = _params64({k: v.detach().numpy() for k, v in m.state_dict().items()})
    x64 = x.double().requires_grad_(True)
    y64 = restated_forward(P, x64, 3, 3, mode)
    ((y64 - tgt.double()) ** 2).mean().backward()
    m = m.to(DEV)
    xg = x.to(DEV).requires_grad_(True)
    y = m(xg)
    y.backward(2.0 * (y.detach() - tgt.to(DEV)) / y.numel())                      # d/dy of mean((y - tgt)^2)
    assert rel(y, y64) < 2e-5
    assert rel(xg.grad, x64.grad) < 1e-4
    n = 0
    for k, p in m.named_parameters():
        if p.ndim > 1:
            assert rel(p.grad, P[k].grad) < 3e-4, (k, rel(p.grad, P[k].grad))
            n += 1
    assert n == 5 * 4 + 2 + 2 * 3 + 1            # 5 MultiRes blocks, 2 stride-2 layers, 2 gates of 3 convolutions, the output layer


# ---------------------------------------------------------------- the CLI path in 3-D ---------------------------------------------------
def test_net3d_interpolator_eager_matches_graph(tmp_path):
    from deep_prior_interpolation_amd import utils as u
    from deep_prior_interpolation_amd.architectures.attention import AttMulResUnet
    from deep_prior_interpolation_amd.main import Interpolator
    from deep_prior_interpolation_amd.parameter import parse_arguments
    args = parse_arguments(["--imgdir", "x", "--datadim", "3d", "--net", "attmultiunet", "--filters", "4", "8", "8", "--inputdepth", "4",
                            "--upsample", "linear", "--epochs", "8", "--gpu", "0"])
    vol = u.hyperbolic_volume((16, 16, 16), seed=3)[..., None] * 40.0
    mask = u.random_trace_mask((16, 16, 16), 0.5, seed=4)[..., None].astype(np.float64)
    res = {}
    for mode in ("eager", "graph"):
        u.set_seed(0)
        T = Interpolator(args, str(tmp_path), device=torch.device("cuda", 0), seed=0)
        T.load_data({"image": vol, "mask": mask, "name": "0"})
        T.build_model()
        T.build_input()
        assert isinstance(T.net, AttMulResUnet) and T.net.nd == 3
        T.optimize(verbose=False, mode=mode, check_every=4)
        res[mode] = (np.array(T.history.loss), T.out_best.copy())
    loss = res["eager"][0]
    assert len(loss) == 8 and np.isfinite(loss).all() and loss[-1] < loss[0]
    np.testing.assert_array_equal(res["graph"][0], loss)
    np.testing.assert_array_equal(res["graph"][1], res["eager"][1])
