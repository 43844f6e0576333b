"""GPU tests of --net part: the partial-convolution kernels against float64 (exact where integer masks make them so), at offset views inside
guard bands and for bitwise reproducibility; the layer through ops and the 2-D net against the reference's recordings; both nets against a
float64 restatement that is first held against the recordings; the nets through the Interpolator."""
import functools
import json

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = 12345.678
EPS = 2.0 ** -24


def G(a, grad=False):
    t = torch.from_numpy(np.array(a, dtype=np.float32)).to(DEV)
    return t.requires_grad_(True) if grad else t


def rel(a, b):
    a = a.detach().cpu().numpy().astype(np.float64) if torch.is_tensor(a) else np.asarray(a, np.float64)
    b = b.detach().cpu().numpy().astype(np.float64) if torch.is_tensor(b) else np.asarray(b, np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(np.linalg.norm((a - b).ravel()) / (np.linalg.norm(b.ravel()) + 1e-30))


def np64(t):
    return t.detach().cpu().numpy().astype(np.float64)


# ---------------------------------------------------------------- the kernels ---------------------------------------------------------
# (Cin, Cm, Cout, D, H, W): the smallest input; a small 2-D case; odd W; 2-D with W % 4 != 0; the nets' deepest level; 1080 voxels: more than
# one block of 256 threads x 4 voxels
CASES = [(1, 1, 1, 1, 1, 1), (3, 1, 2, 1, 2, 3), (5, 5, 6, 4, 5, 6), (4, 4, 3, 1, 6, 34), (48, 48, 48, 2, 2, 2), (7, 1, 5, 5, 12, 18)]
VIEW_CASES = [(3, 1, 2, 1, 2, 3), (5, 5, 6, 4, 5, 6), (4, 4, 3, 1, 6, 34), (7, 1, 5, 5, 12, 18)]
_ID = "Cin%d_Cm%d_Cout%d_%dx%dx%d"


def _box(msum, D, H, W):
    """Zero-padded 3x3x3 window sum (D = 1: 3x3), float64."""
    return F.conv3d(msum.reshape(1, 1, D, H, W), torch.ones((1, 1, 3, 3, 3), dtype=torch.float64), padding=1).reshape(-1)


@functools.lru_cache(maxsize=None)
def _case_data(case):
    """Inputs of one case and the float64 expectation of the four passes; computed once, shared by the tests of the case, never written to.
    The mask holds integers in {-1, 0, 1, 2} with an all-zero slab at the low-W border (3 wide where W allows), so S is exact in fp32.  `c` and
    `dxm` stand in for the results of the convolution launches between the passes."""
    Cin, Cm, Cout, D, H, W = case
    V = D * H * W
    gen = torch.Generator().manual_seed(2000 + sum(p * v for p, v in zip((1, 7, 31, 101, 5, 3), case)))
    x = torch.randn((Cin, V), generator=gen)
    m = torch.randint(-1, 3, (Cm, D, H, W), generator=gen).float()
    if W >= 6:
        m[..., :3] = 0.0
    m = m.reshape(Cm, V)
    c, dy = torch.randn((Cout, V), generator=gen), torch.randn((Cout, V), generator=gen)
    bias, dxm = torch.randn((Cout,), generator=gen), torch.randn((Cin, V), generator=gen)
    x64, m64, c64, dy64, dxm64 = (t.double() for t in (x, m, c, dy, dxm))
    msum = m64.sum(0) if Cm == Cin else Cin * m64[0]
    S = _box(msum, D, H, W)
    hole = S == 0
    Ss = torch.where(hole, torch.ones_like(S), S)
    q = c64 / Ss
    y = torch.where(hole, torch.zeros_like(q), q + bias.double()[:, None])
    dc = torch.where(hole, torch.zeros_like(dy64), dy64 / Ss)
    dyk = torch.where(hole, torch.zeros_like(dy64), dy64)
    prod = dxm64 * x64
    return {"x": x, "m": m, "c": c, "dy": dy, "bias": bias, "dxm": dxm, "xm": x64 * m64, "msum": msum, "S": S, "new_mask": (~hole).double(),
            "y": y, "y_scale": torch.where(hole, torch.zeros_like(q), q.abs() + bias.double().abs()[:, None]), "dc": dc,
            "db": dyk.sum(1), "db_scale": dyk.abs().sum(1), "dx": dxm64 * m64, "dm": prod if Cm == Cin else prod.sum(0, keepdim=True),
            "dm_scale": prod.abs() if Cm == Cin else prod.abs().sum(0, keepdim=True)}


def _padded(n, off):
    return torch.full((off + n + 16,), SENTINEL, device=DEV)


def _run_kernels(case, off=0, bias=True):
    """The four passes on device tensors that start `off` elements into sentinel-filled buffers (off = 0: torch's aligned allocations).
    Returns the outputs as views and the buffers, whose bands outside the views are checked here: nothing is written outside a tensor."""
    from deep_prior_interpolation_amd import _lib
    from deep_prior_interpolation_amd._lib import check, ptr, stream
    Cin, Cm, Cout, D, H, W = case
    V = D * H * W
    d = _case_data(case)
    L = _lib.load()
    sizes = {"x": Cin * V, "m": Cm * V, "c": Cout * V, "dy": Cout * V, "dxm": Cin * V, "xm": Cin * V, "msum": V, "y": Cout * V, "new_mask": V,
             "S": V, "dc": Cout * V, "dx": Cin * V, "dm": Cm * V, "db": Cout}
    buf = {k: _padded(n, off) for k, n in sizes.items()}
    t = {k: b[off:off + sizes[k]] for k, b in buf.items()}
    for k in ("x", "m", "c", "dy", "dxm"):
        t[k].copy_(d[k].reshape(-1).to(DEV))
    assert all(v.data_ptr() % 16 == (4 * off) % 16 for v in t.values())
    before = {k: buf[k].clone() for k in ("x", "m", "c", "dy", "dxm")}
    nws = L.dpi_pconv_norm_bwd_ws_floats(Cout, V)
    assert nws == (((V + 3) // 4 + 255) // 256) * 4 * Cout                 # one row of Cout partials per wave of 64 threads x 4 voxels
    ws = torch.full((nws + 8,), SENTINEL, device=DEV)
    b = d["bias"].to(DEV) if bias else None
    check(L.dpi_pconv_mask_fwd(ptr(t["x"]), ptr(t["m"]), Cin, Cm, V, ptr(t["xm"]), ptr(t["msum"]), stream()), "dpi_pconv_mask_fwd")
    check(L.dpi_pconv_norm_fwd(ptr(t["c"]), ptr(t["msum"]), ptr(b), Cout, D, H, W, ptr(t["y"]), ptr(t["new_mask"]), ptr(t["S"]), stream()),
          "dpi_pconv_norm_fwd")
    check(L.dpi_pconv_norm_bwd(ptr(t["dy"]), ptr(t["S"]), Cout, V, ptr(t["dc"]), ptr(t["db"]), ptr(ws), stream()), "dpi_pconv_norm_bwd")
    check(L.dpi_pconv_mask_bwd(ptr(t["dxm"]), ptr(t["x"]), ptr(t["m"]), Cin, Cm, V, ptr(t["dx"]), ptr(t["dm"]), stream()), "dpi_pconv_mask_bwd")
    torch.cuda.synchronize()
    for k, bb in buf.items():
        assert bool((bb[:off] == SENTINEL).all()) and bool((bb[off + sizes[k]:] == SENTINEL).all()), k
    assert bool((ws[nws:] == SENTINEL).all()) and not bool((ws[:nws] == SENTINEL).any())           # every partial written, none past the end
    for k, bb in before.items():
        assert torch.equal(buf[k], bb), k                                                          # inputs untouched
    return t


@pytest.mark.parametrize("case", CASES, ids=lambda c: _ID % c)
def test_kernels_against_float64(case):
    Cin, Cm, Cout, D, H, W = case
    d = _case_data(case)
    t = _run_kernels(case)
    for k in ("xm", "msum", "S", "new_mask", "dx"):                          # exact: integer masks
        assert np.array_equal(np64(t[k]), d[k].reshape(-1).numpy()), k
    # y = c / S + b: two fp32 roundings, each relative to a term of the sum; dc = dy / S: one
    ey = np.abs(np64(t["y"]) - d["y"].reshape(-1).numpy())
    edc = np.abs(np64(t["dc"]) - d["dc"].reshape(-1).numpy())
    print("pconv %s: y %.2e dc %.2e (units of the scale)" % (case, float((ey / (d["y_scale"].reshape(-1).numpy() + 1e-300)).max()),
                                                           float((edc / (np.abs(d["dc"].reshape(-1).numpy()) + 1e-300)).max())))
    assert bool((ey <= 1e-6 * d["y_scale"].reshape(-1).numpy()).all())
    assert bool((edc <= 1e-6 * np.abs(d["dc"].reshape(-1).numpy())).all())
    # db: an fp32 sum at most 4 (a lane's voxels) + 6 (the butterfly) + the partials per channel + 8 (the finaliser's tree) additions deep
    depth = 18 + 4 * (((V_of(case) + 3) // 4 + 255) // 256)
    assert bool((np.abs(np64(t["db"]) - d["db"].numpy()) <= depth * EPS * d["db_scale"].numpy() + 1e-30).all())
    # dm: one product per channel (Cm = Cin), or Cin fused multiply-adds (Cm = 1)
    edm = np.abs(np64(t["dm"]) - d["dm"].reshape(-1).numpy())
    assert bool((edm <= (1 if Cm == Cin else Cin) * 2 * EPS * d["dm_scale"].reshape(-1).numpy() + 1e-30).all())


def V_of(case):
    return case[3] * case[4] * case[5]


def test_kernels_without_bias_and_in_place():
    """bias = NULL adds nothing and the bias gradient is not asked for; y written over c and dx over dxm (how ops calls them) change nothing."""
    from deep_prior_interpolation_amd import _lib
    from deep_prior_interpolation_amd._lib import check, ptr, stream
    case = (5, 5, 6, 4, 5, 6)
    Cin, Cm, Cout, D, H, W = case
    V = V_of(case)
    d = _case_data(case)
    t = _run_kernels(case)
    t0 = _run_kernels(case, bias=False)
    assert torch.equal(t0["S"], t["S"]) and torch.equal(t0["new_mask"], t["new_mask"])
    q = torch.where(d["S"] == 0, torch.zeros_like(d["c"], dtype=torch.float64), d["c"].double() / torch.where(d["S"] == 0, torch.ones_like(d["S"]), d["S"]))
    assert bool((np.abs(np64(t0["y"]) - q.reshape(-1).numpy()) <= 1e-6 * np.abs(q.reshape(-1).numpy())).all())
    L = _lib.load()
    c, dxm = d["c"].to(DEV).reshape(-1).clone(), d["dxm"].to(DEV).reshape(-1).clone()
    nm, S = torch.empty(V, device=DEV), torch.empty(V, device=DEV)
    check(L.dpi_pconv_norm_fwd(ptr(c), ptr(t["msum"]), ptr(d["bias"].to(DEV)), Cout, D, H, W, ptr(c), ptr(nm), ptr(S), stream()), "norm_fwd")
    check(L.dpi_pconv_mask_bwd(ptr(dxm), None, ptr(t["m"]), Cin, Cm, V, ptr(dxm), None, stream()), "mask_bwd")
    dc = torch.empty(Cout * V, device=DEV)
    check(L.dpi_pconv_norm_bwd(ptr(t["dy"]), ptr(S), Cout, V, ptr(dc), None, None, stream()), "norm_bwd")
    torch.cuda.synchronize()
    assert torch.equal(c, t["y"]) and torch.equal(dxm, t["dx"]) and torch.equal(dc, t["dc"]) and torch.equal(S, t["S"])


@pytest.mark.parametrize("off", [1, 2])
@pytest.mark.parametrize("case", VIEW_CASES, ids=lambda c: _ID % c)
def test_kernels_on_offset_views_inside_guard_bands(case, off):
    """Every tensor at an element offset of 1 (4-byte accesses) and 2 (8-byte where V is even) into sentinel-filled buffers: bit-identical to the
    aligned call, the bias gradient included, and not one element outside the tensors touched (checked in _run_kernels)."""
    t0 = _run_kernels(case)
    t = _run_kernels(case, off=off)
    for k in ("xm", "msum", "y", "new_mask", "S", "dc", "db", "dx", "dm"):
        assert torch.equal(t[k], t0[k]), k


def test_kernels_are_bitwise_reproducible():
    case = (7, 1, 5, 5, 12, 18)
    a, b = _run_kernels(case), _run_kernels(case)
    for k in ("xm", "msum", "y", "new_mask", "S", "dc", "db", "dx", "dm"):
        assert torch.equal(a[k], b[k]), k


# ---------------------------------------------------------------- the layer through ops -------------------------------------------------
@pytest.mark.parametrize("cm", ["cin", "one"])
@pytest.mark.parametrize("nd", [2, 3])
def test_a_mask_of_zeros_gives_zeros_everywhere(nd, cm):
    from deep_prior_interpolation_amd import ops
    gen = torch.Generator().manual_seed(5)
    sp = (4, 6, 10) if nd == 3 else (6, 10)
    x = torch.randn((1, 3) + sp, generator=gen).to(DEV).requires_grad_(True)
    m = torch.zeros((1, 3 if cm == "cin" else 1) + sp, device=DEV, requires_grad=True)
    w = torch.randn((4, 3) + (3,) * nd, generator=gen).to(DEV).requires_grad_(True)
    b = torch.randn(4, generator=gen).to(DEV).requires_grad_(True)
    y, nm = ops.partial_conv(x, m, w, b)
    assert nm.shape == (1, 1) + sp and not nm.requires_grad
    assert not bool(y.any()) and not bool(nm.any())
    gs = torch.autograd.grad(y, (x, m, w, b), torch.randn(y.shape, generator=gen).to(DEV))
    for g_, ref in zip(gs, (x, m, w, b)):
        assert g_.shape == ref.shape and not bool(g_.any())


def _layer(cfg):
    from deep_prior_interpolation_amd.architectures.partial_unet import PartialConv
    return PartialConv(cfg["nd"], cfg["cin"], cfg["cout"], bn=cfg["bn"], bias=cfg["bias"], act_fun=cfg["act"])


@pytest.mark.parametrize("name", ["c2d_bn", "c2d_bias", "c3d_bn_bias", "c3d_plain"])
def test_layer_golden(golden, name):
    """PartialConv against the reference's Partial2DConv / Partial3DConv: BatchNorm and bias on and off, integer masks with holes by cancellation."""
    g = golden("partial")["layers"][name]
    cfg = json.loads(str(g["cfg"]))
    m_ = _layer(cfg)
    assert list(m_.state_dict().keys()) == list(g["state"].keys())
    m_.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in g["state"].items()})
    m_ = m_.to(DEV)
    x, m = G(g["x"], True), G(g["m"], True)
    y, nm = m_(x, m)
    assert int(g["holes_by_cancellation"]) >= 1
    assert np.array_equal(nm.cpu().numpy(), g["new_mask"])                      # the hole set is identical
    assert rel(y, g["y"]) < 2e-5
    y.backward(G(g["dy"]))
    w = m_.input_conv.weight
    e = {"dx": rel(x.grad, g["dx"]), "dm": rel(m.grad, g["dm"]), "dW": rel(w.grad, g["dW"])}
    print("layer %s: y %.2e %s" % (name, rel(y, g["y"]), e))
    assert max(e.values()) < 1e-4
    if cfg["bias"]:
        if cfg["bn"]:         # a bias in front of a BatchNorm: its true gradient is (near) zero — absolute, against the layer's weight gradient
            assert float(np.abs(np64(m_.input_conv.bias.grad) - g["db"]).max()) < 1e-4 * float(np.abs(g["dW"]).max())
        else:
            assert rel(m_.input_conv.bias.grad, g["db"]) < 1e-4
    if cfg["bn"]:
        assert rel(m_.bn.weight.grad, g["dgamma"]) < 1e-4 and rel(m_.bn.bias.grad, g["dbeta"]) < 1e-4


def test_one_channel_mask_equals_its_expansion():
    """A binary one-channel mask and the same mask repeated over the input's channels: Cin * m and m + ... + m are the same integers, so the
    two forms of the kernels agree bit for bit; dm of the one-channel form is the channel sum of the other's."""
    from deep_prior_interpolation_amd import ops
    gen = torch.Generator().manual_seed(8)
    x = torch.randn((1, 5, 3, 6, 10), generator=gen).to(DEV).requires_grad_(True)
    m1 = (torch.rand((1, 1, 3, 6, 10), generator=gen) > 0.5).float().to(DEV).requires_grad_(True)
    m5 = m1.detach().expand(-1, 5, -1, -1, -1).contiguous().requires_grad_(True)
    w = torch.randn((4, 5, 3, 3, 3), generator=gen).to(DEV).requires_grad_(True)
    dy = torch.randn((1, 4, 3, 6, 10), generator=gen).to(DEV)
    (y1, n1), (y5, n5) = ops.partial_conv(x, m1, w, None), ops.partial_conv(x, m5, w, None)
    assert torch.equal(y1, y5) and torch.equal(n1, n5)
    g1, g5 = torch.autograd.grad(y1, (x, m1, w), dy), torch.autograd.grad(y5, (x, m5, w), dy)
    assert torch.equal(g1[0], g5[0]) and torch.equal(g1[2], g5[2])
    assert rel(g1[1], g5[1].sum(1, keepdim=True)) < 1e-6


# ---------------------------------------------------------------- float64 restatement ---------------------------------------------------
# The reference's forward as plain torch.nn.functional calls on the CPU, driven by a module's own state_dict:
#     per level:  xm = x * m;  S = conv(m, ones) under no_grad;  y = S == 0 ? 0 : conv(xm, W) / S + b;  new_mask = (S != 0) on Cout channels
#                 x = down(act(bn(y)));  m = down(new_mask)          (the learned stride-2 convolution on both, bias included)
#     decoder:    up = up2(x5);  up = up2(conv(conv(cat[x_k, up])))  k = 4 .. 1;  out = last_kernel(cat[input, up])
SLOPE = 0.2


def _params64(sd):
    return {k: v.detach().cpu().double().requires_grad_(True) for k, v in sd.items() if v.dtype.is_floating_point and "running_" not in k and "mask_conv" not in k}


def _r_conv(t, w, b=None, stride=1):
    return (F.conv3d if w.ndim == 5 else F.conv2d)(t, w, b, stride=stride, padding=1)


def _r_partial(P, key, x, m, slope):
    w, b = P[key + ".input_conv.weight"], P.get(key + ".input_conv.bias")
    c = _r_conv(x * m, w)
    with torch.no_grad():
        S = _r_conv(m, torch.ones_like(w))
        hole = S == 0
        Ss = S.masked_fill(hole, 1.0)
    y = c / Ss
    if b is not None:
        y = y + b.reshape((1, -1) + (1,) * (w.ndim - 2))
    y = y.masked_fill(hole, 0.0)
    new_mask = (~hole).to(y.dtype)
    if key + ".bn.weight" in P:
        y = F.batch_norm(y, None, None, P[key + ".bn.weight"], P[key + ".bn.bias"], training=True, eps=1e-5)
    return (F.leaky_relu(y, slope) if slope != 1.0 else y), new_mask


def restated_forward(P, inp, mask):
    """mask: the input's channels (the reference's form)."""
    downs, x, m = [], inp, mask
    for i in range(1, 6):
        y, nm = _r_partial(P, "enc%d.partialconv" % i, x, m, SLOPE)
        w, b = P["enc%d.down.weight" % i], P["enc%d.down.bias" % i]
        x, m = _r_conv(y, w, b, 2), _r_conv(nm, w, b, 2)
        downs.append(x)

    def up2(t):
        return F.interpolate(t, scale_factor=2, mode="nearest")
    up = up2(downs[4])
    for name, skip in (("dec4", downs[3]), ("dec3", downs[2]), ("dec2", downs[1]), ("dec1", downs[0])):
        up = up2(_r_conv(_r_conv(torch.cat([skip, up], 1), P[name + ".0.weight"]), P[name + ".1.weight"]))
    t = torch.cat([inp, up], 1)
    for j in range(4):
        t = _r_conv(t, P["last_kernel.%d.weight" % j])
    return t


def _seeded_net(make, seed):
    """Constructor initialisation after torch.manual_seed(seed), then down.weight.abs_(): the recording's state, and a conditioned one (with signed
    `down` weights the deeper masks sum to small signed numbers and single gradients move by 1e-3 between fp32 and float64)."""
    torch.manual_seed(seed)
    net = make()
    with torch.no_grad():
        for k, p in net.named_parameters():
            if k.endswith("down.weight"):
                p.abs_()
    return net


def test_restatement_reproduces_the_reference(golden):
    """Ties the restatement to the reference before it is trusted in 3-D: the layer in float64 against the fp32 recording (y 2e-5, gradients
    1e-4, the hole set identical) and the 2-D net against the recorded output (2e-5)."""
    from deep_prior_interpolation_amd.architectures.partial_unet import PartialUNet
    for name in ("c2d_bias", "c3d_bn_bias"):
        g = golden("partial")["layers"][name]
        cfg = json.loads(str(g["cfg"]))
        P = {"l." + k: torch.from_numpy(np.array(v)).double().requires_grad_(True) for k, v in g["state"].items() if "running" not in k and "num_b" not in k and "mask_conv" not in k}
        x, m = (torch.from_numpy(np.array(g[k])).double().requires_grad_(True) for k in ("x", "m"))
        y, nm = _r_partial(P, "l", x, m, SLOPE if cfg["act"] == "LeakyReLU" else 1.0)
        assert np.array_equal(nm[:, :1].numpy(), g["new_mask"]) and rel(y, g["y"]) < 2e-5
        y.backward(torch.from_numpy(np.array(g["dy"])).double())
        assert rel(x.grad, g["dx"]) < 1e-4 and rel(m.grad, g["dm"]) < 1e-4 and rel(P["l.input_conv.weight"].grad, g["dW"]) < 1e-4
    g = golden("partial")["net2d"]["run"]
    net = _seeded_net(lambda: PartialUNet(3, 2), int(golden("partial")["meta"]["seed"]))
    z, mask = (torch.from_numpy(np.array(g[k])).double() for k in ("z", "mask"))
    with torch.no_grad():
        out = restated_forward(_params64(net.state_dict()), z, mask.expand(-1, 3, -1, -1))
    assert rel(out, g["out"]) < 2e-5


def test_net2d_golden(golden):
    """The reference's PartialUNet(3 -> 2) at (1, 3, 32, 64): same-seed constructor values (bit-identical: test_partial_host.py), down.weight.abs_(),
    a binary mask with a 12-column strip of zeros — as one channel and expanded to the input's."""
    from deep_prior_interpolation_amd.architectures.partial_unet import PartialUNet
    g = golden("partial")["net2d"]["run"]
    net = _seeded_net(lambda: PartialUNet(3, 2), int(golden("partial")["meta"]["seed"])).to(DEV)
    z, mask = G(g["z"]), G(g["mask"])
    with torch.no_grad():
        out1 = net(z, mask)
        out3 = net(z, mask.expand(-1, 3, -1, -1).contiguous())
    print("net2d: %.2e (one channel) %.2e (expanded)" % (rel(out1, g["out"]), rel(out3, g["out"])))
    assert rel(out1, g["out"]) < 2e-5 and rel(out3, g["out"]) < 2e-5


@functools.lru_cache(maxsize=None)
def _restated_case(nd):
    """One forward and backward of the float64 restatement under an MSE loss: computed once per net."""
    from deep_prior_interpolation_amd.architectures.partial_unet import PartialUNet, PartialUNet3D
    cin, shape = (3, (32, 64)) if nd == 2 else (2, (32, 32, 32))
    net = _seeded_net((lambda: PartialUNet(cin, 2)) if nd == 2 else (lambda: PartialUNet3D(cin, 1)), 3)
    gen = torch.Generator().manual_seed(40 + nd)
    x = 0.1 * torch.randn((1, cin) + shape, generator=gen)
    mask = (torch.rand((1, 1) + shape, generator=gen) > 0.4).float()
    mask[..., 20:32] = 0.0
    tgt = torch.randn((1, net.last_kernel[3].weight.shape[0]) + shape, generator=gen)
    P = _params64(net.state_dict())
    y64 = restated_forward(P, x.double(), mask.double().expand((-1, cin) + (-1,) * nd))
    ((y64 - tgt.double()) ** 2).mean().backward()
    return net, x, mask, tgt, y64.detach(), {k: v.grad for k, v in P.items()}


@pytest.mark.parametrize("nd", [2, 3])
def test_nets_against_float64_restatement(nd):
    """PartialUNet at (1, 3, 32, 64) and PartialUNet3D at (1, 2, 32, 32, 32), the smallest size it accepts: output 2e-5, parameter gradients 3e-4.
    partialconv.input_conv.bias (3-D) sits in front of a BatchNorm: where no voxel of the level is a hole (levels 2-5 here) its true gradient is
    zero (1e-15 in float64) and it is compared in absolute terms against the largest entry of that layer's weight gradient.  At the first
    level the holes of the input mask keep y = 0 whatever the bias, the BatchNorm no longer cancels it, and its gradient (0.05 against 5e-5
    for the weight) is compared like every other one."""
    net, x, mask, tgt, y64, g64 = _restated_case(nd)
    m = net.to(DEV)
    m.zero_grad()
    y = m(x.to(DEV), mask.to(DEV))
    y.backward(2.0 * (y.detach() - tgt.to(DEV)) / y.numel())                      # d/dy of mean((y - tgt)^2)
    assert rel(y, y64) < 2e-5, rel(y, y64)
    n, nzero, worst = 0, 0, (0.0, None)
    for k, p in m.named_parameters():
        assert p.grad is not None, k
        wmax = float(g64[k[:-4] + "weight"].abs().max()) if k.endswith("partialconv.input_conv.bias") else 0.0
        if wmax and float(g64[k].abs().max()) <= wmax:
            assert float((p.grad.cpu().double() - g64[k]).abs().max()) < 3e-4 * wmax, k
            nzero += 1
        else:
            e = rel(p.grad, g64[k])
            worst = max(worst, (e, k))
            assert e < 3e-4, (k, e)
        n += 1
    print("net%dd: y %.2e, worst gradient %.2e at %s" % (nd, rel(y, y64), worst[0], worst[1]))
    assert n == (57 if nd == 2 else 62) - 5 - 15 and nzero == (0 if nd == 2 else 4)


# ---------------------------------------------------------------- the CLI path ----------------------------------------------------------
def _interpolator(argv, vol, mask, tmp_path, seed=0):
    from deep_prior_interpolation_amd import utils as u
    from deep_prior_interpolation_amd.architectures.partial_unet import PartialNet
    from deep_prior_interpolation_amd.main import Interpolator
    from deep_prior_interpolation_amd.parameter import parse_arguments
    args = parse_arguments(["--imgdir", "x", "--net", "part", "--gpu", "0"] + argv)
    u.set_seed(seed)
    T = Interpolator(args, str(tmp_path), device=torch.device("cuda", 0), seed=seed)
    T.load_data({"image": vol, "mask": mask, "name": "0"})
    T.build_model()
    T.build_input()
    assert isinstance(T.net, PartialNet)
    return T


def test_net3d_interpolator_eager_matches_graph_and_holdout_runs(tmp_path):
    from deep_prior_interpolation_amd import utils as u
    vol = u.hyperbolic_volume((32, 32, 32), seed=3)[..., None] * 40.0
    mask = u.random_trace_mask((32, 32, 32), 0.5, seed=4)[..., None].astype(np.float64)
    argv = ["--datadim", "3d", "--inputdepth", "4", "--epochs", "8"]
    res = {}
    for mode in ("eager", "graph"):
        T = _interpolator(argv, vol, mask, tmp_path)
        assert T.net.nd == 3 and not T.storage_bf16_ok() and not T.wants_weight_grad_overlap()
        T.optimize(verbose=False, mode=mode, check_every=4)
        res[mode] = (np.array(T.history.loss), T.out_best.copy())
    loss = res["eager"][0]
    assert len(loss) == 8 and np.isfinite(loss).all() and np.isfinite(res["eager"][1]).all()
    np.testing.assert_array_equal(res["graph"][0], loss)                          # the comparison of test_gpu_attention.py: bit for bit
    np.testing.assert_array_equal(res["graph"][1], res["eager"][1])
    T = _interpolator(argv + ["--holdout", "0.2"], vol, mask, tmp_path)
    T.optimize(verbose=False, mode="eager")
    assert len(T.history.loss) == 8 and np.isfinite(T.history.loss).all() and np.isfinite(T.history.val_snr).all()
    # the held-out traces are holes for the net too: its mask is the training mask, one channel
    assert T._net_mask.shape == (1, 1, 32, 32, 32) and torch.equal(T._net_mask, T.training_mask())
    assert float(T._net_mask.sum()) < float(T.mask_.sum())


def test_net25d_loss_falls_below_its_start(tmp_path):
    """--datadim 2.5d at 32 x 64 (a slab of 3 sections): the lowest loss over 200 iterations is below the first.  The curve is spiky by the net's
    nature: on the CPU the reference's net reached 0.41-0.57 of its first value in 200 steps; this run reaches 0.75 on the MI355X
    (0.66 with ReLU, 0.24 under the MSE loss; with 8 input channels it spikes to 80 times its start after 100 steps and recovers slowly)."""
    from deep_prior_interpolation_amd import utils as u
    vol = u.hyperbolic_volume((32, 64, 3), seed=9) * 40.0
    mask = u.random_trace_mask((32, 64, 3), 0.5, seed=10).astype(np.float64)
    T = _interpolator(["--datadim", "2.5d", "--epochs", "200"], vol, mask, tmp_path)          # the CLI's defaults: 64 input channels, Adam 1e-3, MAE
    assert T.net.nd == 2 and T.net.last_kernel[3].weight.shape[0] == 3
    T.optimize(verbose=False)
    loss = np.array(T.history.loss)
    print("2.5d: first %.4g lowest %.4g (%.2f of the first) at %d, last %.4g" % (loss[0], loss.min(), loss.min() / loss[0], int(loss.argmin()), loss[-1]))
    assert len(loss) == 200 and np.isfinite(loss).all()
    assert loss.min() < loss[0]
    assert T._net_mask.shape == (1, 1, 32, 64)
