"""Record the fixtures of --net part by RUNNING THE REFERENCE's classes on the CPU:

    python tools/record_partial_golden.py /path/to/reference

imports architectures/partial_unet.py (and the base.py beside it) from that checkout and writes tests/golden/partial.npz, data only:

  layers/<case>   a freshly constructed Partial2DConv / Partial3DConv (mask_conv = 1, as its constructor leaves it) with BatchNorm and bias on
                  and off: x, m, dy, the state, and y, new_mask (one channel: the reference's are identical), dx, dm, dW, db.  The mask has the
                  input's channels, small integers in {-1, 0, 1, 2} and an all-zero slab touching a border, so the window sum S is exact in
                  fp32: the hole set is the same in every implementation, holes by cancellation included, and |S| >= 1 elsewhere.
  net2d, net3d    key names and shapes of PartialUNet(3 -> 2) and PartialUNet3D(2 -> 1), and per-tensor checksums (float64 sum, first four
                  values) of their constructor initialisation after torch.manual_seed(0)
  net2d/run       PartialUNet(3 -> 2) at (1, 3, 32, 64), constructor initialisation with down.weight.abs_(): z, a one-channel binary mask
                  with a 12-column all-zero strip (handed to the reference expanded to the input's channels) and the output
"""
import importlib
import json
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "partial.npz")
THREADS = 4
SEED = 0


def load_reference(path):
    arch = os.path.join(path, "architectures")
    if not os.path.isfile(os.path.join(arch, "partial_unet.py")):
        raise SystemExit("no architectures/partial_unet.py under %s" % path)
    sys.dont_write_bytecode = True
    pkg = types.ModuleType("ref_architectures")          # the two files only: the package's own __init__ pulls in every net and its imports
    pkg.__path__ = [arch]
    sys.modules["ref_architectures"] = pkg
    return importlib.import_module("ref_architectures.partial_unet")


def npy(t):
    return t.detach().cpu().numpy().copy()


def integer_mask(shape, gen, slab):
    """Values in {-1, 0, 1, 2}; `slab` = (axis, lo, hi) is zeroed over every channel."""
    m = torch.randint(-1, 3, shape, generator=gen).float()
    idx = [slice(None)] * len(shape)
    idx[slab[0]] = slice(slab[1], slab[2])
    m[tuple(idx)] = 0.0
    return m


def record_layer(P, nd, cin, cout, bn, bias, act, spatial, slab, seed):
    gen = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)
    m_ = (P.Partial3DConv if nd == 3 else P.Partial2DConv)(cin, cout, bn=bn, bias=bias, act_fun=act)
    with torch.no_grad():                                  # a BatchNorm affine and a bias that are not the identity
        if bias:
            m_.input_conv.bias.copy_(0.5 * torch.randn(cout, generator=gen))
        if bn:
            m_.bn.weight.copy_(1.0 + 0.3 * torch.randn(cout, generator=gen))
            m_.bn.bias.copy_(0.2 * torch.randn(cout, generator=gen))
    assert bool((m_.mask_conv.weight == 1).all())
    state = {k: npy(v) for k, v in m_.state_dict().items()}
    x = torch.randn((1, cin) + spatial, generator=gen).requires_grad_(True)
    m = integer_mask((1, cin) + spatial, gen, slab).requires_grad_(True)
    y, new_mask = m_(x, m)
    dy = torch.randn(y.shape, generator=gen)
    y.backward(dy)
    assert bool((new_mask == new_mask[:, :1]).all()), "new_mask differs between channels"
    holes = new_mask[0, 0] == 0
    assert 0 < int(holes.sum()) < holes.numel()
    with torch.no_grad():                                  # S on integers, exactly: the recorded hole set is the set S == 0, |S| >= 1 elsewhere
        S = torch.nn.functional.conv3d(m.double().sum(1, keepdim=True).reshape((1, 1) + ((1,) + spatial if nd == 2 else spatial)),
                                       torch.ones((1, 1, 3 if nd == 3 else 1, 3, 3), dtype=torch.float64),
                                       padding=(1 if nd == 3 else 0, 1, 1)).reshape(spatial)
    assert bool(((S == 0) == holes).all()) and float(S[~holes].abs().min()) >= 1.0
    cancel = int(((S == 0) & (torch.nn.functional.max_pool3d(m.detach().abs().amax(1, keepdim=True).reshape((1, 1) + ((1,) + spatial if nd == 2 else spatial)),
                                                              (3 if nd == 3 else 1, 3, 3), 1, (1 if nd == 3 else 0, 1, 1)).reshape(spatial) > 0)).sum())
    d = {"cfg": json.dumps({"nd": nd, "cin": cin, "cout": cout, "bn": bn, "bias": bias, "act": act}), "state": state, "x": npy(x), "m": npy(m),
         "dy": npy(dy), "y": npy(y), "new_mask": npy(new_mask[:, :1]), "dx": npy(x.grad), "dm": npy(m.grad),
         "dW": npy(m_.input_conv.weight.grad), "S": S.numpy().astype(np.float32), "holes_by_cancellation": np.int64(cancel)}
    if bias:
        d["db"] = npy(m_.input_conv.bias.grad)
    if bn:
        d["dgamma"], d["dbeta"] = npy(m_.bn.weight.grad), npy(m_.bn.bias.grad)
    print("layer nd=%d bn=%d bias=%d: %d holes of %d (%d by cancellation)" % (nd, bn, bias, int(holes.sum()), holes.numel(), cancel))
    return d


def checksums(module):
    return {k: np.concatenate([[v.double().sum().item()], v.double().reshape(-1)[:4].numpy()]) for k, v in module.state_dict().items()}


def record_net(make):
    torch.manual_seed(SEED)
    net = make()
    return net, {"keys": np.array(json.dumps([[k, list(v.shape)] for k, v in net.state_dict().items()])), "checksums": checksums(net)}


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    torch.set_num_threads(THREADS)
    P = load_reference(sys.argv[1])
    layers = {
        "c2d_bn": record_layer(P, 2, 4, 6, True, False, "LeakyReLU", (10, 14), (3, 0, 4), 11),
        "c2d_bias": record_layer(P, 2, 3, 5, False, True, "none", (9, 13), (2, 5, 9), 12),
        "c3d_bn_bias": record_layer(P, 3, 3, 4, True, True, "LeakyReLU", (5, 6, 7), (4, 4, 7), 13),
        "c3d_plain": record_layer(P, 3, 2, 3, False, False, "ReLU", (4, 5, 6), (2, 0, 3), 14),
    }
    net2d, d2 = record_net(lambda: P.PartialUNet(3, 2))
    _, d3 = record_net(lambda: P.PartialUNet3D(2, 1))
    assert len(json.loads(str(d2["keys"]))) == 57 and len(json.loads(str(d3["keys"]))) == 62
    gen = torch.Generator().manual_seed(21)
    with torch.no_grad():
        for k, p in net2d.named_parameters():
            if k.endswith("down.weight"):
                p.abs_()
        z = 0.1 * torch.randn((1, 3, 32, 64), generator=gen)
        mask = (torch.rand((1, 1, 32, 64), generator=gen) > 0.4).float()
        mask[..., 20:32] = 0.0
        out = net2d(z, mask.expand(-1, 3, -1, -1).contiguous())
    assert bool(torch.isfinite(out).all())
    d2["run"] = {"z": npy(z), "mask": npy(mask), "out": npy(out)}
    flat = {}

    def rec(prefix, v):
        if isinstance(v, dict):
            for k, x in v.items():
                rec(prefix + "/" + str(k) if prefix else str(k), x)
        else:
            flat[prefix] = np.asarray(v)

    rec("", {"layers": layers, "net2d": d2, "net3d": d3, "meta": {"threads": np.int64(THREADS), "torch": np.array(torch.__version__), "seed": np.int64(SEED)}})
    np.savez_compressed(OUT, **flat)
    print("wrote %s (%.1f kB, %d arrays)" % (OUT, os.path.getsize(OUT) / 1e3, len(flat)))


if __name__ == "__main__":
    main()
