"""Timings of the partial convolution (--net part) on the GPU.  Two measurements, each prints one JSON line:

    python tools/bench_partial.py kernels [--cin 64] [--cout 48] [--patch 128 64 64] [--launches 300] [--rounds 3]
        the four passes around the convolution at the first-level shape of the given patch — dpi_pconv_mask_fwd (one-channel mask, as the
        Interpolator passes it, and a Cin-channel mask, the form of the deeper levels), dpi_pconv_norm_fwd (y over c, with bias),
        dpi_pconv_norm_bwd (with the bias gradient) and dpi_pconv_mask_bwd (dx alone: the first level; with dm: the deeper levels) — and
        dpi_chain_apply on the Cout-channel tensor as the yardstick of a plain 2 C V pass.  HIP events around `launches` back-to-back calls
        of one entry point, the entry points alternating for `rounds` rounds.  ms per call, the bytes each must move (computed from the
        shapes, below), GB/s and the share of the 8 TB/s HBM peak; and that what the timed calls left is right at this size.
    python tools/bench_partial.py e2e [--patches 64 64 64 128 64 64] [--iters 20] [--warmup 5] [--runs 3]
        ms per eager Adam iteration of --datadim 3d --net part (PartialUNet3D, 64 input channels, fp32) at each patch, in alternating runs.

The split of an entry point into its launches comes from a kernel trace of the same command with small counts, in a run of its own:
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/bench_partial.py kernels --launches 20 --rounds 1
"""
import argparse
import json
import os
import sys
from time import perf_counter

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK = 8e12          # bytes per second


def stat(vs):
    return {"mean": float(np.mean(vs)), "min": float(np.min(vs)), "max": float(np.max(vs)), "runs": [float(v) for v in vs]}


def kernels(a):
    import torch
    import torch.nn.functional as F
    from deep_prior_interpolation_amd import _lib
    from deep_prior_interpolation_amd._lib import check, ptr, stream
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    L = _lib.load()
    dev = torch.device("cuda", 0)
    Cin, Cout = a.cin, a.cout
    D, H, W = a.patch
    V = D * H * W
    gen = torch.Generator().manual_seed(0)
    x = torch.randn((Cin, V), generator=gen).to(dev)
    m1 = (torch.rand((1, V), generator=gen) > 0.4).float().to(dev)
    mc = torch.randint(-1, 3, (Cin, V), generator=gen).float().to(dev)
    c0 = torch.randn((Cout, V), generator=gen).to(dev)
    dy = torch.randn((Cout, V), generator=gen).to(dev)
    dxm0 = torch.randn((Cin, V), generator=gen).to(dev)
    bias = torch.randn((Cout,), generator=gen).to(dev)
    xm, c, dc, dxm, dmc = torch.empty_like(x), c0.clone(), torch.empty_like(dy), dxm0.clone(), torch.empty_like(x)
    msum, nm, S, dm1 = (torch.empty(V, device=dev) for _ in range(4))
    db = torch.empty(Cout, device=dev)
    ws = torch.empty(L.dpi_pconv_norm_bwd_ws_floats(Cout, V), dtype=torch.float32, device=dev)
    y = torch.empty_like(c0)
    chain = torch.tensor([1.0, 0.0, 0.2, 1.0, 0.0]).repeat(Cout, 1).to(dev).contiguous()
    st = stream()
    calls = {
        "chain_apply": lambda: check(L.dpi_chain_apply(ptr(c0), ptr(chain), Cout, V, ptr(y), st), "dpi_chain_apply"),
        "mask_fwd_cm1": lambda: check(L.dpi_pconv_mask_fwd(ptr(x), ptr(m1), Cin, 1, V, ptr(xm), ptr(msum), st), "dpi_pconv_mask_fwd"),
        "mask_fwd_cmC": lambda: check(L.dpi_pconv_mask_fwd(ptr(x), ptr(mc), Cin, Cin, V, ptr(xm), ptr(msum), st), "dpi_pconv_mask_fwd"),
        "norm_fwd": lambda: check(L.dpi_pconv_norm_fwd(ptr(c0), ptr(msum), ptr(bias), Cout, D, H, W, ptr(c), ptr(nm), ptr(S), st), "dpi_pconv_norm_fwd"),
        "norm_bwd": lambda: check(L.dpi_pconv_norm_bwd(ptr(dy), ptr(S), Cout, V, ptr(dc), ptr(db), ptr(ws), st), "dpi_pconv_norm_bwd"),
        "mask_bwd_dx": lambda: check(L.dpi_pconv_mask_bwd(ptr(dxm0), None, ptr(m1), Cin, 1, V, ptr(dxm), None, st), "dpi_pconv_mask_bwd"),
        "mask_bwd_dm1": lambda: check(L.dpi_pconv_mask_bwd(ptr(dxm0), ptr(x), ptr(m1), Cin, 1, V, ptr(dxm), ptr(dm1), st), "dpi_pconv_mask_bwd"),
        "mask_bwd_dmC": lambda: check(L.dpi_pconv_mask_bwd(ptr(dxm0), ptr(x), ptr(mc), Cin, Cin, V, ptr(dxm), ptr(dmc), st), "dpi_pconv_mask_bwd"),
    }
    # floats each call must move once: tensors read + tensors written (the 27 window reads of msum come from the caches)
    floats = {"chain_apply": 2 * Cout * V, "mask_fwd_cm1": 2 * Cin * V + 2 * V, "mask_fwd_cmC": 3 * Cin * V + V, "norm_fwd": 2 * Cout * V + 3 * V,
              "norm_bwd": 2 * Cout * V + V, "mask_bwd_dx": 2 * Cin * V + V, "mask_bwd_dm1": 3 * Cin * V + 2 * V, "mask_bwd_dmC": 5 * Cin * V}
    for f in calls.values():                     # warm-up: code objects loaded, every buffer touched
        for _ in range(10):
            f()
    torch.cuda.synchronize(dev)
    ms = {k: [] for k in calls}
    for _ in range(a.rounds):
        for k, f in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.launches):
                f()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1) / a.launches)
    out = {"what": "partial-convolution kernels", "cin": Cin, "cout": Cout, "patch": [D, H, W], "launches_per_figure": a.launches,
           "device": torch.cuda.get_device_name(0)}
    for k in calls:
        rate = 4 * floats[k] / (np.mean(ms[k]) * 1e-3)
        out[k] = dict(stat(ms[k]), bytes=4 * floats[k], gb_per_s=rate / 1e9, share_of_hbm_peak=rate / HBM_PEAK)
    # what was timed is also right at this size (the large-tensor code path): the last calls of the loop, against torch on the device
    calls["mask_fwd_cm1"]()
    calls["norm_fwd"]()
    calls["norm_bwd"]()
    calls["mask_bwd_dm1"]()
    torch.cuda.synchronize(dev)
    Sx = F.conv3d((Cin * m1).view(1, 1, D, H, W), torch.ones((1, 1, 3, 3, 3), device=dev), padding=1).view(1, V)
    hole = Sx == 0
    Ss = torch.where(hole, torch.ones_like(Sx), Sx)
    err = lambda got, want: float((got - want).norm() / want.norm())          # noqa: E731
    out["check"] = {"xm": err(xm, x * m1), "S": float((S.view(1, V) - Sx).abs().max()), "y": err(c, torch.where(hole, torch.zeros_like(c0), c0 / Ss + bias[:, None])),
                    "dc": err(dc, torch.where(hole, torch.zeros_like(dy), dy / Ss)), "db": err(db, torch.where(hole, torch.zeros_like(dy), dy).sum(1)),
                    "dx": err(dxm, dxm0 * m1), "dm": err(dm1, (dxm0 * x).sum(0)), "holes": int(hole.sum())}
    assert max(v for k, v in out["check"].items() if k != "holes") < 1e-5, out["check"]
    print(json.dumps(out))


def make(patch, device):
    from deep_prior_interpolation_amd import ops, utils as u
    from deep_prior_interpolation_amd.main import Interpolator
    from deep_prior_interpolation_amd.optim import FusedAdam
    from deep_prior_interpolation_amd.parameter import parse_arguments
    args = parse_arguments(["--imgdir", "synthetic", "--datadim", "3d", "--net", "part", "--inputdepth", "64", "--loss", "mae",
                            "--lr", "1e-3", "--gain", "40", "--reg_noise_std", "0.03", "--noise_std", "0.1", "--epochs", "3000", "--gpu", "0"])
    vol = u.hyperbolic_volume(tuple(patch), seed=0)
    mask = u.random_trace_mask(tuple(patch), 0.66, seed=1)
    u.set_seed(0)
    T = Interpolator(args, "/tmp", device=device)
    T.load_data({"image": (vol * args.gain)[..., None], "mask": mask[..., None], "name": "0"})
    T.begin_patch(0)
    T.build_model()
    T.build_input()
    T.optimizer = FusedAdam(T.net.parameters(), lr=args.lr)
    ops.set_weight_grad_overlap(T.wants_weight_grad_overlap(), in_graph=False)
    return T


def run(T, iters, device):
    import torch
    torch.cuda.synchronize(device)
    t0 = perf_counter()
    for _ in range(iters):
        T.optimizer.zero_grad()
        T.optimization_loop()
        T.optimizer.step()
    torch.cuda.synchronize(device)
    return (perf_counter() - t0) * 1e3 / iters


def e2e(a):
    import torch
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    assert len(a.patches) % 3 == 0
    dev = torch.device("cuda", 0)
    patches = [tuple(a.patches[i:i + 3]) for i in range(0, len(a.patches), 3)]
    Ts = {p: make(p, dev) for p in patches}
    ms = {p: [] for p in patches}
    for p, T in Ts.items():
        run(T, a.warmup, dev)
    for _ in range(a.runs):
        for p, T in Ts.items():
            ms[p].append(run(T, a.iters, dev))
    out = {"what": "ms per eager Adam iteration, --datadim 3d --net part, fp32, 64 input channels", "iters_per_run": a.iters,
           "device": torch.cuda.get_device_name(0)}
    for p, T in Ts.items():
        out["x".join(str(s) for s in p)] = dict(stat(ms[p]), params=int(T.num_params), last_loss=float(T.history.loss[-1]))
    print(json.dumps(out))


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="cmd", required=True)
    k = sub.add_parser("kernels")
    k.add_argument("--cin", type=int, default=64)
    k.add_argument("--cout", type=int, default=48)
    k.add_argument("--patch", type=int, nargs=3, default=[128, 64, 64])
    k.add_argument("--launches", type=int, default=300)
    k.add_argument("--rounds", type=int, default=3)
    e = sub.add_parser("e2e")
    e.add_argument("--patches", type=int, nargs="+", default=[64, 64, 64, 128, 64, 64])
    e.add_argument("--iters", type=int, default=20)
    e.add_argument("--warmup", type=int, default=5)
    e.add_argument("--runs", type=int, default=3)
    a = ap.parse_args()
    {"kernels": kernels, "e2e": e2e}[a.cmd](a)
