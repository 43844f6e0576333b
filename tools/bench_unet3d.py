"""Timings of the 3-D plain UNet (--datadim 3d --net unet) on the GPU.  Two measurements, each prints one JSON line:

    python tools/bench_unet3d.py kernels [--patch 256 128 128] [--filters 16 32 64 128 256] [--launches 20] [--rounds 3]
        the three launches of the transposed convolution (dpi_deconv4x4x4s2_fwd / _bwd_data / _bwd_weight) of every level of the net at
        the given patch, each alone: HIP events around `launches` back-to-back calls of one entry point, the entry points alternating for
        `rounds` rounds.  ms per call, TF/s at 2 * 64 * Cin * Cout * V flop per launch (V = coarse voxels) and the fraction of the
        157.3 TF fp32 peak; and that what the timed calls left is right at this size (against torch on the device).
    python tools/bench_unet3d.py e2e [--patches 64 64 64 128 64 64 256 128 128] [--iters 10] [--warmup 3] [--runs 3]
        ms per eager Adam iteration of --net unet with --upsample deconv, linear and nearest at each patch (64 input channels, fp32,
        default widths), and of --net multiunet (--upsample nearest, the default) on the same tree beside them, in alternating runs.

The split of an iteration into its launches comes from a kernel trace of the same command with small counts, in a run of its own:
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/bench_unet3d.py e2e --patches 64 64 64 --iters 3 --runs 1
"""
import argparse
import json
import os
import sys
from time import perf_counter

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FP32_PEAK = 157.3e12     # flop per second


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
    st = stream()
    gen = torch.Generator().manual_seed(0)
    out = {"what": "transposed convolution k=4 s=2 p=1, one launch each", "patch": list(a.patch), "filters": list(a.filters),
           "launches_per_figure": a.launches, "device": torch.cuda.get_device_name(0), "levels": {}}
    f = list(a.filters)
    for lvl in range(4, 0, -1):                                        # up4 .. up1: f[lvl] -> f[lvl - 1] from the patch / 2^lvl grid
        Cin, Cout = f[lvl], f[lvl - 1]
        D, H, W = (s >> lvl for s in a.patch)
        V = D * H * W
        x = torch.randn((Cin, D, H, W), generator=gen).to(dev)
        w = (torch.randn((Cin, Cout, 4, 4, 4), generator=gen) / (8 * Cin) ** 0.5).to(dev)
        b = torch.randn((Cout,), generator=gen).to(dev)
        dy = torch.randn((Cout, 2 * D, 2 * H, 2 * W), generator=gen).to(dev)
        y, dx, dw = torch.empty_like(dy), torch.empty_like(x), torch.empty_like(w)
        ws = torch.empty(L.dpi_deconv4x4x4s2_bwd_weight_ws_floats(Cin, Cout, D, H, W), dtype=torch.float32, device=dev)
        calls = {
            "fwd": lambda: check(L.dpi_deconv4x4x4s2_fwd(ptr(x), ptr(w), ptr(b), Cin, Cout, D, H, W, ptr(y), st), "dpi_deconv4x4x4s2_fwd"),
            "bwd_data": lambda: check(L.dpi_deconv4x4x4s2_bwd_data(ptr(dy), ptr(w), Cin, Cout, D, H, W, ptr(dx), st), "dpi_deconv4x4x4s2_bwd_data"),
            "bwd_weight": lambda: check(L.dpi_deconv4x4x4s2_bwd_weight(ptr(x), ptr(dy), Cin, Cout, D, H, W, ptr(dw), ptr(ws), st),
                                        "dpi_deconv4x4x4s2_bwd_weight"),
        }
        for c in calls.values():
            for _ in range(3):
                c()
        torch.cuda.synchronize(dev)
        ms = {k: [] for k in calls}
        for _ in range(a.rounds):
            for k, c in calls.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.launches):
                    c()
                e1.record()
                e1.synchronize()
                ms[k].append(e0.elapsed_time(e1) / a.launches)
        flop = 2.0 * 64 * Cin * Cout * V
        row = {"cin": Cin, "cout": Cout, "coarse": [D, H, W], "gflop_per_launch": flop / 1e9, "ws_mbytes": ws.numel() * 4 / 1e6}
        for k in calls:
            rate = flop / (np.mean(ms[k]) * 1e-3)
            row[k] = dict(stat(ms[k]), tflops=rate / 1e12, fraction_of_fp32_peak=rate / FP32_PEAK)
        # what was timed is right at this size: against aten on the device
        xt, wt = x[None].clone().requires_grad_(True), w.clone().requires_grad_(True)
        yt = F.conv_transpose3d(xt, wt, b, stride=2, padding=1)
        yt.backward(dy[None])
        err = lambda got, want: float((got - want).norm() / want.norm())          # noqa: E731
        row["check"] = {"y": err(y, yt.detach()[0]), "dx": err(dx, xt.grad[0]), "dw": err(dw, wt.grad)}
        assert max(row["check"].values()) < 1e-4, row["check"]
        out["levels"]["up%d" % lvl] = row
        del x, w, dy, y, dx, dw, ws, xt, wt, yt
        torch.cuda.empty_cache()
    tot = {k: sum(r[k]["mean"] for r in out["levels"].values()) for k in ("fwd", "bwd_data", "bwd_weight")}
    gf = sum(r["gflop_per_launch"] for r in out["levels"].values())
    out["all_levels"] = {k: {"ms": v, "tflops": gf / v, "fraction_of_fp32_peak": gf * 1e9 / (v * 1e-3) / FP32_PEAK} for k, v in tot.items()}
    print(json.dumps(out))


def make(patch, net, upsample, device):
    from deep_prior_interpolation_amd import utils as u
    from deep_prior_interpolation_amd.main import Interpolator
    from deep_prior_interpolation_amd.optim import FusedAdam
    from deep_prior_interpolation_amd.parameter import parse_arguments
    extra = ["--inittype", "kaiming"] if net == "unet" else []          # the up path of the plain UNet has no norm: xavier at gain 0.02 passes no gradient
    args = parse_arguments(["--imgdir", "synthetic", "--datadim", "3d", "--net", net, "--upsample", upsample, "--inputdepth", "64", "--loss", "mae",
                            "--lr", "1e-3", "--gain", "40", "--reg_noise_std", "0.03", "--noise_std", "0.1", "--epochs", "3000", "--gpu", "0"] + extra)
    vol = u.hyperbolic_volume(tuple(patch), seed=0)
    mask = u.random_trace_mask(tuple(patch), 0.66, seed=1)
    u.set_seed(0)
    T = Interpolator(args, "/tmp", device=device)
    T.load_data({"image": (vol * args.gain)[..., None], "mask": mask[..., None], "name": "0"})
    T.begin_patch(0)
    T.build_model()
    T.build_input()
    T.optimizer = FusedAdam(T.net.parameters(), lr=args.lr)
    return T


def run(T, iters, device):
    import torch
    from deep_prior_interpolation_amd import ops
    ops.set_weight_grad_overlap(T.wants_weight_grad_overlap(), in_graph=False)
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
    nets = [("unet", "deconv"), ("unet", "linear"), ("unet", "nearest"), ("multiunet", "nearest")]
    out = {"what": "ms per eager Adam iteration, --datadim 3d, fp32, 64 input channels, default widths", "iters_per_run": a.iters,
           "device": torch.cuda.get_device_name(0)}
    for p in patches:                                                  # one patch at a time: four nets of one size share the memory
        Ts = {n: make(p, n[0], n[1], dev) for n in nets}
        ms = {n: [] for n in nets}
        for T in Ts.values():
            run(T, a.warmup, dev)
        for _ in range(a.runs):
            for n, T in Ts.items():
                ms[n].append(run(T, a.iters, dev))
        out["x".join(str(s) for s in p)] = {"%s/%s" % n: dict(stat(ms[n]), params=int(Ts[n].num_params), last_loss=float(Ts[n].history.loss[-1]))
                                            for n in nets}
        del Ts
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="cmd", required=True)
    k = sub.add_parser("kernels")
    k.add_argument("--patch", type=int, nargs=3, default=[256, 128, 128])
    k.add_argument("--filters", type=int, nargs=5, default=[16, 32, 64, 128, 256])
    k.add_argument("--launches", type=int, default=20)
    k.add_argument("--rounds", type=int, default=3)
    e = sub.add_parser("e2e")
    e.add_argument("--patches", type=int, nargs="+", default=[64, 64, 64, 128, 64, 64, 256, 128, 128])
    e.add_argument("--iters", type=int, default=10)
    e.add_argument("--warmup", type=int, default=3)
    e.add_argument("--runs", type=int, default=3)
    a = ap.parse_args()
    {"kernels": kernels, "e2e": e2e}[a.cmd](a)
