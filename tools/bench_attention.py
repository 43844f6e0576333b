"""Timings of the attention gate (--net attmultiunet) on the GPU.  Two measurements, each prints one JSON line:

    python tools/bench_attention.py kernels [--channels 25] [--fine 256 128 128] [--launches 1000] [--rounds 3]
        dpi_chain_apply (the yardstick: it moves the same 2 C V floats as the gate's forward), dpi_attn_gate_fwd and dpi_attn_gate_bwd on a
        C-channel tensor of the given fine size, HIP events around `launches` back-to-back calls of one entry point, the three alternating
        for `rounds` rounds.  ms per call, the bytes each must move, TB/s, the ratios to chain_apply with their targets
        (forward <= 1.25 x, backward <= 1.25 x 1.5 x: its first pass moves 3 C V floats), and the error of what the timed calls left in
        y, dx and the workspace against torch's up-sampling on the device.
    python tools/bench_attention.py e2e [--patch 256 128 128] [--iters 20] [--warmup 5] [--runs 3] [--nets attmultiunet multiunet]
        ms per eager iteration of --datadim 3d with the default filters, fp32, for each net, in alternating runs.

The split of an entry point into its launches (attn_sigmoid_kernel / attn_gate_fwd_kernel; attn_gate_bwd_kernel / attn_gate_bwd_q_kernel) and
the share of the gate launches in an iteration come from a kernel trace of the same commands with small counts, in a run of its own:
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/bench_attention.py kernels --launches 20 --rounds 1
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/bench_attention.py e2e --nets attmultiunet --iters 5 --warmup 2 --runs 1
"""
import argparse
import json
import os
import sys
from time import perf_counter

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stat(vs):
    return {"mean": float(np.mean(vs)), "min": float(np.min(vs)), "max": float(np.max(vs)), "runs": [float(v) for v in vs]}


def kernels(a):
    import torch
    from deep_prior_interpolation_amd import _lib
    from deep_prior_interpolation_amd._lib import check, ptr, stream
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    L = _lib.load()
    dev = torch.device("cuda", 0)
    C = a.channels
    Do, Ho, Wo = a.fine
    assert Do % 2 == 0 and Ho % 2 == 0 and Wo % 2 == 0
    D, H, W = Do // 2, Ho // 2, Wo // 2
    V = Do * Ho * Wo
    gen = torch.Generator().manual_seed(0)
    x = torch.randn((C, V), generator=gen).to(dev)
    dy = torch.randn((C, V), generator=gen).to(dev)
    q = torch.randn((D * H * W,), generator=gen).to(dev)
    y, dx = torch.empty_like(x), torch.empty_like(x)
    s, dq = torch.empty_like(q), torch.empty_like(q)
    ws = torch.empty(L.dpi_attn_gate_bwd_ws_floats(C, D, H, W, 1), dtype=torch.float32, device=dev)
    chain = torch.tensor([1.0, 0.0, 0.2, 1.0, 0.0]).repeat(C, 1).to(dev).contiguous()
    st = stream()
    calls = {
        "chain_apply": lambda: check(L.dpi_chain_apply(ptr(x), ptr(chain), C, V, ptr(y), st), "dpi_chain_apply"),
        "gate_fwd": lambda: check(L.dpi_attn_gate_fwd(ptr(x), ptr(q), C, D, H, W, 1, ptr(s), ptr(y), st), "dpi_attn_gate_fwd"),
        "gate_bwd": lambda: check(L.dpi_attn_gate_bwd(ptr(dy), ptr(x), ptr(s), C, D, H, W, 1, ptr(dx), ptr(dq), ptr(ws), st), "dpi_attn_gate_bwd"),
    }
    floats = {"chain_apply": 2 * C * V, "gate_fwd": 2 * C * V + V // 4, "gate_bwd": 3 * C * V + 2 * V + V // 4}
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
    out = {"what": "attention gate kernels", "channels": C, "fine": [Do, Ho, Wo], "launches_per_figure": a.launches, "device": torch.cuda.get_device_name(0)}
    for k in calls:
        out[k] = dict(stat(ms[k]), bytes=4 * floats[k], tb_per_s=4 * floats[k] / (np.mean(ms[k]) * 1e-3) / 1e12)
    # what was timed is also right at this size (the large-tensor code path): against torch's own up-sampling on the device
    import torch.nn.functional as F
    gate = F.interpolate(torch.sigmoid(q).view(1, 1, D, H, W), scale_factor=2, mode="trilinear", align_corners=False).view(1, V)
    err = lambda got, want: float((got - want).norm() / want.norm())          # noqa: E731
    out["check"] = {"y": err(y, x * gate), "dx": err(dx, dy * gate), "t": err(ws, (dy * x).sum(0))}
    del gate
    assert max(out["check"].values()) < 1e-5, out["check"]
    base = out["chain_apply"]["mean"]
    out["fwd_over_chain_apply"] = {"ratio": out["gate_fwd"]["mean"] / base, "target": 1.25}
    out["bwd_over_chain_apply"] = {"ratio": out["gate_bwd"]["mean"] / base, "target": 1.25 * 1.5}
    print(json.dumps(out))


def make(net, patch, device):
    from deep_prior_interpolation_amd import ops, utils as u
    from deep_prior_interpolation_amd.main import Interpolator
    from deep_prior_interpolation_amd.optim import FusedAdam
    from deep_prior_interpolation_amd.parameter import parse_arguments
    args = parse_arguments(["--imgdir", "synthetic", "--datadim", "3d", "--net", net, "--inputdepth", "64", "--upsample", "nearest", "--loss", "mae",
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
    T._big = T.wants_weight_grad_overlap()
    ops.set_weight_grad_overlap(T._big, in_graph=False)
    return T


def run(T, iters, device):
    import torch
    from deep_prior_interpolation_amd import ops
    ops.set_weight_grad_overlap(T._big, in_graph=False)          # what optimize() sets for this patch
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
    from deep_prior_interpolation_amd import ops
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    dev = torch.device("cuda", 0)
    Ts = {net: make(net, a.patch, dev) for net in a.nets}
    ms = {net: [] for net in a.nets}
    try:
        for net, T in Ts.items():
            run(T, a.warmup, dev)
        for _ in range(a.runs):
            for net, T in Ts.items():
                ms[net].append(run(T, a.iters, dev))
    finally:
        ops.set_weight_grad_overlap(False)
    out = {"what": "ms per eager iteration, --datadim 3d, fp32, default filters", "patch": list(a.patch), "iters_per_run": a.iters,
           "device": torch.cuda.get_device_name(0)}
    for net, T in Ts.items():
        out[net] = dict(stat(ms[net]), params=int(T.num_params), last_loss=float(T.history.loss[-1]) if T.history.loss else None)
    if len(a.nets) == 2:
        out["ratio"] = out[a.nets[0]]["mean"] / out[a.nets[1]]["mean"]
    print(json.dumps(out))


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="cmd", required=True)
    k = sub.add_parser("kernels")
    k.add_argument("--channels", type=int, default=25)
    k.add_argument("--fine", type=int, nargs=3, default=[256, 128, 128])
    k.add_argument("--launches", type=int, default=1000)
    k.add_argument("--rounds", type=int, default=3)
    e = sub.add_parser("e2e")
    e.add_argument("--patch", type=int, nargs=3, default=[256, 128, 128])
    e.add_argument("--iters", type=int, default=20)
    e.add_argument("--warmup", type=int, default=5)
    e.add_argument("--runs", type=int, default=3)
    e.add_argument("--nets", nargs="+", default=["attmultiunet", "multiunet"])
    a = ap.parse_args()
    {"kernels": kernels, "e2e": e2e}[a.cmd](a)
