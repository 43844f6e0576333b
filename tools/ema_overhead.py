"""Cost of --out_ema at the bench geometry: one process, two Interpolators on the same 256x128x128 patch (fp32, the bench's flags), one
without the flag and one with --out_ema 0.99, timed in alternating runs of --iters eager iterations each (the loop optimize() runs at this
size, one read-back per iteration).  Prints one JSON line: ms per iteration of every run, their mean / spread, and the difference.

    python tools/ema_overhead.py [--runs 5] [--iters 20] [--warmup 5] [--beta 0.99] [--patch 256 128 128] [--parent-tree DIR]

--parent-tree DIR: a built checkout of the commit this one is compared with.  Its Adam loop (no flag: it has none) is timed in the same call,
in a fresh child process that imports the package from DIR, before and after this tree's runs; `parent_ms` holds both, `off_vs_parent_ms`
says what the flag costs a run that does not use it.

The pass itself is compared with `rocprofv3 --kernel-trace --stats --output-format csv -- python tools/ema_overhead.py --runs 2 --iters 5
--warmup 2` (profiles/ema/ema_kernel_stats_loss.csv): ema_loss_partial_kernel against loss_partial_kernel in the same trace."""
import argparse
import json
import os
import subprocess
import sys
from time import perf_counter

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def make(patch, beta, device):
    from deep_prior_interpolation_amd import ops, utils as u
    from deep_prior_interpolation_amd.main import Interpolator
    from deep_prior_interpolation_amd.optim import FusedAdam
    from deep_prior_interpolation_amd.parameter import parse_arguments
    args = parse_arguments(["--imgdir", "synthetic", "--datadim", "3d", "--net", "multiunet", "--inputdepth", "64", "--upsample", "nearest",
                            "--loss", "mae", "--lr", "1e-3", "--gain", "40", "--reg_noise_std", "0.03", "--noise_std", "0.1",
                            "--epochs", "3000", "--gpu", "0"] + (["--out_ema", str(beta)] if beta else []))
    vol = u.hyperbolic_volume(tuple(patch), seed=0)
    mask = u.random_trace_mask(tuple(patch), 0.66, seed=1)
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


def stat(vs):
    return {"per_run": [round(v, 3) for v in vs], "mean": round(float(np.mean(vs)), 3), "spread": round(float(np.max(vs) - np.min(vs)), 3)}


def child(a):
    """The no-flag loop of the tree at a.root (this one or another commit's), alone in its process: one JSON line."""
    sys.path.insert(0, a.root)
    import torch
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    T = make(a.patch, 0.0, device)
    run(T, a.warmup, device)
    print(json.dumps(stat([run(T, a.iters, device) for _ in range(a.runs)])))


def time_tree(root, a):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--root", root, "--runs", str(a.runs), "--iters", str(a.iters),
           "--warmup", str(a.warmup), "--patch"] + [str(p) for p in a.patch]
    out = subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=600).stdout
    return json.loads(out.strip().splitlines()[-1])


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--runs", type=int, default=5)
    p.add_argument("--iters", type=int, default=20)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--beta", type=float, default=0.99)
    p.add_argument("--patch", type=int, nargs=3, default=[256, 128, 128])
    p.add_argument("--parent-tree", default=None)
    p.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    p.add_argument("--root", default=ROOT, help=argparse.SUPPRESS)
    a = p.parse_args()
    if a.child:
        return child(a)
    parent = []
    if a.parent_tree:
        parent.append(time_tree(os.path.abspath(a.parent_tree), a))         # before this process opens the device
    sys.path.insert(0, ROOT)
    import torch
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    Ts = {"off": make(a.patch, 0.0, device), "ema": make(a.patch, a.beta, device)}
    for T in Ts.values():
        run(T, a.warmup, device)
    ms = {k: [] for k in Ts}
    for r in range(a.runs):
        for k in (("off", "ema") if r % 2 == 0 else ("ema", "off")):           # alternate the order: no side gets the warmer slot
            ms[k].append(run(Ts[k], a.iters, device))
    res = {"patch": a.patch, "beta": a.beta, "runs": a.runs, "iters": a.iters, "gpu": torch.cuda.get_device_name(device),
           "off_ms": stat(ms["off"]), "ema_ms": stat(ms["ema"])}
    res["diff_ms"] = round(res["ema_ms"]["mean"] - res["off_ms"]["mean"], 3)
    if a.parent_tree:
        torch.cuda.synchronize(device)
        parent.append(time_tree(os.path.abspath(a.parent_tree), a))
        res["parent_ms"] = parent
        pm = float(np.mean([q["mean"] for q in parent]))
        res["off_vs_parent_ms"] = round(res["off_ms"]["mean"] - pm, 3)
        res["ema_vs_parent_ms"] = round(res["ema_ms"]["mean"] - pm, 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
