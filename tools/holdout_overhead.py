"""Cost of --holdout at the bench geometry: one process, two Interpolators on the same 256x128x128 patch (fp32, the bench's flags), one
without a holdout and one with --holdout 0.05, timed in alternating runs of --iters eager iterations each (the loop optimize() runs at this
size, one read-back per iteration).  Prints one JSON line: ms per iteration of every run, their mean / spread, and the difference.

    python tools/holdout_overhead.py [--runs 5] [--iters 20] [--warmup 5] [--holdout 0.05] [--patch 256 128 128]

The loss pass itself is compared with `rocprofv3 --kernel-trace --stats --output-format csv -- python tools/holdout_overhead.py --runs 2 --iters 5
--warmup 2` (profiles/holdout/holdout_kernel_stats_loss.csv):
loss_holdout_partial_kernel against loss_partial_kernel in the same trace."""
import argparse
import json
import os
import sys
from time import perf_counter

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def make(patch, holdout, device):
    from deep_prior_interpolation_amd import ops, utils as u
    from deep_prior_interpolation_amd.main import Interpolator
    from deep_prior_interpolation_amd.optim import FusedAdam
    from deep_prior_interpolation_amd.parameter import parse_arguments
    args = parse_arguments(["--imgdir", "synthetic", "--datadim", "3d", "--net", "multiunet", "--inputdepth", "64", "--upsample", "nearest",
                            "--loss", "mae", "--lr", "1e-3", "--gain", "40", "--reg_noise_std", "0.03", "--noise_std", "0.1",
                            "--epochs", "3000", "--gpu", "0", "--holdout", str(holdout)])
    vol = u.hyperbolic_volume(tuple(patch), seed=0)
    mask = u.random_trace_mask(tuple(patch), 0.66, seed=1)
    T = Interpolator(args, "/tmp", device=device)
    T.load_data({"image": (vol * args.gain)[..., None], "mask": mask[..., None], "name": "0"})
    T.begin_patch(0)
    T.build_model()
    T.build_input()
    T.build_holdout()
    T.optimizer = FusedAdam(T.net.parameters(), lr=args.lr)
    T._big = T.wants_weight_grad_overlap()
    ops.set_weight_grad_overlap(T._big, in_graph=False)
    return T


def run(T, iters, device):
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


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--runs", type=int, default=5)
    p.add_argument("--iters", type=int, default=20)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--holdout", type=float, default=0.05)
    p.add_argument("--patch", type=int, nargs=3, default=[256, 128, 128])
    a = p.parse_args()
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    Ts = {"off": make(a.patch, 0.0, device), "holdout": make(a.patch, a.holdout, device)}
    for T in Ts.values():
        run(T, a.warmup, device)
    ms = {k: [] for k in Ts}
    for r in range(a.runs):
        for k in (("off", "holdout") if r % 2 == 0 else ("holdout", "off")):           # alternate the order: no side gets the warmer slot
            ms[k].append(run(Ts[k], a.iters, device))
    stat = {k + "_ms": {"per_run": [round(v, 3) for v in vs], "mean": round(float(np.mean(vs)), 3),
                "spread": round(float(np.max(vs) - np.min(vs)), 3)} for k, vs in ms.items()}
    T = Ts["holdout"]
    print(json.dumps({"patch": a.patch, "frac": a.holdout, "runs": a.runs, "iters": a.iters,
                      "held_traces": int(T.holdout_sel.sum()), "known_traces": int((T.mask != 0).any(axis=0).sum()),
                      "gpu": torch.cuda.get_device_name(device), **stat,
                      "diff_ms": round(stat["holdout_ms"]["mean"] - stat["off_ms"]["mean"], 3)}))


if __name__ == "__main__":
    main()
