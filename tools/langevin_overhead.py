"""Cost of the Langevin samplers at the bench geometry: ms per eager iteration (the loop optimize() runs at this size, one read-back per
iteration) of --optimizer adam, sgld and psgld on the same 256x128x128 patch (fp32, the bench's flags).  A sampler iteration adds the
moments pass (dpi_moments_update; --posterior_burnin 0, so every timed iteration is a sampled one) and replaces dpi_adam_multi by
dpi_langevin_multi.

    python tools/langevin_overhead.py [--runs 5] [--iters 20] [--warmup 5] [--patch 256 128 128] [--timeout 300]
    python tools/langevin_overhead.py --optimizer psgld ...       # one optimiser, in this process

Without --optimizer the three are measured one after the other, each in a process of its own under its own time limit (nothing else is
started after a failure), and one JSON line with the three results and the differences to adam is printed."""
import argparse
import json
import os
import subprocess
import sys
from time import perf_counter

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def make(patch, optimizer, device):
    from deep_prior_interpolation_amd import ops, utils as u
    from deep_prior_interpolation_amd.main import Interpolator
    from deep_prior_interpolation_amd.parameter import parse_arguments
    extra = [] if optimizer == "adam" else ["--posterior_burnin", "0"]
    args = parse_arguments(["--imgdir", "synthetic", "--datadim", "3d", "--net", "multiunet", "--inputdepth", "64", "--upsample", "nearest",
                            "--loss", "mae", "--lr", "1e-3", "--gain", "40", "--reg_noise_std", "0.03", "--noise_std", "0.1",
                            "--epochs", "3000", "--gpu", "0", "--optimizer", optimizer] + extra)
    vol = u.hyperbolic_volume(tuple(patch), seed=0)
    mask = u.random_trace_mask(tuple(patch), 0.66, seed=1)
    T = Interpolator(args, "/tmp", device=device)
    T.load_data({"image": (vol * args.gain)[..., None], "mask": mask[..., None], "name": "0"})
    T.begin_patch(0)
    T.build_model()
    T.build_input()
    T.optimizer = T.make_optimizer()
    T._big = T.wants_weight_grad_overlap()
    ops.set_weight_grad_overlap(T._big, in_graph=False)
    return T


def run(T, iters, device):
    torch.cuda.synchronize(device)
    t0 = perf_counter()
    for _ in range(iters):
        T.optimizer.zero_grad()
        T.optimization_loop()
        T.optimizer.step()
    torch.cuda.synchronize(device)
    return (perf_counter() - t0) * 1e3 / iters


def measure(a):
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    T = make(a.patch, a.optimizer, device)
    run(T, a.warmup, device)
    ms = [run(T, a.iters, device) for _ in range(a.runs)]
    return {"optimizer": a.optimizer, "patch": a.patch, "runs": a.runs, "iters": a.iters, "per_run": [round(v, 3) for v in ms],
            "mean": round(float(np.mean(ms)), 3), "median": round(float(np.median(ms)), 3), "spread": round(float(np.max(ms) - np.min(ms)), 3),
            "final_loss": float(T.history.loss[-1]), "gpu": torch.cuda.get_device_name(device)}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--optimizer", choices=["adam", "sgld", "psgld"])
    p.add_argument("--runs", type=int, default=5)
    p.add_argument("--iters", type=int, default=20)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--patch", type=int, nargs=3, default=[256, 128, 128])
    p.add_argument("--timeout", type=float, default=300.0, help="seconds per child process")
    a = p.parse_args()
    if a.optimizer is not None:
        print(json.dumps(measure(a)))
        return
    res = {}
    for opt in ("adam", "sgld", "psgld"):
        cmd = [sys.executable, os.path.abspath(__file__), "--optimizer", opt, "--runs", str(a.runs), "--iters", str(a.iters),
               "--warmup", str(a.warmup), "--patch"] + [str(v) for v in a.patch]
        out = subprocess.run(cmd, timeout=a.timeout, check=True, stdout=subprocess.PIPE).stdout.decode()      # raises: nothing more is started
        res[opt] = json.loads(out.strip().splitlines()[-1])
    base = res["adam"]["median"]
    print(json.dumps({"results": res, "extra_ms": {k: round(res[k]["median"] - base, 3) for k in ("sgld", "psgld")},
                      "extra_percent": {k: round(100.0 * (res[k]["median"] - base) / base, 2) for k in ("sgld", "psgld")}}))


if __name__ == "__main__":
    main()
