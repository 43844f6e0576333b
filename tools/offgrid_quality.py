"""What --trace_offsets gives and what it costs.

Quality (default): the 48x32x32 stand-in recorded OFF the grid (utils/synthetic.hyperbolic_traces: the events of hyperbolic_volume evaluated
analytically at x + dx, y + dy), offsets uniform in [-0.5, 0.5] cells, 66 % of the traces missing, the bench's flags.  Measured PAIRED: the
same traces, mask and seed once without the flag (every trace taken to sit on its node, as the reference does) and once with it.  The figure
is the SNR of the selected GRID output against the analytic on-grid truth, hyperbolic_volume(..., background=0), which neither run has seen.
One JSON line per run, then the summary: mean paired difference +- 2 s.e. over the seeds.

    python tools/offgrid_quality.py [--seeds 0 .. 5] [--epochs 3000] [--patch 48 32 32] [--missing 0.66] [--out file.json]

--interp NAME ... (linear, cubic, sinc8: --trace_interp) compares sampling kernels instead: the same traces, mask and seed once per named
kind, all with --trace_offsets, `linear` always among them as the baseline of the paired differences.  Each row also carries the modelling
floor of its kind, computed on the host: the SNR of R(truth) against the recorded traces, i.e. the best data fit a perfect grid output
could reach through that operator.

Cost (--cost): one process, two Interpolators on the same 256x128x128 patch (fp32, the bench's flags), one without the flag and one with
random offsets, timed in alternating runs of --iters eager iterations each (the loop optimize() runs at this size).  --parent-tree DIR names a
built checkout of the commit this one is compared with: its loop is timed in the same call, in a fresh child process that imports the
package from DIR, before and after this tree's runs.  One JSON line.  With --interp NAME ... there is one Interpolator per named kind next to
the one without the flag, all alternating in the one process, and the increments are given over the no-flag loop and over `linear`.

    python tools/offgrid_quality.py --cost [--runs 5] [--iters 20] [--warmup 5] [--patch 256 128 128] [--parent-tree DIR] [--interp NAME ...]
"""
import argparse
import json
import os
import subprocess
import sys
from time import perf_counter

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FLAGS = ["--imgdir", "synthetic", "--datadim", "3d", "--net", "multiunet", "--inputdepth", "64", "--loss", "mae", "--lr", "1e-3", "--gain", "40",
         "--reg_noise_std", "0.03", "--noise_std", "0.1", "--gpu", "0"]


def snr_db(ref, got, where=None):
    ref, got = np.asarray(ref, np.float64), np.asarray(got, np.float64)
    if where is not None:
        ref, got = ref[where], got[where]
    return float(10.0 * np.log10(np.sum(ref ** 2) / np.sum((ref - got) ** 2)))


def random_offsets(shape, seed=2):
    return np.random.RandomState(seed).uniform(-0.5, 0.5, tuple(shape[1:]) + (2,)).astype(np.float32)


def kinds_of(a):
    """--interp as given, `linear` first and once: the baseline of every paired difference."""
    return ["linear"] + [k for k in dict.fromkeys(a.interp) if k != "linear"]


def modelling_floor(shape, off, interp):
    """snr(R(truth), traces) in float64 on the host, R from the library's weight table of `interp`: what a perfect grid output would score
    against the recorded traces through that operator."""
    from deep_prior_interpolation_amd import utils as u
    from deep_prior_interpolation_amd.operators import INTERP_TAPS, interp_weights
    truth = u.hyperbolic_volume(shape, seed=0, background=0).astype(np.float64)
    traces = u.hyperbolic_traces(shape, off, seed=0).astype(np.float64)
    o = np.moveaxis(off, -1, 0)
    w = interp_weights(o, interp).astype(np.float64)
    K, (X, Y) = INTERP_TAPS[interp], shape[1:]
    tx = [np.clip(np.arange(X)[:, None] - K // 2 + (o[0] >= 0) + k, 0, X - 1) for k in range(K)]
    ty = [np.clip(np.arange(Y)[None, :] - K // 2 + (o[1] >= 0) + k, 0, Y - 1) for k in range(K)]
    got = np.zeros_like(truth)
    for kx in range(K):
        inner = np.zeros_like(truth)
        for ky in range(K):
            inner += w[1, ky] * truth[:, tx[kx], ty[ky]]
        got += w[0, kx] * inner
    return snr_db(traces, got)


# ---------------------------------------------------------------- quality ---------------------------------------------------------
def one(flag, seed, a, interp=None):
    from deep_prior_interpolation_amd import utils as u
    from deep_prior_interpolation_amd.main import Interpolator
    from deep_prior_interpolation_amd.parameter import parse_arguments
    args = parse_arguments(FLAGS + ["--upsample", "linear", "--epochs", str(a.epochs)] + (["--trace_offsets", "offsets.npy"] if flag else [])
                           + (["--trace_interp", interp] if interp else []))
    shape = tuple(a.patch)
    off = random_offsets(shape)
    traces = u.hyperbolic_traces(shape, off, seed=0).astype(np.float64) * args.gain           # what was recorded
    truth = u.hyperbolic_volume(shape, seed=0, background=0).astype(np.float64) * args.gain   # what a regular acquisition would have recorded
    mask = u.random_trace_mask(shape, a.missing, seed=1).astype(np.float64)
    data = {"image": traces[..., None], "mask": mask[..., None], "name": "0"}
    if flag:
        data["offsets"] = off
    u.set_seed(seed)
    T = Interpolator(args, "/tmp", seed=seed)
    T.load_data(data)
    T.begin_patch(seed)
    T.build_model()
    T.build_input()
    T.optimize(verbose=False)
    out = np.asarray(T.out_best, dtype=np.float64).reshape(shape)
    return {"flag": bool(flag), **({"interp": interp} if interp else {}), "seed": seed, "epochs": len(T.history.loss), "finite": bool(np.isfinite(T.history.loss).all()),
            "snr_db": snr_db(truth, out), "snr_known_db": snr_db(truth, out, mask > 0), "snr_missing_db": snr_db(truth, out, mask == 0),
            "snr_traces_vs_truth_db": snr_db(truth, traces, mask > 0),          # how far the recorded traces are from the grid's
            "loss_min": float(np.min(T.history.loss)), "ms_per_iter": round(1e3 * T.elapsed / len(T.history.loss), 3)}


def summary(rows):
    seeds = sorted({r["seed"] for r in rows if any(q["seed"] == r["seed"] and q["flag"] != r["flag"] for q in rows)})
    if not seeds:
        return []
    get = lambda s, flag, k: next(r[k] for r in rows if r["seed"] == s and r["flag"] == flag)
    out = {"summary": True, "seeds": len(seeds)}
    for k in ("snr_db", "snr_known_db", "snr_missing_db"):
        d = np.array([get(s, True, k) - get(s, False, k) for s in seeds])
        out[k] = {"off_mean": round(float(np.mean([get(s, False, k) for s in seeds])), 3),
                  "on_mean": round(float(np.mean([get(s, True, k) for s in seeds])), 3),
                  "paired_diff_mean": round(float(d.mean()), 3),
                  "paired_diff_2se": round(float(2.0 * d.std(ddof=1) / np.sqrt(len(d))), 3) if len(d) > 1 else None,
                  "paired_diff_min": round(float(d.min()), 3), "paired_diff_max": round(float(d.max()), 3)}
    return [out]


def summary_interp(rows, kinds):
    """Paired differences of every kind against `linear` over the seeds that have both, next to each kind's floor."""
    out = []
    for kind in kinds[1:]:
        seeds = sorted({r["seed"] for r in rows if r["interp"] == kind} & {r["seed"] for r in rows if r["interp"] == "linear"})
        if not seeds:
            continue
        get = lambda s, i, k: next(r[k] for r in rows if r["seed"] == s and r["interp"] == i)
        res = {"summary": True, "interp": kind, "against": "linear", "seeds": len(seeds),
               "floor_db": get(seeds[0], kind, "floor_db"), "floor_linear_db": get(seeds[0], "linear", "floor_db")}
        for k in ("snr_db", "snr_known_db", "snr_missing_db"):
            d = np.array([get(s, kind, k) - get(s, "linear", k) for s in seeds])
            res[k] = {"linear_mean": round(float(np.mean([get(s, "linear", k) for s in seeds])), 3),
                      "mean": round(float(np.mean([get(s, kind, k) for s in seeds])), 3),
                      "paired_diff_mean": round(float(d.mean()), 3),
                      "paired_diff_2se": round(float(2.0 * d.std(ddof=1) / np.sqrt(len(d))), 3) if len(d) > 1 else None,
                      "paired_diff_min": round(float(d.min()), 3), "paired_diff_max": round(float(d.max()), 3)}
        out.append(res)
    return out


def quality_interp(a):
    import torch
    torch.cuda.set_device(0)
    kinds = kinds_of(a)
    shape = tuple(a.patch)
    floor = {k: round(modelling_floor(shape, random_offsets(shape), k), 3) for k in kinds}
    rows = []
    for seed in a.seeds:                   # seeds outermost: a run that is cut short still has whole groups
        for kind in kinds:
            rows.append(dict(one(True, seed, a, interp=kind), floor_db=floor[kind]))
            print(json.dumps(rows[-1]), flush=True)
            if a.out:
                with open(a.out, "w") as f:
                    json.dump(rows + summary_interp(rows, kinds), f, indent=1)
    for s in summary_interp(rows, kinds):
        print(json.dumps(s), flush=True)


def quality(a):
    if a.interp:
        return quality_interp(a)
    import torch
    torch.cuda.set_device(0)
    rows = []
    for seed in a.seeds:                   # seeds outermost: a run that is cut short still has whole pairs
        for flag in (False, True):
            rows.append(one(flag, seed, a))
            print(json.dumps(rows[-1]), flush=True)
            if a.out:
                with open(a.out, "w") as f:
                    json.dump(rows + summary(rows), f, indent=1)
    for s in summary(rows):
        print(json.dumps(s), flush=True)


# ---------------------------------------------------------------- cost ------------------------------------------------------------
def make(patch, flag, device, interp=None):
    from deep_prior_interpolation_amd import ops, utils as u
    from deep_prior_interpolation_amd.main import Interpolator
    from deep_prior_interpolation_amd.optim import FusedAdam
    from deep_prior_interpolation_amd.parameter import parse_arguments
    args = parse_arguments(FLAGS + ["--upsample", "nearest", "--epochs", "3000"] + (["--trace_offsets", "offsets.npy"] if flag else [])
                           + (["--trace_interp", interp] if interp else []))
    vol = u.hyperbolic_volume(tuple(patch), seed=0)
    mask = u.random_trace_mask(tuple(patch), 0.66, seed=1)
    data = {"image": (vol * args.gain)[..., None], "mask": mask[..., None], "name": "0"}
    if flag:
        data["offsets"] = random_offsets(patch)
    T = Interpolator(args, "/tmp", device=device)
    T.load_data(data)
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
    T = make(a.patch, False, device)
    run(T, a.warmup, device)
    print(json.dumps(stat([run(T, a.iters, device) for _ in range(a.runs)])))


def time_tree(root, a):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--root", root, "--runs", str(a.runs), "--iters", str(a.iters),
           "--warmup", str(a.warmup), "--patch"] + [str(p) for p in a.patch]
    out = subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=600).stdout
    return json.loads(out.strip().splitlines()[-1])


def cost(a):
    parent = []
    if a.parent_tree:
        parent.append(time_tree(os.path.abspath(a.parent_tree), a))         # before this process opens the device
    import torch
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    if a.interp:
        Ts = {"off": make(a.patch, False, device)}
        Ts.update({k: make(a.patch, True, device, interp=k) for k in kinds_of(a)})
    else:
        Ts = {"off": make(a.patch, False, device), "on": make(a.patch, True, device)}
    for T in Ts.values():
        run(T, a.warmup, device)
    ms = {k: [] for k in Ts}
    for r in range(a.runs):
        for k in (list(Ts) if r % 2 == 0 else list(Ts)[::-1]):               # alternate the order: no side gets the warmer slot
            ms[k].append(run(Ts[k], a.iters, device))
    res = {"patch": a.patch, "runs": a.runs, "iters": a.iters, "gpu": torch.cuda.get_device_name(device)}
    res.update({k + "_ms": stat(v) for k, v in ms.items()})
    if a.interp:
        res["diff_vs_off_ms"] = {k: round(res[k + "_ms"]["mean"] - res["off_ms"]["mean"], 3) for k in Ts if k != "off"}
        res["diff_vs_linear_ms"] = {k: round(res[k + "_ms"]["mean"] - res["linear_ms"]["mean"], 3) for k in Ts if k not in ("off", "linear")}
    else:
        res["diff_ms"] = round(res["on_ms"]["mean"] - res["off_ms"]["mean"], 3)
    if a.parent_tree:
        torch.cuda.synchronize(device)
        parent.append(time_tree(os.path.abspath(a.parent_tree), a))
        res["parent_ms"] = parent
        pm = float(np.mean([q["mean"] for q in parent]))
        res["off_vs_parent_ms"] = round(res["off_ms"]["mean"] - pm, 3)
        if not a.interp:
            res["on_vs_parent_ms"] = round(res["on_ms"]["mean"] - pm, 3)
    print(json.dumps(res))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--seeds", type=int, nargs="+", default=list(range(6)))
    p.add_argument("--epochs", type=int, default=3000)
    p.add_argument("--patch", type=int, nargs=3, default=None)
    p.add_argument("--missing", type=float, default=0.66)
    p.add_argument("--out", default=None)
    p.add_argument("--interp", nargs="+", default=None, choices=["linear", "cubic", "sinc8"],
                   help="compare these --trace_interp kinds (linear is always included) instead of the flag against no flag")
    p.add_argument("--cost", action="store_true")
    p.add_argument("--runs", type=int, default=5)
    p.add_argument("--iters", type=int, default=20)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--parent-tree", default=None)
    p.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    p.add_argument("--root", default=ROOT, help=argparse.SUPPRESS)
    a = p.parse_args()
    if a.patch is None:
        a.patch = [256, 128, 128] if (a.cost or a.child) else [48, 32, 32]
    if a.child:
        return child(a)
    sys.path.insert(0, ROOT)
    return cost(a) if a.cost else quality(a)


if __name__ == "__main__":
    main()
