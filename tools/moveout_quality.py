"""What --moveout gives and what it costs.

Quality (default): the stand-in (utils/synthetic.hyperbolic_volume: hyperbolic events with the apex at (0, 0) and the moveout law
c(tau) = 0.9 - 0.3 tau / nt, jittered by +-0.04 per event), the bench's flags.  The table is operators.nmo_table on the MEAN law, so the
jitter stays in as residual moveout; it mutes the empty part of the cube above the first event (about two thirds of it).  Measured PAIRED:
the same traces, mask and seed once without the flag and once per --interp with it.  Two mask kinds, reported separately: `random` = 66 % of
the traces missing at random, `regular` = every third trace along x kept.  The figure is the SNR of the selected output against the
complete volume over the LIVE samples, for every arm.  One JSON line per run, then per mask kind and interp the mean paired difference
+- 2 s.e. over the seeds.

    python tools/moveout_quality.py [--seeds 0 .. 5] [--epochs 3000] [--patch 48 32 32] [--masks random regular] [--interp linear cubic] [--out f.json]

Cost (--cost): the protocol of tools/offgrid_quality.py --cost.  One process, Interpolators on the same 256x128x128 patch (fp32, the bench's
flags), one without the flag and one per --interp with the NMO table, timed in alternating runs of --iters eager iterations each.
--parent-tree DIR names a built checkout of the commit this one is compared with: its no-flag loop is timed in a fresh child process that
imports the package from DIR, before and after this tree's runs.  One JSON line.

    python tools/moveout_quality.py --cost [--runs 5] [--iters 20] [--warmup 5] [--patch 256 128 128] [--parent-tree DIR]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import offgrid_quality as OQ          # noqa: E402  (FLAGS, snr_db, run, stat, time_tree: one timing protocol for the tools)


def standin_table(shape):
    """nmo_table of the stand-in's mean law: offset = nt * r with r the normalised distance from the apex, velocity = 1 / c(tau)."""
    from deep_prior_interpolation_amd.operators import nmo_table
    nt, nx, ny = shape
    off = nt * np.sqrt((np.arange(nx)[:, None] / max(nx, 1)) ** 2 + (np.arange(ny)[None, :] / max(ny, 1)) ** 2)
    return nmo_table(shape, off, lambda tau: 1.0 / (0.9 - 0.3 * tau / nt))


def trace_mask(kind, shape, missing):
    from deep_prior_interpolation_amd import utils as u
    if kind == "random":
        return u.random_trace_mask(shape, missing, seed=1).astype(np.float64)
    m = np.zeros(shape, dtype=np.float64)
    m[:, ::3] = 1.0                                              # regular decimation: every third trace along x
    return m


def flags_for(interp, rest):
    return OQ.FLAGS + (["--moveout", "tau.npy", "--moveout_interp", interp] if interp else []) + rest


# ---------------------------------------------------------------- quality ---------------------------------------------------------
def one(interp, seed, mask_kind, a):
    from deep_prior_interpolation_amd import utils as u
    from deep_prior_interpolation_amd.main import Interpolator
    from deep_prior_interpolation_amd.parameter import parse_arguments
    shape = tuple(a.patch)
    args = parse_arguments(flags_for(interp, ["--upsample", "linear", "--epochs", str(a.epochs)]))
    truth = u.hyperbolic_volume(shape, seed=0).astype(np.float64) * args.gain
    mask = trace_mask(mask_kind, shape, a.missing)
    table = standin_table(shape)
    live = (table >= 0) & (table <= shape[0] - 1)
    data = {"image": truth[..., None], "mask": mask[..., None], "name": "0"}
    if interp:
        data["moveout"] = table
    u.set_seed(seed)
    T = Interpolator(args, "/tmp", seed=seed)
    T.load_data(data)
    T.begin_patch(seed)
    T.build_model()
    T.build_input()
    T.optimize(verbose=False)
    out = np.asarray(T.out_best, dtype=np.float64).reshape(shape)
    return {"flag": bool(interp), "interp": interp, "mask": mask_kind, "seed": seed, "epochs": len(T.history.loss),
            "finite": bool(np.isfinite(T.history.loss).all()), "live_share": round(float(live.mean()), 4),
            "snr_db": OQ.snr_db(truth, out, live), "snr_known_db": OQ.snr_db(truth, out, live & (mask > 0)),
            "snr_missing_db": OQ.snr_db(truth, out, live & (mask == 0)), "snr_all_samples_db": OQ.snr_db(truth, out),
            "loss_min": float(np.min(T.history.loss)), "ms_per_iter": round(1e3 * T.elapsed / len(T.history.loss), 3)}


def summaries(rows, a):
    out = []
    for mk in a.masks:
        for interp in a.interp:
            sub = [r for r in rows if r["mask"] == mk and r["interp"] in (None, interp)]
            for s in OQ.summary(sub):
                out.append(dict(s, mask=mk, interp=interp, patch=a.patch, epochs=a.epochs))
    return out


def quality(a):
    import torch
    torch.cuda.set_device(0)
    rows = []
    for seed in a.seeds:                   # seeds outermost: a run that is cut short still has whole groups
        for mk in a.masks:
            for interp in [None] + list(a.interp):
                rows.append(one(interp, seed, mk, a))
                print(json.dumps(rows[-1]), flush=True)
                if a.out:
                    with open(a.out, "w") as f:
                        json.dump(rows + summaries(rows, a), f, indent=1)
    for s in summaries(rows, a):
        print(json.dumps(s), flush=True)


# ---------------------------------------------------------------- cost ------------------------------------------------------------
def make(patch, interp, device):
    from deep_prior_interpolation_amd import ops, utils as u
    from deep_prior_interpolation_amd.main import Interpolator
    from deep_prior_interpolation_amd.optim import FusedAdam
    from deep_prior_interpolation_amd.parameter import parse_arguments
    args = parse_arguments(flags_for(interp, ["--upsample", "nearest", "--epochs", "3000"]))
    vol = u.hyperbolic_volume(tuple(patch), seed=0)
    mask = u.random_trace_mask(tuple(patch), 0.66, seed=1)
    data = {"image": (vol * args.gain)[..., None], "mask": mask[..., None], "name": "0"}
    if interp:
        data["moveout"] = standin_table(tuple(patch))
    T = Interpolator(args, "/tmp", device=device)
    T.load_data(data)
    T.begin_patch(0)
    T.build_model()
    T.build_input()
    T.optimizer = FusedAdam(T.net.parameters(), lr=args.lr)
    T._big = T.wants_weight_grad_overlap()
    ops.set_weight_grad_overlap(T._big, in_graph=False)
    return T


def cost(a):
    parent = []
    if a.parent_tree:
        parent.append(OQ.time_tree(os.path.abspath(a.parent_tree), a))      # before this process opens the device
    import torch
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    Ts = {"off": make(a.patch, None, device)}
    Ts.update({k: make(a.patch, k, device) for k in a.interp})
    for T in Ts.values():
        OQ.run(T, a.warmup, device)
    ms = {k: [] for k in Ts}
    for r in range(a.runs):
        for k in (list(Ts) if r % 2 == 0 else list(Ts)[::-1]):               # alternate the order: no side gets the warmer slot
            ms[k].append(OQ.run(Ts[k], a.iters, device))
    res = {"patch": a.patch, "runs": a.runs, "iters": a.iters, "gpu": torch.cuda.get_device_name(device)}
    res.update({k + "_ms": OQ.stat(v) for k, v in ms.items()})
    for k in a.interp:
        res[k + "_diff_ms"] = round(res[k + "_ms"]["mean"] - res["off_ms"]["mean"], 3)
    if a.parent_tree:
        torch.cuda.synchronize(device)
        parent.append(OQ.time_tree(os.path.abspath(a.parent_tree), a))
        res["parent_ms"] = parent
        pm = float(np.mean([q["mean"] for q in parent]))
        res["parent_spread_between_runs_ms"] = round(abs(parent[0]["mean"] - parent[1]["mean"]), 3)
        for k in Ts:
            res[k + "_vs_parent_ms"] = round(res[k + "_ms"]["mean"] - pm, 3)
    print(json.dumps(res))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--seeds", type=int, nargs="+", default=list(range(6)))
    p.add_argument("--epochs", type=int, default=3000)
    p.add_argument("--patch", type=int, nargs=3, default=None)
    p.add_argument("--missing", type=float, default=0.66)
    p.add_argument("--masks", nargs="+", default=["random", "regular"], choices=["random", "regular"])
    p.add_argument("--interp", nargs="+", default=["linear", "cubic"], choices=["linear", "cubic"])
    p.add_argument("--out", default=None)
    p.add_argument("--cost", action="store_true")
    p.add_argument("--runs", type=int, default=5)
    p.add_argument("--iters", type=int, default=20)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--parent-tree", default=None)
    a = p.parse_args()
    if a.patch is None:
        a.patch = [256, 128, 128] if a.cost else [48, 32, 32]
    sys.path.insert(0, ROOT)
    return cost(a) if a.cost else quality(a)


if __name__ == "__main__":
    main()
