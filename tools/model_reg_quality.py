"""What --model_reg gives and what it costs.

Quality (default): the 48x32x32 stand-in (utils/synthetic.hyperbolic_volume), 66 % of the traces missing at random (arm b also: every third
trace along x kept), the bench's flags, 3000 EAGER iterations on both sides.  Measured PAIRED: the same traces, mask and seed once without
--model_reg and once per weight with it.  The arms:
    a   --wavelet (the stand-in's Ricker, reflectivity)                without / with --model_reg l1      SNR over all samples
    b   --moveout (NMO table of the mean law) --moveout_interp cubic   without / with --model_reg tv_x    SNR over the live samples
    c   --wavelet --wavelet_model impedance                            without / with --model_reg tv_t    SNR over all samples
Three weights per arm: W = rho * misfit_0 / R_0 with rho in --rho (0.01 0.1 1), misfit_0 and R_0 read at iteration 0 of the unregularised
run of that seed (R_0 is evaluated there on the tensor the network wrote, without entering the loss); every row carries the W it used.  One
JSON line per run, then per arm, mask and rho the mean paired difference of SNR(out_best) +- 2 s.e. over the seeds.

    python tools/model_reg_quality.py [--arms a b] [--seeds 0 .. 5] [--epochs 3000] [--patch 48 32 32] [--rho 0.01 0.1 1] [--out f.json]
                                      [--budget_s S]     (no further seed is begun once one more would pass S seconds; the summary says how many ran)

Cost (--cost): the protocol of tools/offgrid_quality.py --cost.  One process, Interpolators on the same 256x128x128 patch (fp32, the bench's
flags), one without the flag and one per --kinds with it, timed in alternating runs of --iters eager iterations each.  --parent-tree DIR
names a built checkout of the commit this one is compared with: its no-flag loop is timed in a fresh child process that imports the package
from DIR, before and after this tree's runs; "changes nothing when off" is this tree's no-flag loop against the parent's, within the spread
between the parent's own two runs.  One JSON line.

    python tools/model_reg_quality.py --cost [--runs 5] [--iters 20] [--warmup 5] [--patch 256 128 128] [--kinds l1 tv] [--parent-tree DIR]
"""
import argparse
import json
import os
import sys
import tempfile
from time import perf_counter

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import moveout_quality as MQ          # noqa: E402  (standin_table, trace_mask)
import offgrid_quality as OQ          # noqa: E402  (FLAGS, snr_db, run, stat, time_tree: one timing protocol for the tools)
import wavelet_quality as WQ          # noqa: E402  (flags_for: the stand-in's Ricker where --wavelet looks for it)

ARMS = {"a": ("l1", ["random"]), "b": ("tv_x", ["random", "regular"]), "c": ("tv_t", ["random"])}


def arm_flags(arm, shape, imgdir):
    if arm == "b":
        return MQ.flags_for("cubic", [])
    return WQ.flags_for(True, shape, 31, imgdir, ["--wavelet_model", "impedance"] if arm == "c" else [])


# ---------------------------------------------------------------- quality ---------------------------------------------------------
def one(arm, mask_kind, seed, weight, a, imgdir):
    """One run; weight None: the unregularised side, which also reads misfit_0 and R_0."""
    import torch
    from deep_prior_interpolation_amd import ops, utils as u
    from deep_prior_interpolation_amd.main import Interpolator
    from deep_prior_interpolation_amd.parameter import model_reg_axes, parse_arguments
    shape = tuple(a.patch)
    kind = ARMS[arm][0]
    reg = [] if weight is None else ["--model_reg", kind, "--model_reg_weight", repr(float(weight))]
    args = parse_arguments(arm_flags(arm, shape, imgdir) + ["--upsample", "linear", "--epochs", str(a.epochs)] + reg)
    truth = u.hyperbolic_volume(shape, seed=0).astype(np.float64) * args.gain
    mask = MQ.trace_mask(mask_kind, shape, a.missing)
    data = {"image": truth[..., None], "mask": mask[..., None], "name": "0"}
    where = None
    if arm == "b":
        data["moveout"] = MQ.standin_table(shape)
        where = (data["moveout"] >= 0) & (data["moveout"] <= shape[0] - 1)
    u.set_seed(seed)
    T = Interpolator(args, "/tmp", seed=seed)
    T.load_data(data)
    T.begin_patch(seed)
    T.build_model()
    T.build_input()
    first = {}
    if weight is None:
        dims = model_reg_axes(kind, "3d", "xy")
        inner = T._net_forward

        def read_r0(z):
            out = inner(z)
            if not first:
                with torch.no_grad():
                    first["R_0"] = float(ops.model_reg(out.detach(), dims).item())
            return out
        T._net_forward = read_r0
    T.optimize(verbose=False, mode="eager")
    out = np.asarray(T.out_best, dtype=np.float64).reshape(shape)
    h = T.history
    misfit = h.loss if weight is None else h.df
    row = {"arm": arm, "kind": kind, "mask": mask_kind, "seed": seed, "flag": weight is not None, "W": weight, "epochs": len(h.loss),
           "finite": bool(np.isfinite(h.loss).all()), "snr_db": OQ.snr_db(truth, out, where),
           "snr_known_db": OQ.snr_db(truth, out, (mask > 0) if where is None else where & (mask > 0)),
           "snr_missing_db": OQ.snr_db(truth, out, (mask == 0) if where is None else where & (mask == 0)),
           "misfit_0": float(misfit[0]), "misfit_min": float(np.min(misfit)), "ms_per_iter": round(1e3 * T.elapsed / len(h.loss), 3)}
    if weight is None:
        row["R_0"] = first["R_0"]
    else:
        row.update(R_0=float(h.model_reg[0]), R_last=float(h.model_reg[-1]))
    return row


def summaries(rows, a):
    out = []
    for arm in a.arms:
        for mk in ARMS[arm][1]:
            for rho in a.rho:
                sub = [r for r in rows if r["arm"] == arm and r["mask"] == mk and (not r["flag"] or r["rho"] == rho)]
                for s in OQ.summary(sub):
                    out.append(dict(s, arm=arm, kind=ARMS[arm][0], mask=mk, rho=rho, patch=a.patch, epochs=a.epochs,
                                    W_mean=float(np.mean([r["W"] for r in sub if r["flag"]]))))
    return out


def quality(a):
    import torch
    torch.cuda.set_device(0)
    rows = []
    start, per_seed = perf_counter(), 0.0
    with tempfile.TemporaryDirectory() as imgdir:
        for seed in a.seeds:               # seeds outermost: a run that is cut short still has whole groups
            if a.budget_s is not None and perf_counter() - start + per_seed > a.budget_s:
                print(json.dumps({"stopped_before_seed": seed, "elapsed_s": round(perf_counter() - start, 1)}), flush=True)
                break
            t0 = perf_counter()
            for arm in a.arms:
                for mk in ARMS[arm][1]:
                    base = dict(one(arm, mk, seed, None, a, imgdir), rho=None)
                    group = [base]
                    for rho in a.rho:
                        w = rho * base["misfit_0"] / base["R_0"]
                        group.append(dict(one(arm, mk, seed, w, a, imgdir), rho=rho))
                    for r in group:
                        rows.append(r)
                        print(json.dumps(r), flush=True)
                    if a.out:
                        with open(a.out, "w") as f:
                            json.dump(rows + summaries(rows, a), f, indent=1)
            per_seed = perf_counter() - t0
    for s in summaries(rows, a):
        print(json.dumps(s), flush=True)


# ---------------------------------------------------------------- cost ------------------------------------------------------------
def make(patch, kind, device):
    from deep_prior_interpolation_amd import ops, utils as u
    from deep_prior_interpolation_amd.main import Interpolator
    from deep_prior_interpolation_amd.optim import FusedAdam
    from deep_prior_interpolation_amd.parameter import parse_arguments
    args = parse_arguments(OQ.FLAGS + ["--upsample", "nearest", "--epochs", "3000"]
                           + (["--model_reg", kind, "--model_reg_weight", "0.1"] if kind else []))
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


def cost(a):
    parent = []
    if a.parent_tree:
        parent.append(OQ.time_tree(os.path.abspath(a.parent_tree), a))      # before this process opens the device
    import torch
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    Ts = {"off": make(a.patch, None, device)}
    Ts.update({k: make(a.patch, k, device) for k in a.kinds})
    for T in Ts.values():
        OQ.run(T, a.warmup, device)
    ms = {k: [] for k in Ts}
    for r in range(a.runs):
        for k in (list(Ts) if r % 2 == 0 else list(Ts)[::-1]):               # alternate the order: no side gets the warmer slot
            ms[k].append(OQ.run(Ts[k], a.iters, device))
    res = {"patch": a.patch, "runs": a.runs, "iters": a.iters, "gpu": torch.cuda.get_device_name(device)}
    res.update({k + "_ms": OQ.stat(v) for k, v in ms.items()})
    for k in a.kinds:
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
    p.add_argument("--arms", nargs="+", default=["a", "b"], choices=sorted(ARMS))
    p.add_argument("--seeds", type=int, nargs="+", default=list(range(6)))
    p.add_argument("--epochs", type=int, default=3000)
    p.add_argument("--patch", type=int, nargs=3, default=None)
    p.add_argument("--missing", type=float, default=0.66)
    p.add_argument("--rho", type=float, nargs="+", default=[0.01, 0.1, 1.0])
    p.add_argument("--out", default=None)
    p.add_argument("--budget_s", type=float, default=None)
    p.add_argument("--cost", action="store_true")
    p.add_argument("--kinds", nargs="+", default=["l1", "tv"], choices=["l1", "tv_t", "tv_x", "tv"])
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
