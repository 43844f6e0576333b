"""What --wavelet together with --moveout gives under either --wavelet_domain, and what the pair costs.

Quality (default): the protocol of tools/moveout_quality.py.  The stand-in (utils/synthetic.hyperbolic_volume), the bench's flags, the NMO
table of the MEAN law (moveout_quality.standin_table), --moveout_interp cubic, and the stand-in's own wavelet on 31 taps,
utils.ricker(0.055 / s, 1.0, 31) with s = min(1, max(0.25, nt / 256)), the Ricker hyperbolic_volume draws a cube of nt rows with.  Four arms
per seed and mask kind, PAIRED (the same traces, mask and seed):
    moveout   --moveout alone                                                   (the baseline of every difference)
    data      + --wavelet --wavelet_domain data                                 d = W L r
    model     + --wavelet --wavelet_domain model                                d = L W r
    data_l1   data + --model_reg l1 --model_reg_weight 0.001
Two mask kinds, reported separately: `random` = 66 % of the traces missing at random, `regular` = every third trace along x kept.  The
figure is the SNR of the selected output against the complete volume over the samples that are live in EVERY arm, i.e. the eroded map of
`data`; `eroded_share` is the part of the cube the erosion takes beyond L's mutes.  One JSON line per run, then per mask kind and arm the
mean paired difference against `moveout` +- 2 s.e. over the seeds.

    python tools/prestack_quality.py [--seeds 0 .. 5] [--epochs 3000] [--patch 48 32 32] [--masks random regular] [--out f.json]

Cost (--cost): the protocol of tools/moveout_quality.py --cost.  One process, Interpolators on the same 256x128x128 patch (fp32, the
bench's flags): no flag, --moveout alone, and the pair under both domains, timed in alternating runs of --iters eager iterations each.
--parent-tree DIR names a built checkout of the commit this one is compared with: its no-flag loop and its --moveout loop are each timed
in a fresh child process that imports the package from DIR, before and after this tree's runs; the gap between the two visits is the
parent's own run-to-run gap, below which nothing is claimed.  One JSON line.

    python tools/prestack_quality.py --cost [--runs 5] [--iters 20] [--warmup 5] [--patch 256 128 128] [--parent-tree DIR]
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import moveout_quality as MQ          # noqa: E402  (standin_table, trace_mask)
import offgrid_quality as OQ          # noqa: E402  (FLAGS, snr_db, run, stat: one timing protocol for the tools)

TAPS = 31                              # taps of the Ricker handed to --wavelet
MOV = ["--moveout", "tau.npy", "--moveout_interp", "cubic"]
PAIR = MOV + ["--wavelet", "w.npy", "--wavelet_domain"]
ARMS = {"moveout": MOV, "data": PAIR + ["data"], "model": PAIR + ["model"],
        "data_l1": PAIR + ["data", "--model_reg", "l1", "--model_reg_weight", "0.001"]}


def arguments(arm, rest, imgdir, shape):
    from deep_prior_interpolation_amd import utils as u
    from deep_prior_interpolation_amd.parameter import parse_arguments
    s = min(1.0, max(0.25, shape[0] / 256.0))
    np.save(os.path.join(imgdir, "w.npy"), u.ricker(0.055 / s, 1.0, TAPS))          # the Ricker the stand-in of this size was drawn with
    flags = [imgdir if f == "synthetic" else f for f in OQ.FLAGS]
    return parse_arguments(flags + (ARMS[arm] if arm != "off" else []) + rest)


def common_live(shape):
    """(the samples live in every arm, L's live map): the eroded map of `data` is inside L's, which `moveout` and `model` use."""
    from deep_prior_interpolation_amd.operators import Moveout, erode_live
    live = Moveout(MQ.standin_table(shape), "cubic").live
    return erode_live(live, TAPS, 0), live


# ---------------------------------------------------------------- quality ---------------------------------------------------------
def one(arm, seed, mask_kind, a):
    from deep_prior_interpolation_amd import utils as u
    from deep_prior_interpolation_amd.main import Interpolator
    shape = tuple(a.patch)
    args = arguments(arm, ["--upsample", "linear", "--epochs", str(a.epochs)], a.imgdir, shape)
    truth = u.hyperbolic_volume(shape, seed=0).astype(np.float64) * args.gain
    mask = MQ.trace_mask(mask_kind, shape, a.missing)
    both, live = common_live(shape)
    data = {"image": truth[..., None], "mask": mask[..., None], "name": "0", "moveout": MQ.standin_table(shape)}
    u.set_seed(seed)
    T = Interpolator(args, a.imgdir, seed=seed)
    T.load_data(data)
    T.begin_patch(seed)
    T.build_model()
    T.build_input()
    T.optimize(verbose=False)
    out = np.asarray(T.out_best, dtype=np.float64).reshape(shape)
    return {"flag": arm != "moveout", "arm": arm, "mask": mask_kind, "seed": seed, "epochs": len(T.history.loss),
            "finite": bool(np.isfinite(T.history.loss).all()), "live_share": round(float(live.mean()), 4),
            "eroded_share": round(float(live.mean() - both.mean()), 4),
            "snr_db": OQ.snr_db(truth, out, both), "snr_known_db": OQ.snr_db(truth, out, both & (mask > 0)),
            "snr_missing_db": OQ.snr_db(truth, out, both & (mask == 0)), "snr_L_live_db": OQ.snr_db(truth, out, live),
            "loss_min": float(np.min(T.history.loss)), "ms_per_iter": round(1e3 * T.elapsed / len(T.history.loss), 3)}


def summaries(rows, a):
    out = []
    for mk in a.masks:
        for arm in list(ARMS)[1:]:
            sub = [r for r in rows if r["mask"] == mk and r["arm"] in ("moveout", arm)]
            for s in OQ.summary(sub):
                out.append(dict(s, mask=mk, arm=arm, against="moveout", patch=a.patch, epochs=a.epochs))
    return out


def quality(a):
    import torch
    torch.cuda.set_device(0)
    rows = []
    for seed in a.seeds:                   # seeds outermost: a run that is cut short still has whole groups
        for mk in a.masks:
            for arm in ARMS:
                rows.append(one(arm, seed, mk, a))
                print(json.dumps(rows[-1]), flush=True)
                if a.out:
                    with open(a.out, "w") as f:
                        json.dump(rows + summaries(rows, a), f, indent=1)
    for s in summaries(rows, a):
        print(json.dumps(s), flush=True)


# ---------------------------------------------------------------- cost ------------------------------------------------------------
def make(patch, arm, device, imgdir):
    from deep_prior_interpolation_amd import ops, utils as u
    from deep_prior_interpolation_amd.main import Interpolator
    from deep_prior_interpolation_amd.optim import FusedAdam
    args = arguments(arm, ["--upsample", "nearest", "--epochs", "3000"], imgdir, tuple(patch))
    vol = u.hyperbolic_volume(tuple(patch), seed=0)
    mask = u.random_trace_mask(tuple(patch), 0.66, seed=1)
    data = {"image": (vol * args.gain)[..., None], "mask": mask[..., None], "name": "0"}
    if arm != "off":
        data["moveout"] = MQ.standin_table(tuple(patch))
    T = Interpolator(args, imgdir, device=device)
    T.load_data(data)
    T.begin_patch(0)
    T.build_model()
    T.build_input()
    T.optimizer = FusedAdam(T.net.parameters(), lr=args.lr)
    T._big = T.wants_weight_grad_overlap()
    ops.set_weight_grad_overlap(T._big, in_graph=False)
    return T


def child(a):
    """One loop (`off` or `moveout`) of the tree at a.root, alone in its process: one JSON line."""
    sys.path.insert(0, a.root)
    import torch
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    T = make(a.patch, a.arm, device, a.imgdir)
    OQ.run(T, a.warmup, device)
    print(json.dumps(OQ.stat([OQ.run(T, a.iters, device) for _ in range(a.runs)])))


def time_tree(root, arm, a):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--root", root, "--arm", arm, "--runs", str(a.runs), "--iters", str(a.iters),
           "--warmup", str(a.warmup), "--imgdir", a.imgdir, "--patch"] + [str(p) for p in a.patch]
    out = subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=600).stdout
    return json.loads(out.strip().splitlines()[-1])


def cost(a):
    arms = ("off", "moveout", "data", "model")
    parent = {k: [] for k in arms[:2]}
    if a.parent_tree:
        for k in parent:                   # before this process opens the device
            parent[k].append(time_tree(os.path.abspath(a.parent_tree), k, a))
    import torch
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    Ts = {k: make(a.patch, k, device, a.imgdir) for k in arms}
    for T in Ts.values():
        OQ.run(T, a.warmup, device)
    ms = {k: [] for k in Ts}
    for r in range(a.runs):
        for k in (list(Ts) if r % 2 == 0 else list(Ts)[::-1]):               # alternate the order: no arm gets the warmer slot
            ms[k].append(OQ.run(Ts[k], a.iters, device))
    both, live = common_live(tuple(a.patch))
    res = {"patch": a.patch, "runs": a.runs, "iters": a.iters, "gpu": torch.cuda.get_device_name(device), "wavelet_taps": TAPS,
           "live_share": round(float(live.mean()), 4), "eroded_share": round(float(live.mean() - both.mean()), 4)}
    res.update({k + "_ms": OQ.stat(v) for k, v in ms.items()})
    for k in arms[2:]:
        res[k + "_minus_moveout_ms"] = round(res[k + "_ms"]["mean"] - res["moveout_ms"]["mean"], 3)
        res[k + "_minus_off_ms"] = round(res[k + "_ms"]["mean"] - res["off_ms"]["mean"], 3)
    if a.parent_tree:
        torch.cuda.synchronize(device)
        for k in parent:
            parent[k].append(time_tree(os.path.abspath(a.parent_tree), k, a))
            pm = float(np.mean([q["mean"] for q in parent[k]]))
            res["parent_%s_ms" % k] = parent[k]
            res["parent_%s_gap_between_visits_ms" % k] = round(abs(parent[k][0]["mean"] - parent[k][1]["mean"]), 3)
            for arm in arms:
                res["%s_minus_parent_%s_ms" % (arm, k)] = round(res[arm + "_ms"]["mean"] - pm, 3)
    print(json.dumps(res))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--seeds", type=int, nargs="+", default=list(range(6)))
    p.add_argument("--epochs", type=int, default=3000)
    p.add_argument("--patch", type=int, nargs=3, default=None)
    p.add_argument("--missing", type=float, default=0.66)
    p.add_argument("--masks", nargs="+", default=["random", "regular"], choices=["random", "regular"])
    p.add_argument("--out", default=None)
    p.add_argument("--imgdir", default=None, help="where w.npy goes (a temporary folder by default)")
    p.add_argument("--cost", action="store_true")
    p.add_argument("--runs", type=int, default=5)
    p.add_argument("--iters", type=int, default=20)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--parent-tree", default=None)
    p.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    p.add_argument("--root", default=ROOT, help=argparse.SUPPRESS)
    p.add_argument("--arm", default="off", choices=["off", "moveout"], help=argparse.SUPPRESS)
    a = p.parse_args()
    if a.patch is None:
        a.patch = [256, 128, 128] if (a.cost or a.child) else [48, 32, 32]
    if a.imgdir is None:
        import tempfile
        a.imgdir = tempfile.mkdtemp(prefix="prestack_quality_")
    if a.child:
        return child(a)
    sys.path.insert(0, ROOT)
    return cost(a) if a.cost else quality(a)


if __name__ == "__main__":
    main()
