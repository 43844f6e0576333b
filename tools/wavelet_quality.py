"""What --wavelet gives and what it costs.

Quality (default): the 48x32x32 stand-in (utils/synthetic.hyperbolic_volume: hyperbolic events drawn with a Ricker wavelet of 0.055 / s
cycles per sample, s the stand-in's sampling factor), 66 % of the traces missing, the bench's flags.  Measured PAIRED: the same traces, mask
and seed once without the flag and once with --wavelet on that Ricker (--taps samples, reflectivity).  The figure is the SNR of the selected
output against the complete noise-free volume.  --noise SIGMA adds white noise of SIGMA times the volume's standard deviation to the traces
both runs see; white noise is mostly outside the wavelet's band, which is where the constraint should matter.  One JSON line per run, then
the summary: mean paired difference +- 2 s.e. over the seeds.

    python tools/wavelet_quality.py [--seeds 0 .. 5] [--epochs 3000] [--patch 48 32 32] [--missing 0.66] [--noise 0.0] [--taps 31] [--out f.json]

Cost (--cost): the protocol of tools/offgrid_quality.py --cost.  One process, two Interpolators on the same 256x128x128 patch (fp32, the
bench's flags), one without the flag and one with a 65-tap Ricker, timed in alternating runs of --iters eager iterations each.
--parent-tree DIR names a built checkout of the commit this one is compared with: its no-flag loop is timed in a fresh child process that
imports the package from DIR, before and after this tree's runs.  One JSON line.

    python tools/wavelet_quality.py --cost [--runs 5] [--iters 20] [--warmup 5] [--patch 256 128 128] [--taps 65] [--parent-tree DIR]
"""
import argparse
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import offgrid_quality as OQ          # noqa: E402  (FLAGS, snr_db, run, stat, time_tree: one timing protocol for both tools)


def wavelet_file(shape, taps, imgdir):
    """The Ricker the stand-in of this size was drawn with, written where --wavelet looks for it."""
    from deep_prior_interpolation_amd import utils as u
    s = min(1.0, max(0.25, shape[0] / 256.0))
    np.save(os.path.join(imgdir, "ricker.npy"), u.ricker(0.055 / s, 1.0, taps))
    return ["--imgdir", imgdir, "--wavelet", "ricker.npy"]


def flags_for(flag, shape, taps, imgdir, rest):
    base = [f for f in OQ.FLAGS]
    if flag:
        i = base.index("--imgdir")
        base = base[:i] + base[i + 2:] + wavelet_file(shape, taps, imgdir)
    return base + rest


# ---------------------------------------------------------------- quality ---------------------------------------------------------
def one(flag, seed, a, imgdir):
    from deep_prior_interpolation_amd import utils as u
    from deep_prior_interpolation_amd.main import Interpolator
    from deep_prior_interpolation_amd.parameter import parse_arguments
    shape = tuple(a.patch)
    args = parse_arguments(flags_for(flag, shape, a.taps, imgdir, ["--upsample", "linear", "--epochs", str(a.epochs)]))
    clean = u.hyperbolic_volume(shape, seed=0).astype(np.float64)
    noise = np.random.RandomState(77).standard_normal(shape) * (a.noise * clean.std())          # the same noise for every seed and both sides
    mask = u.random_trace_mask(shape, a.missing, seed=1).astype(np.float64)
    data = {"image": ((clean + noise) * args.gain)[..., None], "mask": mask[..., None], "name": "0"}
    u.set_seed(seed)
    T = Interpolator(args, "/tmp", seed=seed)
    T.load_data(data)
    T.begin_patch(seed)
    T.build_model()
    T.build_input()
    T.optimize(verbose=False)
    out = np.asarray(T.out_best, dtype=np.float64).reshape(shape)
    truth = clean * args.gain
    return {"flag": bool(flag), "seed": seed, "noise": a.noise, "epochs": len(T.history.loss), "finite": bool(np.isfinite(T.history.loss).all()),
            "snr_db": OQ.snr_db(truth, out), "snr_known_db": OQ.snr_db(truth, out, mask > 0), "snr_missing_db": OQ.snr_db(truth, out, mask == 0),
            "snr_traces_vs_truth_db": OQ.snr_db(truth, (clean + noise) * args.gain, mask > 0) if a.noise > 0 else None,
            "loss_min": float(np.min(T.history.loss)), "ms_per_iter": round(1e3 * T.elapsed / len(T.history.loss), 3)}


def quality(a):
    import torch
    torch.cuda.set_device(0)
    rows = []
    with tempfile.TemporaryDirectory() as imgdir:
        for seed in a.seeds:               # seeds outermost: a run that is cut short still has whole pairs
            for flag in (False, True):
                rows.append(one(flag, seed, a, imgdir))
                print(json.dumps(rows[-1]), flush=True)
                if a.out:
                    with open(a.out, "w") as f:
                        json.dump(rows + OQ.summary(rows), f, indent=1)
    for s in OQ.summary(rows):
        print(json.dumps(dict(s, noise=a.noise, taps=a.taps)), flush=True)


# ---------------------------------------------------------------- cost ------------------------------------------------------------
def make(patch, flag, taps, device, imgdir):
    from deep_prior_interpolation_amd import ops, utils as u
    from deep_prior_interpolation_amd.main import Interpolator
    from deep_prior_interpolation_amd.optim import FusedAdam
    from deep_prior_interpolation_amd.parameter import parse_arguments
    args = parse_arguments(flags_for(flag, tuple(patch), taps, imgdir, ["--upsample", "nearest", "--epochs", "3000"]))
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
    with tempfile.TemporaryDirectory() as imgdir:
        Ts = {"off": make(a.patch, False, a.taps, device, imgdir), "on": make(a.patch, True, a.taps, device, imgdir)}
    for T in Ts.values():
        OQ.run(T, a.warmup, device)
    ms = {k: [] for k in Ts}
    for r in range(a.runs):
        for k in (list(Ts) if r % 2 == 0 else list(Ts)[::-1]):               # alternate the order: no side gets the warmer slot
            ms[k].append(OQ.run(Ts[k], a.iters, device))
    res = {"patch": a.patch, "taps": a.taps, "runs": a.runs, "iters": a.iters, "gpu": torch.cuda.get_device_name(device)}
    res.update({k + "_ms": OQ.stat(v) for k, v in ms.items()})
    res["diff_ms"] = round(res["on_ms"]["mean"] - res["off_ms"]["mean"], 3)
    if a.parent_tree:
        torch.cuda.synchronize(device)
        parent.append(OQ.time_tree(os.path.abspath(a.parent_tree), a))
        res["parent_ms"] = parent
        pm = float(np.mean([q["mean"] for q in parent]))
        res["off_vs_parent_ms"] = round(res["off_ms"]["mean"] - pm, 3)
        res["on_vs_parent_ms"] = round(res["on_ms"]["mean"] - pm, 3)
    print(json.dumps(res))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--seeds", type=int, nargs="+", default=list(range(6)))
    p.add_argument("--epochs", type=int, default=3000)
    p.add_argument("--patch", type=int, nargs=3, default=None)
    p.add_argument("--missing", type=float, default=0.66)
    p.add_argument("--noise", type=float, default=0.0, help="white noise on the traces, in units of the volume's standard deviation")
    p.add_argument("--taps", type=int, default=None, help="length of the Ricker (odd): 31 for the quality runs, 65 for --cost")
    p.add_argument("--out", default=None)
    p.add_argument("--cost", action="store_true")
    p.add_argument("--runs", type=int, default=5)
    p.add_argument("--iters", type=int, default=20)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--parent-tree", default=None)
    a = p.parse_args()
    if a.patch is None:
        a.patch = [256, 128, 128] if a.cost else [48, 32, 32]
    if a.taps is None:
        a.taps = 65 if a.cost else 31
    sys.path.insert(0, ROOT)
    return cost(a) if a.cost else quality(a)


if __name__ == "__main__":
    main()
