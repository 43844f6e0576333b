"""What --net unet gives on the 48x32x32 synthetic stand-in (tools/ema_quality.py conventions: notebook-like cube, 66 % missing traces, the
bench's flags) beside --net multiunet, PAIRED over seeds: the same data, mask and seed for both nets.  SNR(out_best) against the full
volume, computed on the host.  One JSON line per run, then one summary line per net and one for the paired difference: mean +- 2 s.e.

    python tools/unet3d_quality.py [--seeds 0 .. 5] [--epochs 3000] [--upsample deconv] [--inittype kaiming] [--patch 48 32 32] [--out file.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def one(net, seed, a):
    from deep_prior_interpolation_amd import utils as u
    from deep_prior_interpolation_amd.main import Interpolator
    from deep_prior_interpolation_amd.parameter import parse_arguments
    # the plain UNet has no norm in its up path: the default xavier gain of 0.02 passes no gradient through it (README)
    own = ["--net", "unet", "--upsample", a.upsample, "--inittype", a.inittype] if net == "unet" else ["--net", "multiunet", "--upsample", "linear"]
    args = parse_arguments(["--imgdir", "synthetic", "--datadim", "3d", "--inputdepth", "64", "--loss", "mae", "--lr", "1e-3", "--gain", "40",
                            "--reg_noise_std", "0.03", "--noise_std", "0.1", "--epochs", str(a.epochs), "--gpu", "0"] + own)
    shape = tuple(a.patch)
    vol = u.hyperbolic_volume(shape, seed=0, background=0.02)
    mask = u.random_trace_mask(shape, a.missing, seed=1)
    u.set_seed(seed)
    T = Interpolator(args, "/tmp", seed=seed)
    T.load_data({"image": (vol * args.gain)[..., None].astype(np.float64), "mask": mask[..., None].astype(np.float64), "name": "0"})
    T.begin_patch(seed)
    T.build_model()
    T.build_input()
    T.optimize(verbose=False)
    h = T.history
    target = vol.astype(np.float64) * args.gain
    snr = float(10.0 * np.log10(np.sum(target ** 2) / np.sum((target - np.asarray(T.out_best, dtype=np.float64).reshape(target.shape)) ** 2)))
    return {"net": net, "seed": seed, "epochs": len(h.loss), "finite": bool(np.isfinite(h.loss).all()), "params": int(T.num_params),
            "snr_out_best_db": snr, "loss_first": float(h.loss[0]), "loss_min": float(np.min(h.loss)), "seconds": round(T.elapsed, 2)}


def summary(rows):
    out = []
    by = {n: {r["seed"]: r["snr_out_best_db"] for r in rows if r["net"] == n} for n in ("multiunet", "unet")}

    def ms(v):
        v = np.asarray(v, dtype=np.float64)
        return {"seeds": len(v), "mean_db": round(float(v.mean()), 3), "two_se_db": None if len(v) < 2 else round(float(2 * v.std(ddof=1) / np.sqrt(len(v))), 3)}
    for n, d in by.items():
        if d:
            out.append(dict({"summary": n}, **ms(list(d.values()))))
    both = sorted(set(by["multiunet"]) & set(by["unet"]))
    if both:
        out.append(dict({"summary": "unet - multiunet, paired"}, **ms([by["unet"][s] - by["multiunet"][s] for s in both])))
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--seeds", type=int, nargs="+", default=list(range(6)))
    p.add_argument("--epochs", type=int, default=3000)
    p.add_argument("--patch", type=int, nargs=3, default=[48, 32, 32])
    p.add_argument("--missing", type=float, default=0.66)
    p.add_argument("--upsample", default="deconv", choices=["deconv", "linear", "nearest"])
    p.add_argument("--inittype", default="kaiming")
    p.add_argument("--out", default=None)
    a = p.parse_args()
    torch.cuda.set_device(0)
    rows = []
    for seed in a.seeds:                   # seeds outermost: a run that is cut short still has whole pairs
        for net in ("multiunet", "unet"):
            rows.append(one(net, seed, a))
            print(json.dumps(rows[-1]), flush=True)
            if a.out:
                with open(a.out, "w") as f:
                    json.dump(rows + summary(rows), f, indent=1)
    for s in summary(rows):
        print(json.dumps(s), flush=True)


if __name__ == "__main__":
    main()
