"""What the Langevin samplers give on the 48x32x32 synthetic stand-in (tools/full_run.py conventions: notebook-like cube, 66 % missing
traces, the bench's flags): SNR of the posterior mean against the SNR of Adam's out_best, the mean of posterior_std over missing and over
known traces, and the correlation of posterior_std with |mean - truth| on the missing traces.  One JSON line per (optimiser, seed).

    python tools/langevin_quality.py [--seeds 0 1 2] [--epochs 3000] [--optimizers adam sgld psgld] [--temperature T] [--out file.json]
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


def one(optimizer, seed, a):
    from deep_prior_interpolation_amd import utils as u
    from deep_prior_interpolation_amd.main import Interpolator
    from deep_prior_interpolation_amd.parameter import parse_arguments
    extra = ["--optimizer", optimizer]
    if optimizer != "adam" and a.temperature is not None:
        extra += ["--langevin_temperature", str(a.temperature)]
    args = parse_arguments(["--imgdir", "synthetic", "--datadim", "3d", "--net", "multiunet", "--inputdepth", "64", "--upsample", "linear",
                            "--loss", "mae", "--lr", "1e-3", "--gain", "40", "--reg_noise_std", "0.03", "--noise_std", "0.1",
                            "--epochs", str(a.epochs), "--gpu", "0"] + extra)
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
    target = vol.astype(np.float64) * args.gain
    snr = lambda o: float(10.0 * np.log10(np.sum(target ** 2) / np.sum((target - np.asarray(o, dtype=np.float64)) ** 2)))
    res = {"optimizer": optimizer, "seed": seed, "epochs": len(T.history.loss), "finite": bool(np.isfinite(T.history.loss).all()),
           "snr_output_db": snr(T.out_best), "final_loss": float(T.history.loss[-1])}
    if optimizer != "adam":
        res["temperature"] = T.optimizer.temperature
        res["posterior_samples"] = T.posterior_samples
        res["snr_selected_db"] = snr(T.output_selected)
        if T.posterior_std is not None:
            std = np.asarray(T.posterior_std, dtype=np.float64)
            miss = np.broadcast_to(mask == 0, std.shape)
            err = np.abs(np.asarray(T.out_best, dtype=np.float64) - target)
            res["std_mean_missing"] = float(std[miss].mean())
            res["std_mean_known"] = float(std[~miss].mean())
            res["abs_err_mean_missing"] = float(err[miss].mean())
            res["corr_std_abs_err_missing"] = float(np.corrcoef(std[miss], err[miss])[0, 1])
    return res


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--seeds", type=int, nargs="+", default=[0, 1, 2])
    p.add_argument("--epochs", type=int, default=3000)
    p.add_argument("--patch", type=int, nargs=3, default=[48, 32, 32])
    p.add_argument("--missing", type=float, default=0.66)
    p.add_argument("--optimizers", nargs="+", default=["adam", "sgld", "psgld"])
    p.add_argument("--temperature", type=float, default=None, help="--langevin_temperature of the samplers (default: unset = 1/N)")
    p.add_argument("--out", default=None)
    a = p.parse_args()
    torch.cuda.set_device(0)
    rows = []
    for opt in a.optimizers:
        for seed in a.seeds:
            rows.append(one(opt, seed, a))
            print(json.dumps(rows[-1]), flush=True)
            if a.out:
                with open(a.out, "w") as f:
                    json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
