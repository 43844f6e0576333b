"""What --moveout_offset gives: the protocol of tools/moveout_quality.py with the table scanned from the data.

The stand-in (utils/synthetic.hyperbolic_volume: apex at (0, 0), law c(tau) = 0.9 - 0.3 tau / nt jittered by +-0.04 per event), the bench's
flags, PAIRED runs: the same traces, mask and seed in four arms:
    none     no moveout
    mean     --moveout on tools/moveout_quality.py:standin_table, the table of the law the stand-in was generated from
    scan     --moveout_offset: the table of the law picked by the semblance scan over the known traces (one gather: the volume)
    stretch  the same with --moveout_stretch
    smooth, smooth_stretch   `scan` / `stretch` with --moveout_smooth L, one arm per L of --smooth, reported as smooth:L / smooth_stretch:L
Two mask kinds, reported separately: `random` = 66 % of the traces missing at random, `regular` = every third trace along x kept.  The
figure is the SNR of the selected output against the complete volume over the samples the MEAN-law table leaves live, the same region
for every arm (a sample an arm mutes inside it counts with its zero); `snr_own_live_db` is the same over the arm's own live samples.
Each scanned arm also reports the error of its picked law against 1 / (0.9 - 0.3 tau / nt) in cells per sample over the rows with events
(rows whose best semblance is above half the panel's maximum), the roughness of its table (mean |d^2 tau / dt^2|: the absolute second
difference along t over triples of consecutive live samples of a trace; the `mean` arm reports it too) and the table's distance from
the mean-law table in rows, median and 90th percentile over the samples live in both.  One JSON line per run, then per mask kind and
arm the mean paired difference +- 2 s.e. over the seeds against `none`, `mean` and `scan`, whatever its sign.

    python tools/velocity_scan_quality.py [--seeds 0 .. 5] [--epochs 3000] [--patch 48 32 32] [--masks random regular] [--vscan 1.0 1.8 33]
                                          [--stretch 1.5] [--arms none mean scan stretch smooth smooth_stretch] [--smooth 4 8 12]
                                          [--table host|device] [--out f.json] [--budget-s SECONDS]

--budget-s: no further seed is started once the time used plus the longest seed so far would pass it, so a run that has to fit a time
slot ends with whole seeds and its summary.
"""
import argparse
import json
import os
import sys
from time import perf_counter

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import moveout_quality as MQ          # noqa: E402  (standin_table, trace_mask)
import offgrid_quality as OQ          # noqa: E402  (FLAGS, snr_db)

ARMS = ["none", "mean", "scan", "stretch", "smooth", "smooth_stretch"]
BASES = ("none", "mean", "scan")


def roughness(table):
    """mean |d^2 tau / dt^2| over triples of consecutive live samples of a trace."""
    tab = np.asarray(table, dtype=np.float64).reshape(table.shape[0], -1)
    live = (tab >= 0) & (tab <= tab.shape[0] - 1)
    ok = live[:-2] & live[1:-1] & live[2:]
    return round(float(np.abs(tab[2:] - 2.0 * tab[1:-1] + tab[:-2])[ok].mean()), 4)


def labels(a):
    """The arms as run and reported: a smoothed arm once per length."""
    return [x for arm in a.arms for x in (["%s:%g" % (arm, L) for L in a.smooth] if arm.startswith("smooth") else [arm])]


def offsets(shape):
    nt, nx, ny = shape
    return nt * np.sqrt((np.arange(nx)[:, None] / max(nx, 1)) ** 2 + (np.arange(ny)[None, :] / max(ny, 1)) ** 2)


def scanned(truth, mask, shape, a, stretch, smooth=0.0):
    from deep_prior_interpolation_amd.operators import scan_table
    known = mask > 0
    res = scan_table(np.where(known, truth, 0.0), known, offsets(shape), a.vscan[0], a.vscan[1], int(a.vscan[2]), gather="volume", window=a.window,
                     min_fold=a.min_fold, max_step=a.max_step, stretch_mute=stretch, smooth=smooth, table=a.table)
    nt = shape[0]
    law = 1.0 / (0.9 - 0.3 * np.arange(nt) / nt)
    best = res["panel"][0].max(axis=1)
    rows = best > 0.5 * best.max()
    err = np.abs(res["velocity"][0] - law)[rows]
    info = {"law_rows": int(rows.sum()), "law_err_median": round(float(np.median(err)), 4), "law_err_max": round(float(err.max()), 4),
            "velocity_step": round(float(res["velocities"][1] - res["velocities"][0]), 4) if len(res["velocities"]) > 1 else None,
            "panel_max": round(float(best.max()), 3), "smooth": smooth, "table_roughness": roughness(res["table"])}
    mean_table = MQ.standin_table(shape)
    both = (mean_table >= 0) & (mean_table <= nt - 1) & (res["table"] >= 0) & (res["table"] <= nt - 1)
    dist = np.abs(res["table"] - mean_table)[both]
    info.update(table_err_median=round(float(np.median(dist)), 3), table_err_p90=round(float(np.percentile(dist, 90)), 3))
    return res, info


def one(arm, seed, mask_kind, a):
    from deep_prior_interpolation_amd import utils as u
    from deep_prior_interpolation_amd.main import Interpolator
    from deep_prior_interpolation_amd.parameter import parse_arguments
    shape = tuple(a.patch)
    label = arm
    arm, _, length = arm.partition(":")
    smooth = float(length) if length else 0.0
    scan = ["--moveout_offset", "off.npy", "--moveout_vscan"] + [str(v) for v in a.vscan]
    smoothed = ["--moveout_smooth", str(smooth)] + (["--moveout_table", a.table] if a.table != "host" else [])
    extra = {"none": [], "mean": ["--moveout", "tau.npy"], "scan": scan, "stretch": scan + ["--moveout_stretch", str(a.stretch)],
             "smooth": scan + smoothed, "smooth_stretch": scan + ["--moveout_stretch", str(a.stretch)] + smoothed}[arm]
    args = parse_arguments(OQ.FLAGS + ["--upsample", "linear", "--epochs", str(a.epochs)] + extra)
    truth = u.hyperbolic_volume(shape, seed=0).astype(np.float64) * args.gain
    mask = MQ.trace_mask(mask_kind, shape, a.missing)
    mean_table = MQ.standin_table(shape)
    region = (mean_table >= 0) & (mean_table <= shape[0] - 1)
    data = {"image": truth[..., None], "mask": mask[..., None], "name": "0"}
    info, own = {}, np.ones(shape, dtype=bool)
    if arm == "mean":
        data["moveout"], own = mean_table, region
        info = {"table_roughness": roughness(mean_table)}
    elif arm != "none":
        res, info = scanned(truth, mask, shape, a, a.stretch if arm.endswith("stretch") else None, smooth)
        data["moveout"], data["moveout_velocity"] = res["table"], res["velocity"][0]
        own = (res["table"] >= 0) & (res["table"] <= shape[0] - 1)
    u.set_seed(seed)
    T = Interpolator(args, "/tmp", seed=seed)
    T.load_data(data)
    T.begin_patch(seed)
    T.build_model()
    T.build_input()
    T.optimize(verbose=False)
    out = np.asarray(T.out_best, dtype=np.float64).reshape(shape)
    return dict({"arm": label, "mask": mask_kind, "seed": seed, "epochs": len(T.history.loss), "finite": bool(np.isfinite(T.history.loss).all()),
                 "region_share": round(float(region.mean()), 4), "own_live_share": round(float(own.mean()), 4),
                 "snr_db": OQ.snr_db(truth, out, region), "snr_missing_db": OQ.snr_db(truth, out, region & (mask == 0)),
                 "snr_own_live_db": OQ.snr_db(truth, out, own), "snr_all_samples_db": OQ.snr_db(truth, out),
                 "loss_min": float(np.min(T.history.loss)), "ms_per_iter": round(1e3 * T.elapsed / len(T.history.loss), 3)}, **info)


def summaries(rows, a):
    out = []
    for mk in a.masks:
        for arm in labels(a):
            for base in BASES:
                if arm == base or base not in a.arms or arm in BASES[:BASES.index(base) + 1]:
                    continue
                get = lambda s, r_arm, k: next((r.get(k) for r in rows if r["seed"] == s and r["arm"] == r_arm and r["mask"] == mk), None)
                seeds = [s for s in a.seeds if get(s, arm, "snr_db") is not None and get(s, base, "snr_db") is not None]
                if not seeds:
                    continue
                res = {"summary": True, "mask": mk, "arm": arm, "against": base, "seeds": len(seeds), "patch": a.patch, "epochs": a.epochs}
                if get(seeds[0], arm, "table_roughness") is not None:
                    res.update({k: get(seeds[0], arm, k) for k in ("table_roughness", "table_err_median", "table_err_p90", "law_err_median")
                                if get(seeds[0], arm, k) is not None})
                for k in ("snr_db", "snr_missing_db"):
                    d = np.array([get(s, arm, k) - get(s, base, k) for s in seeds])
                    res[k] = {"base_mean": round(float(np.mean([get(s, base, k) for s in seeds])), 3),
                              "arm_mean": round(float(np.mean([get(s, arm, k) for s in seeds])), 3),
                              "paired_diff_mean": round(float(d.mean()), 3),
                              "paired_diff_2se": round(float(2.0 * d.std(ddof=1) / np.sqrt(len(d))), 3) if len(d) > 1 else None,
                              "paired_diff_min": round(float(d.min()), 3), "paired_diff_max": round(float(d.max()), 3)}
                out.append(res)
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--seeds", type=int, nargs="+", default=list(range(6)))
    p.add_argument("--epochs", type=int, default=3000)
    p.add_argument("--patch", type=int, nargs=3, default=[48, 32, 32])
    p.add_argument("--missing", type=float, default=0.66)
    p.add_argument("--masks", nargs="+", default=["random", "regular"], choices=["random", "regular"])
    p.add_argument("--arms", nargs="+", default=ARMS, choices=ARMS)
    p.add_argument("--vscan", type=float, nargs=3, default=[1.0, 1.8, 33])
    p.add_argument("--stretch", type=float, default=1.5)
    p.add_argument("--smooth", type=float, nargs="+", default=[4.0, 8.0, 12.0], help="the lengths L of the smooth / smooth_stretch arms")
    p.add_argument("--table", default="host", choices=["host", "device"], help="where the scanned arms build their table")
    p.add_argument("--window", type=int, default=2)
    p.add_argument("--min_fold", type=int, default=4)
    p.add_argument("--max_step", type=int, default=1)
    p.add_argument("--out", default=None)
    p.add_argument("--budget-s", type=float, default=None)
    a = p.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    torch.cuda.set_device(0)
    rows = []
    start, longest = perf_counter(), 0.0
    for seed in a.seeds:                   # seeds outermost: a run that is cut short still has whole groups
        t0 = perf_counter()
        if a.budget_s is not None and rows and (t0 - start) + longest > a.budget_s:
            print(json.dumps({"stopped_before_seed": seed, "used_s": round(t0 - start, 1), "budget_s": a.budget_s}), flush=True)
            a.seeds = [s for s in a.seeds if any(r["seed"] == s for r in rows)]
            break
        for mk in a.masks:
            for arm in labels(a):
                rows.append(one(arm, seed, mk, a))
                print(json.dumps(rows[-1]), flush=True)
                if a.out:
                    with open(a.out, "w") as f:
                        json.dump(rows + summaries(rows, a), f, indent=1)
        longest = max(longest, perf_counter() - t0)
    for s in summaries(rows, a):
        print(json.dumps(s), flush=True)


if __name__ == "__main__":
    main()
