"""Kernel time of the --moveout operator against the bytes it has to move.

Forward and adjoint (dpi_moveout_fwd, dpi_moveout_adj, one launch each; pair_us = their sum) on a (1, 1, T, X, Y) fp32 tensor (default 256 x 128 x
128), for linear and cubic, with the NMO table of the stand-in's mean law (tools/moveout_quality.standin_table: about a third of the
samples live) and with the identity table (every sample live, one tap with weight 1).  The floor is a device-to-device copy of one such
tensor, timed the same way: what reading and writing the tensor once costs.  Timing: device events around `--reps` launches on one
stream, after `--warmup` launches; `--runs` such windows per variant, forward, adjoint and the copy alternating inside one process; mean and
spread (max - min over the windows).  One JSON line for the copy and one per table and interp.

    python tools/moveout_bench.py [--shape 256 128 128] [--runs 7] [--reps 200] [--warmup 20]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--shape", type=int, nargs=3, default=[256, 128, 128], help="T X Y")
    p.add_argument("--runs", type=int, default=7)
    p.add_argument("--reps", type=int, default=200)
    p.add_argument("--warmup", type=int, default=20)
    a = p.parse_args()
    import torch
    from deep_prior_interpolation_amd.operators import Moveout, shift_table
    from moveout_quality import standin_table
    if not torch.cuda.is_available():
        raise SystemExit("moveout_bench needs a HIP device: a CPU cannot time these kernels")
    assert a.runs * a.reps >= 1000, "at least 1000 launches per variant"
    torch.cuda.set_device(0)
    shape = tuple(a.shape)
    tables = {"nmo": standin_table(shape), "identity": shift_table(shape, np.zeros(shape[1:]))}
    x = torch.randn((1, 1) + shape, device="cuda")
    y = torch.empty_like(x)
    variants = {}
    for tname, tab in tables.items():
        for interp in ("linear", "cubic"):
            op = Moveout(tab, interp)
            op.upload("cuda")
            for adjoint in (False, True):
                variants["%s_%s_%s" % (tname, interp, "adj" if adjoint else "fwd")] = (lambda op=op, adjoint=adjoint: op._matvec(x, adjoint),
                                                                                     float(op.live.mean()))
    variants["copy"] = (lambda: y.copy_(x), 1.0)

    def window(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(a.reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / a.reps              # microseconds per launch

    for fn, _ in variants.values():
        for _ in range(a.warmup):
            fn()
    us = {k: [] for k in variants}
    for r in range(a.runs):
        for k in (list(variants) if r % 2 == 0 else list(variants)[::-1]):
            us[k].append(window(variants[k][0]))
    stat = lambda v: {"per_run": [round(q, 2) for q in v], "mean": round(float(np.mean(v)), 2), "spread": round(float(np.max(v) - np.min(v)), 2)}
    floor = float(np.mean(us["copy"]))
    head = {"shape": a.shape, "runs": a.runs, "reps": a.reps, "gpu": torch.cuda.get_device_name(0)}
    print(json.dumps(dict(head, variant="copy", us=stat(us["copy"]), GBps=round(2 * 4 * x.numel() / floor / 1e3, 1))), flush=True)
    for tname in tables:
        for interp in ("linear", "cubic"):
            f, b = us["%s_%s_fwd" % (tname, interp)], us["%s_%s_adj" % (tname, interp)]
            print(json.dumps(dict(head, variant="%s_%s" % (tname, interp), live_share=round(variants["%s_%s_fwd" % (tname, interp)][1], 4),
                                  fwd_us=stat(f), adj_us=stat(b), pair_us=round(float(np.mean(f) + np.mean(b)), 2),
                                  fwd_times_the_copy=round(float(np.mean(f)) / floor, 2), adj_times_the_copy=round(float(np.mean(b)) / floor, 2))),
                  flush=True)


if __name__ == "__main__":
    main()
