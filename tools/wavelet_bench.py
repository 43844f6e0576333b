"""Kernel time of the --wavelet operator against what the existing kernels would do for the same arithmetic.

Forward + adjoint of one call pair on a [C][T][S] fp32 tensor (default C = 1, 256 x (128 * 128), K = 65), for diff = 0 and diff = 1:
    new        dpi_wavelet_fwd + dpi_wavelet_adj                                            (2 launches)
    baseline   diff = 0: dpi_fir_axis0 (taps) + dpi_fir_axis0 (reversed taps)               (2 launches)
               diff = 1: dpi_diff_axis + dpi_fir_axis0, then dpi_fir_axis0 + dpi_diff_axis  (4 launches, two intermediate tensors)
Before anything is timed the two are compared element by element (they compute the same sums).  Timing: device events around `--reps` pairs
on one stream, after `--warmup` pairs; `--runs` such windows per variant, new and baseline alternating inside one process; mean and spread
(max - min over the windows) per variant.  Bytes are what the algorithm has to move at least (read once, write once, each way).  One JSON
line per diff value.

    python tools/wavelet_bench.py [--shape 1 256 16384] [--K 65] [--runs 7] [--reps 200] [--warmup 20]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--shape", type=int, nargs=3, default=[1, 256, 128 * 128], help="C T S")
    p.add_argument("--K", type=int, default=65)
    p.add_argument("--runs", type=int, default=7)
    p.add_argument("--reps", type=int, default=200)
    p.add_argument("--warmup", type=int, default=20)
    a = p.parse_args()
    import torch
    from deep_prior_interpolation_amd import _lib, utils as u
    if not torch.cuda.is_available():
        raise SystemExit("wavelet_bench needs a HIP device: a CPU cannot time these kernels")
    torch.cuda.set_device(0)
    L, P, st = _lib.load(), _lib.ptr, _lib.stream()
    C_, T, S = a.shape
    K = a.K
    w = u.ricker(0.055, 1.0, K, dtype=np.float32)
    w[K // 2 + 1:] *= np.float32(0.5)                            # asymmetric: forward and adjoint are different filters
    taps, rev = torch.from_numpy(w).cuda(), torch.from_numpy(w[::-1].copy()).cuda()
    x = torch.randn((C_, T, S), device="cuda")
    y1, y2, tmp = torch.empty_like(x), torch.empty_like(x), torch.empty_like(x)
    n_outer = C_

    def new(diff, src=x):
        _lib.check(L.dpi_wavelet_fwd(P(src), P(taps), K, diff, C_, T, S, P(y1), st), "dpi_wavelet_fwd")
        _lib.check(L.dpi_wavelet_adj(P(src), P(taps), K, diff, C_, T, S, P(y2), st), "dpi_wavelet_adj")

    def base(diff, src=x):
        if diff:
            _lib.check(L.dpi_diff_axis(P(src), n_outer, T, S, 0, 1.0, 0, P(tmp), st), "dpi_diff_axis")
            _lib.check(L.dpi_fir_axis0(P(tmp), P(taps), K, C_, T, S, P(y1), st), "dpi_fir_axis0")
            _lib.check(L.dpi_fir_axis0(P(src), P(rev), K, C_, T, S, P(tmp), st), "dpi_fir_axis0")
            _lib.check(L.dpi_diff_axis(P(tmp), n_outer, T, S, 0, 1.0, 1, P(y2), st), "dpi_diff_axis")
        else:
            _lib.check(L.dpi_fir_axis0(P(src), P(taps), K, C_, T, S, P(y1), st), "dpi_fir_axis0")
            _lib.check(L.dpi_fir_axis0(P(src), P(rev), K, C_, T, S, P(y2), st), "dpi_fir_axis0")

    def window(fn, diff):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(a.reps):
            fn(diff)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / a.reps              # microseconds per forward + adjoint pair

    stat = lambda v: {"per_run": [round(q, 2) for q in v], "mean": round(float(np.mean(v)), 2), "spread": round(float(np.max(v) - np.min(v)), 2)}
    for diff in (0, 1):
        new(diff)
        got = (y1.clone(), y2.clone())
        base(diff)
        torch.cuda.synchronize()
        worst = max(float((g - b).abs().max()) for g, b in zip(got, (y1, y2)))
        for fn in (new, base):
            for _ in range(a.warmup):
                fn(diff)
        us = {"new": [], "baseline": []}
        for r in range(a.runs):
            for name, fn in ((("new", new), ("baseline", base)) if r % 2 == 0 else (("baseline", base), ("new", new))):
                us[name].append(window(fn, diff))
        res = {"shape": a.shape, "K": K, "diff": diff, "runs": a.runs, "reps": a.reps, "gpu": torch.cuda.get_device_name(0),
               "max_abs_difference_new_vs_baseline": worst, "new_us": stat(us["new"]), "baseline_us": stat(us["baseline"])}
        res["speedup"] = round(res["baseline_us"]["mean"] / res["new_us"]["mean"], 2)
        min_bytes = 4 * 4 * C_ * T * S                            # forward and adjoint: one read and one write each
        res["new_min_bytes_GBps"] = round(min_bytes / (res["new_us"]["mean"] * 1e-6) / 1e9, 1)
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
