"""Kernel time of the trace-sampling operator alone: dpi_trace_resample_fwd / _adj for K = 2, 4, 8 next to the bilinear pair
dpi_trace_sample_fwd / _adj, in one process.  Device events around a batch of launches, a warm-up first, at least --seconds of launches
per figure; the achieved rate counts 8 bytes per sample (one read, one write), the traffic both designs are bound by.  One JSON line.

    python tools/trace_resample_bench.py [--rows 256] [--traces 128 128] [--seconds 1.0]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(launch, seconds, torch):
    for _ in range(20):
        launch()
    torch.cuda.synchronize()
    batch, total_ms, n = 50, 0.0, 0
    while total_ms < 1e3 * seconds:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(batch):
            launch()
        e1.record()
        e1.synchronize()
        total_ms += e0.elapsed_time(e1)
        n += batch
    return 1e3 * total_ms / n          # microseconds per launch


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--rows", type=int, default=256, help="C * T")
    p.add_argument("--traces", type=int, nargs=2, default=[128, 128])
    p.add_argument("--seconds", type=float, default=1.0)
    a = p.parse_args()
    import torch
    from deep_prior_interpolation_amd import _lib
    from deep_prior_interpolation_amd.operators import INTERP_TAPS, interp_weights
    torch.cuda.set_device(0)
    L = _lib.load()
    X, Y = a.traces
    off = np.random.RandomState(2).uniform(-0.5, 0.5, (2, X, Y)).astype(np.float32)
    offd = torch.from_numpy(off).cuda()
    x = torch.randn(1, a.rows, X, Y, device="cuda")
    y = torch.empty_like(x)
    nbytes = 8.0 * x.numel()
    st = _lib.stream()
    res = {"rows": a.rows, "traces": [X, Y], "gpu": torch.cuda.get_device_name(0), "bytes_per_launch": nbytes}

    def row(us):
        return {"us": round(us, 2), "TB_per_s": round(nbytes / us * 1e-6, 3)}

    for name, fn in (("fwd", L.dpi_trace_sample_fwd), ("adj", L.dpi_trace_sample_adj)):
        res["bilinear_" + name] = row(timed(lambda: fn(_lib.ptr(x), _lib.ptr(offd), 1, a.rows, X, Y, _lib.ptr(y), st), a.seconds, torch))
    for interp, K in INTERP_TAPS.items():
        w = torch.from_numpy(interp_weights(off, interp)).cuda()
        for name, fn in (("fwd", L.dpi_trace_resample_fwd), ("adj", L.dpi_trace_resample_adj)):
            us = timed(lambda: fn(_lib.ptr(x), _lib.ptr(w), _lib.ptr(offd), K, 1, a.rows, X, Y, _lib.ptr(y), st), a.seconds, torch)
            res["K%d_%s" % (K, name)] = row(us)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
