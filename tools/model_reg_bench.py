"""Kernel time of the --model_reg penalty against the bytes it has to move.

dpi_model_reg (the value-and-gradient launch plus its one-wave finish) on a (1, 1, T, X, Y) fp32 tensor (default 256 x 128 x 128) for the
four kinds l1, tv_t, tv_x, tv, into preallocated buffers.  The figure beside it is a device-to-device copy of one such tensor, timed the
same way in the same process: the same bytes in, the same bytes out.  Timing: device events around `--reps` launches on one stream, after
`--warmup` launches; `--runs` such windows per variant, the variants alternating; mean and spread (max - min over the windows).  One JSON
line for the copy and one per kind.

    python tools/model_reg_bench.py [--shape 256 128 128] [--runs 7] [--reps 200] [--warmup 20]
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
    p.add_argument("--shape", type=int, nargs=3, default=[256, 128, 128], help="T X Y")
    p.add_argument("--runs", type=int, default=7)
    p.add_argument("--reps", type=int, default=200)
    p.add_argument("--warmup", type=int, default=20)
    a = p.parse_args()
    import torch
    from deep_prior_interpolation_amd import _lib
    from deep_prior_interpolation_amd.parameter import MODEL_REG_KINDS, model_reg_axes
    if not torch.cuda.is_available():
        raise SystemExit("model_reg_bench needs a HIP device: a CPU cannot time these kernels")
    assert a.runs * a.reps >= 1000, "at least 1000 launches per variant"
    torch.cuda.set_device(0)
    L = _lib.load()
    T, X, Y = a.shape
    x = torch.randn((1, 1, T, X, Y), device="cuda")
    y = torch.empty_like(x)
    grad = torch.empty_like(x)
    ws = torch.empty(L.dpi_model_reg_ws_doubles(x.numel()), dtype=torch.float64, device="cuda")
    res = torch.empty(1, dtype=torch.float64, device="cuda")

    def launch(bits):
        _lib.check(L.dpi_model_reg(_lib.ptr(x), 1, T, X, Y, bits, _lib.ptr(grad), _lib.ptr(ws), _lib.ptr(res), _lib.stream()), "dpi_model_reg")

    bits = {k: sum(1 << (d - 2) for d in model_reg_axes(k, "3d", "xy")) for k in MODEL_REG_KINDS}
    variants = {k: (lambda b=b: launch(b)) for k, b in bits.items()}
    variants["copy"] = lambda: y.copy_(x)

    def window(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(a.reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / a.reps              # microseconds per launch

    for fn in variants.values():
        for _ in range(a.warmup):
            fn()
    us = {k: [] for k in variants}
    for r in range(a.runs):
        for k in (list(variants) if r % 2 == 0 else list(variants)[::-1]):
            us[k].append(window(variants[k]))
    stat = lambda v: {"per_run": [round(q, 2) for q in v], "mean": round(float(np.mean(v)), 2), "spread": round(float(np.max(v) - np.min(v)), 2)}
    floor = float(np.mean(us["copy"]))
    nbytes = 2 * 4 * x.numel()
    head = {"shape": a.shape, "runs": a.runs, "reps": a.reps, "gpu": torch.cuda.get_device_name(0)}
    print(json.dumps(dict(head, variant="copy", us=stat(us["copy"]), GBps=round(nbytes / floor / 1e3, 1))), flush=True)
    for k in MODEL_REG_KINDS:
        m = float(np.mean(us[k]))
        print(json.dumps(dict(head, variant=k, axes=bits[k], us=stat(us[k]), GBps_of_one_read_one_write=round(nbytes / m / 1e3, 1),
                              times_the_copy=round(m / floor, 2))), flush=True)


if __name__ == "__main__":
    main()
