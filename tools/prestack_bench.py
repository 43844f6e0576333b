"""Kernel time of the fused forward of --wavelet_domain data against the two launches it replaces: the record of an experiment.

The fused entry point dpi_wavelet_moveout_fwd lost this comparison and is NOT in the tree (DESIGN.md 3.2 has the numbers).  The kernel,
its declaration and its ctypes prototype are kept as docs/experiments/wavelet_moveout_fwd.patch; to repeat the measurement:

    git apply docs/experiments/wavelet_moveout_fwd.patch && make -C deep_prior_interpolation_amd/csrc && python tools/prestack_bench.py

Without the patch the tool stops with this advice.

d = W L m on a (1, 1, T, X, Y) fp32 tensor (default 256 x 128 x 128), a wavelet of K = 65 taps, the NMO table of the stand-in's mean law
(tools/moveout_quality.standin_table) and, as the case without mutes, the identity table, for linear and cubic:
    fused   dpi_wavelet_moveout_fwd                                   (1 launch, L m never written)
    chain   dpi_moveout_fwd, then dpi_wavelet_fwd with diff = 0       (2 launches and the intermediate tensor: the path without the entry)
Before anything is timed the two results are compared bit for bit.  Timing: device events around `--reps` calls on one stream, after
`--warmup` calls; `--runs` such windows per variant, fused and chain alternating inside one process; mean and spread (max - min over the
windows) per variant.  The fused forward counts as faster only if the difference of the means exceeds the larger of the two spreads.  One
JSON line per table and interp.

    python tools/prestack_bench.py [--shape 256 128 128] [--K 65] [--runs 7] [--reps 200] [--warmup 20]
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
    p.add_argument("--K", type=int, default=65)
    p.add_argument("--runs", type=int, default=7)
    p.add_argument("--reps", type=int, default=200)
    p.add_argument("--warmup", type=int, default=20)
    a = p.parse_args()
    import torch
    from deep_prior_interpolation_amd import _lib, utils as u
    from deep_prior_interpolation_amd.operators import Moveout, shift_table
    from moveout_quality import standin_table
    if "dpi_wavelet_moveout_fwd" not in _lib.SIGNATURES:
        raise SystemExit("prestack_bench times dpi_wavelet_moveout_fwd, which is not in the tree: apply docs/experiments/"
                         "wavelet_moveout_fwd.patch and rebuild the library first (see the head of this file)")
    if not torch.cuda.is_available():
        raise SystemExit("prestack_bench needs a HIP device: a CPU cannot time these kernels")
    assert a.runs * a.reps >= 1000, "at least 1000 launches per variant"
    torch.cuda.set_device(0)
    L, P, st = _lib.load(), _lib.ptr, _lib.stream()
    shape = tuple(a.shape)
    T, S, K = shape[0], shape[1] * shape[2], a.K
    taps = torch.from_numpy(u.ricker(0.055, 1.0, K, dtype=np.float32)).cuda()
    x = torch.randn((1, 1) + shape, device="cuda")
    mid, y = torch.empty_like(x), torch.empty_like(x)
    tables = {"nmo": standin_table(shape), "identity": shift_table(shape, np.zeros(shape[1:]))}

    def window(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(a.reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / a.reps              # microseconds per forward pass

    stat = lambda v: {"per_run": [round(q, 2) for q in v], "mean": round(float(np.mean(v)), 2), "spread": round(float(np.max(v) - np.min(v)), 2)}
    for tname, tab in tables.items():
        for interp in ("linear", "cubic"):
            op = Moveout(tab, interp)
            tau, _ = op.upload("cuda")

            def fused():
                _lib.check(L.dpi_wavelet_moveout_fwd(P(x), P(tau), op.kind, P(taps), K, 1, T, S, P(y), st), "dpi_wavelet_moveout_fwd")

            def chain():
                _lib.check(L.dpi_moveout_fwd(P(x), P(tau), op.kind, 1, T, S, P(mid), st), "dpi_moveout_fwd")
                _lib.check(L.dpi_wavelet_fwd(P(mid), P(taps), K, 0, 1, T, S, P(y), st), "dpi_wavelet_fwd")

            fused()
            got = y.clone()
            chain()
            torch.cuda.synchronize()
            same = bool(torch.equal(got.view(torch.int32), y.view(torch.int32)))
            for fn in (fused, chain):
                for _ in range(a.warmup):
                    fn()
            us = {"fused": [], "chain": []}
            for r in range(a.runs):
                for name, fn in ((("fused", fused), ("chain", chain)) if r % 2 == 0 else (("chain", chain), ("fused", fused))):
                    us[name].append(window(fn))
            res = {"shape": list(shape), "K": K, "table": tname, "interp": interp, "live": round(float(op.live.mean()), 3), "runs": a.runs,
                   "reps": a.reps, "gpu": torch.cuda.get_device_name(0), "same_bits": same, "fused_us": stat(us["fused"]),
                   "chain_us": stat(us["chain"])}
            gain = res["chain_us"]["mean"] - res["fused_us"]["mean"]
            res["chain_minus_fused_us"] = round(gain, 2)
            res["faster_beyond_spread"] = bool(gain > max(res["fused_us"]["spread"], res["chain_us"]["spread"]))
            print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
