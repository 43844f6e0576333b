"""Kernel time of the semblance scan of --moveout_offset.

dpi_semblance_sums on a (T, X, Y) fp32 volume (default 256 x 128 x 128, 66 % of the traces unknown) with NV trial velocities (default 64),
for the three gather layouts `volume`, `x` and `y`, into preallocated buffers.  Beside each: the float64 numpy restatement of the same sums
on this host (timed on --host-nv of the velocities and scaled to NV; the sums of those velocities are compared with the kernel's), and a
device-to-device copy of `d`, timed the same way in the same process: the launch reads d and mask once per velocity, so
NV x 2 reads = NV x one copy (one read and one write) is the time the bytes alone take out of the caches.  Timing: device events around
--reps launches on one stream after --warmup launches; --runs such windows per variant, the variants alternating; mean and spread
(max - min over the windows).  One JSON line for the copy and one per layout.

    python tools/velocity_scan_bench.py [--shape 256 128 128] [--nv 64] [--host-nv 4] [--runs 5] [--reps 5] [--warmup 2]

--tables times the stage after the scan instead, the table build of a law per gather, for the three layouts: operators.nmo_table on this
host, gather by gather as scan_table calls it (--parent-tree DIR: the function of that checkout, e.g. the commit this one is compared
with; one build per layout, a host clock), against operators.nmo_table_device (--moveout_table device) with its copies to and from the
device, a host clock around --reps calls that each end in a device-to-host copy, --runs windows after --warmup calls, the layouts
alternating.  The floor beside them is one (T, S) float64 array copied from the device the same way.  Each line says whether the two
tables have the same bits.

    python tools/velocity_scan_bench.py --tables [--shape 256 128 128] [--runs 5] [--reps 3] [--warmup 2] [--stretch S] [--parent-tree DIR]
"""
import argparse
import json
import os
import sys
from time import perf_counter

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def host_sums(d, known, off, vel, stretch, geo):
    """The restatement (include/dpi_hip.h, dpi_semblance_sums) in float64 numpy: (num, den, cnt) as (G, NV, T)."""
    T = d.shape[0]
    G, gs, n, ts = geo
    num, den = np.zeros((G, len(vel), T)), np.zeros((G, len(vel), T))
    cnt = np.zeros((G, len(vel), T), dtype=np.int32)
    tau = np.arange(T, dtype=np.float64)[:, None]
    for g in range(G):
        cols = (g * gs + np.arange(n) * ts)[None]
        for j, v in enumerate(vel):
            x = off[cols] / v
            t = np.sqrt(tau * tau + x * x)
            live = t <= T - 1
            if stretch is not None:
                live &= t <= stretch * tau
            i = np.minimum(np.floor(np.where(live, t, 0.0)).astype(np.int64), T - 2)
            live &= known[i, cols] & known[i + 1, cols]
            f = np.where(live, t, 0.0) - i
            a = np.where(live, (1.0 - f) * d[i, cols] + f * d[i + 1, cols], 0.0)
            num[g, j], den[g, j], cnt[g, j] = a.sum(1), (a * a).sum(1), live.sum(1)
    return num, den, cnt


def host_table(nmo_table, shape, off, laws, gather, stretch):
    """The host path of operators.scan_table."""
    if gather == "volume":
        return nmo_table(shape, off, laws[0], stretch)
    axis = 2 if gather == "y" else 1
    return np.stack([nmo_table((shape[0], shape[3 - axis]), np.take(off, g, axis=axis - 1), laws[g], stretch) for g in range(shape[axis])], axis=axis)


def tables(a):
    import torch
    from deep_prior_interpolation_amd.operators import GATHERS, gather_geometry, nmo_table_device
    if not torch.cuda.is_available():
        raise SystemExit("velocity_scan_bench needs a HIP device: a CPU cannot time this kernel")
    torch.cuda.set_device(0)
    if a.parent_tree:                                            # nmo_table of that checkout: its module alone, without its package
        origin = os.path.join(os.path.abspath(a.parent_tree), "deep_prior_interpolation_amd", "operators", "moveout.py")
        src = open(origin).read().replace("from .. import _lib", "_lib = None").replace("from .base import LinearOperator", "LinearOperator = object")
        mod = {"__name__": "parent_moveout_tables"}
        exec(compile(src, origin, "exec"), mod)
        nmo_table = mod["nmo_table"]
    else:
        from deep_prior_interpolation_amd.operators import nmo_table
    shape = tuple(a.shape)
    T, X, Y = shape
    off = T * np.sqrt((np.arange(X)[:, None] / X) ** 2 + (np.arange(Y)[None, :] / Y) ** 2)
    rng = np.random.RandomState(0)
    grid = np.linspace(1.0, 1.8, 33)
    laws = {}
    for k in GATHERS:                                            # staircase picks: a walk of at most one grid step per row, one per gather
        G = gather_geometry(shape, k)[0]
        laws[k] = grid[np.clip(np.cumsum(rng.randint(-1, 2, (G, T)), axis=1) + 12, 0, 32)]
    dev = lambda k: nmo_table_device(shape, off, laws[k], gather=k, stretch_mute=a.stretch)
    flat = torch.zeros((T, X * Y), dtype=torch.float64, device="cuda")
    variants = {k: (lambda k=k: dev(k)) for k in GATHERS}
    variants["copy"] = lambda: flat.cpu().numpy()

    def window(fn):
        torch.cuda.synchronize()
        t0 = perf_counter()
        for _ in range(a.reps):
            fn()                                                 # ends in a device-to-host copy: synchronous
        return (perf_counter() - t0) * 1e3 / a.reps              # milliseconds per build

    for fn in variants.values():
        for _ in range(a.warmup):
            fn()
    ms = {k: [] for k in variants}
    for r in range(a.runs):
        for k in (list(variants) if r % 2 == 0 else list(variants)[::-1]):
            ms[k].append(window(variants[k]))
    stat = lambda q: {"per_run": [round(x, 3) for x in q], "mean": round(float(np.mean(q)), 3), "spread": round(float(np.max(q) - np.min(q)), 3)}
    head = {"shape": a.shape, "runs": a.runs, "reps": a.reps, "stretch": a.stretch, "gpu": torch.cuda.get_device_name(0),
            "host": "parent tree" if a.parent_tree else "this tree"}
    copy = float(np.mean(ms["copy"]))
    print(json.dumps(dict(head, variant="copy_of_one_table_to_the_host", ms=stat(ms["copy"]), GBps=round(8 * flat.numel() / copy / 1e6, 2))), flush=True)
    for k in GATHERS:
        t0 = perf_counter()
        want = host_table(nmo_table, shape, off, laws[k], k, a.stretch)
        host_s = perf_counter() - t0
        got = dev(k)
        live = want != -1.0
        mean = float(np.mean(ms[k]))
        print(json.dumps(dict(head, variant=k, gathers=int(laws[k].shape[0]), device_ms=stat(ms[k]), host_s=round(host_s, 3),
                              times_faster_than_host=round(host_s * 1e3 / mean, 1), times_the_copy=round(mean / copy, 2),
                              live_share=round(float(live.mean()), 4), live_maps_equal=bool(np.array_equal(got != -1.0, live)),
                              bit_identical=bool(np.array_equal(got, want)), max_abs_diff=float(np.max(np.abs(got - want))))), flush=True)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--shape", type=int, nargs=3, default=[256, 128, 128], help="T X Y")
    p.add_argument("--nv", type=int, default=64)
    p.add_argument("--host-nv", type=int, default=4, help="velocities the numpy restatement is run on (its time is scaled to --nv)")
    p.add_argument("--stretch", type=float, default=None)
    p.add_argument("--runs", type=int, default=5)
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--tables", action="store_true", help="time the table build (host nmo_table against nmo_table_device) instead of the scan")
    p.add_argument("--parent-tree", default=None, help="--tables: a checkout whose operators.nmo_table is the host side")
    a = p.parse_args()
    if a.tables:
        return tables(a)
    import torch
    from deep_prior_interpolation_amd import _lib, utils as u
    from deep_prior_interpolation_amd.operators import GATHERS, gather_geometry
    if not torch.cuda.is_available():
        raise SystemExit("velocity_scan_bench needs a HIP device: a CPU cannot time this kernel")
    torch.cuda.set_device(0)
    L = _lib.load()
    T, X, Y = a.shape
    S = X * Y
    vol = (u.hyperbolic_volume(tuple(a.shape), seed=0) * 40.0).astype(np.float32)
    known = np.broadcast_to(u.random_trace_mask(tuple(a.shape), 0.66, seed=1) > 0, vol.shape)
    off = T * np.sqrt((np.arange(X)[:, None] / X) ** 2 + (np.arange(Y)[None, :] / Y) ** 2)
    vel = np.linspace(1.0, 1.8, a.nv)
    d = torch.from_numpy(np.where(known, vol, 0).astype(np.float32).reshape(T, S)).cuda()
    m = torch.from_numpy(known.astype(np.float32).reshape(T, S)).cuda()
    o, v = torch.from_numpy(off.reshape(-1)).cuda(), torch.from_numpy(vel).cuda()
    y = torch.empty_like(d)
    geos = {k: gather_geometry(tuple(a.shape), k) for k in GATHERS}
    out = {k: (torch.empty((g[0], a.nv, T), dtype=torch.float64, device="cuda"), torch.empty((g[0], a.nv, T), dtype=torch.float64, device="cuda"),
               torch.empty((g[0], a.nv, T), dtype=torch.int32, device="cuda")) for k, g in geos.items()}
    stretch = 0.0 if a.stretch is None else a.stretch

    def launch(k, nv=a.nv):
        g, (num, den, cnt) = geos[k], out[k]
        _lib.check(L.dpi_semblance_sums(_lib.ptr(d), _lib.ptr(m), _lib.ptr(o), _lib.ptr(v), nv, stretch, T, S, g[0], g[1], g[2], g[3], _lib.ptr(num),
                                        _lib.ptr(den), _lib.ptr(cnt), _lib.stream()), "dpi_semblance_sums")

    variants = {k: (lambda k=k: launch(k)) for k in GATHERS}
    variants["copy"] = lambda: y.copy_(d)

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
    stat = lambda q: {"per_run": [round(x, 2) for x in q], "mean": round(float(np.mean(q)), 2), "spread": round(float(np.max(q) - np.min(q)), 2)}
    copy = float(np.mean(us["copy"]))
    head = {"shape": a.shape, "nv": a.nv, "runs": a.runs, "reps": a.reps, "gpu": torch.cuda.get_device_name(0)}
    print(json.dumps(dict(head, variant="copy_of_d", us=stat(us["copy"]), GBps=round(2 * 4 * d.numel() / copy / 1e3, 1))), flush=True)
    d64, kn = d.cpu().numpy().astype(np.float64), known.reshape(T, S)
    hv = max(1, min(a.host_nv, a.nv))
    pick = np.unique(np.linspace(0, a.nv - 1, hv).astype(int))
    for k in GATHERS:
        t0 = perf_counter()
        rn, rd, rc = host_sums(d64, kn, off.reshape(-1), vel[pick], a.stretch, geos[k])
        host_s = (perf_counter() - t0) * a.nv / len(pick)
        launch(k)
        torch.cuda.synchronize()
        num, den, cnt = (t.cpu().numpy()[:, pick] for t in out[k])
        mean = float(np.mean(us[k]))
        print(json.dumps(dict(head, variant=k, geometry=list(geos[k]), us=stat(us[k]), ms=round(mean / 1e3, 3),
                              numpy_float64_s_scaled_to_nv=round(host_s, 2), numpy_velocities_timed=int(len(pick)),
                              times_faster_than_numpy=round(host_s * 1e6 / mean, 1),
                              floor_us_nv_copies_of_d=round(a.nv * copy, 1), times_the_floor=round(mean / (a.nv * copy), 2),
                              share_of_a_3000_iteration_patch_of_88_7_s=round(mean / 1e6 / 88.7, 6),
                              cnt_equal=bool(np.array_equal(cnt, rc)),
                              num_max_rel_err=float(np.max(np.abs(num - rn)) / max(np.max(np.abs(rn)), 1e-300)),
                              den_max_rel_err=float(np.max(np.abs(den - rd)) / max(np.max(np.abs(rd)), 1e-300)))), flush=True)


if __name__ == "__main__":
    main()
