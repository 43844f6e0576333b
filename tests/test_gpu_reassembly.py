"""GPU tests of the weighted re-assembly: dpi_overlap_add_weighted / dpi_overlap_finalize_weighted against a float64 numpy restatement
written here (it imports nothing of the host code under test), through guarded buffers; the host refusals; DeviceBlendAccumulator; and
the drivers end to end (--reassembly cover --blend taper, the std volume of a sampler run, the untouched default).

Bars: rtol 1e-5, atol 1e-6 — those of test_overlap_add_vs_oracle.  The kernel's sums are fp32 (weights, products and at most 8 terms per
sample at these shapes): a float32 numpy emulation of the same arithmetic stays within 1.0e-6 absolute of float64 on unit-variance data
BEFORE the division by the gain (40 here)."""
import itertools
import os

import numpy as np
import pytest
import torch

from gpu_guard import guard

pytestmark = pytest.mark.gpu
DEV = "cuda"
RTOL, ATOL = 1e-5, 1e-6
GAIN = 40.0

# name: (volume, patch, stride, offset (floats) of the accumulator, offset of the patches)
CASES = {
    "scalar": ((21, 19, 25), (8, 6, 10), (4, 4, 6), 0, 0),           # W, pw and the W origins are no multiples of 4
    "vector": ((24, 16, 32), (8, 8, 16), (4, 4, 8), 0, 0),           # every row, origin and base on 16 bytes
    "vector_acc_off1": ((24, 16, 32), (8, 8, 16), (4, 4, 8), 1, 0),  # the same shape on bases moved by one float: must fall back
    "vector_patch_off1": ((24, 16, 32), (8, 8, 16), (4, 4, 8), 0, 1),
}


# ---------------------------------------------------------------- the restatement -------------------------------------------------------
def _ref_axis_origins(n, d, s, cover):
    org = list(range(0, n - d + 1, s))
    if cover and org[-1] != n - d:
        org.append(n - d)
    return org


def _ref_origins(shape, dim, stride, cover):
    return [tuple(o) for o in itertools.product(*[_ref_axis_origins(n, d, s, cover) for n, d, s in zip(shape, dim, stride)])]


def _ref_ramp(d, s):
    L = max(0, min(d - s, d // 2))
    return np.array([np.sin(np.pi * (i + 0.5) / (2 * L)) ** 2 for i in range(L)])


def _ref_window(n, d, s, o, taper):
    w = np.ones(d)
    if taper:
        for i, r in enumerate(_ref_ramp(d, s)):
            if o > 0:
                w[i] *= r
            if o + d < n:
                w[d - 1 - i] *= r
    return w


def _ref_blend(patches, origins, shape, dim, stride, taper, spread=False):
    num, den = np.zeros(shape), np.zeros(shape)
    for p, org in zip(patches, origins):
        w = np.ones(())
        for n, d, s, o in zip(shape, dim, stride, org):
            w = np.multiply.outer(w, _ref_window(n, d, s, o, taper))
        sl = tuple(slice(o, o + d) for o, d in zip(org, dim))
        num[sl] += w * (np.asarray(p, np.float64) ** 2 if spread else np.asarray(p, np.float64))
        den[sl] += w
    out = num / den
    return np.sqrt(out) if spread else out


def _ref_weight_sum(origins, shape, dim, stride, taper):
    tot = np.zeros(shape)
    for org in origins:
        w = np.ones(())
        for n, d, s, o in zip(shape, dim, stride, org):
            w = np.multiply.outer(w, _ref_window(n, d, s, o, taper))
        tot[tuple(slice(o, o + d) for o, d in zip(org, dim))] += w
    return tot


def _sides(shape, dim, org):
    m = 0
    for k, (n, d, o) in enumerate(zip(shape, dim, org)):
        m |= (int(o > 0) << (2 * k)) | (int(o + d < n) << (2 * k + 1))
    return m


def _ramp_args(dim, stride, taper):
    """Device tables (kept alive by the caller) and the (ptr, length) x 3 arguments."""
    tabs = [torch.from_numpy(_ref_ramp(d, s).astype(np.float32)).to(DEV) if taper and len(_ref_ramp(d, s)) else None for d, s in zip(dim, stride)]
    args = []
    for t in tabs:
        args += [None if t is None else t.data_ptr(), 0 if t is None else t.numel()]
    return tabs, args


@pytest.fixture(scope="module")
def lib():
    from deep_prior_interpolation_amd import _lib
    return _lib.load()


# ---------------------------------------------------------------- kernels ---------------------------------------------------------------
@pytest.mark.parametrize("taper", [True, False], ids=["taper", "flat"])
@pytest.mark.parametrize("K", [2, 3])
@pytest.mark.parametrize("case", list(CASES))
def test_kernels_against_the_restatement(lib, case, K, taper):
    from deep_prior_interpolation_amd import _lib
    shape, dim, stride, acc_off, patch_off = CASES[case]
    origins = _ref_origins(shape, dim, stride, True)
    if case == "scalar":
        assert len(origins) == 100 and any(o[2] % 4 for o in origins)
    rng = np.random.RandomState(0)
    pn = int(np.prod(dim))
    n = int(np.prod(shape))
    pa = rng.randn(len(origins), *dim).astype(np.float32)
    sd = np.abs(rng.randn(len(origins), *dim)).astype(np.float32)
    g_mean = guard(pa.size, torch.float32, DEV, fill=torch.from_numpy(pa), offset=patch_off)
    g_std = guard(sd.size, torch.float32, DEV, fill=torch.from_numpy(sd), offset=patch_off)
    g_acc = guard(K * n, torch.float32, DEV, fill=torch.zeros(K * n), offset=acc_off)
    g_om = guard(n, torch.float32, DEV, offset=acc_off)
    g_os = guard(n, torch.float32, DEV, offset=acc_off)
    assert g_acc.payload.data_ptr() % 16 == 4 * acc_off and g_mean.payload.data_ptr() % 16 == 4 * patch_off
    tabs, ramps = _ramp_args(dim, stride, taper)
    for i, org in enumerate(origins):
        _lib.check(lib.dpi_overlap_add_weighted(g_mean.payload.data_ptr() + 4 * pn * i, (g_std.payload.data_ptr() + 4 * pn * i) if K == 3 else None,
                                                *dim, *org, *ramps, _sides(shape, dim, org), g_acc.payload.data_ptr(), K, *shape, _lib.stream()),
                   "dpi_overlap_add_weighted")
    _lib.check(lib.dpi_overlap_finalize_weighted(g_acc.payload.data_ptr(), K, *shape, GAIN, g_om.payload.data_ptr(),
                                                 g_os.payload.data_ptr() if K == 3 else None, _lib.stream()), "dpi_overlap_finalize_weighted")
    torch.cuda.synchronize()
    for g, what in ((g_mean, "mean patches"), (g_std, "std patches"), (g_acc, "acc"), (g_om, "out_mean"), (g_os, "out_std")):
        g.check(what)
    assert torch.equal(g_mean.payload.cpu(), torch.from_numpy(pa).reshape(-1)) and torch.equal(g_std.payload.cpu(), torch.from_numpy(sd).reshape(-1))
    acc = g_acc.payload.cpu().numpy().reshape((K,) + shape).astype(np.float64)
    np.testing.assert_allclose(acc[0], _ref_weight_sum(origins, shape, dim, stride, taper), rtol=RTOL, atol=ATOL)
    got = g_om.payload.cpu().numpy().reshape(shape)
    print("mean: max |err| %.3e" % np.abs(got - _ref_blend(pa, origins, shape, dim, stride, taper) / GAIN).max())
    np.testing.assert_allclose(got, _ref_blend(pa, origins, shape, dim, stride, taper) / GAIN, rtol=RTOL, atol=ATOL)
    if K == 3:
        got = g_os.payload.cpu().numpy().reshape(shape)
        ref = _ref_blend(sd, origins, shape, dim, stride, taper, spread=True) / GAIN
        print("std: max |err| %.3e" % np.abs(got - ref).max())
        assert (got >= 0).all()
        np.testing.assert_allclose(got, ref, rtol=RTOL, atol=ATOL)
    else:
        assert bool(torch.isnan(g_os.payload).all())                 # no std volume asked for: never written


def test_negative_gain_and_zero_weight(lib):
    """gain < 0: the mean changes sign, the std does not; a sample no window reached gives 0 in both."""
    from deep_prior_interpolation_amd import _lib
    shape, dim = (8, 8, 12), (4, 4, 8)
    p = torch.full(dim, 3.0, device=DEV)
    s = torch.full(dim, 2.0, device=DEV)
    acc = torch.zeros((3,) + shape, device=DEV)
    _lib.check(lib.dpi_overlap_add_weighted(p.data_ptr(), s.data_ptr(), *dim, 2, 1, 4, None, 0, None, 0, None, 0, 0, acc.data_ptr(), 3, *shape,
                                            _lib.stream()), "add")
    mean, std = torch.full(shape, float("nan"), device=DEV), torch.full(shape, float("nan"), device=DEV)
    _lib.check(lib.dpi_overlap_finalize_weighted(acc.data_ptr(), 3, *shape, -2.0, mean.data_ptr(), std.data_ptr(), _lib.stream()), "finalize")
    ref_m, ref_s = np.zeros(shape, np.float32), np.zeros(shape, np.float32)
    ref_m[2:6, 1:5, 4:12], ref_s[2:6, 1:5, 4:12] = -1.5, 1.0
    np.testing.assert_array_equal(mean.cpu().numpy(), ref_m)
    np.testing.assert_array_equal(std.cpu().numpy(), ref_s)


def test_bad_arguments_are_refused(lib):
    shape, dim = (12, 12, 16), (8, 8, 8)
    n = int(np.prod(shape))
    g_acc = guard(3 * n, torch.float32, DEV, fill=torch.arange(3 * n, dtype=torch.float32))
    g_out = guard(n, torch.float32, DEV)
    p = torch.ones(dim, device=DEV)
    r = torch.full((4,), 0.5, device=DEV)
    before, out_before = g_acc.bits(), g_out.bits()
    A, P_, R, st = g_acc.payload.data_ptr(), p.data_ptr(), r.data_ptr(), torch.cuda.current_stream().cuda_stream

    def add(mean=P_, std=None, org=(0, 0, 0), ls=(4, 4, 4), sides=63, K=2, ramp=R, acc=A):
        return lib.dpi_overlap_add_weighted(mean, std, *dim, *org, ramp, ls[0], ramp, ls[1], ramp, ls[2], sides, acc, K, *shape, st)

    def fin(K=2, gain=GAIN, out=g_out.payload.data_ptr(), out_std=None, acc=A):
        return lib.dpi_overlap_finalize_weighted(acc, K, *shape, gain, out, out_std, st)
    bad = {
        "patch past the end of W": lambda: add(org=(0, 0, 9)),
        "patch past the end of D": lambda: add(org=(5, 0, 0)),
        "negative origin": lambda: add(org=(0, -1, 0)),
        "K = 3 without a std patch": lambda: add(K=3),
        "K = 2 with a std patch": lambda: add(std=P_),
        "K = 4": lambda: add(std=P_, K=4),
        "ramp longer than half the patch": lambda: add(ls=(4, 5, 4)),
        "negative ramp length": lambda: add(ls=(-1, 4, 4)),
        "ramp without its table": lambda: add(ramp=None),
        "unknown side bits": lambda: add(sides=64),
        "no patch": lambda: add(mean=None),
        "no accumulator": lambda: add(acc=None),
        "gain 0": lambda: fin(gain=0.0),
        "finalize K = 1": lambda: fin(K=1),
        "std volume without the variance plane": lambda: fin(K=2, out_std=g_out.payload.data_ptr()),
        "no output": lambda: fin(out=None),
    }
    for what, call in bad.items():
        assert call() != 0, what
        msg = lib.dpi_last_error()
        assert msg and b"overlap_" in msg, what
    torch.cuda.synchronize()
    assert g_acc.untouched(before) and g_out.untouched(out_before)         # nothing was launched
    g_acc.check("acc")
    g_out.check("out")
    assert add() == 0 and add(std=P_, K=3) == 0 and fin() == 0             # the same calls with good arguments go through
    torch.cuda.synchronize()
    g_acc.check("acc")
    g_out.check("out")


# ---------------------------------------------------------------- the accumulator -------------------------------------------------------
@pytest.mark.parametrize("taper", [True, False], ids=["taper", "flat"])
@pytest.mark.parametrize("shape,dim,stride", [((21, 19, 25), (8, 6, 10), (4, 4, 6)), ((24, 20, 36), (16, 16, 16), (8, 8, 8))])
def test_identity_on_the_device(shape, dim, stride, taper):
    """Patches cut from a volume come back as the volume, at full shape (and a spread field |v| as |v|)."""
    from deep_prior_interpolation_amd.parallel import DeviceBlendAccumulator
    vol = np.random.RandomState(1).randn(*shape).astype(np.float32)
    acc = DeviceBlendAccumulator(shape, dim, stride, DEV, taper=taper, with_std=True)
    assert tuple(acc.tensor().shape) == (3,) + shape                         # ONE stacked buffer: one all-reduce
    for org in _ref_origins(shape, dim, stride, True):
        p = vol[tuple(slice(o, o + d) for o, d in zip(org, dim))]
        acc.add(torch.from_numpy(np.ascontiguousarray(p)).to(DEV), org, std=np.abs(p))
    rec = acc.finalize(1.0)
    assert rec.shape == shape and acc.std_volume.shape == shape
    np.testing.assert_allclose(rec, vol, rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(acc.std_volume, np.abs(vol), rtol=RTOL, atol=ATOL)


def test_accumulator_without_a_std_counts_it_as_zero():
    from deep_prior_interpolation_amd import _lib
    from deep_prior_interpolation_amd.parallel import DeviceBlendAccumulator
    shape, dim, stride = (12, 8, 8), (8, 8, 8), (4, 8, 8)
    acc = DeviceBlendAccumulator(shape, dim, stride, DEV, taper=False, with_std=True)
    acc.add(np.ones(dim, np.float32), (0, 0, 0), std=np.full(dim, 2.0, np.float32))
    acc.add(np.ones(dim, np.float32), (4, 0, 0))                              # a skipped patch: no spread
    rec = acc.finalize(1.0)
    np.testing.assert_array_equal(rec, np.ones(shape, np.float32))
    ref = np.zeros(shape)
    ref[:4], ref[4:8] = 2.0, np.sqrt(2.0)
    np.testing.assert_allclose(acc.std_volume, ref, rtol=RTOL, atol=ATOL)
    with pytest.raises(_lib.DpiError):
        DeviceBlendAccumulator(shape, dim, stride, DEV).add(np.ones(dim, np.float32), (0, 0, 0), std=np.ones(dim, np.float32))
    with pytest.raises(_lib.DpiError):
        acc.add(np.ones((4, 8, 8), np.float32), (0, 0, 0))


# ---------------------------------------------------------------- end to end ------------------------------------------------------------
VOL, PATCH, STRIDE, E2E_GAIN = (24, 20, 20), (16, 16, 16), (8, 8, 8), 10.0


def _run_job(tmp_path, monkeypatch, outdir, extra, conc=1):
    from deep_prior_interpolation_amd import parallel, utils as u
    d = tmp_path / "data"
    if not d.exists():
        d.mkdir()
        np.save(d / "vol.npy", u.hyperbolic_volume(VOL, seed=1).astype(np.float32))
        np.save(d / "mask.npy", np.broadcast_to(u.random_trace_mask(VOL, 0.5, seed=2), VOL).astype(np.float32))
    monkeypatch.chdir(tmp_path)
    for k, v in (("RANK", "0"), ("WORLD_SIZE", "1"), ("LOCAL_RANK", "0"), ("DPI_CONCURRENT_PATCHES", str(conc))):
        monkeypatch.setenv(k, v)
    parallel.main(["--imgdir", str(d), "--imgname", "vol.npy", "--maskname", "mask.npy", "--datadim", "3d", "--patch_shape", "16", "16", "16",
                   "--patch_stride", "8", "8", "8", "--filters", "4", "8", "--skip", "4", "--inputdepth", "4", "--epochs", "4", "--gpu", "0",
                   "--gain", str(E2E_GAIN), "--outdir", outdir] + extra)
    out = os.path.join("results", outdir)
    names = sorted(f for f in os.listdir(out) if f.endswith("_run.npy"))
    return out, [np.load(os.path.join(out, f), allow_pickle=True).item() for f in names]


@pytest.mark.parametrize("conc", [1, 2])
def test_cover_and_taper_end_to_end(tmp_path, monkeypatch, conc):
    out, runs = _run_job(tmp_path, monkeypatch, "cover", ["--reassembly", "cover", "--blend", "taper"], conc)
    origins = _ref_origins(VOL, PATCH, STRIDE, True)
    assert len(runs) == 8 == len(origins)
    rec = np.load(os.path.join(out, "reconstructed.npy"))
    assert rec.shape == VOL and np.isfinite(rec).all()
    ref = _ref_blend([r["output"] for r in runs], origins, VOL, PATCH, STRIDE, True) / E2E_GAIN
    print("max |err| %.3e, max |ref| %.3e" % (np.abs(rec - ref).max(), np.abs(ref).max()))
    np.testing.assert_allclose(rec, ref, rtol=RTOL, atol=ATOL)
    assert not os.path.exists(os.path.join(out, "reconstructed_std.npy"))
    assert "cover" in open(os.path.join(out, "args.txt")).read()


@pytest.mark.parametrize("conc", [1, 2])
def test_std_volume_end_to_end(tmp_path, monkeypatch, conc):
    out, runs = _run_job(tmp_path, monkeypatch, "sgld", ["--reassembly", "cover", "--blend", "taper", "--optimizer", "sgld", "--posterior_burnin", "1"],
                         conc)
    origins = _ref_origins(VOL, PATCH, STRIDE, True)
    assert len(runs) == 8 and all(r["posterior_samples"] == 3 and r["posterior_std"].shape == PATCH for r in runs)
    rec, std = np.load(os.path.join(out, "reconstructed.npy")), np.load(os.path.join(out, "reconstructed_std.npy"))
    assert rec.shape == VOL and std.shape == VOL and np.isfinite(rec).all() and np.isfinite(std).all()
    assert (std >= 0).all() and std.max() > 0
    np.testing.assert_allclose(rec, _ref_blend([r["output"] for r in runs], origins, VOL, PATCH, STRIDE, True) / E2E_GAIN, rtol=RTOL, atol=ATOL)
    ref = _ref_blend([r["posterior_std"] for r in runs], origins, VOL, PATCH, STRIDE, True, spread=True) / E2E_GAIN
    print("std: max |err| %.3e, max |ref| %.3e" % (np.abs(std - ref).max(), np.abs(ref).max()))
    np.testing.assert_allclose(std, ref, rtol=RTOL, atol=ATOL)


def test_default_flags_keep_the_cropped_volume_and_its_bytes(tmp_path, monkeypatch):
    from deep_prior_interpolation_amd.parallel import DeviceOverlapAccumulator
    out, runs = _run_job(tmp_path, monkeypatch, "default", [])
    cropped = (24, 16, 16)
    assert len(runs) == 2
    rec = np.load(os.path.join(out, "reconstructed.npy"))
    assert rec.shape == cropped and not os.path.exists(os.path.join(out, "reconstructed_std.npy"))
    acc = DeviceOverlapAccumulator(cropped, PATCH, STRIDE, DEV)
    for r, org in zip(runs, _ref_origins(VOL, PATCH, STRIDE, False)):
        acc.add(r["output"], org)
    np.testing.assert_array_equal(rec, acc.finalize(E2E_GAIN))


def test_2d_job_is_reassembled_on_the_host(tmp_path, monkeypatch):
    """2-D data: result files only, rank 0 re-assembles them through data.reconstruct_patches — covering windows, taper, std volume."""
    from deep_prior_interpolation_amd import parallel
    shape, dim, stride = (24, 20), (16, 16), (8, 8)
    t, x = np.meshgrid(np.arange(shape[0]), np.arange(shape[1]), indexing="ij")
    d = tmp_path / "data"
    d.mkdir()
    np.save(d / "sec.npy", np.sin(0.4 * t + 0.2 * x).astype(np.float32))
    np.save(d / "mask.npy", np.broadcast_to((np.arange(shape[1]) % 3 != 0).astype(np.float32), shape).copy())
    monkeypatch.chdir(tmp_path)
    for k, v in (("RANK", "0"), ("WORLD_SIZE", "1"), ("LOCAL_RANK", "0")):
        monkeypatch.setenv(k, v)
    parallel.main(["--imgdir", str(d), "--imgname", "sec.npy", "--maskname", "mask.npy", "--datadim", "2d", "--patch_shape", "16", "16",
                   "--patch_stride", "8", "8", "--filters", "4", "8", "--skip", "4", "--inputdepth", "4", "--epochs", "4", "--gpu", "0",
                   "--gain", str(E2E_GAIN), "--outdir", "sec", "--reassembly", "cover", "--blend", "taper", "--optimizer", "sgld",
                   "--posterior_burnin", "1"])
    out = os.path.join("results", "sec")
    runs = [np.load(os.path.join(out, f), allow_pickle=True).item() for f in sorted(os.listdir(out)) if f.endswith("_run.npy")]
    origins = _ref_origins(shape, dim, stride, True)
    assert len(runs) == 4 == len(origins)
    rec, std = np.load(os.path.join(out, "reconstructed.npy")), np.load(os.path.join(out, "reconstructed_std.npy"))
    assert rec.shape == shape and std.shape == shape and (std >= 0).all() and std.max() > 0
    np.testing.assert_allclose(rec, _ref_blend([r["output"][..., 0] for r in runs], origins, shape, dim, stride, True) / E2E_GAIN,
                               rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(std, _ref_blend([r["posterior_std"][..., 0] for r in runs], origins, shape, dim, stride, True, spread=True) / E2E_GAIN,
                               rtol=RTOL, atol=ATOL)
