"""Host-side tests of the full-volume re-assembly (--reassembly cover, --blend taper, the std volume): covering origins, taper windows,
the weighted overlap-add in float64, data.extract_patches / reconstruct_patches through files, the parser, the exported symbols and a
2-rank gloo run.  No GPU needed.  `_ref_*` below restate the arithmetic on their own (they import nothing of the code under test)."""
import os
import re
import socket
import subprocess
from argparse import Namespace

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [((21, 19, 25), (8, 6, 10), (4, 4, 6)), ((37, 33, 41), (16, 16, 16), (8, 8, 8))]
DIVISIBLE = ((20, 18, 22), (8, 6, 10), (4, 4, 6))
NEW = ("dpi_overlap_add_weighted", "dpi_overlap_finalize_weighted")


# ---------------------------------------------------------------- the restatement -------------------------------------------------------
def _ref_axis_origins(n, d, s, cover):
    org = list(range(0, n - d + 1, s))
    if cover and org[-1] != n - d:
        org.append(n - d)
    return org


def _ref_origins(shape, dim, stride, cover):
    import itertools
    return [tuple(o) for o in itertools.product(*[_ref_axis_origins(n, d, s, cover) for n, d, s in zip(shape, dim, stride)])]


def _ref_window(n, d, s, o, taper):
    L = min(d - s, d // 2) if taper else 0
    w = np.ones(d)
    for i in range(max(L, 0)):
        r = np.sin(np.pi * (i + 0.5) / (2 * L)) ** 2
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
        num[sl] += w * (np.asarray(p, np.float64) ** 2 if spread else p)
        den[sl] += w
    out = num / den
    return np.sqrt(out) if spread else out


def _cut(vol, origins, dim):
    return [vol[tuple(slice(o, o + d) for o, d in zip(org, dim))] for org in origins]


# ---------------------------------------------------------------- origins ---------------------------------------------------------------
@pytest.mark.parametrize("shape,dim,stride", SHAPES + [DIVISIBLE])
def test_crop_origins_are_todays(shape, dim, stride):
    from deep_prior_interpolation_amd import utils as u
    grid = [(n - d) // s + 1 for n, d, s in zip(shape, dim, stride)]
    today = np.stack(np.meshgrid(*[np.arange(g) for g in grid], indexing="ij"), axis=-1).reshape(-1, 3) * np.asarray(stride)[None, :]
    for got in (u.window_origins(shape, dim, stride), u.window_origins(shape, dim, stride, cover=False)):
        np.testing.assert_array_equal(got, today)
        assert got.dtype == today.dtype
    assert u.reassembled_shape(shape, dim, stride) == u.in_content_cropped_shape(shape, dim, stride)


@pytest.mark.parametrize("shape,dim,stride", SHAPES)
def test_cover_origins_reach_the_end_of_every_axis(shape, dim, stride):
    from deep_prior_interpolation_amd import utils as u
    org = u.window_origins(shape, dim, stride, cover=True)
    assert [tuple(int(v) for v in o) for o in org] == _ref_origins(shape, dim, stride, True)         # C order of the per-axis lists
    assert tuple(org[-1]) == tuple(n - d for n, d in zip(shape, dim))
    assert len(set(map(tuple, org))) == len(org)
    hits = np.zeros(shape, int)
    for o in org:
        hits[tuple(slice(a, a + d) for a, d in zip(o, dim))] += 1
    assert hits.min() >= 1
    if shape == (21, 19, 25):
        assert len(org) == 100
    assert u.reassembled_shape(shape, dim, stride, cover=True) == shape


def test_cover_adds_nothing_on_a_divisible_shape():
    from deep_prior_interpolation_amd import utils as u
    shape, dim, stride = DIVISIBLE
    np.testing.assert_array_equal(u.window_origins(shape, dim, stride, cover=True), u.window_origins(shape, dim, stride))


def test_cover_refuses_an_axis_shorter_than_the_patch():
    from deep_prior_interpolation_amd import utils as u
    with pytest.raises(ValueError, match="axis 1"):
        u.window_origins((21, 5, 25), (8, 6, 10), (4, 4, 6), cover=True)
    with pytest.raises(ValueError, match="axis 1"):
        u.reassembled_shape((21, 5, 25), (8, 6, 10), (4, 4, 6), cover=True)


# ---------------------------------------------------------------- windows ---------------------------------------------------------------
def test_ramp_definition():
    from deep_prior_interpolation_amd import utils as u
    assert u.taper_length(16, 8) == 8 and u.taper_length(16, 4) == 8 and u.taper_length(10, 6) == 4 and u.taper_length(8, 8) == 0
    r = u.taper_ramp(16, 8)
    np.testing.assert_allclose(r, [np.sin(np.pi * (i + 0.5) / 16) ** 2 for i in range(8)], rtol=0, atol=1e-15)
    assert (r > 0).all() and (r < 1).all() and (np.diff(r) > 0).all()
    np.testing.assert_array_equal(u.axis_window(40, 8, 8, 8), np.ones(8))                      # L = 0
    np.testing.assert_array_equal(u.axis_window(40, 16, 8, 8, taper=False), np.ones(16))       # flat


@pytest.mark.parametrize("shape,dim,stride", SHAPES + [DIVISIBLE])
@pytest.mark.parametrize("cover", [False, True])
def test_window_sums(shape, dim, stride, cover):
    """Regular grid (s >= d/2 on every axis of these shapes): the windows sum to exactly 1 wherever the grid reaches; with the edge-flush
    windows the sum only grows.  A side on the volume's edge is not tapered; every weight is > 0."""
    from deep_prior_interpolation_amd import utils as u
    out_shape = u.reassembled_shape(shape, dim, stride, cover)
    tot = np.zeros(out_shape)
    for o in u.window_origins(shape, dim, stride, cover=cover):
        w = u.patch_window(out_shape, dim, stride, o)
        assert w.shape == dim and (w > 0).all() and w.max() <= 1.0
        for k, (n, d, a) in enumerate(zip(out_shape, dim, o)):
            ax = u.axis_window(n, d, stride[k], a)
            np.testing.assert_allclose(ax, _ref_window(n, d, stride[k], int(a), True), rtol=0, atol=1e-15)
            if a == 0:
                assert ax[0] == 1.0
            if a + d == n:
                assert ax[-1] == 1.0
        tot[tuple(slice(a, a + d) for a, d in zip(o, dim))] += w
    if cover:
        assert tot.min() >= 1 - 1e-12
    else:
        assert np.abs(tot - 1).max() <= 1e-12


# ---------------------------------------------------------------- re-assembly -----------------------------------------------------------
@pytest.mark.parametrize("shape,dim,stride", SHAPES)
@pytest.mark.parametrize("cover", [False, True])
@pytest.mark.parametrize("blend", ["flat", "taper"])
def test_identity(shape, dim, stride, cover, blend):
    from deep_prior_interpolation_amd import utils as u
    vol = np.random.RandomState(0).randn(*shape)
    org = u.window_origins(shape, dim, stride, cover=cover)
    pa = u.extract_at(vol, org, dim)
    out_shape = u.reassembled_shape(shape, dim, stride, cover)
    rec = u.reassemble(pa, org, out_shape, dim, stride, blend)
    assert rec.shape == (shape if cover else u.in_content_cropped_shape(shape, dim, stride)) and rec.dtype == np.float64
    assert np.abs(rec - vol[tuple(slice(0, n) for n in out_shape)]).max() <= 1e-12
    sd = u.reassemble(np.abs(pa), org, out_shape, dim, stride, blend, spread=True)            # sqrt(sum(w v^2) / sum(w)) of one field: |v|
    assert np.abs(sd - np.abs(vol)[tuple(slice(0, n) for n in out_shape)]).max() <= 1e-12


@pytest.mark.parametrize("shape,dim,stride", SHAPES + [((11, 7), (4, 3), (3, 2))])
def test_defaults_equal_patch_extractor_reconstruct_bit_for_bit(shape, dim, stride):
    from deep_prior_interpolation_amd import utils as u
    pe = u.PatchExtractor(dim=dim, stride=stride)
    pa = pe.extract(np.random.RandomState(1).randn(*shape))
    outs = (pa * 1.5 + np.random.RandomState(2).randn(*pa.shape)).astype(np.float32)          # patches that disagree in the overlaps
    old = pe.reconstruct(outs)
    new = u.reassemble(outs.reshape((-1,) + dim), u.window_origins(shape, dim, stride), u.reassembled_shape(shape, dim, stride), dim, stride, "flat")
    assert new.dtype == old.dtype and new.shape == old.shape
    np.testing.assert_array_equal(new, old)


@pytest.mark.parametrize("blend,spread", [("taper", False), ("taper", True), ("flat", True)])
def test_reassemble_against_the_restatement(blend, spread):
    from deep_prior_interpolation_amd import utils as u
    shape, dim, stride = SHAPES[0]
    org = u.window_origins(shape, dim, stride, cover=True)
    pa = np.random.RandomState(3).randn(len(org), *dim)
    got = u.reassemble(pa, org, shape, dim, stride, blend, spread=spread)
    ref = _ref_blend(pa, _ref_origins(shape, dim, stride, True), shape, dim, stride, blend == "taper", spread)
    np.testing.assert_allclose(got, ref, rtol=1e-12, atol=1e-12)


def test_seam_bound():
    """Windows along one axis, patch k constant at k, d = 16, s = 8 (L = 8): between the centres of two neighbours the blend is
    k + r[i], and |r[i+1] - r[i]| = |sin(pi (i + 1) / L) sin(pi / (2 L))| <= pi / (2 L); the box average jumps by 1/2 at every window edge."""
    from deep_prior_interpolation_amd import utils as u
    shape, dim, stride = (72, 4, 4), (16, 4, 4), (8, 4, 4)
    org = u.window_origins(shape, dim, stride)
    pa = np.stack([np.full(dim, float(k)) for k in range(len(org))])
    L = u.taper_length(16, 8)
    assert L == 8 and len(org) == 8
    tapered = u.reassemble(pa, org, shape, dim, stride, "taper")
    flat = u.reassemble(pa, org, shape, dim, stride, "flat")
    assert np.abs(np.diff(tapered, axis=0)).max() <= np.pi / (2 * L) + 1e-9
    assert np.abs(np.diff(flat, axis=0)).max() >= 0.5 - 1e-9
    assert np.abs(tapered[:, 0, 0] - _ref_blend(pa, [tuple(o) for o in org], shape, dim, stride, True)[:, 0, 0]).max() <= 1e-12


# ---------------------------------------------------------------- through files ---------------------------------------------------------
def _file_args(tmp_path, datadim, vol, patch_shape, patch_stride, extra=()):
    from deep_prior_interpolation_amd.parameter import parse_arguments
    d = tmp_path / "data"
    d.mkdir(exist_ok=True)
    np.save(d / "vol.npy", vol)
    np.save(d / "mask.npy", (np.random.RandomState(9).rand(*vol.shape) > 0.3).astype(np.float64))
    return parse_arguments(["--imgdir", str(d), "--imgname", "vol.npy", "--maskname", "mask.npy", "--datadim", datadim, "--gain", "40",
                            "--outdir", "run", "--patch_shape"] + [str(v) for v in patch_shape] + ["--patch_stride"] +
                           [str(v) for v in patch_stride] + list(extra))


@pytest.mark.parametrize("datadim,shape,dim,stride", [("2d", (23, 17), (8, 6), (4, 4)), ("3d", (13, 11, 14), (8, 6, 10), (4, 4, 6))])
def test_extract_and_reconstruct_patches_through_files(tmp_path, datadim, shape, dim, stride):
    from deep_prior_interpolation_amd import data as D
    vol = np.random.RandomState(4).randn(*shape)
    args = _file_args(tmp_path, datadim, vol, dim, stride, ["--reassembly", "cover", "--blend", "taper"])
    origins = _ref_origins(shape, dim, stride, True)
    ps = D.extract_patches(args)
    assert len(ps) == len(origins) and [p["name"] for p in ps] == [str(i).zfill(len(ps[0]["name"])) for i in range(len(ps))]
    for p, ref in zip(ps, _cut(vol, origins, dim)):
        np.testing.assert_array_equal(p["image"][..., 0], ref * 40.0)
    out = tmp_path / "results" / "run"
    out.mkdir(parents=True)
    rng = np.random.RandomState(5)
    outs, stds = [], []
    for i, p in enumerate(ps):
        o = (p["image"][..., 0] + rng.randn(*dim)).astype(np.float32)
        s = None if i == 1 else np.abs(rng.randn(*dim)).astype(np.float32)                     # patch 1: no spread recorded -> counts as 0
        outs.append(o)
        stds.append(np.zeros(dim, np.float32) if s is None else s)
        # a skipped patch is stored with a trailing singleton channel (patch 0 here)
        np.save(out / (p["name"] + "_run.npy"), {"output": o[..., None] if i == 0 else o, "posterior_std": s, "history": [], "elapsed": "0:00:01"})
    rec = D.reconstruct_patches(args, results_root=str(tmp_path / "results"))
    std = D.reconstruct_patches(args, results_root=str(tmp_path / "results"), field="posterior_std")
    assert rec.shape == shape and std.shape == shape and (std >= 0).all()
    np.testing.assert_allclose(rec, _ref_blend(outs, origins, shape, dim, stride, True) / 40.0, rtol=1e-6, atol=1e-7)      # float32 patches
    np.testing.assert_allclose(std, _ref_blend(stds, origins, shape, dim, stride, True, spread=True) / 40.0, rtol=1e-6, atol=1e-7)
    with pytest.raises(ValueError):
        D.reconstruct_patches(args, results_root=str(tmp_path / "results"), field="history")


def test_default_flags_through_files_are_the_reference_flow(tmp_path):
    from deep_prior_interpolation_amd import data as D, utils as u
    shape, dim, stride = (13, 11, 14), (8, 6, 10), (4, 4, 6)
    vol = np.random.RandomState(4).randn(*shape)
    args = _file_args(tmp_path, "3d", vol, dim, stride)
    ps = D.extract_patches(args)
    pe = u.PatchExtractor(dim=dim, stride=stride)
    pa = pe.extract(vol)
    assert len(ps) == int(np.prod(pa.shape[:3]))
    out = tmp_path / "results" / "run"
    out.mkdir(parents=True)
    for p in ps:
        np.save(out / (p["name"] + "_run.npy"), {"output": p["image"][..., 0], "history": [], "elapsed": "0:00:01"})
    rec = D.reconstruct_patches(args, results_root=str(tmp_path / "results"))
    np.testing.assert_array_equal(rec, pe.reconstruct(pa * 40.0) / 40.0)
    older = Namespace(**{k: v for k, v in vars(args).items() if k not in ("reassembly", "blend")})     # an args.txt from before the flags
    np.testing.assert_array_equal(D.reconstruct_patches(older, results_root=str(tmp_path / "results")), rec)
    assert len(D.extract_patches(older)) == len(ps)


def test_cover_refuses_a_short_axis_through_extract_patches(tmp_path):
    from deep_prior_interpolation_amd import data as D
    args = _file_args(tmp_path, "3d", np.zeros((13, 5, 14)), (8, 6, 10), (4, 4, 6), ["--reassembly", "cover"])
    with pytest.raises(ValueError, match="axis 1"):
        D.extract_patches(args)


# ---------------------------------------------------------------- parser / ABI ----------------------------------------------------------
def test_parser_defaults_and_choices(tmp_path):
    from deep_prior_interpolation_amd import utils as u
    from deep_prior_interpolation_amd.parameter import parse_arguments
    base = ["--imgdir", "x", "--datadim", "3d"]
    a = parse_arguments(base)
    assert a.reassembly == "crop" and a.blend == "flat"
    b = parse_arguments(base + ["--reassembly", "cover", "--blend", "taper"])
    assert b.reassembly == "cover" and b.blend == "taper"
    for bad in (["--reassembly", "pad"], ["--blend", "hann"]):
        with pytest.raises(SystemExit):
            parse_arguments(base + bad)
    u.write_args(str(tmp_path / "args.txt"), b)
    c = u.read_args(str(tmp_path / "args.txt"))
    assert c.reassembly == "cover" and c.blend == "taper"


def test_header_table_and_library_list_the_entry_points():
    from deep_prior_interpolation_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dpi_hip.h")).read(), flags=re.S)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, txt)
        assert name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["dpi_overlap_add_weighted"][1]) == 21 and len(_lib.SIGNATURES["dpi_overlap_finalize_weighted"][1]) == 9
    assert _lib.ABI_VERSION == 406              # unchanged: a stale library fails on the unresolved symbols instead
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    exported = set(re.findall(r"\bT (dpi_[a-z0-9_]+)", out))
    assert set(NEW) <= exported
    assert _lib.load().dpi_version() == 406


# ---------------------------------------------------------------- accumulators ----------------------------------------------------------
def _fake_optimise(i, patch):
    return patch * 1.5 + 0.01 * i


@pytest.mark.parametrize("taper", [False, True])
def test_host_blend_accumulator_with_std(taper):
    from deep_prior_interpolation_amd import parallel as P
    shape, dim, stride = SHAPES[0]
    origins = _ref_origins(shape, dim, stride, True)
    rng = np.random.RandomState(6)
    pa, sd = rng.randn(len(origins), *dim), np.abs(rng.randn(len(origins), *dim))
    sd[3] = 0.0
    acc = P.HostBlendAccumulator(shape, dim, stride, taper=taper, with_std=True)
    for i, o in enumerate(origins):
        acc.add(pa[i], o, std=None if i == 3 else sd[i])
    assert tuple(acc.tensor().shape) == (3,) + shape
    mean = acc.finalize(-40.0)
    np.testing.assert_allclose(mean, _ref_blend(pa, origins, shape, dim, stride, taper) / -40.0, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(acc.std_volume, _ref_blend(sd, origins, shape, dim, stride, taper, spread=True) / 40.0, rtol=1e-12, atol=1e-12)
    assert (acc.std_volume >= 0).all()


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _worker(rank, world, port, shape, dim, stride, gain, outdir):
    import torch.distributed as dist
    from deep_prior_interpolation_amd import parallel as P
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    vol = np.random.RandomState(0).randn(*shape)
    origins = _ref_origins(shape, dim, stride, True)
    rec, mine = P.run_patches(_cut(vol, origins, dim), origins, shape, dim, stride, gain, _fake_optimise, rank, world,
                              reassembly="cover", blend="taper")
    np.save(os.path.join(outdir, "rec_%d.npy" % rank), rec)
    np.save(os.path.join(outdir, "mine_%d.npy" % rank), np.array(mine))
    dist.destroy_process_group()


def test_two_rank_weighted_reassembly_equals_one_rank(tmp_path):
    import torch.multiprocessing as mp
    from deep_prior_interpolation_amd import parallel as P
    shape, dim, stride, gain = (21, 19, 25), (8, 6, 10), (4, 4, 6), 40.0
    mp.spawn(_worker, args=(2, _free_port(), shape, dim, stride, gain, str(tmp_path)), nprocs=2, join=True)
    vol = np.random.RandomState(0).randn(*shape)
    origins = _ref_origins(shape, dim, stride, True)
    patches = _cut(vol, origins, dim)
    one, mine = P.run_patches(patches, origins, shape, dim, stride, gain, _fake_optimise, reassembly="cover", blend="taper")
    assert one.shape == shape and mine == list(range(100))
    r0, r1 = np.load(tmp_path / "rec_0.npy"), np.load(tmp_path / "rec_1.npy")
    np.testing.assert_array_equal(r0, r1)
    np.testing.assert_allclose(r0, one, rtol=1e-12, atol=1e-12)
    ref = _ref_blend([_fake_optimise(i, p) for i, p in enumerate(patches)], origins, shape, dim, stride, True) / gain
    np.testing.assert_allclose(one, ref, rtol=1e-12, atol=1e-12)
    m0, m1 = list(np.load(tmp_path / "mine_0.npy")), list(np.load(tmp_path / "mine_1.npy"))
    assert sorted(m0 + m1) == list(range(100)) and not set(m0) & set(m1)
