"""CPU-side tests: the drop-in host surface against the golden vectors recorded from the reference, the C-ABI
library's exported symbols, and the 'no CPU fallback' contract.  No GPU needed."""
import json
import os
import re
import subprocess
from argparse import Namespace

import numpy as np
import pytest
import torch

from conftest import ROOT, jstr

from deep_prior_interpolation_amd import utils as u
from deep_prior_interpolation_amd import data as D
from deep_prior_interpolation_amd.architectures import get_net
from deep_prior_interpolation_amd.parameter import parse_arguments, net_args_are_same


# ---------------------------------------------------------------- C ABI -------------------------------------------
def _header_symbols():
    txt = open(os.path.join(ROOT, "include", "dpi_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(dpi_[a-z0-9_]+)\s*\(", txt)))


def test_library_exports_every_declared_symbol():
    from deep_prior_interpolation_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    syms = _header_symbols()
    assert len(syms) >= 25
    assert sorted(_lib.SIGNATURES.keys()) == syms            # the ctypes table covers the header, nothing more
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    exported = set(re.findall(r"\bT (dpi_[a-z0-9_]+)", out))
    assert set(syms) <= exported, set(syms) - exported
    lib = _lib.load()                                         # loads without a GPU; no compute call made
    assert lib.dpi_version() >= 301
    assert lib.dpi_stat_blocks(4, 1 << 20) > 0


def test_no_cpu_fallback():
    from deep_prior_interpolation_amd import ops, _lib
    x = torch.randn(1, 2, 4, 4, 4)
    w = torch.randn(3, 2, 3, 3, 3)
    with pytest.raises(_lib.DpiError):
        ops.conv(x, w, None, 1)
    with pytest.raises(_lib.DpiError):
        ops.batch_norm(x, torch.ones(2), torch.zeros(2))
    a = parse_arguments(["--imgdir", "x", "--datadim", "3d", "--filters", "4", "8", "--skip", "4", "--inputdepth", "2"])
    with pytest.raises(_lib.DpiError):
        get_net(a, 1)(x)


# ---------------------------------------------------------------- networks ----------------------------------------
def _args(argv, net=None):
    a = parse_arguments(argv)
    if net:
        a.net = net
    return a


STRUCT = {
    "mulresunet3d_default": (["--imgdir", "x", "--datadim", "3d"], 1, None),
    "mulresunet2d_default": (["--imgdir", "x", "--datadim", "2d"], 1, None),
    "mulresunet25d_c8": (["--imgdir", "x", "--datadim", "2.5d", "--imgchannel", "8"], 8, None),
    "skip3d_a12": (["--imgdir", "x", "--datadim", "3d", "--filters", "16", "32", "64", "128", "128", "--skip", "4", "4", "4", "4", "4"], 1, "skip"),
    "mulresunet3d_noskip": (["--imgdir", "x", "--datadim", "3d", "--filters", "4", "8", "16", "--skip", "0", "4"], 1, None),
}


@pytest.mark.parametrize("tag", list(STRUCT))
def test_state_dict_keys_and_param_counts(golden, tag):
    argv, outch, net = STRUCT[tag]
    n = get_net(_args(argv, net), outch)
    keys = [[k, list(v.shape)] for k, v in n.state_dict().items()]
    assert keys == jstr(golden("structure")[tag]["keys"])           # same names, shapes AND order
    assert sum(p.numel() for p in n.parameters()) == int(golden("structure")[tag]["num_params"])


def test_param_counts_survey():
    assert sum(p.numel() for p in get_net(_args(STRUCT["mulresunet3d_default"][0]), 1).parameters()) == 5923614
    assert sum(p.numel() for p in get_net(_args(STRUCT["mulresunet2d_default"][0]), 1).parameters()) == 2186704


@pytest.mark.parametrize("name", ["net_mulresunet3d_tiny_trilinear_mae", "net_skip3d_tiny", "net_mulresunet2d_tiny",
                                  "net_mulresunet25d_tiny", "net_mulresunet3d_tiny_odd"])
def test_same_seed_init_is_bit_identical(golden, name):
    """set_seed(0) + get_net + init_weights reproduces the reference's initial state_dict exactly
    (same construction order => same RNG consumption)."""
    g = golden(name)
    ns = Namespace(**jstr(g["args"]))
    u.set_seed(0)
    oc = g["image"].shape[-1] if ns.imgchannel is None else ns.imgchannel
    net = get_net(ns, oc)
    u.init_weights(net, ns.inittype, ns.initgain)
    sd = net.state_dict()
    assert list(sd.keys()) == list(g["init_state"].keys())
    for k, v in g["init_state"].items():
        assert np.array_equal(sd[k].numpy(), v), k


def test_out_of_scope_nets_are_loud():
    for net in ("attmultiunet", "part"):
        with pytest.raises(NotImplementedError):
            get_net(_args(["--imgdir", "x", "--datadim", "2d", "--net", net]), 1)


# ---------------------------------------------------------------- parameter ---------------------------------------
def test_parameter_defaults_and_postprocessing():
    a = parse_arguments(["--imgdir", "d"])
    assert (a.gain, a.datadim, a.net, a.filters, a.skip, a.inputdepth) == (2e3, "2d", "multiunet", [16, 32, 64, 128, 256], [16, 32, 64, 128], 64)
    assert (a.upsample, a.inittype, a.initgain, a.loss, a.epochs, a.lr) == ("nearest", "xavier", 0.02, "mae", 2001, 1e-3)
    assert a.param_noise is True and a.reg_noise_std == 0.03 and a.noise_std == 0.1 and a.noise_dist == "n"
    assert a.patch_shape == [-1, -1] and a.patch_stride == [-1, -1] and a.earlystop_patience == 2001 and a.netdir == []
    assert (a.lr_factor, a.lr_thresh, a.lr_patience, a.earlystop_min_delta, a.lowpass_ntaps) == (0.9, 1e-5, 100, 1.0, 7)
    b = parse_arguments(["--imgdir", "d", "--datadim", "3d", "--upsample", "linear", "-e", "10", "--param_noise"])
    assert b.upsample == "trilinear" and b.patch_shape == [-1, -1, -1] and b.epochs == 10 and b.param_noise is False
    c = parse_arguments(["--imgdir", "d", "--datadim", "2.5d", "--upsample", "linear", "--iter", "7"])
    assert c.upsample == "bilinear" and c.epochs == 7
    assert parse_arguments(["--imgdir", "d", "--net", "skip"]).net == "skip"


def test_parameter_matches_reference_args(golden):
    """Every key the reference's Namespace has (recorded in the fixtures) exists here with the same value."""
    g = golden("net_mulresunet3d_tiny_trilinear_mae")
    ref = jstr(g["args"])
    mine = vars(parse_arguments(jstr(g["argv"]) + ["--epochs", str(ref["epochs"])]))
    for k, v in ref.items():
        if k in ("param_noise",):       # the fixture run sets param_noise=False programmatically
            continue
        assert mine[k] == v, k
    assert net_args_are_same(Namespace(**ref), Namespace(**mine))
    other = dict(mine)
    other["inputdepth"] = 3
    assert not net_args_are_same(Namespace(**ref), Namespace(**other))


# ---------------------------------------------------------------- data / patches ----------------------------------
def test_patch_extractor_golden(golden):
    for tag, c in golden("host")["pe"].items():
        dim, stride = tuple(int(v) for v in c["dim"]), tuple(int(v) for v in c["stride"])
        pe = u.PatchExtractor(dim=dim, stride=stride)
        pa = pe.extract(c["vol"])
        np.testing.assert_array_equal(pa, c["patches"])
        assert pe.in_content_cropped_shape == tuple(c["cropped_shape"])
        assert u.count_patches(c["vol"].shape, dim, stride) == int(c["count"])
        assert u.patch_array_shape(c["vol"].shape, dim, stride) == tuple(c["array_shape"])
        np.testing.assert_allclose(pe.reconstruct(c["patches2"]), c["recon2"], rtol=1e-14, atol=1e-14)
        org = u.window_origins(c["vol"].shape, dim, stride)
        flat = pa.reshape((-1,) + dim)
        for p, o in zip(flat, org):        # plain definition: window w starts at w*stride, C order
            np.testing.assert_array_equal(p, c["vol"][tuple(slice(a, a + d) for a, d in zip(o, dim))])


def test_extract_and_reconstruct_patches_golden(golden, tmp_path):
    g = golden("host")["data"]
    np.save(tmp_path / "orig.npy", g["vol"])
    np.save(tmp_path / "mask.npy", g["mask"])
    nanvol = g["vol"].copy()
    nanvol[g["mask"] == 0] = np.nan
    np.save(tmp_path / "nan.npy", nanvol)
    for tag in ("3d_bin", "3d_nan", "3d_full", "25d_xy", "25d_tx", "25d_ty"):
        c = g[tag]
        args = parse_arguments(["--imgdir", str(tmp_path), "--imgname", "orig.npy", "--outdir", "r_" + tag] + jstr(c["argv"]))
        ps = D.extract_patches(args)
        assert [p["name"] for p in ps] == jstr(c["names"])
        np.testing.assert_array_equal(np.stack([p["image"] for p in ps]), c["images"])
        np.testing.assert_array_equal(np.stack([p["mask"] for p in ps]), c["masks"])
        if "recon" in c:
            rdir = tmp_path / "results" / ("r_" + tag)
            os.makedirs(rdir)
            # The reference reads the result files in unsorted glob (= directory) order (data.py:99, SURVEY
            # App. B.7); the fixture records that order.  We sort by name on purpose, so hand our reader the
            # sequence the reference actually consumed: the k-th file of ITS order gets the k-th sorted name.
            seq = [c["outputs"][int(n)] for n in jstr(c["glob_order"])]
            for p, o in zip(ps, seq):
                np.save(rdir / (p["name"] + "_run.npy"), {"output": o, "elapsed": "0h:0m:1s", "history": None, "device": "x"})
            rec = D.reconstruct_patches(args, results_root=str(tmp_path / "results"))
            np.testing.assert_allclose(rec, c["recon"], rtol=1e-13, atol=1e-13)


def test_masks_metrics_generic_golden(golden):
    g = golden("host")
    np.testing.assert_array_equal(u.bool2bin(g["bool2bin"]["in"]), g["bool2bin"]["out"])
    np.random.seed(0)
    np.testing.assert_array_equal(u.build_mask(np.ones((6, 5, 4)), 0.5), g["build_mask"]["rand3d"])
    np.random.seed(0)
    np.testing.assert_array_equal(u.build_mask(np.ones((6, 10)), 0.3), g["build_mask"]["rand2d"])
    np.testing.assert_array_equal(u.build_mask(np.ones((4, 12)), 0.66, regular=True), g["build_mask"]["reg_hi"])
    np.testing.assert_array_equal(u.build_mask(np.ones((4, 12)), 0.25, regular=True), g["build_mask"]["reg_lo"])
    np.random.seed(1)
    np.testing.assert_array_equal(u.add_rand_mask(g["data"]["mask"], 0.3), g["add_rand_mask"]["out3d"])
    m = g["metrics"]
    a, b = torch.from_numpy(m["out"]), torch.from_numpy(m["tgt"])
    assert abs(u.snr(a, b).item() - float(m["snr"])) < 1e-5 and abs(u.pcorr(a, b).item() - float(m["pcorr"])) < 1e-6
    assert abs(u.snr(m["out"].astype(np.float64), m["tgt"].astype(np.float64)) - float(m["snr_np"])) < 1e-10
    H = u.History(3000)
    H.append((0.0123, 4.5, 0.87))
    H.lr.append(1e-3)
    assert H.log_message(0) == str(g["history"]["msg"]) and H.zfill == int(g["history"]["zfill"]) and len(H) == 1
    gg = g["generic"]
    assert [u.ten_digit(n) for n in (1, 9, 10, 343, 2001, 99999)] == list(gg["ten_digit"])
    assert [u.sec2time(s) for s in (0, 59.9, 61, 3600, 6739.4)] == jstr(gg["sec2time"])
    assert [u.time2sec(s) for s in ("0h:0m:59s", "1h:52m:19s")] == list(gg["time2sec"])
    assert [u.nextpow2(n) for n in (1, 2, 3, 64, 65, 1000)] == list(gg["nextpow2"])
    st = u.EarlyStopping(patience=40, min_delta=1.0, percentage=True)
    got = [bool(st.step(l)) for l in g["earlystop"]["losses"]]
    first = int(np.argmax(g["earlystop"]["stop"]))
    assert got[:first + 1] == list(g["earlystop"]["stop"][:first + 1])
    assert u.EarlyStopping(patience=3).step(float("nan")) is False      # first value only sets `best`
    es = u.EarlyStopping(patience=3)
    es.step(1.0)
    assert es.step(float("nan")) is True                                  # NaN stops immediately (utils/torch.py:247)


def test_args_json_roundtrip(tmp_path):
    a = parse_arguments(["--imgdir", "d", "--datadim", "3d", "--patch_shape", "64", "64", "64"])
    u.write_args(tmp_path / "args.txt", a)
    assert vars(u.read_args(tmp_path / "args.txt")) == vars(a)
    assert json.load(open(tmp_path / "args.txt"))["patch_shape"] == [64, 64, 64]


def test_lines_known_answer(golden):
    ln = golden("host")["lines"]
    img = ln["original"].astype(np.float64)
    std = torch.std(torch.from_numpy((img * ln["mask"]).astype(np.float32))).item()
    assert "%.2e" % std == "3.62e-02"        # proof_of_concept_2D.ipynb:308


def test_unet_structure(golden):
    """--net unet builds the plain UNet with the reference class's state_dict keys, shapes and order."""
    from deep_prior_interpolation_amd.architectures import UNet
    for mode in ("deconv", "bilinear", "nearest"):
        n = UNet(6, 2, [2, 4, 8, 16, 32], upsample_mode=mode, act_fun="LeakyReLU")
        assert [[k, list(v.shape)] for k, v in n.state_dict().items()] == jstr(golden("unet")[mode]["keys"])
    a = parse_arguments(["--imgdir", "x", "--datadim", "2d", "--net", "unet", "--upsample", "linear"])
    assert type(get_net(a, 1)).__name__ == "UNet"
    assert sum(p.numel() for p in UNet(64, 1).parameters()) == 2472129     # class defaults ('deconv'), 64-ch input


def test_hyperbolic3d_stand_in_statistics():
    """the stand-in for the absent datasets/hyperbolic3d must look like the notebook's data to the optimiser:
    `std(gain * img * mask)` at gain 40 with 66 % of the traces missing inside the notebook's printed 3.94 .. 5.16
    (proof_of_concept_3D.ipynb:355,362), no large exactly-zero part (the round-1/2 cube was 72-90 % zeros, std 1.5, and kept the MAE
    loss on the all-zero plateau for 1400-2700 iterations; the notebook's curve leaves 0 dB at ~220), events filling the lower part
    of the patch as in the notebook's figures, and the same picture at every size used by the parity runs."""
    for shape in [(256, 128, 128), (128, 64, 64), (48, 32, 32)]:
        for seed in (0, 1):
            vol = u.hyperbolic_volume(shape, seed=seed)
            mask = u.random_trace_mask(shape, 0.66, seed=1)
            assert vol.dtype == np.float32 and vol.shape == shape and np.isfinite(vol).all()
            std = u.coarse_std(vol, mask, gain=40.0)
            assert 3.9 <= std <= 5.2, (shape, seed, std)
            zero_frac = float((np.abs(vol) < 1e-3 * np.abs(vol).max()).mean())
            assert zero_frac < 0.06, (shape, seed, zero_frac)
            nt = shape[0]
            top, bottom = vol[: nt // 5], vol[nt // 2:]
            assert bottom.std() > 5.0 * top.std()          # events live below the first hyperbola; above it only the weak background
    # deterministic in (shape, seed); the sparse round-1/2 cube is still available for the fixtures recorded on it
    assert np.array_equal(u.hyperbolic_volume((48, 32, 32), seed=3), u.hyperbolic_volume((48, 32, 32), seed=3))
    old = u.sparse_hyperbolic_volume((256, 128, 128), seed=0)
    assert u.coarse_std(old, u.random_trace_mask((256, 128, 128), 0.66, seed=1)) < 2.5


def test_skip2d_structure(golden):
    """2-D `Skip` (reference architectures/skip.py:5-48): state_dict keys, order and shapes equal the reference's, so checkpoints of
    either implementation load in the other (the class is unreachable through `get_net` on both sides)."""
    from deep_prior_interpolation_amd.architectures.skip import Skip
    for mode in ("nearest", "bilinear"):
        g = golden("skip2d")[mode]
        m = Skip(num_input_channels=5, num_output_channels=2, num_channels_down=[4, 6], num_channels_up=[4, 6], num_channels_skip=[2, 3],
                 upsample_mode=mode, act_fun="LeakyReLU")
        assert [[k, list(v.shape)] for k, v in m.state_dict().items()] == jstr(g["keys"])
    with pytest.raises(NotImplementedError):
        Skip(pad="reflection")


def test_get_net_reaches_the_2d_skip_net_for_configs3(golden):
    """BASELINE configs[3] ("--datadim 2.5d skip-net"): `--net skip` with a 2-D / 2.5-D datadim builds the 2-D `Skip` hourglass (upstream's
    get_net falls through to MulResUnet there, architectures/__init__.py:41-53; documented deviation).  Keys, order and shapes equal the
    state the REFERENCE's Skip class had inside the reference's Interpolator (oracle/make_golden.py gen_lines_skip)."""
    from deep_prior_interpolation_amd.architectures import Skip, get_net
    from deep_prior_interpolation_amd.parameter import parse_arguments
    for name, dd in (("net_lines25d_skip_tiny", ["--datadim", "2.5d", "--imgchannel", "4", "--slice", "tx"]), ("net_lines2d_skip_tiny", ["--datadim", "2d"])):
        g = golden(name)
        a = parse_arguments(["--imgdir", "x", "--net", "skip", "--filters", "4", "8", "16", "--skip", "2", "2", "2", "--inputdepth", "8",
                             "--upsample", "linear"] + dd)
        ref = jstr(g["args"])
        assert ref["net"] == "skip" and ref["datadim"] == a.datadim and ref["upsample"] == a.upsample
        net = get_net(a, 4 if a.datadim == "2.5d" else 1)
        assert isinstance(net, Skip)
        assert [(k, tuple(v.shape)) for k, v in net.state_dict().items()] == [(k, tuple(np.asarray(v).shape)) for k, v in g["init_state"].items()]
        assert sum(p.numel() for p in net.parameters()) == int(g["num_params"])
    a = parse_arguments(["--imgdir", "x", "--datadim", "2d", "--net", "skip"])          # default --skip has one width less than --filters
    with pytest.raises(ValueError):
        get_net(a, 1)
    assert not isinstance(get_net(parse_arguments(["--imgdir", "x", "--datadim", "2d"]), 1), Skip)          # the default stays MulResUnet


def test_branch_stream_host_logic_knows_the_deep_branch_width(monkeypatch):
    """Round 5: the ResPath half of a level join is started on the branch stream BEFORE the deeper U has run (ops.skip_begin), so the concat
    buffer must be sized from the module tree: `_deep_channels` = the channels the deeper branch hands to its Upsample = what the decoder
    block behind the join expects beyond the skip width (reference mulresunet.py:227-243).  Also: outside an Interpolator iteration the
    schedule helpers are inert (a bare loss.backward() joins per node, no branch stream)."""
    from deep_prior_interpolation_amd import ops
    from deep_prior_interpolation_amd.architectures import mulresunet as M
    net = get_net(parse_arguments(["--imgdir", "x", "--datadim", "3d", "--net", "multiunet", "--inputdepth", "64"]), 1)
    seen = 0

    def walk(seq):
        nonlocal seen
        mods = list(seq._modules.values())
        for a, b in zip(mods, mods[1:]):
            if isinstance(a, M.SkipConcat) and isinstance(b, M.MultiResBlock):
                skip, deeper = list(a._modules.values())
                skip_ch = skip[0].conv3x3._parts()[0].weight.shape[0]
                need = b.shortcut._parts()[0].weight.shape[1] - skip_ch
                assert M._deep_channels(list(deeper._modules.values())[:-1]) == need
                seen += 1
                for m in deeper._modules.values():
                    if isinstance(m, torch.nn.Sequential) and not isinstance(m, (M.MultiResBlock,)):
                        walk(m)
    walk(net)
    assert seen == 4                                            # four level joins in the default five-scale net
    # the switch as a fresh process has it: a big-patch GPU test earlier in the same session may have left it on (ops.set_weight_grad_overlap)
    monkeypatch.setattr(ops.sched, "overlap", os.environ.get("DPI_OVERLAP_WGRAD", "0") == "1")
    assert ops.sched.join_at == "step" and not ops.sched.in_iteration
    assert not ops.sched.branch_on()                                  # no iteration, no weight-gradient overlap: the serial schedule
    ops.begin_iteration()
    try:
        assert ops.sched.in_iteration and not ops.sched.branch_on()     # still off: the overlap is only switched on for >= 2^20-voxel patches on a GPU
    finally:
        ops.finish_backward()
    assert not ops.sched.in_iteration and not ops.sched.side_keep


def test_polyphase_identity_behind_design_section_7():
    """DESIGN §7 item 4 (next structural step, not on the product path): trilinear x2 up-sampling followed by a 3x3x3 convolution is a set of
    coarse-grid 3x3x3 stencils with folded weights, 8 parity classes x 27 border classes — checked against torch's interpolate + conv3d in
    float64 (reference architectures/base.py: nn.Upsample(scale_factor=2, mode='trilinear') feeding the decoder's first convolution)."""
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location("polyphase_check", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "polyphase_check.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.main()


# ---------------------------------------------------------------- parity mode: the reference's own input stream -----
def _parity_interpolator(seed, vol, mask, argv_extra=(), param_noise=False, device="cpu"):
    """An Interpolator prepared exactly as oracle/make_snr_spread.py prepares the reference's (u.set_seed -> Interpolator -> load_data ->
    build_model -> build_input), with --noise_source torch_cpu.  device="cpu" only carries the HOST side (weights, z, the perturbed input):
    the forward needs the HIP library."""
    from deep_prior_interpolation_amd.main import Interpolator
    args = parse_arguments(["--imgdir", "synthetic", "--datadim", "3d", "--net", "multiunet", "--inputdepth", "64", "--upsample", "linear",
                            "--loss", "mae", "--lr", "1e-3", "--gain", "40", "--reg_noise_std", "0.03", "--noise_std", "0.1",
                            "--noise_source", "torch_cpu"] + list(argv_extra))
    args.param_noise = param_noise
    u.set_seed(seed)
    T = Interpolator(args, "/tmp", device=torch.device(device), seed=seed)
    T.load_data({"image": (vol.astype(np.float64) * args.gain)[..., None], "mask": mask.astype(np.float64)[..., None], "name": "0"})
    T.build_model()
    T.build_input()
    return T, args


def test_torch_cpu_noise_source_reproduces_the_reference_stream():
    """--noise_source torch_cpu must hand the network the reference's own iteration-0 input: same seed -> bit-identical initial weights
    (test_same_seed_init_is_bit_identical), the same z and the same first perturbation, in the order of reference main.py:59-64,148-150.
    Checked WITHOUT a GPU: the oracle's forward on that input against the iteration-0 loss / SNR / PCORR the reference itself recorded
    (tests/golden/snr_spread.npz, oracle/make_snr_spread.py: 48x32x32, default 5.9 M-parameter net, seeds 0 and 1).  A wrong draw order
    or a different z gives a different loss in the third digit (the seeds differ from each other by 3e-3)."""
    from oracle import dpi_oracle as O
    z = np.load(os.path.join(ROOT, "tests", "golden", "snr_spread.npz"))
    assert str(z["torch"]) == torch.__version__, "the CPU generator's stream is pinned to the torch build that recorded the fixture"
    vol, mask = z["volume"], z["mask"].astype(np.float32)
    for k in (0, 1):
        seed = int(z["seed"][k])
        T, a = _parity_interpolator(seed, vol, mask)
        inp = T.perturbed_input()
        assert inp.shape == (1, 64) + vol.shape and not torch.equal(inp, T.input_)
        S = O.NetState({n: v.detach().clone() for n, v in T.net.state_dict().items()})
        with torch.no_grad():
            out = O.net_forward(S, inp, {"ndim": 3, "filters": a.filters, "skip": a.skip, "upsample": "trilinear"})
        loss = O.masked_loss(out, T.img_, T.mask_, "mae").item()
        assert abs(loss - float(z["loss"][k, 0])) <= 1e-5 * abs(loss), (seed, loss, float(z["loss"][k, 0]))
        assert abs(O.snr(out, T.img_).item() - float(z["snr"][k, 0])) < 1e-3
        assert abs(O.pcorr(out, T.img_).item() - float(z["pcorr"][k, 0])) < 1e-4


def test_torch_cpu_noise_source_draws_the_param_noise_the_reference_discards():
    """With --param_noise (the CLI default) the reference draws one normal_() per 4-D / 5-D parameter before the input perturbation and throws
    the result away (main.py:143-145): parity mode must move the generator by the same amount — and not touch the weights."""
    vol = np.zeros((8, 8, 8), np.float32)
    vol[2:5] = 1.0
    mask = np.ones_like(vol)
    small = ["--filters", "4", "8", "--skip", "4", "--inputdepth", "2"]
    T, _ = _parity_interpolator(3, vol, mask, small, param_noise=True)
    w0 = {n: v.clone() for n, v in T.net.state_dict().items()}
    state = torch.get_rng_state()
    got = T.perturbed_input()
    torch.set_rng_state(state)
    for p in T.net.parameters():
        if p.ndim in (4, 5):
            p.detach().clone().normal_()
    want = T._z_cpu.clone()
    want += 0.03 * want.clone().normal_()
    assert torch.equal(got, want)
    assert all(torch.equal(v, w0[n]) for n, v in T.net.state_dict().items())
    T2, _ = _parity_interpolator(3, vol, mask, small, param_noise=False)
    assert torch.equal(T2._z_cpu, T._z_cpu) and not torch.equal(T2.perturbed_input(), got)
