"""Flows around the hot path on the GPU: checkpoint / transfer learning (--savemodel, --netdir, --start_from_prev),
the anti-aliasing add-on in the loop (row 3, BASELINE configs[3]) and the POCS-regularised loop (row 4, reference main_pocs.py)."""
import os
import shutil

import numpy as np
import pytest
import torch

from oracle import dpi_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def rel(a, b):
    a = a.detach().cpu().numpy().astype(np.float64) if torch.is_tensor(a) else np.asarray(a, np.float64)
    b = b.detach().cpu().numpy().astype(np.float64) if torch.is_tensor(b) else np.asarray(b, np.float64)
    return float(np.linalg.norm((a - b).ravel()) / (np.linalg.norm(b.ravel()) + 1e-30))


# ---------------------------------------------------------------------------------------------------------------------------
def test_reference_checkpoint_loads_through_build_model(golden, tmp_path, monkeypatch):
    """A state_dict + args.txt written by the REFERENCE (main.py:238-240, utils/generic.py:46) goes through
    Interpolator.build_model(netpath=...) (main.py:101-110: read_args -> net_args_are_same -> get_net -> load_state_dict) and
    the HIP forward reproduces the reference's output for the recorded input."""
    from deep_prior_interpolation_amd.main import Interpolator
    from deep_prior_interpolation_amd.parameter import parse_arguments
    io = golden("ckpt_ref_io")
    monkeypatch.chdir(tmp_path)
    os.makedirs("results")
    shutil.copytree(os.path.join(GOLD, "ckpt_ref"), "results/ckpt_ref")
    argv = ["--imgdir", "x", "--datadim", "3d", "--filters", "4", "8", "16", "--skip", "4", "8", "--inputdepth", "8", "--upsample", "linear",
            "--net", "load", "--netdir", "ckpt_ref/0_model.pth", "--epochs", "2", "--gpu", "0"]
    a = parse_arguments(argv)
    T = Interpolator(a, str(tmp_path))
    rng = np.random.RandomState(0)
    T.load_data({"image": rng.randn(16, 16, 16, 1), "mask": np.ones((16, 16, 16, 1)), "name": "0"})
    T.build_model(netpath=a.netdir[0])
    sd = T.net.state_dict()
    assert list(sd.keys()) == list(io["state"].keys())
    for k, v in io["state"].items():
        np.testing.assert_array_equal(sd[k].cpu().numpy(), v, err_msg=k)       # incl. running stats and num_batches_tracked
    y = T.net(torch.from_numpy(io["x"]).to(DEV))
    assert rel(y, io["y"]) < 2e-5
    # incompatible run settings are refused (parameter.py:133-173): a different --inputdepth must trip net_args_are_same
    b = parse_arguments([x if x != "8" or argv[i - 1] != "--inputdepth" else "6" for i, x in enumerate(argv)])
    T2 = Interpolator(b, str(tmp_path))
    T2.load_data({"image": rng.randn(16, 16, 16, 1), "mask": np.ones((16, 16, 16, 1)), "name": "0"})
    with pytest.raises(AssertionError):
        T2.build_model(netpath=b.netdir[0])


def _survey(tmp_path, shape=(32, 16, 16)):
    from deep_prior_interpolation_amd import utils as u
    d = tmp_path / "data"
    d.mkdir(exist_ok=True)
    np.save(d / "original.npy", u.sparse_hyperbolic_volume(shape, seed=5).astype(np.float32))
    np.save(d / "mask.npy", u.random_trace_mask(shape, 0.5, seed=6).astype(np.float32))
    return ["--imgdir", str(d), "--imgname", "original.npy", "--maskname", "mask.npy", "--datadim", "3d", "--patch_shape", "16", "16", "16",
            "--patch_stride", "16", "16", "16", "--filters", "4", "8", "--skip", "4", "--inputdepth", "8", "--upsample", "linear", "--gain", "2", "--gpu", "0"]


def test_savemodel_then_netdir_round_trip(tmp_path, monkeypatch):
    """--savemodel writes <patch>_model.pth per patch (main.py:238-240); a second run with --net load --netdir <one path per patch>
    starts every patch from those weights (main.py:105-110, 286-290): its iteration-0 loss equals the loss the saved weights
    give, not the loss of a fresh initialisation."""
    from deep_prior_interpolation_amd import main as dmain
    common = _survey(tmp_path)
    monkeypatch.chdir(tmp_path)
    dmain.main(common + ["--epochs", "20", "--outdir", "first", "--savemodel"])
    names = sorted(f for f in os.listdir("results/first") if f.endswith("_model.pth"))
    assert names == ["0_model.pth", "1_model.pth"]
    first = [np.load("results/first/%d_run.npy" % i, allow_pickle=True).item() for i in range(2)]
    dmain.main(common + ["--epochs", "3", "--outdir", "second", "--net", "load", "--netdir", "first/0_model.pth", "first/1_model.pth",
                         "--savemodel"])
    second = [np.load("results/second/%d_run.npy" % i, allow_pickle=True).item() for i in range(2)]
    for i in range(2):
        l_first, l_second = first[i]["history"].loss, second[i]["history"].loss
        print("patch %d: first run", i, ["%.4f" % v for v in l_first], "second run (loaded)", ["%.4f" % v for v in l_second])
        # continues from the optimised weights, not from scratch: the first loss sits at the END of the first run's curve
        assert l_second[0] < 0.9 * l_first[0]
        assert abs(l_second[0] - l_first[-1]) < abs(l_second[0] - l_first[0])
    # the checkpoint written by the second run loads into a fresh net with identical keys
    sd = torch.load("results/second/0_model.pth", map_location="cpu")
    ref = torch.load("results/first/0_model.pth", map_location="cpu")
    assert list(sd.keys()) == list(ref.keys()) and all(sd[k].shape == ref[k].shape for k in sd)
    assert int(sd[[k for k in sd if k.endswith("num_batches_tracked")][0]]) == 20 + 3


def test_start_from_prev_keeps_weights_across_patches(tmp_path, monkeypatch):
    """--start_from_prev (main.py:286): the model is built once; patch 1 starts from patch 0's optimised weights."""
    from deep_prior_interpolation_amd import main as dmain
    common = _survey(tmp_path)
    monkeypatch.chdir(tmp_path)
    calls = []
    orig = dmain.Interpolator.build_model
    monkeypatch.setattr(dmain.Interpolator, "build_model", lambda self, netpath=None: (calls.append(1), orig(self, netpath))[1])
    dmain.main(common + ["--epochs", "8", "--outdir", "fresh", "--savemodel"])
    n_fresh = len(calls)
    dmain.main(common + ["--epochs", "8", "--outdir", "chain", "--start_from_prev", "--savemodel"])
    assert n_fresh == 2 and len(calls) - n_fresh == 1

    def nbt(run):        # BatchNorm step counter of patch 1's saved model: 8 for a fresh net, 16 when patch 0's net was kept
        sd = torch.load("results/%s/1_model.pth" % run, map_location="cpu")
        return int(sd[[k for k in sd if k.endswith("num_batches_tracked")][0]])
    assert nbt("fresh") == 8 and nbt("chain") == 16
    fresh = np.load("results/fresh/1_run.npy", allow_pickle=True).item()["history"].loss
    chain = np.load("results/chain/1_run.npy", allow_pickle=True).item()["history"].loss
    assert abs(chain[0] - fresh[0]) > 1e-6 * fresh[0]            # patch 1 did not start from a fresh initialisation


# ---------------------------------------------------------------------------------------------------------------------------
def _lines_interpolator(golden, extra, epochs, cls=None):
    from deep_prior_interpolation_amd.main import Interpolator
    from deep_prior_interpolation_amd.parameter import parse_arguments
    from deep_prior_interpolation_amd import utils as u
    ln = golden("host")["lines"]
    a = parse_arguments(["--imgdir", "x", "--datadim", "2d", "--filters", "4", "8", "16", "--skip", "4", "8", "--inputdepth", "8",
                         "--upsample", "linear", "--gain", "1", "--epochs", str(epochs), "--gpu", "0"] + extra)
    u.set_seed(0)
    T = (cls or Interpolator)(a, "/tmp")
    T.load_data({"image": ln["original"].astype(np.float64), "mask": ln["mask"].astype(np.float64), "name": "0"})
    T.build_model()
    T.build_input()
    T.build_regularizer()
    return T, a


def test_antialiasing_addon_in_the_loop_on_lines(golden):
    """configs[3]: the 2-D section datasets/lines with the directional-Laplacian regulariser.  Iteration 0: total = main +
    aa_weight * mean|Hale2D(dips) out| with the regulariser value checked against the numpy oracle on the HIP output; then a
    short run must decrease the total and keep the split history (HistoryReg)."""
    from deep_prior_interpolation_amd import utils as u
    T, a = _lines_interpolator(golden, ["--aa_weight", "0.5", "--aa_smooth", "2.0"], 1)
    assert isinstance(T.history, u.HistoryReg) and not T.graph_capable()
    T.optimize(verbose=False)
    out0 = np.asarray(T.out_best, dtype=np.float64)[..., 0][None, None]                 # (H,W,1) -> BCHW
    dips = T._aa_op.dips.cpu().numpy().astype(np.float64)
    reg_ref = np.abs(O.hale2d_np(out0, dips)).mean()
    assert abs(T.history.reg[0] - reg_ref) < 1e-4 * reg_ref + 1e-9
    assert abs(T.history.loss[0] - (T.history.df[0] + 0.5 * T.history.reg[0])) < 1e-6 * abs(T.history.loss[0])
    # dips estimated from the decimated section agree with the oracle's estimate on the same input
    # (fp32 like the reference; the angle is ill-conditioned where the tensor is nearly diagonal — see tests/test_gpu_operators.py)
    phi_ref, an_ref = O.structure_tensor_dips_np((T.img_ * T.mask_).cpu().numpy(), smooth=2.0, dtype=np.float32)
    d = np.abs(dips - phi_ref)
    well = (np.abs(phi_ref) > 1e-3) & np.isfinite(an_ref) & (np.abs(an_ref) > 1e-2)
    assert np.median(d[well]) < 1e-3 and np.mean(d < 5e-3) > 0.8
    T, a = _lines_interpolator(golden, ["--aa_weight", "0.5"], 30)
    T.optimize(verbose=False)
    h = T.history
    assert len(h) == 30 and np.isfinite(h.loss).all() and h.loss[-1] < 0.5 * h.loss[0] and h.reg[-1] < h.reg[0]
    # gradient of the regulariser reaches the weights: same seed without the add-on gives a different trajectory
    T0, _ = _lines_interpolator(golden, [], 30)
    T0.optimize(verbose=False, mode="eager")
    assert abs(T0.history.loss[5] - h.df[5]) > 1e-6 * abs(h.df[5])


def test_pocs_regularised_loop(golden):
    """reference main_pocs.py:160-220 on the HIP path (torch.fft transform, HIP threshold / projection kernels): iteration 0
    against the numpy oracle of utils/pocs.py evaluated on the HIP output, both weighting modes, then a short run."""
    from deep_prior_interpolation_amd import main_pocs, utils as u
    from deep_prior_interpolation_amd.parameter import parse_arguments
    shape = (16, 12, 20)
    vol = u.sparse_hyperbolic_volume(shape, seed=2)[..., None] * 2.0
    mask = u.random_trace_mask(shape, 0.5, seed=3)[..., None].astype(np.float64)
    for weight in (None, 0.3):
        argv = ["--imgdir", "x", "--datadim", "3d", "--filters", "4", "8", "--skip", "4", "--inputdepth", "8", "--upsample", "linear",
                "--epochs", "1", "--gpu", "0", "--pocs_alpha", "0.1", "--pocs_thresh", "5"] + ([] if weight is None else ["--pocs_weight", str(weight)])
        a = parse_arguments(argv)
        u.set_seed(0)
        T = main_pocs.Interpolator(a, "/tmp")
        T.load_data({"image": vol.astype(np.float64), "mask": mask, "name": "0"})
        T.build_model()
        T.build_input()
        T.build_regularizer()
        T.optimize(verbose=False)
        out0 = np.asarray(T.out_best, dtype=np.float64)[None, None]
        img, msk = T.img_.cpu().numpy().astype(np.float64), T.mask_.cpu().numpy().astype(np.float64)
        pocs_ref, _ = O.pocs_np(out0, 0.1, img * msk, msk, 5.0)
        reg_ref = np.mean((out0 - pocs_ref) ** 2)
        main_ref = np.mean(np.abs(out0 * msk - img * msk))
        h = T.history
        assert abs(h.df[0] - main_ref) < 1e-5 * main_ref
        assert abs(h.reg[0] - reg_ref) < 2e-3 * reg_ref
        eps = main_ref / reg_ref if weight is None else weight
        assert abs(h.loss[0] - (main_ref + eps * reg_ref)) < 2e-3 * abs(h.loss[0])
        assert T.reg_data.shape == (1,) + shape and np.isfinite(T.reg_data).all()
    a = parse_arguments(argv[:argv.index("--epochs")] + ["--epochs", "25"] + argv[argv.index("--epochs") + 2:])
    u.set_seed(0)
    T = main_pocs.Interpolator(a, "/tmp")
    T.load_data({"image": vol.astype(np.float64), "mask": mask, "name": "0"})
    T.build_model()
    T.build_input()
    T.build_regularizer()
    T.optimize(verbose=False)
    assert len(T.history) == 25 and np.isfinite(T.history.loss).all() and T.history.df[-1] < 0.7 * T.history.df[0]


def test_respath_dropout_order(monkeypatch):
    """ResPath with dropout p > 0: the 3-D block is add -> act -> BN -> dropout (mulresunet.py:109-112), the 2-D one
    add -> act -> dropout -> BN (mulresunet.py:59-64), each with exactly one dropout."""
    from deep_prior_interpolation_amd import ops
    from deep_prior_interpolation_amd.architectures import mulresunet as M
    order = []
    real_bn, real_dr = ops.batch_norm, ops.channel_dropout
    monkeypatch.setattr(ops, "batch_norm", lambda *a, **k: (order.append("bn"), real_bn(*a, **k))[1])
    monkeypatch.setattr(ops, "channel_dropout", lambda *a, **k: (order.append("dr"), real_dr(*a, **k))[1])
    for nd, shape in ((3, (1, 5, 4, 6, 8)), (2, (1, 5, 9, 8))):
        rp = M.ResPath(nd, 5, 4, drop=0.3).to(DEV)
        del order[:]
        rp(torch.randn(shape, device=DEV))
        tail = [o for o in order if o in ("bn", "dr")][-2:]
        assert tail == (["bn", "dr"] if nd == 3 else ["dr", "bn"]), (nd, order)
        assert order.count("dr") == 1


def test_main_pocs_cli_writes_reference_result_layout(tmp_path, monkeypatch):
    """python -m deep_prior_interpolation_amd.main_pocs <flags>: same result-file layout as the reference's main_pocs.py
    (main_pocs.py:262-275: the `_run.npy` dict carries the last POCS projection under 'pocs', history is a HistoryReg)."""
    from deep_prior_interpolation_amd import main_pocs, utils as u
    common = _survey(tmp_path)
    monkeypatch.chdir(tmp_path)
    main_pocs.main(common + ["--epochs", "4", "--outdir", "pocs", "--pocs_alpha", "0.2", "--pocs_thresh", "10"])
    files = sorted(f for f in os.listdir("results/pocs") if f.endswith("_run.npy"))
    assert files == ["0_run.npy", "1_run.npy"]
    r = np.load("results/pocs/0_run.npy", allow_pickle=True).item()
    assert set(r) >= {"device", "elapsed", "outpath", "history", "mask", "image", "output", "noise", "pocs"}
    assert isinstance(r["history"], u.HistoryReg) and len(r["history"]) == 4 and np.isfinite(r["history"].reg).all()
    assert r["pocs"].shape == (1, 16, 16, 16) and r["output"].shape == (16, 16, 16)
    assert os.path.exists("results/pocs/args.txt")


def test_antialiasing_addon_on_25d_slabs(golden):
    """configs[3] as stated: --datadim 2.5d (slices of the lines section as channels of a 2-D net) with the anti-aliasing add-on:
    one dip field and one directional Laplacian per slice (Hale2D on a multi-channel BCHW tensor), regulariser value against the
    numpy oracle at iteration 0."""
    from deep_prior_interpolation_amd import utils as u
    from deep_prior_interpolation_amd.main import Interpolator
    from deep_prior_interpolation_amd.parameter import parse_arguments
    g = golden("net_lines25d_tiny")
    a = parse_arguments(["--imgdir", "x", "--datadim", "2.5d", "--imgchannel", "4", "--slice", "tx", "--filters", "4", "8", "16", "--skip", "4", "8",
                         "--inputdepth", "8", "--upsample", "linear", "--gain", "1", "--epochs", "1", "--gpu", "0", "--aa_weight", "0.25"])
    u.set_seed(0)
    T = Interpolator(a, "/tmp")
    T.load_data({"image": g["image"], "mask": g["mask"], "name": "0"})
    T.build_model()
    T.build_input()
    T.build_regularizer()
    assert tuple(T._aa_op.dips.shape) == (1, 4, 170, 100)
    T.optimize(verbose=False)
    out0 = np.asarray(T.out_best, dtype=np.float64).transpose(2, 0, 1)[None]            # (H,W,C) -> BCHW
    reg_ref = np.abs(O.hale2d_np(out0, T._aa_op.dips.cpu().numpy().astype(np.float64))).mean()
    assert abs(T.history.reg[0] - reg_ref) < 1e-4 * reg_ref + 1e-9
    assert abs(T.history.loss[0] - (T.history.df[0] + 0.25 * T.history.reg[0])) < 1e-6 * abs(T.history.loss[0])


def test_configs3_as_written_skip_net_on_25d_slabs_with_antialiasing(golden):
    """BASELINE configs[3] in the stated combination: `--datadim 2.5d --net skip` (2-D Skip hourglass, reference architectures/skip.py:5-48,
    reached through get_net — a documented deviation, upstream falls through to MulResUnet) on the datasets/lines slabs WITH the
    anti-aliasing regulariser in the loop.  The net itself is pinned by the reference-recorded trajectory (test_gpu_nets.py,
    net_lines25d_skip_tiny); here: the same initial state and first input reproduce the reference's iteration-0 data loss with the add-on
    switched on, the regulariser value matches the numpy oracle on the HIP output, and a 30-iteration run decreases both terms."""
    from deep_prior_interpolation_amd import utils as u
    from deep_prior_interpolation_amd.architectures import Skip
    from deep_prior_interpolation_amd.main import Interpolator
    from deep_prior_interpolation_amd.parameter import parse_arguments
    g = golden("net_lines25d_skip_tiny")
    argv = ["--imgdir", "x", "--datadim", "2.5d", "--imgchannel", "4", "--slice", "tx", "--net", "skip", "--filters", "4", "8", "16", "--skip", "2", "2", "2",
            "--inputdepth", "8", "--upsample", "linear", "--gain", "1", "--gpu", "0", "--aa_weight", "0.25"]

    def make(epochs):
        a = parse_arguments(argv + ["--epochs", str(epochs)])
        u.set_seed(0)
        T = Interpolator(a, "/tmp")
        T.load_data({"image": g["image"], "mask": g["mask"], "name": "0"})
        T.build_model()
        T.build_input()
        T.build_regularizer()
        return T
    T = make(1)
    assert isinstance(T.net, Skip) and isinstance(T.history, u.HistoryReg) and tuple(T._aa_op.dips.shape) == (1, 4, 170, 100)
    sd = T.net.state_dict()
    assert list(sd.keys()) == list(g["init_state"].keys())
    T.net.load_state_dict({k: torch.from_numpy(np.asarray(v)).to(sd[k].dtype) for k, v in g["init_state"].items()})
    T.optimize(net_inputs=[torch.from_numpy(g["net_inputs"][0]).cuda()], verbose=False)
    assert abs(T.history.df[0] - g["loss"][0]) <= 1e-5 * abs(g["loss"][0])          # the data term is the reference's iteration-0 loss
    out0 = np.asarray(T.out_best, dtype=np.float64).transpose(2, 0, 1)[None]            # (H,W,C) -> BCHW
    reg_ref = np.abs(O.hale2d_np(out0, T._aa_op.dips.cpu().numpy().astype(np.float64))).mean()
    assert abs(T.history.reg[0] - reg_ref) < 1e-4 * reg_ref + 1e-9
    assert abs(T.history.loss[0] - (T.history.df[0] + 0.25 * T.history.reg[0])) < 1e-6 * abs(T.history.loss[0])
    T = make(30)
    T.optimize(verbose=False)
    h = T.history
    assert len(h) == 30 and np.isfinite(h.loss).all() and h.loss[-1] < 0.7 * h.loss[0] and h.reg[-1] < h.reg[0]


@pytest.mark.parametrize("shape", [(20, 18, 36), (17, 19, 22), (32, 32, 64)])
def test_precision_modes_through_the_loop_at_awkward_shapes(shape):
    """--precision fp32 / bf16 / split through Interpolator.optimize on shapes that mix the kernel families inside one net: rows
    that are / are not whole float4 (the bf16 backward-weight kernel needs them, the fp32 kernels take the rest), odd extents
    (ragged tiles at every level, crops after up-sampling).  Same seed, same noise stream: iteration 0 is the same forward pass,
    so its loss must agree to the mode's operand rounding (bf16: 2^-9 per operand -> 5e-3; split: fp32 class -> 2e-5), and ten
    iterations must stay finite and on the same loss level."""
    from deep_prior_interpolation_amd import ops, utils as u
    from deep_prior_interpolation_amd.main import Interpolator
    from deep_prior_interpolation_amd.parameter import parse_arguments
    vol = u.sparse_hyperbolic_volume(shape, seed=3)
    mask = u.random_trace_mask(shape, 0.5, seed=4)
    losses = {}
    try:
        for prec in ("fp32", "bf16", "bf16mm", "split"):
            args = parse_arguments(["--imgdir", "synthetic", "--datadim", "3d", "--net", "multiunet", "--inputdepth", "16", "--upsample", "linear",
                                    "--loss", "mae", "--lr", "1e-3", "--gain", "40", "--epochs", "10", "--gpu", "0", "--precision", prec])
            u.set_seed(7)
            T = Interpolator(args, "/tmp", seed=7)
            T.load_data({"image": (vol.astype(np.float64) * 40)[..., None], "mask": mask.astype(np.float64)[..., None], "name": "0"})
            T.build_model()
            T.build_input()
            T.optimize(verbose=False)
            losses[prec] = np.array(T.history.loss)
            assert np.isfinite(losses[prec]).all() and np.isfinite(np.asarray(T.out_best)).all(), prec
    finally:
        ops.set_precision("fp32")
        ops.set_storage("fp32")
    ref = losses["fp32"]
    print(shape, {k: [round(float(x), 5) for x in v[:3]] for k, v in losses.items()})
    assert abs(losses["bf16"][0] - ref[0]) <= 5e-3 * ref[0]             # bf16 storage (round 4) + operands
    assert abs(losses["bf16mm"][0] - ref[0]) <= 5e-3 * ref[0]           # operands only
    assert abs(losses["split"][0] - ref[0]) <= 2e-5 * ref[0]
    for prec in ("bf16", "bf16mm", "split"):
        assert abs(losses[prec][-1] - ref[-1]) <= 0.1 * ref[-1], prec


# ---------------------------------------------------------------- round 6: stream-schedule invariants, parity noise source -------------
def _tiny_default_interpolator(shape=(16, 16, 16), extra=(), epochs=3):
    from deep_prior_interpolation_amd import utils as u
    from deep_prior_interpolation_amd.main import Interpolator
    from deep_prior_interpolation_amd.parameter import parse_arguments
    a = parse_arguments(["--imgdir", "x", "--datadim", "3d", "--upsample", "linear", "--gain", "40", "--epochs", str(epochs), "--gpu", "0"] + list(extra))
    vol = u.hyperbolic_volume(shape, seed=0)
    mask = u.random_trace_mask(shape, 0.5, seed=1)
    u.set_seed(0)
    T = Interpolator(a, "/tmp")
    T.load_data({"image": (vol.astype(np.float64) * a.gain)[..., None], "mask": mask.astype(np.float64)[..., None], "name": "0"})
    T.build_model()
    T.build_input()
    return T, a


def test_deferred_gradients_must_be_adopted_by_autograd():
    """with the once-per-step join the fused nodes hand autograd weight gradients the side stream has not written yet; that is
    sound only if AccumulateGrad adopts the tensor (.grad None at the start of backward).  A surviving .grad (zero_grad(set_to_none=False), a
    loop that keeps gradients) makes autograd ADD on the main stream, ahead of the producer: it must be refused loudly, the streams joined and the
    per-iteration state reset — and the next clean iteration must work."""
    from deep_prior_interpolation_amd import _lib, ops
    from deep_prior_interpolation_amd.optim import FusedAdam
    T, a = _tiny_default_interpolator()
    T.optimizer = FusedAdam(T.net.parameters(), lr=a.lr)
    with pytest.raises(_lib.DpiError):
        T.optimizer.zero_grad(set_to_none=False)
    ops.set_weight_grad_overlap(True)
    try:
        T.optimizer.zero_grad()
        T.optimization_loop()                                   # clean iteration: every deferred gradient is a parameter's .grad
        assert not ops.sched.in_iteration and not ops.sched.deferred
        w = next(p for p in T.net.parameters() if p.ndim == 5)
        g_clean = w.grad.clone()
        for p in T.net.parameters():                             # what zero_grad(set_to_none=False) leaves behind
            if p.grad is not None:
                p.grad = torch.zeros_like(p.grad)
        with pytest.raises(_lib.DpiError, match="side / branch stream"):
            T.optimization_loop()
        assert not ops.sched.in_iteration and not ops.sched.deferred and not ops.sched.side_keep
        T.optimizer.zero_grad()
        T.optimization_loop()
        assert torch.isfinite(w.grad).all() and w.grad.shape == g_clean.shape
    finally:
        ops.set_weight_grad_overlap(False)
        ops.abort_iteration()


def test_an_iteration_that_raises_leaves_no_iteration_state_behind(monkeypatch):
    from deep_prior_interpolation_amd import ops
    from deep_prior_interpolation_amd.optim import FusedAdam
    T, a = _tiny_default_interpolator()
    T.optimizer = FusedAdam(T.net.parameters(), lr=a.lr)
    ops.set_weight_grad_overlap(True)
    try:
        def boom(*_a, **_k):
            raise RuntimeError("boom")
        monkeypatch.setattr(ops, "masked_loss", boom)
        with pytest.raises(RuntimeError, match="boom"):
            T.optimization_loop()
        assert not ops.sched.in_iteration and not ops.sched.side_keep and not ops.sched.deferred and not ops.sched.branch_open
    finally:
        ops.set_weight_grad_overlap(False)


def test_torch_cpu_noise_source_runs_eagerly_and_is_reproducible():
    """--noise_source torch_cpu: z and the perturbation come from torch's CPU generator — the loop cannot be a graph (auto picks eager, explicit
    graph mode is refused) and two runs from the same seed give the same trajectory; the Philox default gives another."""
    runs = []
    for src in ("torch_cpu", "torch_cpu", "philox"):
        T, a = _tiny_default_interpolator(extra=["--noise_source", src], epochs=4)
        assert T.graph_capable() == (src == "philox")
        if src == "torch_cpu":
            with pytest.raises(ValueError):
                T.optimize(verbose=False, mode="graph")
            assert T._z_cpu is not None and torch.equal(T._z_cpu, T.input_.cpu())
        T.optimize(verbose=False)
        runs.append(np.array(T.history.loss))
    assert len(runs[0]) == 4 and np.array_equal(runs[0], runs[1])
    assert not np.allclose(runs[0][1:], runs[2][1:], rtol=1e-6)
