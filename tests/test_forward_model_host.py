"""The forward model between the network and the loss, without a GPU: stage order and tracking with stand-in operators, selection and
clean, the keys of the result file per flag set, nn.Module's own methods on the operator classes, and net_args_are_same's error list."""
from argparse import Namespace

import numpy as np
import pytest
import torch

from deep_prior_interpolation_amd import utils as u
from deep_prior_interpolation_amd.forward_model import ForwardModel, Stage
from deep_prior_interpolation_amd.operators import (AVOLinearModelling, AxisDerivative, ConvolutionalModelling, Moveout, TraceSampling,
                                                    VerticalConv, VerticalGrad)
from deep_prior_interpolation_amd.parameter import net_args_are_same, parse_arguments
from deep_prior_interpolation_amd.utils.slopes import Hale2D, Hale2DSections

BASE = ["--imgdir", "x"]
FACTOR = {"avo": 2.0, "wavelet": 3.0, "moveout": 5.0, "sampling": 7.0}


class Scale:
    """A pure-torch linear map that records its calls: (name, the tensor it was given)."""

    def __init__(self, name, calls):
        self.name, self.calls = name, calls

    def __call__(self, x):
        self.calls.append((self.name, x))
        return x * FACTOR[self.name]


def _stand_ins(names, tracked=("wavelet",), args=None):
    calls = []
    stages = [Stage(n, Scale(n, calls), "data" if n == "sampling" else "model", n in tracked) for n in names]
    return ForwardModel(args or parse_arguments(BASE), stages=stages), calls


# ---------------------------------------------------------------- 1. stage order and tracking -------------------------------------
def test_stage_order_and_tracking():
    fm, calls = _stand_ins(("sampling", "moveout", "wavelet", "avo"))          # given in the wrong order on purpose
    assert [s.name for s in fm.stages] == ["avo", "wavelet", "moveout", "sampling"]
    x = torch.arange(6.0).reshape(1, 1, 3, 2).requires_grad_()
    out = fm.apply_model(x)
    assert [n for n, _ in calls] == ["avo", "wavelet", "moveout"]
    assert torch.equal(out, x * 30.0)
    # pre is the detached input of the tracked stage: behind the AVO stage, in front of the wavelet
    assert torch.equal(fm.pre, x.detach() * 2.0) and not fm.pre.requires_grad and calls[1][1].requires_grad
    del calls[:]
    data = fm.apply_data(out)
    assert [n for n, _ in calls] == ["sampling"] and calls[0][1] is out and torch.equal(data, out * 7.0)


def test_no_stage_is_the_identity():
    fm = ForwardModel(parse_arguments(BASE))
    x = torch.ones(1, 1, 2, 2)
    assert fm.stages == [] and fm.apply_model(x) is x and fm.apply_data(x) is x and fm.pre is None
    assert fm.stage("wavelet") is None and fm.net_outchannel(5) == 5 and fm.volumes() == []


def test_two_tracked_stages_are_refused():
    with pytest.raises(ValueError, match="wavelet and moveout"):
        _stand_ins(("wavelet", "moveout"), tracked=("wavelet", "moveout"))
    _stand_ins(("wavelet", "moveout"), tracked=("moveout",))


# ---------------------------------------------------------------- 2. selection and clean ------------------------------------------
def test_selection_and_clean():
    fm, _ = _stand_ins(("avo", "wavelet"))
    assert fm.model("wavelet") is None                           # nothing selected yet
    x = torch.arange(24.0).reshape(1, 2, 3, 4)
    fm.apply_model(x)
    assert fm.best is None and fm.model("wavelet") is None
    fm.select()
    assert fm.best is fm.pre                                     # a reference, not a copy
    m = fm.model("wavelet")
    assert m.shape == (3, 4, 2) and np.array_equal(m, (x * 2.0)[0].permute(1, 2, 0).numpy())
    fm.apply_model(x + 1.0)
    assert fm.best is not fm.pre and np.array_equal(fm.model("wavelet"), m)      # the next iterate does not touch the selected one
    assert fm.model("moveout") is None and fm.model("sampling") is None
    fm.clean()
    assert fm.pre is None and fm.best is None and fm.model("wavelet") is None


@pytest.mark.parametrize("extra", [["--out_ema", "0.9"], ["--optimizer", "sgld"]])
def test_an_average_of_iterates_has_no_tracked_model(extra):
    fm, _ = _stand_ins(("wavelet",), args=parse_arguments(BASE + extra))
    fm.apply_model(torch.ones(1, 1, 3, 4))
    fm.select()
    assert fm.best is not None and fm.model("wavelet") is None and fm.volumes() == []


# ---------------------------------------------------------------- 3. run-file keys -------------------------------------------------
AVO = ["--datadim", "2.5d", "--slice", "tx", "--imgchannel", "4", "--avo_theta", "0", "10", "20", "30"]
AVO_KEYS = {"avo_theta", "avo_vsvp", "avo_linearization", "avo_model"}
WAV_KEYS = {"wavelet", "wavelet_model_kind", "wavelet_model"}
MOV_KEYS = {"moveout", "moveout_interp", "moveout_model"}
OFF_KEYS = {"trace_offsets", "trace_interp"}
# flag set -> (argv, the shape of a patch, the keys save_result writes for it)
RUN_CASES = {
    "none": (["--datadim", "3d"], (6, 5, 4, 1), set()),
    "avo": (AVO, (6, 5, 4), AVO_KEYS),
    "wavelet": (["--datadim", "3d", "--wavelet", "w.npy", "--wavelet_model", "impedance"], (6, 5, 4, 1), WAV_KEYS),
    "avo+wavelet": (AVO + ["--wavelet", "w.npy"], (6, 5, 4), AVO_KEYS | WAV_KEYS),
    "moveout": (["--datadim", "3d", "--moveout", "tau.npy", "--moveout_interp", "cubic"], (6, 5, 4, 1), MOV_KEYS),
    "trace_offsets": (["--datadim", "3d", "--trace_offsets", "off.npy"], (6, 5, 4, 1), OFF_KEYS),
    "trace_offsets+wavelet": (["--datadim", "3d", "--trace_offsets", "off.npy", "--wavelet", "w.npy"], (6, 5, 4, 1), OFF_KEYS | WAV_KEYS),
}


@pytest.mark.parametrize("case", list(RUN_CASES))
def test_run_fields(tmp_path, case):
    argv, shape, keys = RUN_CASES[case]
    wavelet = u.ricker(25.0, 0.004, 9)
    np.save(tmp_path / "w.npy", wavelet)
    fm = ForwardModel(parse_arguments(["--imgdir", str(tmp_path)] + argv))
    assert [s.name for s in fm.stages] == [n for n in ("avo", "wavelet", "moveout", "sampling") if n.replace("sampling", "trace_offsets") in case]
    rng = np.random.RandomState(3)
    table = np.arange(6.0)[:, None, None] - rng.randint(0, 3, (1, 5, 4))
    offsets = rng.uniform(-0.5, 0.5, (5, 4, 2)).astype(np.float32)
    mask = np.ones(shape)
    mask[:, 2] = 0                                               # unknown traces: their offsets are zeroed
    data = {"moveout": table} if "moveout" in case else {"offsets": offsets} if "trace_offsets" in case else {}
    live = fm.load_patch(data, shape, mask, torch.device("cpu"), "0")
    run = fm.run_fields()
    assert set(run) == keys
    assert all(run[k] is None for k in keys if k.endswith("_model"))          # nothing was optimised
    assert (live is None) == ("moveout" not in case)
    if "avo" in case:
        assert run["avo_theta"] == [0.0, 10.0, 20.0, 30.0] and run["avo_vsvp"] == 0.5 and run["avo_linearization"] == "akirich"
        assert fm.net_outchannel(4) == 3 and fm.stage("avo").op.nt0 == 6 and ("avo_model", "reconstructed_avo.npy") in fm.volumes()
        out = rng.standard_normal(shape).astype(np.float32)
        assert fm.run_fields(out)["avo_model"].shape == (6, 5, 3) and fm.run_fields(out)["avo_model"].dtype == np.float32
    if "wavelet" in case:
        kind = "impedance" if case == "wavelet" else "reflectivity"
        assert run["wavelet_model_kind"] == kind and run["wavelet"].dtype == np.float32
        assert np.array_equal(run["wavelet"], (wavelet / 2 if kind == "impedance" else wavelet).astype(np.float32))
        assert ("wavelet_model", "reconstructed_model.npy") in fm.volumes()
    if "moveout" in case:
        assert run["moveout_interp"] == "cubic" and np.array_equal(run["moveout"], table.astype(np.float32))
        assert np.array_equal(live, table >= 0) and fm.volumes() == [("moveout_model", "reconstructed_flat.npy")]
    if "trace_offsets" in case:
        assert run["trace_interp"] == "linear" and np.array_equal(run["trace_offsets"], offsets * (mask[0, :, :, :1] != 0))
        assert run["trace_offsets"] is fm.trace_offsets and not run["trace_offsets"][2].any()


def test_load_patch_keeps_the_messages(tmp_path):
    shape, mask = (6, 5, 4, 1), np.ones((6, 5, 4, 1))
    off = ForwardModel(parse_arguments(BASE + ["--datadim", "3d"]))
    with pytest.raises(ValueError, match="carries a moveout table but --moveout is off"):
        off.load_patch({"moveout": np.zeros((6, 5, 4))}, shape, mask, "cpu", "7")
    with pytest.raises(ValueError, match="patch 7 carries trace offsets but --trace_offsets is off"):
        off.load_patch({"offsets": np.zeros((5, 4, 2))}, shape, mask, "cpu", "7")
    on = ForwardModel(parse_arguments(BASE + ["--datadim", "3d", "--trace_offsets", "off.npy"]))
    with pytest.raises(ValueError, match="--trace_offsets off.npy: patch 7 carries no offsets"):
        on.load_patch({}, shape, mask, "cpu", "7")
    with pytest.raises(ValueError, match=r"--trace_offsets: offsets \(5, 3, 2\) do not belong"):
        on.load_patch({"offsets": np.zeros((5, 3, 2))}, shape, mask, "cpu", "7")
    with pytest.raises(ValueError, match="--wavelet .*missing.npy"):
        ForwardModel(parse_arguments(["--imgdir", str(tmp_path), "--wavelet", "missing.npy"]))


# ---------------------------------------------------------------- 4. nn.Module's own methods --------------------------------------
@pytest.mark.parametrize("build", [
    lambda: AVOLinearModelling([0, 10, 20]), lambda: ConvolutionalModelling(np.array([1.0])), lambda: Moveout(np.zeros((1, 1))),
    lambda: TraceSampling(np.zeros((2, 1, 1))), lambda: VerticalConv([1.0]), lambda: AxisDerivative(0), lambda: VerticalGrad(),
    lambda: Hale2D(torch.zeros(1, 1, 1, 1)), lambda: Hale2DSections(torch.zeros(1, 1, 1, 1, 1), torch.zeros(1, 1, 1, 1, 1))],
    ids=["AVOLinearModelling", "ConvolutionalModelling", "Moveout", "TraceSampling", "VerticalConv", "AxisDerivative", "VerticalGrad",
         "Hale2D", "Hale2DSections"])
def test_module_methods_return_the_operator(build):
    op = build()
    assert op.float() is op and op.to("cpu") is op and op.cpu() is op
    holder = torch.nn.Sequential(op)                             # as a registered submodule of something that is moved
    assert holder.to("cpu")[0] is op


# ---------------------------------------------------------------- 5. net_args_are_same ---------------------------------------------
OURS = {"avo_theta": [0.0, 10.0, 20.0], "trace_offsets": "off.npy", "trace_interp": "cubic", "wavelet": "w.npy",
        "wavelet_model": "impedance", "moveout": "tau.npy", "moveout_interp": "cubic"}


def _printed_errors(capsys, a, b):
    capsys.readouterr()
    same = net_args_are_same(a, b)
    lines = capsys.readouterr().out.splitlines()
    return same, (lines[-1] if not same else None)


@pytest.mark.parametrize("key", list(OURS))
def test_net_args_differ_in_one_key(capsys, key):
    now = parse_arguments(BASE)
    other = Namespace(**dict(vars(now), **{key: OURS[key]}))
    assert _printed_errors(capsys, now, other) == (False, key) and _printed_errors(capsys, other, now) == (False, key)
    assert _printed_errors(capsys, other, Namespace(**vars(other))) == (True, None)
    # the key absent in the saved file: the default, i.e. the same as `now` and different from `other`
    saved = Namespace(**{k: v for k, v in vars(now).items() if k != key})
    assert _printed_errors(capsys, now, saved) == (True, None) and _printed_errors(capsys, saved, now) == (True, None)
    assert _printed_errors(capsys, other, saved) == (False, key)


def test_net_args_error_list_keeps_its_order(capsys):
    now = parse_arguments(BASE)
    other = Namespace(**dict(vars(now), inputdepth=now.inputdepth + 1, **OURS))
    same, line = _printed_errors(capsys, now, other)
    assert not same and line == "inputdepth, avo_theta, trace_offsets, trace_interp, wavelet, wavelet_model, moveout, moveout_interp"
    ints = Namespace(**dict(vars(now), avo_theta=[0, 10, 20]))
    assert _printed_errors(capsys, Namespace(**dict(vars(now), avo_theta=OURS["avo_theta"])), ints) == (True, None)      # compared as floats
