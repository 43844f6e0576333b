"""The life-cycle of one patch (Interpolator.take_patch / prepare_patch / run_patch / output_for_reassembly) and the sequential
command-line driver built on it (main.run_cli), on the host: a subclass records the calls and stubs every step that needs the library."""
import numpy as np
import pytest
import torch

from deep_prior_interpolation_amd import main as dmain
from deep_prior_interpolation_amd.parameter import parse_arguments

SHAPE = (8, 8, 8, 1)
BUILD_AND_LOOP = ("begin_patch", "build_model", "build_input", "build_regularizer", "optimize")


class Recorder(dmain.Interpolator):
    """Records (step, argument) in call order.  load_data, begin_patch and clean are the real ones; the rest is stubbed."""

    def __init__(self, args, outpath, device="cpu", seed=0):
        super().__init__(args, outpath, device=device, seed=seed)
        self.calls = []

    def names(self):
        return [c[0] for c in self.calls]

    def load_data(self, data):
        self.calls.append(("load_data", data["name"]))
        return super().load_data(data)

    def begin_patch(self, index, base_seed=0):
        self.calls.append(("begin_patch", index))
        super().begin_patch(index, base_seed)

    def build_model(self, netpath=None):
        self.calls.append(("build_model", netpath))
        self.net = object()

    def build_input(self):
        self.calls.append(("build_input", None))

    def build_regularizer(self):
        self.calls.append(("build_regularizer", None))

    def optimize(self, net_inputs=None, verbose=True, mode="auto", check_every=64):
        self.calls.append(("optimize", verbose))
        self.out_best, self.elapsed = self.img.copy(), 1.0

    def save_result(self):
        self.calls.append(("save_result", self.image_name))

    def clean(self):
        self.calls.append(("clean", self.image_name))
        super().clean()


def make(tmp_path, *flags):
    return Recorder(parse_arguments(["--imgdir", "x", "--datadim", "3d", "--epochs", "3"] + list(flags)), str(tmp_path))


def patch(name, scale=1.0, masked=True):
    rng = np.random.RandomState(3)
    img = rng.standard_normal(SHAPE)
    img = scale * (img - img.mean()) / img.std()
    mask = np.broadcast_to((rng.rand(1, 8, 8, 1) > 0.4).astype(np.float64), SHAPE).copy() if masked else np.zeros(SHAPE)
    return {"image": img, "mask": mask, "name": name}


def test_a_live_patch_goes_through_the_steps_in_order(tmp_path):
    T = make(tmp_path)
    assert T.run_patch(5, patch("005"), verbose=False) is True
    assert T.names() == ["load_data"] + list(BUILD_AND_LOOP)
    assert T.calls[0] == ("load_data", "005") and T.calls[1] == ("begin_patch", 5) and T.calls[-1] == ("optimize", False)
    assert T.patch_index == 5 and T.patch_std > 0.1


def test_a_flat_patch_is_its_own_result(tmp_path):
    T = make(tmp_path)
    p = patch("000", masked=False)
    assert T.run_patch(0, p, verbose=False) is False
    assert T.names() == ["load_data"]
    assert np.array_equal(T.out_best, p["image"] * p["mask"]) and T.elapsed == 0.0 and T.patch_std == 0.0
    out = T.output_for_reassembly()
    assert torch.is_tensor(out) and out.device.type == "cpu" and out.dtype == torch.float32 and tuple(out.shape) == SHAPE[:-1]
    assert np.array_equal(out.numpy(), T.out_best[..., 0].astype(np.float32))


@pytest.mark.parametrize("std, live", [(1e-13, False), (1e-6, True)])
def test_the_flat_patch_threshold(tmp_path, std, live):
    """std of the masked data 0 within 1e-12 is flat."""
    T = make(tmp_path)
    p = patch("000", scale=1.0)
    p["image"] *= std / float(torch.std(torch.from_numpy(p["image"] * p["mask"]).float()))
    assert T.take_patch(0, p) is live
    assert T.patch_std == pytest.approx(std, rel=1e-3)
    assert T.names() == ["load_data"]                                    # take_patch loads and decides, nothing more
    assert (T.elapsed == 0.0 and np.array_equal(T.out_best, p["image"] * p["mask"])) is (not live)


@pytest.mark.parametrize("chained", [False, True])
def test_start_from_prev_keeps_the_net_of_the_patch_before(tmp_path, chained):
    T = make(tmp_path, *(["--start_from_prev"] if chained else []))
    for i in range(2):
        assert T.run_patch(i, patch(str(i)), verbose=False)
        T.clean()
    built = [c for c in T.calls if c[0] == "build_model"]
    assert built == [("build_model", None)] * (1 if chained else 2)
    first = T.names()[:T.names().index("clean")]
    assert first == ["load_data"] + list(BUILD_AND_LOOP)                 # the first patch always builds its net
    # ... and nothing else of the second patch is left out
    second = T.names()[len(first) + 1:-1]
    assert second == ["load_data"] + [s for s in BUILD_AND_LOOP if not (chained and s == "build_model")]


def test_netdir_names_the_net_of_every_patch(tmp_path):
    T = make(tmp_path, "--netdir", "a", "b")
    for i in range(2):
        T.run_patch(i, patch(str(i)), verbose=False)
        T.clean()
    assert [c for c in T.calls if c[0] == "build_model"] == [("build_model", "a"), ("build_model", "b")]


def test_the_cli_driver_saves_and_cleans_every_patch_in_order(tmp_path, monkeypatch, capsys):
    """Two patches of 8^3 from a (16, 8, 8) volume, the second without a known trace (flat)."""
    made = []

    class Cli(Recorder):
        def __init__(self, args, outpath):
            super().__init__(args, outpath, device="cpu")
            made.append(self)
    d = tmp_path / "data"
    d.mkdir()
    rng = np.random.RandomState(0)
    mask = (rng.rand(1, 8, 8) > 0.4) * np.ones((16, 1, 1))
    mask[8:] = 0.0
    np.save(d / "vol.npy", rng.standard_normal((16, 8, 8)))
    np.save(d / "mask.npy", mask)
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(dmain.u, "set_gpu", lambda id=-1: 0)             # device selection: the one step of the driver that needs a GPU
    dmain.run_cli(Cli, ["--imgdir", str(d), "--imgname", "vol.npy", "--maskname", "mask.npy", "--datadim", "3d", "--patch_shape", "8", "8", "8",
                        "--patch_stride", "8", "8", "8", "--epochs", "3", "--outdir", "cli"])
    (T,) = made
    assert T.outpath == "./results/cli" and (tmp_path / "results" / "cli" / "args.txt").exists()
    assert T.calls == [("load_data", "0"), ("begin_patch", 0), ("build_model", None), ("build_input", None), ("build_regularizer", None),
                       ("optimize", True), ("save_result", "0"), ("clean", "0"),
                       ("load_data", "1"), ("save_result", "1"), ("clean", "1")]
    out = capsys.readouterr().out
    assert out.count("The data shape is (8, 8, 8, 1), the std of coarse data is") == 2 and out.count("skipping...") == 1
    assert "Processing 2 patches" in out and out.rstrip().endswith("Interpolation done! Saved to ./results/cli")
