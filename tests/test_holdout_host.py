"""CPU tests of --holdout (self-validation on held-out traces): the flag, the per-trace split and its independence from the
reference's random streams, the masks it implies, the history classes and the C ABI rows of the two new entry points."""
import json
import os
import re
import subprocess
from argparse import Namespace

import numpy as np
import pytest
import torch

from conftest import ROOT
from deep_prior_interpolation_amd import utils as u
from deep_prior_interpolation_amd.parameter import parse_arguments

BASE = ["--imgdir", "x", "--datadim", "3d"]


def _mask(shape=(8, 64, 64, 1), rate=0.5, seed=0):
    rng = np.random.RandomState(seed)
    tr = (rng.rand(1, *shape[1:]) > rate).astype(np.float64)
    return np.broadcast_to(tr, shape).copy()


def _interp(argv, mask, index, device="cpu"):
    from deep_prior_interpolation_amd.main import Interpolator
    T = Interpolator(parse_arguments(BASE + argv), "/tmp", device=device)
    T.load_data({"image": np.random.RandomState(1).randn(*mask.shape), "mask": mask, "name": "p%d" % index})
    T.begin_patch(index)
    T.build_holdout()
    return T


# ---------------------------------------------------------------- flag ------------------------------------------------------------------
def test_flag_default_range_and_args_roundtrip(tmp_path):
    assert parse_arguments(BASE).holdout == 0.0
    assert parse_arguments(BASE + ["--holdout", "0.5"]).holdout == 0.5
    assert parse_arguments(BASE + ["--holdout", "0"]).holdout == 0.0
    for bad in ("-0.01", "0.51", "1", "nan"):
        with pytest.raises(ValueError):
            parse_arguments(BASE + ["--holdout", bad])
    a = parse_arguments(BASE + ["--holdout", "0.1"])
    p = str(tmp_path / "args.txt")
    u.write_args(p, a)
    b = u.read_args(p)
    assert b.holdout == 0.1 and vars(b) == json.loads(json.dumps(vars(a)))


def test_namespace_without_the_key_means_off():
    """args.txt written by the reference and the Namespace(**golden args) of the tests have no `holdout` key."""
    from deep_prior_interpolation_amd.main import Interpolator
    a = vars(parse_arguments(BASE))
    a.pop("holdout")
    T = Interpolator(Namespace(**a), "/tmp", device="cpu")
    assert T.holdout == 0.0 and type(T.history) is u.History
    T.load_data({"image": np.ones((4, 4, 4, 1)), "mask": _mask((4, 4, 4, 1)), "name": "0"})
    T.build_holdout()
    assert T.holdout_sel is None and T._holdout_dev is None
    with pytest.raises(ValueError):
        Interpolator(Namespace(**dict(a, holdout=0.7)), "/tmp", device="cpu")


def test_pocs_refuses_holdout():
    from deep_prior_interpolation_amd.main_pocs import Interpolator
    with pytest.raises(ValueError, match="holdout"):
        Interpolator(parse_arguments(BASE + ["--holdout", "0.1"]), "/tmp", device="cpu")


# ---------------------------------------------------------------- split -----------------------------------------------------------------
def test_split_reproducible_and_per_patch_seeded():
    m = _mask()
    a = u.holdout_traces(m, 0.1, 5)
    np.testing.assert_array_equal(a, u.holdout_traces(m, 0.1, 5))
    assert not np.array_equal(a, u.holdout_traces(m, 0.1, 6))
    assert a.shape == m.shape[1:] and a.dtype == np.float32
    T1, T2 = _interp(["--holdout", "0.2"], m, 3), _interp(["--holdout", "0.2"], m, 3)
    np.testing.assert_array_equal(T1.holdout_sel, T2.holdout_sel)
    np.testing.assert_array_equal(T1.holdout_sel, u.holdout_traces(m, 0.2, 3))
    assert not np.array_equal(T1.holdout_sel, _interp(["--holdout", "0.2"], m, 4).holdout_sel)
    # device layout (C, X, Y) of the (X, Y, C) selection
    np.testing.assert_array_equal(T1._holdout_dev.numpy(), np.moveaxis(T1.holdout_sel, -1, 0))


def test_split_holds_out_whole_known_traces_only():
    m = _mask((6, 32, 24, 2))
    m[2:, 0, 0, 0] = 0                          # a trace with a few known samples still counts as known
    m[:, 0, 1, 0] = 0
    m[3, 0, 1, 0] = 1
    sel = u.holdout_traces(m, 0.5, 11)
    known = (m != 0).any(axis=0)
    assert np.all(sel[~known] == 0)
    assert set(np.unique(sel)) <= {0.0, 1.0}
    m_tr, m_ho = u.holdout_masks(m, sel)
    np.testing.assert_array_equal(m_tr + m_ho, m)
    np.testing.assert_array_equal(m_tr * m_ho, np.zeros_like(m))
    # whole traces: along t the held-out mask is the known mask of the trace or zero
    assert np.all((m_ho == m) | (m_ho == 0))
    assert np.all(np.all(m_ho == m, axis=0) | np.all(m_ho == 0, axis=0))


@pytest.mark.parametrize("frac", [0.05, 0.2, 0.5])
def test_held_fraction_is_binomial(frac):
    m = _mask((4, 64, 64, 1), rate=0.3)
    known = int((m != 0).any(axis=0).sum())
    for seed in range(3):
        k = int(u.holdout_traces(m, frac, seed).sum())
        sd = np.sqrt(known * frac * (1 - frac))
        assert abs(k - known * frac) <= 4 * sd, (k, known, frac)


def test_split_leaves_global_generators_alone():
    m = _mask()
    np.random.seed(123)
    torch.manual_seed(321)
    st_np, st_t = np.random.get_state(), torch.get_rng_state()
    u.holdout_traces(m, 0.3, 7)
    assert torch.equal(torch.get_rng_state(), st_t)
    T = _interp(["--holdout", "0.3"], m, 2)          # begin_patch reseeds torch: compare the draw itself
    st_t2 = torch.get_rng_state()
    T.build_holdout()
    assert torch.equal(torch.get_rng_state(), st_t2)
    after = np.random.get_state()
    assert after[0] == st_np[0] and np.array_equal(after[1], st_np[1]) and after[2:] == st_np[2:]
    u.holdout_traces(m, 0.3, 7)
    assert torch.equal(torch.get_rng_state(), st_t2)


def test_empty_and_full_holdout_raise():
    one = np.zeros((4, 8, 8, 1))
    one[:, 3, 3, 0] = 1
    with pytest.raises(ValueError, match="patch 'p9'.*held out no known trace"):
        u.holdout_traces(_mask((4, 2, 2, 1), rate=0.0), 1e-9, 0, name="p9")           # four known traces, nothing held out
    # a single known trace: held out -> nothing left to train on; kept -> nothing held out
    for seed in range(8):
        with pytest.raises(ValueError, match="patch 'lone'"):
            u.holdout_traces(one, 0.5, seed, name="lone")
    with pytest.raises(ValueError):
        u.holdout_traces(_mask(), 0.6, 0)


def test_data_forgetting_term_leaves_out_the_held_out_traces():
    """--data_forgetting_factor adds img * mask to the network input for the first iterations: with --holdout it is built from the training
    traces only (img * m_tr), and neither z nor the initial weights move."""
    m = _mask((8, 16, 16, 1), rate=0.3)
    argv = ["--noise_dist", "u", "--inputdepth", "4", "--filters", "4", "8", "--skip", "4", "--data_forgetting_factor", "5"]
    Ts = {}
    for frac in (0.0, 0.3):
        from deep_prior_interpolation_amd.main import Interpolator
        T = Interpolator(parse_arguments(BASE + argv + ["--holdout", str(frac)]), "/tmp", device="cpu")
        T.load_data({"image": np.random.RandomState(1).randn(*m.shape) + 3.0, "mask": m, "name": "0"})
        T.begin_patch(4)
        T.build_model()
        T.build_input()
        Ts[frac] = T
    T0, T1 = Ts[0.0], Ts[0.3]
    assert torch.equal(T0.input_, T1.input_)
    for (k, v0), v1 in zip(T0.net.state_dict().items(), T1.net.state_dict().values()):
        assert torch.equal(v0, v1), k
    held = (np.moveaxis(T1.holdout_sel, -1, 0) > 0)[0]               # (X, Y) of the single channel; the term is (1, inputdepth, T, X, Y)
    assert held.sum() > 0
    d = T1.add_data_[0].numpy()
    assert np.all(d[:, :, held] == 0)
    known_kept = (np.moveaxis((m != 0).any(axis=0), -1, 0) & ~held)[0]
    assert np.all(d[:, :, known_kept] != 0)
    assert np.any(T0.add_data_[0].numpy()[:, :, held] != 0)         # without a holdout those traces are in the term
    np.testing.assert_array_equal(T1.training_mask().numpy(), u.holdout_masks(m, T1.holdout_sel)[0].transpose(3, 0, 1, 2)[None])
    assert T0.training_mask() is T0.mask_


# ---------------------------------------------------------------- history ---------------------------------------------------------------
def test_history_classes():
    from deep_prior_interpolation_amd.main import Interpolator
    assert type(Interpolator(parse_arguments(BASE), "/tmp", device="cpu").history) is u.History
    T = Interpolator(parse_arguments(BASE + ["--holdout", "0.1"]), "/tmp", device="cpu")
    h = T.history
    assert isinstance(h, u.HistoryHoldout) and isinstance(h, u.History)
    h.append((1.0, 2.0, 0.5))
    h.lr.append(1e-3)
    h.append_val(0.25, 3.5)
    assert len(h) == 1
    msg = h.log_message(0)
    assert "VAL = 2.50e-01" in msg and "VSNR = +3.50 dB" in msg and "Loss = +1.00e+00" in msg
    r = u.HistoryRegHoldout(10)
    r.append((1.0, 0.9, 0.1, 2.0, 0.5))
    r.lr.append(1e-3)
    r.append_val(0.5, 1.0)
    assert len(r) == 1 and "REG = 1.00e-01" in r.log_message(0) and "VSNR = +1.00 dB" in r.log_message(0)
    assert not hasattr(u.History(3), "val_loss") and not hasattr(u.HistoryReg(3), "val_loss")


# ---------------------------------------------------------------- C ABI -----------------------------------------------------------------
def test_abi_rows_of_the_new_entry_points():
    from deep_prior_interpolation_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dpi_hip.h")).read(), flags=re.S)
    for name in ("dpi_masked_loss_holdout", "dpi_loop_control_holdout"):
        assert re.search(r"\b%s\s*\(" % name, txt)
        assert name in _lib.SIGNATURES
    assert _lib.ABI_VERSION == 406
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    assert "dpi_masked_loss_holdout" in out and "dpi_loop_control_holdout" in out
    assert _lib.load().dpi_version() == 406
