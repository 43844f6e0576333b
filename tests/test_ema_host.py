"""CPU tests of --out_ema (the output selected from a running average of the iterates): the flag and what it refuses, the C ABI rows of
the two new entry points, the host selection rule and the history classes."""
import json
import pickle
from argparse import Namespace

import numpy as np
import pytest

from deep_prior_interpolation_amd import utils as u
from deep_prior_interpolation_amd.parameter import parse_arguments

BASE = ["--imgdir", "x", "--datadim", "3d"]


# ---------------------------------------------------------------- flag ------------------------------------------------------------------
def test_flag_default_range_and_args_roundtrip(tmp_path):
    assert parse_arguments(BASE).out_ema == 0.0
    assert parse_arguments(BASE + ["--out_ema", "0.99"]).out_ema == 0.99
    assert parse_arguments(BASE + ["--out_ema", "0"]).out_ema == 0.0
    for bad in ("1.0", "-0.1", "1.5", "nan"):
        with pytest.raises(ValueError, match="out_ema"):
            parse_arguments(BASE + ["--out_ema", bad])
    a = parse_arguments(BASE + ["--out_ema", "0.9", "--holdout", "0.1"])
    p = str(tmp_path / "args.txt")
    u.write_args(p, a)
    b = u.read_args(p)
    assert b.out_ema == 0.9 and vars(b) == json.loads(json.dumps(vars(a)))


@pytest.mark.parametrize("sampler", ["sgld", "psgld"])
def test_flag_refuses_a_sampler(sampler):
    with pytest.raises(ValueError, match="out_ema"):
        parse_arguments(BASE + ["--out_ema", "0.9", "--optimizer", sampler])
    assert parse_arguments(BASE + ["--optimizer", sampler]).out_ema == 0.0


def test_pocs_refuses_out_ema():
    from deep_prior_interpolation_amd.main_pocs import Interpolator
    with pytest.raises(ValueError, match="out_ema"):
        Interpolator(parse_arguments(BASE + ["--out_ema", "0.5"]), "/tmp", device="cpu")
    Interpolator(parse_arguments(BASE), "/tmp", device="cpu")


def test_namespace_without_the_key_means_off():
    """args.txt written by the reference and the Namespace(**golden args) of the tests have no `out_ema` key."""
    from deep_prior_interpolation_amd.main import Interpolator
    a = vars(parse_arguments(BASE))
    a.pop("out_ema")
    T = Interpolator(Namespace(**a), "/tmp", device="cpu")
    assert T.out_ema == 0.0 and type(T.history) is u.History
    for bad in (1.0, -0.5):
        with pytest.raises(ValueError, match="out_ema"):
            Interpolator(Namespace(**dict(a, out_ema=bad)), "/tmp", device="cpu")
    with pytest.raises(ValueError, match="out_ema"):
        Interpolator(Namespace(**dict(a, out_ema=0.9, optimizer="psgld")), "/tmp", device="cpu")
    T = Interpolator(Namespace(**dict(a, out_ema=0.9)), "/tmp", device="cpu")
    assert T.out_ema == 0.9 and type(T.history) is u.HistoryEma
    T = Interpolator(Namespace(**dict(a, out_ema=0.9, holdout=0.1)), "/tmp", device="cpu")
    assert type(T.history) is u.HistoryHoldoutEma
    T.clean()
    assert type(T.history) is u.HistoryHoldoutEma and T._ema_avg is None and T.ema_min is None


# ---------------------------------------------------------------- ABI -------------------------------------------------------------------
def test_abi_rows():
    import ctypes as C
    from deep_prior_interpolation_amd import _lib
    assert _lib.ABI_VERSION == 406
    res, args = _lib.SIGNATURES["dpi_ema_loss"]
    assert res is C.c_int and len(args) == 15 and args[9] is C.c_float and args[7] is C.c_size_t
    res, args = _lib.SIGNATURES["dpi_loop_control_ema"]
    assert res is C.c_int and len(args) == 18 and args[2] is C.c_int
    # the rules follow the state / history pointers exactly as in dpi_loop_control
    assert args[9:] == _lib.SIGNATURES["dpi_loop_control"][1][7:]


def test_header_declares_both():
    import os
    from conftest import ROOT
    h = open(os.path.join(ROOT, "include", "dpi_hip.h")).read()
    assert "int dpi_ema_loss(const float* out, float* avg, const float* img, const float* mask, const float* sel" in h
    assert "int dpi_loop_control_ema(const double* metrics, const double* ema_metrics, int has_holdout, double* state" in h


# ---------------------------------------------------------------- selection rule ---------------------------------------------------------
def test_selection_rule_on_a_script():
    """Eight rows with a tie (the later iterate wins) and a NaN (never selects, and does not poison the minimum)."""
    nan = float("nan")
    script = [1.0, 0.8, 0.8, nan, 0.9, 0.7, 0.7, 0.75]
    want = [(True, 1.0, 0), (True, 0.8, 1), (True, 0.8, 2), (False, 0.8, 2), (False, 0.8, 2), (True, 0.7, 5), (True, 0.7, 6), (False, 0.7, 6)]
    best, best_iter, got = None, None, []
    for it, q in enumerate(script):
        improved, best, best_iter = u.select_latest_min(it, q, best, best_iter)
        got.append((improved, best, best_iter))
    assert got == want


def test_selection_rule_after_a_nan_start():
    """Iteration 0 always selects — a NaN too, and then nothing compares below it: the rule of the device kernel."""
    improved, best, best_iter = u.select_latest_min(0, float("nan"), None, None)
    assert improved and best != best and best_iter == 0
    assert u.select_latest_min(1, 0.5, best, best_iter)[0] is False
    # a new patch starts again at iteration 0, whatever the state held
    assert u.select_latest_min(0, 3.0, 0.1, 17) == (True, 3.0, 0)


# ---------------------------------------------------------------- history ---------------------------------------------------------------
@pytest.mark.parametrize("reg", [False, True])
@pytest.mark.parametrize("holdout", [False, True])
def test_history_classes_roundtrip(reg, holdout):
    cls = u.history_class(reg, holdout, True)
    assert cls is {(False, False): u.HistoryEma, (True, False): u.HistoryRegEma, (False, True): u.HistoryHoldoutEma,
                   (True, True): u.HistoryRegHoldoutEma}[(reg, holdout)]
    assert issubclass(cls, u.history_class(reg, holdout, False))
    h = cls(100)
    for k in range(3):
        h.append((1.0 - 0.1 * k, 0.9, 0.05, 5.0 + k, 0.5) if reg else (1.0 - 0.1 * k, 5.0 + k, 0.5))
        h.lr.append(1e-3)
        if holdout:
            h.append_val(2.0 - 0.1 * k, 3.0 + k)
            h.append_ema(0.7 - 0.1 * k, 6.0 + k, 1.7 - 0.1 * k, 4.0 + k)
        else:
            h.append_ema(0.7 - 0.1 * k, 6.0 + k)
    assert len(h) == 3
    assert h.ema_loss == [0.7 - 0.1 * k for k in range(3)] and h.ema_snr == [6.0, 7.0, 8.0]
    assert hasattr(h, "ema_val_loss") == holdout
    if holdout:
        assert h.ema_val_loss == [1.7 - 0.1 * k for k in range(3)] and h.ema_val_snr == [4.0, 5.0, 6.0]
        assert h.val_snr == [3.0, 4.0, 5.0]
    msg = h.log_message(2)
    assert "ESNR = +8.00 dB" in msg and "SNR = +7.00 dB" in msg and ("EVSNR = +6.00 dB" in msg) == holdout
    g = pickle.loads(pickle.dumps(h))                      # what np.save does to it inside <patch>_run.npy
    assert type(g) is cls and vars(g) == vars(h) and "ESNR" in str(g)
    h.ema_snr.pop()
    with pytest.raises(AssertionError):
        len(h)


def test_history_class_without_the_flag_is_todays():
    assert u.history_class(False, False, False) is u.History and u.history_class(True, False, False) is u.HistoryReg
    assert u.history_class(False, True, False) is u.HistoryHoldout and u.history_class(True, True, False) is u.HistoryRegHoldout
    assert not hasattr(u.History(10), "ema_loss")
    assert np.isfinite(len(u.History(10)))
