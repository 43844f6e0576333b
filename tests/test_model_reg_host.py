"""--model_reg without a GPU: the flags and their refusals, the axes of every kind, the numpy restatement of tests/model_reg_cases.py
against central finite differences, the history classes and the ABI table."""
import ctypes as C
import os
import pickle
import subprocess
from argparse import Namespace

import numpy as np
import pytest

from conftest import ROOT

import model_reg_cases as MR
from deep_prior_interpolation_amd import _lib, utils as u
from deep_prior_interpolation_amd.parameter import check_model_reg, model_reg_axes, parse_arguments

BASE = ["--imgdir", "x"]


# ---------------------------------------------------------------- flags -----------------------------------------------------------
def test_flags_parse_and_are_off_by_default():
    a = parse_arguments(BASE)
    assert a.model_reg is None and a.model_reg_weight == 0.0 and check_model_reg(a) is None
    a = parse_arguments(BASE + ["--datadim", "3d", "--model_reg", "tv_x", "--model_reg_weight", "0.25"])
    assert check_model_reg(a) == ("tv_x", 0.25, (3, 4))
    assert check_model_reg(Namespace()) is None and check_model_reg(Namespace(datadim="2d", slice="xy")) is None
    with pytest.raises(SystemExit):
        parse_arguments(BASE + ["--model_reg", "huber", "--model_reg_weight", "1"])


@pytest.mark.parametrize("weight", [None, "0", "-1", "inf", "nan"])
def test_a_kind_needs_a_finite_positive_weight(weight):
    argv = BASE + ["--model_reg", "l1"] + ([] if weight is None else ["--model_reg_weight", weight])
    with pytest.raises(ValueError, match="--model_reg"):
        parse_arguments(argv)


def test_a_weight_without_a_kind_is_refused():
    with pytest.raises(ValueError, match="--model_reg_weight"):
        parse_arguments(BASE + ["--model_reg_weight", "0.1"])
    with pytest.raises(ValueError, match="--model_reg_weight"):
        check_model_reg(Namespace(model_reg_weight=0.5))


def test_tv_t_is_refused_where_time_is_in_the_channels():
    with pytest.raises(ValueError, match="--model_reg tv_t"):
        parse_arguments(BASE + ["--datadim", "2.5d", "--slice", "xy", "--model_reg", "tv_t", "--model_reg_weight", "1"])
    for kind in ("l1", "tv_x", "tv"):
        parse_arguments(BASE + ["--datadim", "2.5d", "--slice", "xy", "--model_reg", kind, "--model_reg_weight", "1"])


def test_main_pocs_refuses_the_flag():
    from deep_prior_interpolation_amd.main_pocs import Interpolator
    with pytest.raises(ValueError, match="--model_reg"):
        Interpolator(parse_arguments(BASE + ["--model_reg", "l1", "--model_reg_weight", "1"]), "/tmp", device="cpu")


def test_the_flag_composes_with_the_operators_and_add_ons():
    for extra in (["--datadim", "3d", "--wavelet", "w.npy"], ["--datadim", "3d", "--moveout", "tau.npy", "--moveout_interp", "cubic"],
                  ["--datadim", "3d", "--trace_offsets", "off.npy"], ["--holdout", "0.2", "--out_ema", "0.9"], ["--aa_weight", "0.5"],
                  ["--optimizer", "psgld"], ["--datadim", "3d", "--precision", "bf16"], ["--net", "attmultiunet"], ["--net", "part"],
                  ["--datadim", "2.5d", "--slice", "tx", "--imgchannel", "3", "--avo_theta", "0", "10", "20"]):
        a = parse_arguments(BASE + extra + ["--model_reg", "tv", "--model_reg_weight", "0.5"])
        assert check_model_reg(a)[:2] == ("tv", 0.5)


AXES = {       # (datadim, slice) -> kind -> dims of the device tensor
    "2d": {"l1": (), "tv_t": (2,), "tv_x": (3,), "tv": (2, 3)},
    "3d": {"l1": (), "tv_t": (2,), "tv_x": (3, 4), "tv": (2, 3, 4)},
    "2.5d-t": {"l1": (), "tv_t": (2,), "tv_x": (3,), "tv": (2, 3)},
    "2.5d-xy": {"l1": (), "tv_t": None, "tv_x": (2, 3), "tv": (2, 3)},
}


@pytest.mark.parametrize("slice_", ["tx", "ty", "xy"])
@pytest.mark.parametrize("datadim", ["2d", "3d", "2.5d"])
@pytest.mark.parametrize("kind", ["l1", "tv_t", "tv_x", "tv"])
def test_model_reg_axes(kind, datadim, slice_):
    want = AXES[datadim if datadim != "2.5d" else ("2.5d-xy" if slice_ == "xy" else "2.5d-t")][kind]
    if want is None:
        with pytest.raises(ValueError, match="--model_reg tv_t"):
            model_reg_axes(kind, datadim, slice_)
    else:
        assert model_reg_axes(kind, datadim, slice_) == want
    with pytest.raises(ValueError, match="--model_reg"):
        model_reg_axes("huber", datadim, slice_)


# ---------------------------------------------------------------- the restatement -------------------------------------------------
H = 1e-6


def _distinct(shape, seed):
    """O(1) float64 values on a grid of spacing 0.01, every one used once and none within 0.0025 of zero: every pairwise difference and
    every |value| exceeds 10 h, so no kink of R lies within h of the point in any coordinate."""
    n = int(np.prod(shape))
    m = ((np.random.RandomState(seed).permutation(n) - n // 2 + 0.25) * 0.01).reshape(shape)
    s = np.sort(m.reshape(-1))
    assert np.diff(s).min() > 10 * H and np.abs(m).min() > 10 * H and np.abs(m).max() < 4.0
    return m


@pytest.mark.parametrize("axes", MR.AXES)
@pytest.mark.parametrize("shape", [(2, 3, 4, 5), (1, 1, 6, 7), (3, 5, 1, 4)])
def test_gradient_equals_central_differences(shape, axes):
    """R is piecewise linear and no kink lies within h: the central difference is the gradient up to the rounding of the two values.
    Each value is a float64 sum of n_terms terms divided by N, off by at most (n_terms + 1) * 2^-53 * sum|terms| / N in all, and moving
    one coordinate by h rounds the (at most 6) terms it enters by 2^-53 * 4 each; the difference of the two is divided by 2 h."""
    m = _distinct(shape, seed=axes)
    R, k, n_terms, total = MR.restate(m, axes)
    grad = k / m.size
    bar = (2 * (n_terms + 1) * 2.0 ** -53 * total / m.size + 2 * 6 * 4 * 2.0 ** -53 / m.size) / (2 * H)
    worst = 0.0
    for i in np.ndindex(*shape):
        p, q = m.copy(), m.copy()
        p[i] += H
        q[i] -= H
        fd = (MR.restate(p, axes)[0] - MR.restate(q, axes)[0]) / (p[i] - q[i])
        worst = max(worst, abs(fd - grad[i]))
    print("axes %d %s: worst |fd - grad| = %.3e, bar %.3e" % (axes, shape, worst, bar))
    assert worst <= bar
    assert (np.abs(grad).max() > 0) == (axes == 0 or any(axes >> a & 1 and shape[a + 1] > 1 for a in range(3)))


def test_ties_follow_sgn_0_is_0():
    m = np.array([[[[1.0, 1.0, 2.0, 0.0, 0.0]]]], dtype=np.float32)
    R, k, n_terms, total = MR.restate(m, 4)
    assert k.reshape(-1).tolist() == [0, -1, 2, -1, 0] and n_terms == 4 and R == 3.0 / 5.0
    R, k, n_terms, _ = MR.restate(m, 0)
    assert k.reshape(-1).tolist() == [1, 1, 1, 0, 0] and n_terms == 5 and R == 4.0 / 5.0
    assert MR.restate(m, 3)[0] == 0.0 and not MR.restate(m, 3)[1].any()          # axes of extent 1 contribute nothing
    ints = MR.integers((3, 9, 6, 5))
    for axes in MR.AXES:
        k = MR.restate(ints, axes)[1]
        assert (k == 0).any() and np.abs(k).max() <= max(1, 2 * bin(axes).count("1"))
    assert np.array_equal(MR.grad32(np.array([[[[3, -2]]]])), np.array([[[[1.5, -1.0]]]], dtype=np.float32))


def test_channels_are_never_differenced_and_every_axis_is_its_own_sum():
    m = MR.generic((3, 4, 5, 6))
    for axes in MR.AXES:
        R, k, n, tot = MR.restate(m, axes)
        per = [MR.restate(m[c:c + 1], axes) for c in range(3)]
        assert np.array_equal(k, np.concatenate([p[1] for p in per])) and n == sum(p[2] for p in per)
        assert abs(tot - sum(p[3] for p in per)) <= 1e-12 * tot
    assert np.array_equal(MR.restate(m, 7)[1], sum(MR.restate(m, 1 << a)[1] for a in range(3)))
    assert MR.dims_to_bits((2, 3, 4), 5) == 7 and MR.dims_to_bits((2, 3), 4) == 6 and MR.dims_to_bits((3,), 4) == 4 and MR.dims_to_bits((), 4) == 0
    assert MR.as_4d(np.zeros((1, 2, 3, 4))).shape == (2, 1, 3, 4) and MR.as_4d(np.zeros((1, 2, 3, 4, 5))).shape == (2, 3, 4, 5)


# ---------------------------------------------------------------- history ---------------------------------------------------------
def test_history_class_with_three_arguments_is_unchanged():
    want = {(False, False, False): u.History, (True, False, False): u.HistoryReg, (False, True, False): u.HistoryHoldout,
            (True, True, False): u.HistoryRegHoldout, (False, False, True): u.HistoryEma, (True, False, True): u.HistoryRegEma,
            (False, True, True): u.HistoryHoldoutEma, (True, True, True): u.HistoryRegHoldoutEma}
    assert len(set(want.values())) == 8
    for key, cls in want.items():
        assert u.history_class(*key) is cls and u.history_class(*key, model_reg=False) is cls
        assert not hasattr(cls(10), "model_reg")


@pytest.mark.parametrize("ema", [False, True])
@pytest.mark.parametrize("holdout", [False, True])
def test_history_with_model_reg(holdout, ema):
    classes = {u.history_class(reg, holdout, ema, model_reg=True) for reg in (False, True)}
    assert len(classes) == 1                                     # always of the HistoryReg family
    cls = classes.pop()
    assert issubclass(cls, u.HistoryReg) and cls is getattr(u, cls.__name__)          # an importable module-level name
    h = cls(100)
    for it in range(2):
        h.append((1.5 + it, 1.0, 0.0, 12.0, 0.9))
        h.append_model_reg(0.25 + it)
        h.lr.append(1e-3)
        if holdout:
            h.append_val(0.5, 3.0)
        if ema:
            h.append_ema(0.4, 4.0, *((0.3, 2.0) if holdout else ()))
    assert len(h) == 2 and h.model_reg == [0.25, 1.25] and h.reg == [0.0, 0.0] and h.df == [1.0, 1.0]
    msg = h.log_message(1)
    assert "MREG = 1.25e+00" in msg and "REG = 0.00e+00" in msg and ("VAL" in msg) == holdout and ("ESNR" in msg) == ema
    assert "MREG" in str(h)
    back = pickle.loads(pickle.dumps(h))
    assert type(back) is cls and vars(back) == vars(h) and back.log_message(0) == h.log_message(0)


# ---------------------------------------------------------------- ABI -------------------------------------------------------------
def test_abi_table_header_exports_and_makefile_name_the_entry_points():
    I, P, Z = C.c_int, C.c_void_p, C.c_size_t
    assert _lib.SIGNATURES["dpi_model_reg_ws_doubles"] == (Z, [Z])
    assert _lib.SIGNATURES["dpi_model_reg"] == (I, [P, I, Z, Z, Z, I, P, P, P, P])
    h = open(os.path.join(ROOT, "include", "dpi_hip.h")).read()
    assert "size_t dpi_model_reg_ws_doubles(size_t n);" in h
    assert "int dpi_model_reg(const float* m, int C, size_t n0, size_t n1, size_t n2, int axes" in h
    assert "model_reg.hip" in open(os.path.join(ROOT, "deep_prior_interpolation_amd", "csrc", "Makefile")).read()
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    exported = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    for name in ("dpi_model_reg_ws_doubles", "dpi_model_reg"):
        assert " T %s\n" % name in exported
    assert _lib.load().dpi_model_reg_ws_doubles(1 << 20) >= 1
