"""Host-side tests of the Langevin samplers (--optimizer sgld | psgld): header / ctypes table / exported symbols, the parser, the sample
count formula and the recorded fixture.  No GPU needed."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE = ["--imgdir", "x", "--datadim", "3d", "--epochs", "101"]
NEW = ("dpi_langevin_multi", "dpi_moments_update")


def _parse(extra=()):
    from deep_prior_interpolation_amd.parameter import parse_arguments
    return parse_arguments(BASE + list(extra))


def test_header_table_and_library_list_the_entry_points():
    from deep_prior_interpolation_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dpi_hip.h")).read(), flags=re.S)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, txt)
        assert name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["dpi_langevin_multi"][1]) == 14 and len(_lib.SIGNATURES["dpi_moments_update"][1]) == 9
    assert _lib.ABI_VERSION == 406              # unchanged: a stale library fails on the unresolved symbols instead
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    exported = set(re.findall(r"\bT (dpi_[a-z0-9_]+)", out))
    assert set(NEW) <= exported
    assert _lib.load().dpi_version() == 406


def test_parser_defaults():
    a = _parse()
    assert a.optimizer == "adam" and a.weight_decay == 0.0 and a.sgld_noise_scale == 0.1
    assert a.psgld_beta == 0.99 and a.psgld_lambda == 1e-8 and a.langevin_temperature is None
    assert a.posterior_burnin == 101 // 2 and a.posterior_thin == 1
    for opt in ("sgld", "psgld"):
        a = _parse(["--optimizer", opt])
        assert a.optimizer == opt and a.posterior_burnin == 50 and a.posterior_thin == 1 and a.langevin_temperature is None
    a = _parse(["--optimizer", "psgld", "--posterior_burnin", "7", "--posterior_thin", "3", "--langevin_temperature", "1", "--weight_decay", "0.5"])
    assert (a.posterior_burnin, a.posterior_thin, a.langevin_temperature, a.weight_decay) == (7, 3, 1.0, 0.5)
    assert _parse(["--optimizer", "sgld", "--posterior_burnin", "0", "--langevin_temperature", "0"]).posterior_burnin == 0


@pytest.mark.parametrize("extra", [["--weight_decay", "-1"], ["--sgld_noise_scale", "-0.1"], ["--psgld_beta", "-0.5"], ["--psgld_beta", "1.5"],
                                   ["--psgld_lambda=-1e-8"], ["--langevin_temperature", "-1"], ["--posterior_burnin", "-1"],
                                   ["--posterior_thin", "0"]])
def test_parser_refuses_out_of_range_values(extra):
    with pytest.raises(ValueError):
        _parse(["--optimizer", "psgld"] + extra)


@pytest.mark.parametrize("extra", [["--posterior_burnin", "5"], ["--posterior_thin", "1"], ["--langevin_temperature", "1"]])
def test_sampler_only_flags_need_a_sampler(extra):
    with pytest.raises(ValueError, match="sampler"):
        _parse(extra)
    with pytest.raises(ValueError, match="sampler"):
        _parse(["--optimizer", "adam"] + extra)


def test_parser_refuses_an_unknown_optimizer():
    with pytest.raises(SystemExit):
        _parse(["--optimizer", "sgd"])


def test_main_pocs_refuses_a_sampler():
    from deep_prior_interpolation_amd import main_pocs
    a = _parse(["--optimizer", "sgld"])
    with pytest.raises(ValueError, match="main_pocs does not support --optimizer"):
        main_pocs.Interpolator(a, "/tmp", device="cpu")


def test_fused_langevin_refuses_what_is_out_of_scope():
    import torch
    from deep_prior_interpolation_amd.optim import FusedLangevin
    p = [torch.nn.Parameter(torch.zeros(3))]
    for kw in (dict(momentum=0.9), dict(dampening=0.1), dict(nesterov=True), dict(centered=True), dict(temperature=-1.0), dict(noise="numpy")):
        with pytest.raises(ValueError):
            FusedLangevin(p, "psgld", 1e-2, **kw)
    with pytest.raises(ValueError):
        FusedLangevin(p, "sgd", 1e-2)


@pytest.mark.parametrize("iterations, burn_in, thin, want", [
    (0, 0, 1, 0), (1, 0, 1, 1), (1, 1, 1, 0), (12, 4, 2, 4), (13, 4, 2, 5), (10, 5, 1, 5), (10, 0, 5, 2), (11, 0, 5, 3),
    (3, 50, 1, 0),          # early stop before the burn-in
    (64 * 2 + 3, 3, 2, 64), (100, 99, 7, 1)])
def test_sample_count(iterations, burn_in, thin, want):
    from deep_prior_interpolation_amd.optim import posterior_sample_count
    assert posterior_sample_count(iterations, burn_in, thin) == want
    assert want == sum(1 for it in range(iterations) if it >= burn_in and (it - burn_in) % thin == 0)      # the kernel's rule, restated


def test_sample_count_refuses_bad_arguments():
    from deep_prior_interpolation_amd.optim import posterior_sample_count
    with pytest.raises(ValueError):
        posterior_sample_count(10, 0, 0)
    with pytest.raises(ValueError):
        posterior_sample_count(10, -1, 1)


def test_fixture_has_the_four_cases():
    f = np.load(os.path.join(ROOT, "tests", "golden", "langevin.npz"))
    assert list(f["cases"]) == ["sgld", "sgld_wd", "psgld", "psgld_wd"]
    shapes = [tuple(s) for s in json.loads(str(f["shapes"]))]
    assert [int(np.prod(s)) for s in shapes] == [1, 3, 1025, 405]
    for case in f["cases"]:
        h = json.loads(str(f[case + "/hyper"]))
        assert h["kind"] == case.split("_")[0] and (h["weight_decay"] != 0) == case.endswith("_wd")
        assert f[case + "/seeds"].shape == (4,)
        for i, s in enumerate(shapes):
            assert f["%s/p%d_init" % (case, i)].shape == s
            for step in range(4):
                names = ["g", "xi", "p"] + (["V"] if h["kind"] == "psgld" else [])
                arrs = [f["%s/%s%d_%d" % (case, k, step, i)] for k in names]
                assert all(a.shape == s and a.dtype == np.float32 and np.isfinite(a).all() for a in arrs)
            assert not np.array_equal(f["%s/p3_%d" % (case, i)], f["%s/p%d_init" % (case, i)])
