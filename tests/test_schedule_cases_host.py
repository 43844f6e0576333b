"""tests/schedule_cases.py against parameter.py, without a GPU: the table the device test (tests/test_gpu_schedule_matrix.py) runs under the
big-patch stream schedule names every --net, --optimizer and --upsample choice, every row is a command line the parser takes, and every
patch is small enough that only the device test's patch of wants_weight_grad_overlap sends it down that schedule."""
import numpy as np

import schedule_cases as S
from deep_prior_interpolation_amd.parameter import _FLAGS, parse_arguments


def _choices(flag):
    return next(kw["choices"] for flags, kw in _FLAGS if flag in flags)


def _parsed():
    return {r.name: parse_arguments(["--imgdir", "x"] + r.argv + S.COMMON) for r in S.ROWS}


def test_every_net_optimizer_and_upsample_choice_has_a_row():
    args = _parsed().values()
    nets = {a.net for a in args}
    assert not nets & set(S.EXCLUDED_NETS) and all(len(why) > 20 for why in S.EXCLUDED_NETS.values())
    assert nets | set(S.EXCLUDED_NETS) == set(_choices("--net")), "a --net choice without a row in tests/schedule_cases.py"
    assert set(S.EXCLUDED_NETS) <= {"part", "load"}
    assert {a.optimizer for a in args} == set(_choices("--optimizer"))
    # postprocess() spells `linear` as bilinear / trilinear
    named = {"linear" if a.upsample in ("bilinear", "trilinear") else a.upsample for a in args}
    assert named == set(_choices("--upsample"))
    assert {a.datadim for a in args} == set(_choices("--datadim"))
    for net in nets - {"unet"}:                                  # the unet rows are UNet3D's; every other net runs in 3-D and on a 2.5-D slab
        dims = {a.datadim for a in args if a.net == net}
        assert "3d" in dims and "2.5d" in dims, (net, dims)


def test_rows_are_small_short_and_well_formed():
    names = [r.name for r in S.ROWS]
    assert len(set(names)) == len(names)
    parsed = _parsed()
    for r in S.ROWS:
        a = parsed[r.name]
        assert r.mode in ("eager", "graph") and 3 <= a.epochs <= 4
        assert len(r.shape) == {"3d": 4, "2d": 3, "2.5d": 3}[a.datadim] and (a.datadim == "2.5d" or r.shape[-1] == 1)
        if a.datadim == "2.5d":
            assert r.shape[-1] == a.imgchannel
        voxels = int(np.prod(r.shape[:-1]))
        assert 4096 <= voxels < (1 << 20)                        # several workgroups at the finest level, yet under the size rule
        assert set(r.extra) <= {"data", "wavelet", "offsets"}
        assert ("wavelet" in r.extra) == (a.wavelet is not None) and ("offsets" in r.extra) == (a.trace_offsets is not None)
        assert (r.extra.get("data") == "avo") == (a.avo_theta is not None)
        # the branch stream belongs to the 3-D MultiRes-UNet with fusable ResPaths
        assert r.branch == (a.net == "multiunet" and a.datadim == "3d" and a.activation == "LeakyReLU" and a.dropout == 0.0)
        if r.mode == "graph":                                    # what Interpolator._eager_reasons would refuse to capture
            assert a.aa_weight == 0.0 and a.data_forgetting_factor == 0 and a.save_every is None
    graph = [r for r in S.ROWS if r.mode == "graph"]
    assert {parsed[r.name].net for r in graph} == {"multiunet", "attmultiunet"}


def test_the_add_ons_behind_the_net_are_all_named():
    args = list(_parsed().values())
    assert any(a.wavelet and a.wavelet_model == "impedance" and a.trace_offsets and a.trace_interp == "sinc8" for a in args)
    assert any(a.holdout == 0.25 and a.out_ema == 0.9 for a in args)
    assert any(a.optimizer == "psgld" and a.holdout > 0 for a in args) and any(a.optimizer == "sgld" for a in args)
    assert any(a.aa_weight > 0 and a.datadim == "3d" for a in args)
    assert any(a.data_forgetting_factor != 0 for a in args)
    assert {a.loss for a in args} == {"mae", "mse"}
    assert any(a.avo_theta is not None and len(a.avo_theta) == 4 and a.wavelet for a in args)
    assert any(a.precision == "bf16" and a.net == "attmultiunet" for a in args)
    assert any(a.activation != "LeakyReLU" and a.net == "multiunet" and a.datadim == "3d" for a in args)
    unet = [a for a in args if a.net == "unet"]
    assert {(a.upsample, all(f % 16 == 0 for f in a.filters)) for a in unet} == {(m, w) for m in ("deconv", "trilinear") for w in (False, True)}
