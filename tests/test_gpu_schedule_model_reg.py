"""--model_reg under the big-patch stream schedule: one row in the treatment of tests/test_gpu_schedule_matrix.py.  With the flag the
network's output has two gradient consumers — the misfit behind the forward model and the penalty — whose sum feeds the last layer, whose
weight gradient is the first launch to leave the main stream.  The serial and the streamed schedule are compared bit for bit, with the
late-producer spin on (the helpers and the calibrated spin are those of the matrix test)."""
import numpy as np
import pytest

import schedule_cases as S
from test_gpu_schedule_matrix import _arguments, _late_producers, _optimise, _patch, _snapshot, differing, sleep_cycles  # noqa: F401

pytestmark = pytest.mark.gpu

ROWS = [
    S._row("model_reg-tv", S.M3 + ["--model_reg", "tv", "--model_reg_weight", "0.5"], S.S3, ("model_reg", "reg"), branch=True),
    S._row("model_reg-l1-wavelet", S.M3 + ["--wavelet", "w.npy", "--model_reg", "l1", "--model_reg_weight", "0.5"], S.S3,
           ("model_reg", "wavelet_model"), branch=True, wavelet=S.RICKER),
]


@pytest.mark.parametrize("row", ROWS, ids=[r.name for r in ROWS])
def test_streamed_schedule_reproduces_the_serial_bits(row, tmp_path, monkeypatch, sleep_cycles):  # noqa: F811
    from deep_prior_interpolation_amd import nn as hnn, ops
    args = _arguments(row, tmp_path)
    data = _patch(row, args.gain)
    assert int(np.prod(row.shape[:-1])) < (1 << 20) and row.mode == "eager"
    try:
        T = _optimise(row, args, data, tmp_path, monkeypatch, streamed=False)
        serial = _snapshot(T)
        loss, mreg = serial["history.loss"], serial["history.model_reg"]
        assert len(loss) == args.epochs and np.isfinite(loss).all() and len(set(loss.tolist())) > 1, loss
        assert len(mreg) == args.epochs and (mreg > 0).all() and not T.graph_capable()
        for name in row.fields:
            assert name in serial or "history." + name in serial, "%s: the run has no %s" % (row.name, name)
        del T
        calls = {"side": 0, "branch": 0}
        _late_producers(monkeypatch, sleep_cycles, calls)
        for k in range(2):
            calls["side"] = calls["branch"] = 0
            T = _optimise(row, args, data, tmp_path, monkeypatch, streamed=True)
            sched = ops.sched
            assert sched.overlap and not sched.overlap_in_graph
            assert sched.deferred == [] and not sched.in_iteration and not sched.side_keep and not sched.side_used
            convs = sum(1 for m in T.net.modules() if isinstance(m, (hnn.Conv2d, hnn.Conv3d)) and m.weight.grad is not None)
            assert convs > 0 and sched.side_rr == convs, (sched.side_rr, convs)
            assert calls["side"] == convs * args.epochs, (calls, convs)
            assert calls["branch"] > 0, calls
            bad = differing(serial, _snapshot(T))
            assert not bad, "%s, streamed run %d: not the bits of the serial schedule: %s" % (row.name, k, bad)
            del T
    finally:
        ops.abort_iteration()
        ops.set_weight_grad_overlap(False, in_graph=False)
        ops.set_precision("fp32")
        ops.set_storage("fp32")
