"""--wavelet_domain under the big-patch stream schedule: one row per domain in the treatment of tests/test_gpu_schedule_matrix.py.  Behind
the network's last layer, whose weight gradient is the first launch to leave the main stream, now stand both operators as ONE autograd
node (operators.PrestackModelling: two launches each way, in the order of the domain).  The serial and
the streamed schedule are compared bit for bit, both models included, with the late-producer spin on (the helpers and the calibrated spin
are those of the matrix test)."""
import numpy as np
import pytest

import schedule_cases as S
from test_gpu_schedule_matrix import _arguments, _late_producers, _optimise, _patch, _snapshot, differing, sleep_cycles  # noqa: F401

pytestmark = pytest.mark.gpu

PAIR = ["--wavelet", "w.npy", "--moveout", "tau.npy", "--moveout_interp", "cubic"]
ROWS = [
    S._row("prestack-data", S.M3 + PAIR + ["--wavelet_domain", "data"], S.S3, ("wavelet_model", "moveout_model"), branch=True, wavelet=S.RICKER),
    S._row("prestack-model", S.M3 + PAIR + ["--wavelet_domain", "model", "--wavelet_model", "impedance"], S.S3,
           ("wavelet_model", "moveout_model"), branch=True, wavelet=S.RICKER),
]


def _table(shape):
    """The NMO table of the stand-in's mean law on (T, X, Y) (tests/test_moveout_host.py: standin_nmo)."""
    from deep_prior_interpolation_amd.operators import nmo_table
    nt, nx, ny = shape
    off = nt * np.sqrt((np.arange(nx)[:, None] / nx) ** 2 + (np.arange(ny)[None] / ny) ** 2)
    return nmo_table(shape, off, lambda tau: 1.0 / (0.9 - 0.3 * tau / nt))


def _both_models(T):
    snap = _snapshot(T)
    model = T.moveout_model()
    if model is not None:
        snap["moveout_model"] = np.asarray(model)
    return snap


@pytest.mark.parametrize("row", ROWS, ids=[r.name for r in ROWS])
def test_streamed_schedule_reproduces_the_serial_bits(row, tmp_path, monkeypatch, sleep_cycles):  # noqa: F811
    from deep_prior_interpolation_amd import nn as hnn, ops
    args = _arguments(row, tmp_path)
    data = _patch(row, args.gain)
    data["moveout"] = _table(row.shape[:-1])
    assert int(np.prod(row.shape[:-1])) < (1 << 20) and row.mode == "eager"
    try:
        T = _optimise(row, args, data, tmp_path, monkeypatch, streamed=False)
        serial = _both_models(T)
        loss = serial["history.loss"]
        assert len(loss) == args.epochs and np.isfinite(loss).all() and len(set(loss.tolist())) > 1, loss
        fm = T.forward_model
        assert fm.pair is not None and fm.pair.domain == args.wavelet_domain
        assert 0 < fm.live.mean() < 1 and T.mask_.sum().item() > 0
        for name in row.fields:
            assert name in serial, "%s: the run has no %s" % (row.name, name)
        del T, fm
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
            bad = differing(serial, _both_models(T))
            assert not bad, "%s, streamed run %d: not the bits of the serial schedule: %s" % (row.name, k, bad)
            del T
    finally:
        ops.abort_iteration()
        ops.set_weight_grad_overlap(False, in_graph=False)
        ops.set_precision("fp32")
        ops.set_storage("fp32")
