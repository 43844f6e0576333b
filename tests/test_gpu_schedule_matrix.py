"""Every net and loss add-on under the big-patch stream schedule: the rows of tests/schedule_cases.py, each optimised under the serial
schedule (ops.sched.join_at = "node", no branch stream) and under the streamed one (weight gradients on the two side streams, joined once
per step, the ResPath half of a level join on the branch stream), compared BIT FOR BIT — the same kernels on the same operands in the same
per-tensor order, so there is no tolerance to choose.  The patches are small; Interpolator.wants_weight_grad_overlap is patched to answer
as it does from 2^20 voxels on, as in test_gpu_nets.test_branch_stream_schedule_is_bit_identical_to_the_serial_one, beside which this stands.

Late producers instead of luck.  On a small patch the side and branch streams are idle and finish long before anybody reads what they
wrote, so a missing wait would rarely show.  In the streamed eager runs every hand-over to a side stream (Schedule.side_stream) and to the
branch stream (Schedule.branch) is followed by a spin kernel on that stream, queued behind the main stream's work of that moment: every
side-stream dw and every branch-stream ResPath result is written DELAY_MS late.  A consumer that does not wait reads the memory before it is
written, an operand handed back to the allocator before the join is overwritten before it is read: either changes the bits.

Calibration (MI355X, HIP events around torch.cuda._sleep, which busy-waits on this runtime): see DELAY_MS below."""
import os

import numpy as np
import pytest
import torch

import schedule_cases as S

pytestmark = pytest.mark.gpu

# torch.cuda._sleep(n) on the MI355X, HIP events around it: 1e6 / 1e7 / 1e8 cycles last 0.42 / 4.18 / 41.84 ms, i.e. 2.39e6 cycles per
# millisecond (the spin counts shader clocks of ~2.4 GHz), and 4 779 406 cycles lasted 2.00 ms.  The rate is not hard-coded: `sleep_cycles`
# measures it again in every session and checks the spin it hands out.
# The longest single convolution launch of one iteration (ops.KernelTimer, every row's shape, iteration 0 with its first-launch costs
# included): forward 2.99 ms in the attmultiunet-3d-bf16 row and 1.83 ms in the first fp32 row of the session, 0.53 ms in the
# rows of the same net after it; backward-weight 0.65 ms, backward-data 0.10 ms at most.  DELAY_MS is above all of them and above the 1 ms
# floor.  The widest rows hand over 38 weight gradients and 6 branch sections per iteration: 44 x 3 ms x 4 iterations = 0.53 s of
# added delay per run if nothing overlapped (the two side streams spin side by side: about half of that in practice).
DELAY_MS = 3.0


@pytest.fixture(scope="module")
def sleep_cycles():
    """Cycles torch.cuda._sleep needs for DELAY_MS, from two timed spins of this session (their difference removes the launch overhead)
    — and the proof that the spin of that length really lasts DELAY_MS on this device."""
    def spin_ms(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        torch.cuda._sleep(n)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)
    spin_ms(20_000_000)                                        # loads the kernel; a few milliseconds for the shader clock to settle
    lo, hi = 1_000_000, 11_000_000
    per_ms = (hi - lo) / max(spin_ms(hi) - spin_ms(lo), 1e-6)
    cycles = int(np.ceil(DELAY_MS * per_ms))
    got = spin_ms(cycles)
    for _ in range(3):                                         # the clock rose since the two spins: lengthen once or twice, then give up
        if got >= DELAY_MS:
            break
        cycles = int(np.ceil(cycles * min(2.0, 1.05 * DELAY_MS / max(got, 1e-3))))
        got = spin_ms(cycles)
    print("torch.cuda._sleep: %.0f cycles per ms; %d cycles for %.1f ms last %.2f ms" % (per_ms, cycles, DELAY_MS, got))
    assert DELAY_MS <= got <= 5.0 * DELAY_MS, "torch.cuda._sleep(%d) lasted %.3f ms: it does not busy-wait as calibrated" % (cycles, got)
    return cycles


def _patch(row, gain):
    from deep_prior_interpolation_amd import utils as u
    shape = row.shape
    if row.extra.get("data") == "avo":
        vol = u.avo_gathers(shape, S.THETA, vsvp=0.5, seed=0)
    elif len(shape) == 4:
        vol = u.hyperbolic_volume(shape[:3], seed=4)[..., None]
    else:
        vol = u.hyperbolic_volume(shape, seed=4)               # (T, X, sections)
    traces = u.random_trace_mask(shape[:3] if len(shape) == 4 else shape[:2] + (1,), 0.6, seed=5)          # constant along t
    if len(shape) == 4:
        traces = traces[..., None]
    data = {"image": vol.astype(np.float64) * gain, "mask": np.broadcast_to(traces, vol.shape).astype(np.float64).copy(), "name": "0"}
    if "offsets" in row.extra:
        data["offsets"] = np.random.RandomState(row.extra["offsets"]).uniform(-0.5, 0.5, shape[1:3] + (2,)).astype(np.float32)
    return data


def _arguments(row, imgdir):
    from deep_prior_interpolation_amd import utils as u
    from deep_prior_interpolation_amd.parameter import parse_arguments
    if "wavelet" in row.extra:
        np.save(os.path.join(imgdir, "w.npy"), u.ricker(*row.extra["wavelet"]))
    return parse_arguments(["--imgdir", str(imgdir)] + row.argv + S.COMMON)


def _optimise(row, args, data, outdir, monkeypatch, streamed):
    """One run, built as the existing schedule test builds it.  streamed=False: per-node joins and no branch stream; a graph row's serial
    run also keeps the weight gradients on the main stream (the captured iteration of a small patch)."""
    from deep_prior_interpolation_amd import ops, utils as u
    from deep_prior_interpolation_amd.main import Interpolator
    monkeypatch.setattr(ops.sched, "join_at", "step" if streamed else "node")
    monkeypatch.setattr(ops.sched, "branch_streams", streamed)
    u.set_seed(0)
    T = Interpolator(args, str(outdir))
    T.load_data(data)
    T.begin_patch(0)
    T.build_model()
    T.build_input()
    T.build_regularizer()
    overlap = streamed or row.mode == "eager"
    monkeypatch.setattr(T, "wants_weight_grad_overlap", lambda: overlap)       # the schedule of the >= 2^20-voxel patches on a small one
    T.optimize(verbose=False, mode=row.mode, check_every=2)
    torch.cuda.synchronize()
    return T


def _snapshot(T):
    """Everything the run produced, as host arrays (None entries dropped)."""
    cpu = lambda t: t.detach().cpu().numpy().copy()
    out = {"history." + k: np.asarray(v) for k, v in vars(T.history).items() if isinstance(v, (list, np.ndarray))}
    out["out_best"] = np.array(T.out_best)
    out["best_iter"] = np.asarray(-1 if T.best_iter is None else T.best_iter)
    out["iterations"] = np.asarray(T.iiter)
    out.update(("state." + k, cpu(v)) for k, v in T.net.state_dict().items())
    out.update(("optimizer." + k, cpu(getattr(T.optimizer, k))) for k in ("exp_avg", "exp_avg_sq", "step_lr"))
    products = {"wavelet_model": T.wavelet_model(), "avo_model": T.avo_model(), "posterior_std": T.posterior_std,
                "output_selected": T.output_selected, "posterior_snr": T.posterior_snr, "posterior_val_snr": T.posterior_val_snr,
                "ema_best": None if (T.out_ema <= 0.0 or T._ema_best is None) else cpu(T._ema_best)}
    out.update((k, np.asarray(v)) for k, v in products.items() if v is not None)
    return out


def differing(ref, got):
    """Names of the entries of two snapshots that are not the same bits (missing ones included)."""
    bad = [k for k in sorted(set(ref) | set(got)) if k not in ref or k not in got]
    for k in sorted(set(ref) & set(got)):
        a, b = ref[k], got[k]
        if a.shape != b.shape or a.dtype != b.dtype or a.tobytes() != b.tobytes():
            bad.append(k)
    return bad


def _late_producers(monkeypatch, cycles, calls):
    """Count the hand-overs to the side and branch streams and, with cycles > 0, make what those streams produce late (module docstring)."""
    from deep_prior_interpolation_amd import ops
    sched = ops.sched
    side_stream, branch = sched.side_stream, sched.branch

    def late_side_stream():
        st = side_stream()
        calls["side"] += 1
        if cycles:
            st.wait_stream(torch.cuda.current_stream())        # as the caller is about to: the spin starts where the main stream stands
            with torch.cuda.stream(st):
                torch.cuda._sleep(cycles)
        return st

    def late_branch(kind, *tensors):
        ctx = branch(kind, *tensors)                           # has ordered the branch stream behind the current one
        calls["branch"] += 1
        if cycles:
            with torch.cuda.stream(sched._branch_streams[(torch.cuda.current_device(), kind)]):
                torch.cuda._sleep(cycles)
        return ctx
    monkeypatch.setattr(sched, "side_stream", late_side_stream)
    monkeypatch.setattr(sched, "branch", late_branch)


@pytest.mark.parametrize("row", S.ROWS, ids=[r.name for r in S.ROWS])
def test_streamed_schedule_reproduces_the_serial_bits(row, tmp_path, monkeypatch, sleep_cycles):
    from deep_prior_interpolation_amd import nn as hnn, ops
    args = _arguments(row, tmp_path)
    data = _patch(row, args.gain)
    assert int(np.prod(row.shape[:-1])) < (1 << 20)            # the size rule alone would keep the serial schedule
    graph = row.mode == "graph"
    try:
        T = _optimise(row, args, data, tmp_path, monkeypatch, streamed=False)
        serial = _snapshot(T)
        loss = serial["history.loss"]
        assert len(loss) == args.epochs and np.isfinite(loss).all() and len(set(loss.tolist())) > 1, loss
        for name in row.fields:
            assert name in serial or "history." + name in serial, "%s: the run has no %s" % (row.name, name)
        if args.precision == "bf16" and args.net != "multiunet":
            assert not T.storage_bf16_ok()                     # operand rounding only: the tensors stay fp32
        del T
        calls = {"side": 0, "branch": 0}
        _late_producers(monkeypatch, 0 if graph else sleep_cycles, calls)      # no delay inside a captured iteration: the rows only count
        for k in range(1 if graph else 2):
            calls["side"] = calls["branch"] = 0
            T = _optimise(row, args, data, tmp_path, monkeypatch, streamed=True)
            sched = ops.sched
            assert sched.overlap and sched.overlap_in_graph == graph
            assert sched.deferred == [] and not sched.in_iteration and not sched.side_keep and not sched.side_used
            convs = sum(1 for m in T.net.modules() if isinstance(m, (hnn.Conv2d, hnn.Conv3d)) and m.weight.grad is not None)
            assert convs > 0 and sched.side_rr == convs, (sched.side_rr, convs)
            # eager: every iteration hands every weight gradient over; graph: iteration 0 and the captured one
            assert calls["side"] == convs * (2 if graph else args.epochs), (calls, convs)
            assert (calls["branch"] > 0) == row.branch, calls
            bad = differing(serial, _snapshot(T))
            assert not bad, "%s, streamed run %d: not the bits of the serial schedule: %s" % (row.name, k, bad)
            del T
    finally:
        ops.abort_iteration()
        ops.set_weight_grad_overlap(False, in_graph=False)
        ops.set_precision("fp32")
        ops.set_storage("fp32")


@pytest.mark.parametrize("datadim,shape", [("3d", (128, 128, 64, 1)), ("2.5d", (1024, 1024, 3))], ids=["3d", "25d"])
def test_net_part_keeps_the_serial_schedule_at_size(datadim, shape, tmp_path, monkeypatch):
    """--net part on a patch of 2^20 voxels: the size rule says "streams", the net's rule (every `down` convolution is used twice, autograd
    accumulates its weight gradient on the main stream) must win; tests/test_gpu_partial.py asserts the same at 32^3, where the size rule
    alone already says no.  And what optimize(mode="auto") does with such a patch: without the streams a big patch is eager only when
    the run is short — from 1000 iterations on it is captured, as its docstring states.  Data only: no net is built, no iteration runs."""
    from deep_prior_interpolation_amd import ops
    from deep_prior_interpolation_amd.main import Interpolator
    from deep_prior_interpolation_amd.parameter import parse_arguments
    extra = ["--datadim", datadim] + (["--slice", "tx", "--imgchannel", "3"] if datadim == "2.5d" else [])
    chosen = {}
    for epochs, net in ((2001, "part"), (999, "part"), (2001, "multiunet")):
        a = parse_arguments(["--imgdir", "x", "--net", net, "--gpu", "0", "--epochs", str(epochs)] + extra)
        T = Interpolator(a, str(tmp_path))
        T.load_data({"image": np.zeros(shape), "mask": np.ones(shape), "name": "0"})
        assert int(np.prod(T.img.shape[:-1])) >= (1 << 20) and T._eager_reasons() == ["size"]
        assert T.wants_weight_grad_overlap() == (net != "part")
        ran = []

        class Optimizer:
            param_groups = [{"lr": a.lr}]

            def zero_grad(self):
                ran.append("eager")
                raise StopIteration                             # the eager loop was entered: that is all this test asks

            def step(self):
                raise AssertionError("no iteration may run")
        monkeypatch.setattr(T, "make_optimizer", Optimizer)
        monkeypatch.setattr(T, "_optimize_graph", lambda verbose, check_every: ran.append("graph"))
        try:
            T.optimize(verbose=False, mode="auto")
        except StopIteration:
            pass
        finally:
            overlap = ops.sched.overlap
            ops.set_weight_grad_overlap(False, in_graph=False)
        assert overlap == (net != "part")                      # what optimize() switched on for the patch
        chosen[(net, epochs)] = ran
    assert chosen == {("part", 2001): ["graph"], ("part", 999): ["eager"], ("multiunet", 2001): ["eager"]}, chosen
