"""What a convolution launch may touch, on a device: the rows of tests/conv_contract_cases.py through the C ABI with every buffer owned by
the test — exactly as large as the sizing query says, pre-filled with NaN where the launch must write, and inside guard bands
(tests/gpu_guard.py).  DESIGN.md §1: "what Python allocates cannot drift from what a launch writes".

 - outputs (y, dx) are channel slices [c0, c0 + C) of a larger channel-planar buffer, as the product's concat buffers hand them over:
   one element past the end is the neighbouring layer's activation.  With an odd voxel count the slice starts 4-byte (bf16: 2-byte) aligned;
 - `stat_partials` holds exactly dpi_conv_fwd_stat_blocks * Cout * 2 doubles: a row the kernel does not write stays NaN, a row too many
   lands in the band;
 - workspaces hold exactly dpi_conv_*_ws_floats floats (NULL and 0 where the query says 0);
 - launch variants that are chosen from a pointer's address run at the natural (256-byte-aligned) address and with the deciding pointer
   moved by the smallest element offset that flips the choice (ADDRESS_CASES; the input offsets of the table rows).  An offset case is
   launched only where the code that takes it is written for that alignment: buffer loads of whole dwords (fp32) or of single 16-bit
   elements (bf16 rows of class 2), element-wise stores, and — the VALU and 1x1x1 backward-weight kernels, the plan's fall-back for views
   that are not 16-byte aligned — vector loads only where the tensor's base allows them (dpi_vec4_base in csrc/common.h), element-wise
   loads otherwise.  Where an entry point refuses an alignment (REFUSALS) the error code, the message and the untouched buffers are
   asserted instead.

The only accuracy reference is the fp64 oracle (oracle/dpi_oracle.py on the chained input); statistics are compared with float64 sums of
the output the GPU stored.  No bar is new: 2e-6 norm-wise for fp32 outputs and 5e-6 for weight gradients (tests/test_gpu_ops.py), half a
bf16 ulp for bf16 outputs of bf16-representable operands, one ulp after two stores, 4e-3 norm-wise where the bf16 arithmetic mode rounds
a chained operand, and rtol 1e-9 / atol 1e-7 * max_c sum|y_c| for the statistics (tests/test_gpu_bf16_storage.py).  The kernels are never
a reference for each other: the two runs of an address-chosen pair are different kernels and are not compared.

A launch that returns DPI_E_LAUNCH, or a device fault at the synchronisation after a launch, ends the WHOLE pytest session with exit
status 3 (pytest.exit), files collected after this one included: nothing more is started on a device that may have faulted.  A run that
ends that way is truncated, not passed.

The knobs a row changes are put back to the values the library started with (conv_contract_cases.knob_defaults, which follows the
DPI_* variables the library itself reads)."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

from oracle import dpi_oracle as O

import conv_contract_cases as T
from gpu_guard import guard, guard_slice
from test_gpu_bf16_storage import half_ulp_ok

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
F32 = torch.float32
DEFAULTS = T.knob_defaults(os.environ)
IO_X, IO_Y, IO_DY, IO_DX = 1, 2, 4, 8


def _rows(launcher):
    rows = [c for c in T.CASES if c.launcher == launcher]
    return pytest.mark.parametrize("case", rows, ids=[T.case_id(c) for c in rows])


@pytest.fixture(scope="module")
def lib():
    from deep_prior_interpolation_amd import _lib
    return _lib


class knobs:
    """dpi_set_option keys of one row, restored on the way out; ops.py memoises workspace sizes per descriptor, so its cache is dropped
    after every change."""

    def __init__(self, lib, options):
        self.lib, self.options = lib, options

    def _set(self, options):
        from deep_prior_interpolation_amd import ops
        L = self.lib.load()
        for key, value in options.items():
            L.set_option(key, value)
        ops.reset_ws_cache()

    def __enter__(self):
        self._set(self.options)

    def __exit__(self, *exc):
        self._set({k: DEFAULTS[k] for k in self.options})


def rel(a, b):
    a, b = a.detach().double().cpu().reshape(-1), b.detach().double().cpu().reshape(-1)
    return float((a - b).norm() / (b.norm() + 1e-300))


def desc_of(lib, c, cout=None, k=None):
    k = c.k if k is None else k
    return lib.ConvDesc(c.cin, c.cout if cout is None else cout, c.shape[0], c.shape[1], c.shape[2], k, c.kd if k == c.k else 1, c.stride, c.precision, c.io)


def out_shape(c):
    D, H, W = c.shape
    o = lambda n, k, s: (n + 2 * ((k - 1) // 2) - k) // s + 1
    return (o(D, c.kd, c.stride if c.kd > 1 else 1), o(H, c.k, c.stride), o(W, c.k, c.stride))


def _values(shape, gen, exact_bf16, scale=1.0):
    v = torch.randn(shape, generator=gen) * scale
    return v.to(BF).float() if exact_bf16 else v


def _conv64(x, w, b, c):
    """fp64 oracle on [C][D][H][W] / [Cout][Cin][kd][k][k]; 2-D layers (kd = 1 on D = 1) through the oracle's conv2d."""
    if c.kd == 1 and w.shape[-1] == 3:
        return O.conv_nd(x[None, :, 0], w[:, :, 0], b, c.stride)[0][:, None]
    return O.conv_nd(x[None], w, b, c.stride)[0]


@functools.lru_cache(maxsize=None)
def _problem(idx):
    """Operands and fp64 oracle results of row `idx`, computed once and shared by every test of the row (nothing here is modified later).
    Tensors that live in HBM as bf16, and every operand of the bf16 arithmetic mode, hold bf16-representable values: products are then
    exact and only the rounding of the store and the fp32 accumulation separate the GPU from the oracle."""
    c = T.CASES[idx]
    gen = torch.Generator().manual_seed(1000 + idx)
    exact = c.io != 0 or c.precision == 1
    cout = c.cout[0] if isinstance(c.cout, tuple) else c.cout
    taps = c.kd * c.k * c.k
    p = {"x": _values((c.cin,) + tuple(c.shape), gen, exact), "w": _values((cout, c.cin, c.kd, c.k, c.k), gen, exact, 1.0 / np.sqrt(c.cin * taps)),
         "b": _values((cout,), gen, exact), "dy": _values((cout,) + out_shape(c), gen, exact)}
    cin = c.cin
    p["chain"] = torch.stack([torch.rand(cin, generator=gen) + 0.5, torch.randn(cin, generator=gen) * 0.3, torch.full((cin,), 0.2),
                              torch.rand(cin, generator=gen) + 0.5, torch.randn(cin, generator=gen) * 0.1], 1).contiguous()
    ps, pb, sl, qs, qb = (p["chain"][:, i].double().view(cin, 1, 1, 1) for i in range(5))
    v = ps * p["x"].double() + pb
    tx = qs * torch.where(v > 0, v, v * sl) + qb
    w64, b64, dy64 = p["w"].double(), p["b"].double(), p["dy"].double()
    if c.launcher == "fwd":
        p["y_chained"], p["y_plain"] = _conv64(tx, w64, b64, c), _conv64(p["x"].double(), w64, b64, c)
    elif c.launcher == "bwd_weight":
        runs = [("dw_plain", p["x"].double()), ("dw_chained", tx)]
        if c.precision == 1:                                 # the bf16 kernels round T(x) to bf16 as an operand: the oracle on that operand,
            f = [p["chain"][:, i].view(cin, 1, 1, 1) for i in range(5)]        # T(x) in fp32 as apply_chain computes it (no contraction)
            v32 = f[0] * p["x"] + f[1]
            runs.append(("dw_chained_rounded", (f[3] * torch.where(v32 > 0, v32, v32 * f[2]) + f[4]).to(BF).double()))
        for name, xin in runs:
            wr = w64.clone().requires_grad_(True)
            (_conv64(xin, wr, None, c) * dy64).sum().backward()
            p[name] = wr.grad
    else:
        xr = torch.zeros((cin,) + tuple(c.shape), dtype=torch.float64, requires_grad=True)
        loss = (_conv64(xr, w64, None, c) * dy64).sum()
        if c.launcher == "bwd_data_dual":
            c1 = c.cout[1]
            p["w1"] = _values((c1, cin, 1, 1, 1), gen, exact, 1.0 / np.sqrt(c1))
            p["dy1"] = _values((c1,) + tuple(c.shape), gen, exact)
            loss = loss + (O.conv_nd(xr[None], p["w1"].double(), None, 1)[0] * p["dy1"].double()).sum()
        loss.backward()
        p["dx"] = xr.grad
        p["base"] = _values((cin,) + tuple(c.shape), gen, (c.io & IO_DX) != 0)
    return p


def _dt(c, bit):
    return BF if c.io & bit else F32


def _out_guard(C_, V, dtype, off, fill=None):
    """The output tensor of a launch: a channel slice (off = None), or a buffer of its own moved by `off` elements (address-chosen variants)."""
    if off is None:
        return guard_slice(C_, V, dtype, DEV, fill=fill)
    return guard(C_ * V, dtype, DEV, fill=fill, offset=off, shape=(C_, V))


def _check_out(got, ref, c, what, rounded_operand=False, slack=0.503):
    """got: the stored output [C][V]; ref: the fp64 oracle.  Every element written, and at the project's bar for this kind of launch."""
    assert bool(torch.isfinite(got).all()), "%s: %d elements were not written (NaN pre-fill left)" % (what, int((~torch.isfinite(got)).sum()))
    ref = ref.reshape(got.shape)
    if rounded_operand:
        assert rel(got, ref) < 4e-3, (what, rel(got, ref))          # bf16 arithmetic mode: T(x) is rounded to bf16 as an operand
    elif got.dtype == BF:
        half_ulp_ok(got, ref, what, slack=slack)
    else:
        assert rel(got, ref) < 2e-6, (what, rel(got, ref))


def run_fwd(lib, c, idx, x_off=0, y_off=None, chained=True, partials=True, workspace=True):
    L = lib.load()
    p = _problem(idx)
    d = desc_of(lib, c)
    Vo = int(np.prod(out_shape(c)))
    nblk, fws = L.dpi_conv_fwd_stat_blocks(C.byref(d)), L.dpi_conv_fwd_ws_floats(C.byref(d))
    assert nblk > 0
    xg = guard(p["x"].numel(), _dt(c, IO_X), DEV, fill=p["x"], offset=x_off)
    yg = _out_guard(c.cout, Vo, _dt(c, IO_Y), y_off)
    pg = guard(nblk * c.cout * 2, torch.float64, DEV) if partials else None
    wg = guard(fws, F32, DEV) if workspace and fws else None
    w, b, chain = p["w"].to(DEV), p["b"].to(DEV), p["chain"].to(DEV) if chained else None
    guards = [("x", xg), ("y", yg), ("stat_partials", pg), ("ws", wg)]
    call = lambda: L.dpi_conv_fwd_ws(C.byref(d), xg.payload.data_ptr(), lib.ptr(chain), lib.ptr(w), lib.ptr(b), yg.payload.data_ptr(),
                                     pg.payload.data_ptr() if pg else None, wg.payload.data_ptr() if wg else None, fws if wg else 0, lib.stream())
    return call, guards, yg, pg, nblk


def _launch(lib, rc, what):
    """The launch must succeed.  A launch error means the device may be in a faulted state: the session ends here instead of starting
    further work on it."""
    if rc == -2:                                                     # DPI_E_LAUNCH
        pytest.exit("%s: %s" % (what, lib.load().dpi_last_error().decode()), returncode=3)
    lib.check(rc, what)


def _check_guards(guards, what):
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:                                        # a device fault: nothing more is started on this GPU
        pytest.exit("%s: %s" % (what, e), returncode=3)
    for name, g in guards:
        if g is not None:
            g.check("%s: %s" % (what, name))


@_rows("fwd")
def test_forward_writes_exactly_what_it_declares(lib, case):
    """y = conv(T(x), w) + bias into a NaN channel slice, partial rows and workspace sized exactly from the queries: bands intact, every
    declared partial written, every output element written, y at the oracle bar, row sums of the partials = float64 sums of the stored y.
    Then the launch an ABI-300 caller makes (no statistics, no workspace, no chain), and the row's input offsets."""
    idx = T.CASES.index(case)
    p = _problem(idx)
    with knobs(lib, case.options):
        for x_off in (0,) + case.offsets:
            what = "%s x+%d" % (T.case_id(case), x_off)
            call, guards, yg, pg, nblk = run_fwd(lib, case, idx, x_off=x_off)
            _launch(lib, call(), what)
            _check_guards(guards, what)
            part = pg.payload.view(nblk, case.cout, 2)
            assert bool(torch.isfinite(part).all()), "%s: %d of %d declared partial rows were not written" % (
                what, int((~torch.isfinite(part).all(2).all(1)).sum()), nblk)
            _check_out(yg.payload, p["y_chained"], case, what + " y", rounded_operand=case.precision == 1 and case.reaches["fwd"] == T.SCRATCH)
            ys = yg.payload.double().cpu()
            s = part.sum(0).cpu()
            np.testing.assert_allclose(s[:, 0].numpy(), ys.sum(1).numpy(), rtol=1e-9, atol=1e-7 * float(ys.abs().sum(1).max()), err_msg=what)
            np.testing.assert_allclose(s[:, 1].numpy(), (ys * ys).sum(1).numpy(), rtol=1e-9, err_msg=what)
        what = T.case_id(case) + " (no statistics, no workspace, no chain)"
        call, guards, yg, _, _ = run_fwd(lib, case, idx, chained=False, partials=False, workspace=False)
        _launch(lib, call(), what)
        _check_guards(guards, what)
        _check_out(yg.payload, p["y_plain"], case, what + " y")


def run_bwd_data(lib, c, idx, accumulate, dy_off=0, dx_off=None, workspace=True, dy1_off=0):
    L = lib.load()
    p = _problem(idx)
    dual = c.launcher == "bwd_data_dual"
    d = desc_of(lib, c, cout=c.cout[0] if dual else None)
    V, bws = int(np.prod(c.shape)), L.dpi_conv_bwd_data_ws_floats(C.byref(d))
    dyg = guard(p["dy"].numel(), _dt(c, IO_DY), DEV, fill=p["dy"], offset=dy_off)
    dxg = _out_guard(c.cin, V, _dt(c, IO_DX), dx_off, fill=p["base"] if accumulate else None)
    wg = guard(bws, F32, DEV) if workspace and bws else None
    w = p["w"].to(DEV)
    guards = [("dy", dyg), ("dx", dxg), ("ws", wg)]
    ws_args = (wg.payload.data_ptr() if wg else None, bws if wg else 0, lib.stream())
    if dual:
        d1 = desc_of(lib, c, cout=c.cout[1], k=1)
        dy1g = guard(p["dy1"].numel(), _dt(c, IO_DY), DEV, fill=p["dy1"], offset=dy1_off)
        w1 = p["w1"].to(DEV)
        guards.append(("dy1", dy1g))
        call = lambda: L.dpi_conv_bwd_data_dual(C.byref(d), dyg.payload.data_ptr(), lib.ptr(w), C.byref(d1), dy1g.payload.data_ptr(), lib.ptr(w1),
                                                dxg.payload.data_ptr(), accumulate, *ws_args)
    else:
        call = lambda: L.dpi_conv_bwd_data_ws(C.byref(d), dyg.payload.data_ptr(), lib.ptr(w), dxg.payload.data_ptr(), accumulate, *ws_args)
    return call, guards, dxg


def _bwd_data_row(lib, case, slack):
    idx = T.CASES.index(case)
    p = _problem(idx)
    with knobs(lib, case.options):
        runs = [(off, acc, True) for off in (0,) + case.offsets for acc in (0, 1)] + [(0, 0, False)]
        for dy_off, acc, workspace in runs:
            what = "%s dy+%d accumulate=%d%s" % (T.case_id(case), dy_off, acc, "" if workspace else " (no workspace)")
            call, guards, dxg = run_bwd_data(lib, case, idx, acc, dy_off=dy_off, workspace=workspace)
            _launch(lib, call(), what)
            _check_guards(guards, what)
            _check_out(dxg.payload, p["dx"] + p["base"].double() if acc else p["dx"], case, what + " dx", slack=slack)


@_rows("bwd_data")
def test_backward_data_writes_exactly_its_slice(lib, case):
    """dx (+)= conv_transpose(dy, w) into a channel slice: stride 1 (flipped forward families, the split with its exactly sized workspace
    and without one), the three stride-2 kernels; accumulate = 0 on a NaN slice (every element written), accumulate = 1 on a random base."""
    _bwd_data_row(lib, case, 0.503)


@_rows("bwd_data_dual")
def test_backward_data_dual_writes_exactly_its_slice(lib, case):
    """dpi_conv_bwd_data_dual, fused and as two launches.  A bf16 dx takes the one-ulp slack tests/test_gpu_bf16_storage.py documents
    for two stores (the 1x1x1 launch rounds, the 3x3x3 launch adds and rounds again)."""
    _bwd_data_row(lib, case, 1.01)


@_rows("bwd_weight")
def test_backward_weight_four_launches_in_an_exact_workspace(lib, case):
    """The four launches dpi_conv_bwd_weight_ws_floats is the maximum over — a chain on x or none, x / dy aligned or moved by one
    element (bf16 tensors: one and two elements, 2 and 4 bytes) — each with a NaN dw and a workspace of exactly the queried size:
    dw written everywhere and at 5e-6 against the fp64 oracle, bands intact.  The bf16 backward-weight kernels (aligned bf16 tensors,
    precision 1) round a chained T(x) to bf16 as an operand: that one launch is held to the pair of bars of
    test_pointwise_backward_weight_on_the_bf16_mfma — 4e-3 against the exact oracle, and 2e-4 against the oracle fed the bf16-rounded
    T(x) (a few values round the other way: fp32 association of the chain) unless it meets the 5e-6 outright."""
    L = lib.load()
    idx = T.CASES.index(case)
    p = _problem(idx)
    d = desc_of(lib, case)
    with knobs(lib, case.options):
        wws = L.dpi_conv_bwd_weight_ws_floats(C.byref(d))
        assert wws > 0
        w_elems = p["w"].numel()
        chain = p["chain"].to(DEV)
        for off in (0,) + case.offsets:
            xg = guard(p["x"].numel(), _dt(case, IO_X), DEV, fill=p["x"], offset=off)
            dyg = guard(p["dy"].numel(), _dt(case, IO_DY), DEV, fill=p["dy"], offset=off)
            for chained in (False, True):
                what = "%s x,dy+%d%s" % (T.case_id(case), off, " chained" if chained else "")
                dwg, wg = guard(w_elems, F32, DEV), guard(wws, F32, DEV)
                _launch(lib, L.dpi_conv_bwd_weight(C.byref(d), xg.payload.data_ptr(), lib.ptr(chain) if chained else None, dyg.payload.data_ptr(),
                                                dwg.payload.data_ptr(), wg.payload.data_ptr(), wws, lib.stream()), what)
                _check_guards([("x", xg), ("dy", dyg), ("dw", dwg), ("ws", wg)], what)
                dw = dwg.payload
                assert bool(torch.isfinite(dw).all()), "%s: %d elements of dw were not written" % (what, int((~torch.isfinite(dw)).sum()))
                ref = p["dw_chained" if chained else "dw_plain"]
                # the bf16 kernels (3x3x3: conv_bf16_bwd_weight; 1x1x1: chosen inside conv_pw_bwd_weight_mfma) take aligned tensors only.
                # Which launch is theirs comes from the row's `reaches`, not from the plan of this run: test_contract_cases_cover_the_planner
                # (tests/test_host_asan.py) pins `reaches` to the planner's answer, so a launch that moved to an fp32 kernel fails there.
                rounds = chained and off == 0 and case.precision == 1 and (case.k == 1 or case.reaches["bwd_weight_chained"] == "conv_bf16_bwd_weight")
                err = rel(dw, ref)
                if rounds:
                    err_r = rel(dw, p["dw_chained_rounded"])
                    print("%s: %.3g against the exact oracle, %.3g against the oracle on bf16(T(x))" % (what, err, err_r))
                    assert err < 4e-3, (what, err)
                    assert err_r < 2e-4 or err < 5e-6, (what, err_r, err)
                else:
                    assert err < 5e-6, (what, err)


# ---- variants chosen from the address of the OUTPUT ------------------------------------------------------------------------------------
# (launcher, cin, cout, shape, stride, precision, io, options) of a table row, the element offsets of y / dx to run it at, and the choice
# with its shape condition as the code states it.  Offset 0 is a buffer of its own at a 256-byte-aligned address.
def _row(launcher, cin, cout, shape, stride=1, precision=0, io=0, options=None):
    hits = [c for c in T.CASES if (c.launcher, c.cin, c.cout, tuple(c.shape), c.stride, c.precision, c.io, c.options) ==
            (launcher, cin, cout, tuple(shape), stride, precision, io, dict(options or {}))]
    assert len(hits) == 1, (launcher, cin, cout, shape)
    return hits[0]


ADDRESS_CASES = [
    # conv_mfma.hip, stride-2 backward-data epilogue: vec2 = fp32 dx, even W and V, dx 8-byte aligned -> float2 stores, else scalar
    (_row("bwd_data", 9, 20, (8, 8, 40), stride=2), (0, 1)),
    # conv_direct.hip, dpi_conv_bwd_data_ws: the bf16 stride-2 kernel needs dx 4-byte aligned (dword stores), else conv_bwd_data_s2_mfma
    (_row("bwd_data", 16, 16, (4, 6, 16), stride=2, precision=1, io=15), (0, 1)),
    # conv_mfma.hip epilogue, bf16 y: pairs = even Wo and Vo, y 4-byte aligned -> one dword per two voxels, else 2-byte stores
    (_row("fwd", 16, 16, (4, 8, 16), io=15), (0, 1)),
    # conv_bf16_mfma.hip, conv_bf16_kernel epilogue: the same choice
    (_row("fwd", 16, 16, (4, 8, 16), precision=1, io=15, options=T.BF), (0, 1)),
    # conv_bf16_mfma.hip, conv_bf16_s2_kernel epilogue: the same choice (Wo = 8, Vo = 48)
    (_row("fwd", 16, 16, (4, 6, 16), stride=2, precision=1, io=15), (0, 1)),
]


@pytest.mark.parametrize("case,offsets", ADDRESS_CASES, ids=[T.case_id(c) for c, _ in ADDRESS_CASES])
def test_output_address_chosen_variants(lib, case, offsets):
    """The variants a launch chooses from the address of its OUTPUT, on the same data at the natural address and with the output moved
    by one element: both at the oracle bar, bands intact.  (Variants chosen from an INPUT address — vectorised stride-2 staging, the
    aligned 4x4x1 kernel, the bf16 stride-2 backward-data kernel's dy, every backward-weight choice — are the `offsets` of the table
    rows and run in the tests above.)"""
    idx = T.CASES.index(case)
    p = _problem(idx)
    with knobs(lib, case.options):
        for off in offsets:
            what = "%s out+%d" % (T.case_id(case), off)
            if case.launcher == "fwd":
                call, guards, yg, pg, nblk = run_fwd(lib, case, idx, y_off=off, chained=False)
                _launch(lib, call(), what)
                _check_guards(guards, what)
                assert bool(torch.isfinite(pg.payload).all()), what
                _check_out(yg.payload, p["y_plain"], case, what + " y")
            else:
                for acc in (0, 1):
                    call, guards, dxg = run_bwd_data(lib, case, idx, acc, dx_off=off)
                    _launch(lib, call(), what)
                    _check_guards(guards, what)
                    _check_out(dxg.payload, p["dx"] + p["base"].double() if acc else p["dx"], case, what + " dx accumulate=%d" % acc)


# ---- alignments an entry point refuses ---------------------------------------------------------------------------------------------------
REFUSALS = [
    # conv_bf16_mfma.hip: the bf16 stencil kernel stages a bf16 input in 8-byte pieces
    (_row("fwd", 16, 16, (4, 8, 16), precision=1, io=15, options=T.BF), (1, 2)),
    (_row("bwd_data", 16, 16, (4, 8, 16), precision=1, io=15, options=T.BF), (1, 2)),
    # ... and so does the bf16 stride-2 forward kernel
    (_row("fwd", 16, 16, (4, 6, 16), stride=2, precision=1, io=15), (1, 2)),
    # the fused pair on the bf16 stencil kernel: dy (of the 3x3x3 layer), and dy1 (of the 1x1x1 layer) alone
    (_row("bwd_data_dual", 16, (16, 16), (4, 8, 16), precision=1, io=15, options=T.BF), (1, 2)),
]


@pytest.mark.parametrize("case,offsets", REFUSALS, ids=[T.case_id(c) for c, _ in REFUSALS])
def test_refused_alignments_launch_nothing(lib, case, offsets):
    """A bf16 input that is not 8-byte aligned (moved by one or two elements): DPI_E_ARG, a message that names the tensor as the entry
    point does (x, dy, dy1), and the NaN output, the NaN partials and every band exactly as they were."""
    L = lib.load()
    idx = T.CASES.index(case)
    runs = [(off, "x" if case.launcher == "fwd" else "dy") for off in offsets]
    if case.launcher == "bwd_data_dual":
        runs += [(off, "dy1") for off in offsets]
    with knobs(lib, case.options):
        for off, tensor in runs:
            if case.launcher == "fwd":
                call, guards, out, pg, _ = run_fwd(lib, case, idx, x_off=off)
            else:
                call, guards, out = run_bwd_data(lib, case, idx, 0, **{"dy_off" if tensor == "dy" else "dy1_off": off})
                pg = None
            before = out.bits(), pg.bits() if pg else None
            rc = call()
            torch.cuda.synchronize()
            msg = L.dpi_last_error().decode()
            assert rc == -1, (rc, msg)                                   # DPI_E_ARG
            assert "the bf16 input tensor %s must be 8-byte aligned" % tensor in msg, msg
            assert out.untouched(before[0]) and (pg is None or pg.untouched(before[1])), "a refused launch wrote its output"
            _check_guards(guards, T.case_id(case))


# ---- the other two address-chosen launches ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("off", [0, 1])
def test_upsample_adjoint_row_wide_path_and_its_fallback(lib, off):
    """dpi_upsample2x_bwd, linear, separable passes: the row-wide first pass needs Wo == 2 W, even W, Wo % 4 == 0 and 16-byte-aligned dy
    and workspace; with dy moved by one float the axis kernel takes the pass.  Against the float64 adjoint of the oracle's up-sampling
    (autograd through oracle.upsample2x) at the 2e-6 norm-wise of the fp32 outputs; workspace exactly as queried, dx pre-filled with NaN."""
    L = lib.load()
    Cn, D, H, W = 3, 3, 5, 6
    Do, Ho, Wo = 2 * D, 2 * H, 2 * W
    gen = torch.Generator().manual_seed(11)
    dy = torch.randn((Cn, Do, Ho, Wo), generator=gen)
    xr = torch.zeros((1, Cn, D, H, W), dtype=torch.float64, requires_grad=True)
    (O.upsample2x(xr, "trilinear")[0] * dy.double()).sum().backward()
    n_ws = L.dpi_upsample2x_bwd_ws_floats(Cn, D, H, W, Do, Ho, Wo, 1)
    assert n_ws > 0
    dyg = guard(dy.numel(), F32, DEV, fill=dy, offset=off)
    dxg = guard_slice(Cn, D * H * W, F32, DEV)
    wg = guard(n_ws, F32, DEV)
    _launch(lib, L.dpi_upsample2x_bwd(dyg.payload.data_ptr(), Cn, D, H, W, Do, Ho, Wo, 1, dxg.payload.data_ptr(), wg.payload.data_ptr(), lib.stream()),
              "dpi_upsample2x_bwd")
    _check_guards([("dy", dyg), ("dx", dxg), ("ws", wg)], "upsample2x_bwd dy+%d" % off)
    assert bool(torch.isfinite(dxg.payload).all())
    assert rel(dxg.payload, xr.grad[0].reshape(Cn, -1)) < 2e-6


@pytest.mark.parametrize("adjoint", [0, 1])
@pytest.mark.parametrize("off", [0, 1])
def test_hale_sections_vector_path_and_its_fallback(lib, off, adjoint):
    """dpi_hale_sections: four samples per thread where Y % 4 == 0 and x, coef, y are 16-byte aligned, one sample per thread otherwise (x
    moved by one float).  Forward against the float64 Hale2D restatement of tests/test_gpu_antialias3d.py, section by section, at that
    file's tolerance; the adjoint against the transpose of that restatement's matrix, at the same tolerance."""
    from test_gpu_antialias3d import sections_np
    L = lib.load()
    Cn, Tn, X, Y = 2, 7, 5, 8
    rng = np.random.RandomState(3)
    shape = (Cn, Tn, X, Y)
    ptx, pty = rng.randn(*shape), rng.randn(*shape)
    coef = np.stack([np.cos(ptx) ** 2, -np.cos(ptx) * np.sin(ptx), np.sin(ptx) ** 2, np.cos(pty) ** 2, -np.cos(pty) * np.sin(pty), np.sin(pty) ** 2])
    n = int(np.prod(shape))
    cg = guard(6 * n, F32, DEV, fill=torch.from_numpy(coef).float())
    if not adjoint:
        z = rng.randn(*shape)
        xg = guard(n, F32, DEV, fill=torch.from_numpy(z).float(), offset=off)
        yg = guard(2 * n, F32, DEV)
        ref = np.stack(sections_np(z, ptx, pty))
    else:
        g = rng.randn(2, *shape)
        xg = guard(2 * n, F32, DEV, fill=torch.from_numpy(g).float(), offset=off)
        yg = guard(n, F32, DEV)
        # the transpose of the float64 restatement: its matrix from the n unit vectors (row i = the two outputs for input sample i)
        eye = np.eye(n).reshape((n,) + shape)
        A0 = np.stack([sections_np(e, ptx, pty)[0] for e in eye]).reshape(n, n)
        A1 = np.stack([sections_np(e, ptx, pty)[1] for e in eye]).reshape(n, n)
        ref = (A0 @ g[0].reshape(n) + A1 @ g[1].reshape(n)).reshape(shape)
    _launch(lib, L.dpi_hale_sections(xg.payload.data_ptr(), cg.payload.data_ptr(), Cn, Tn, X, Y, adjoint, yg.payload.data_ptr(), lib.stream()), "dpi_hale_sections")
    _check_guards([("x", xg), ("coef", cg), ("y", yg)], "hale_sections x+%d adjoint=%d" % (off, adjoint))
    got = yg.payload.cpu().numpy().reshape(ref.shape)
    assert np.isfinite(got).all()
    np.testing.assert_allclose(got, ref, rtol=1e-4, atol=1e-5 * np.abs(ref).max())
