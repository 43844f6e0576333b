"""What a launch of the residual-join BatchNorm backward computes and may touch: dpi_join_bwd and its fallback pieces
dpi_bn_bwd_apply_fork[_io] / dpi_bn_bwd_apply_dual[_io] on the rows of tests/join_cases.py through the C ABI, every buffer owned by the
test.  Inputs (tensors and per-channel tables) sit inside guard bands; tensors a launch may write are NaN-filled channel slices of a
larger buffer (guard_slice), vectors NaN-filled buffers inside bands; `ws` has exactly dpi_join_bwd_ws_doubles doubles, `coef` 8 C floats,
`dgb` 6 C, `dgb_f` 2 (hi - lo), partial rows exactly dpi_stat_blocks * C * 2 (fork range: * (hi - lo) * 2).  After every launch: _launch,
_check_guards (both end the session on a launch error or a device fault, as in test_gpu_conv_contract.py), every declared element
finite, and the values against the float64 restatements of join_cases.py (held against float64 autograd by
tests/test_join_refs_host.py, which also shows that these checks fail on a wrong kernel).  Kernels are never a reference for each other.

Bars (none is new): 2e-5 norm-wise on fp32 dx tensors and 2e-4 on per-channel gradients (test_join_bwd_two_pass...), half a bf16 ulp
(half_ulp_ok, slack 0.503) for a bf16 tensor against the restatement on the widened operands; the follow-up partial rows of fork / dual
against float64 span sums of the dx / dxb the launch STORED, |got - float64| <= (k 2^-24 + n 2^-53) sum|term| with k = 4 and 10
(bn_bwd_reduce's arithmetic: `ls += g; lq = fmaf(g, xh, lq)`); with a handful of voxels (V <= 5, handed statistics) the per-channel
outputs against the magnitudes of their terms, |got - ref| <= 2e-4 sum|term| (the V == 1 branch of test_bn_bwd_two_phase)."""
import time

import numpy as np
import pytest
import torch

import elementwise_cases as E
import join_cases as J
from gpu_guard import guard, guard_slice
from test_gpu_conv_contract import _check_guards, _launch

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
S02 = float(np.float32(0.2))                       # the slope as the kernels receive it
K_FOLLOW = torch.tensor([4.0, 10.0], dtype=F64)


@pytest.fixture(scope="module")
def lib():
    from deep_prior_interpolation_amd import _lib
    return _lib


def sl(v):
    """A slope of the case tables as the C ABI passes it."""
    return 1.0 if v == 1.0 else S02


# ---- buffers -----------------------------------------------------------------------------------------------------------------------------
def _aligned(g, V):
    if V % 4 == 0:
        assert g.payload.data_ptr() % (4 * g.payload.element_size()) == 0, "test buffer off the alignment a channel slice has"
    return g


def gin(t, dtype=F32):
    """An input tensor [C][V] inside guard bands at a 256-byte-aligned address; None stays None."""
    return None if t is None else _aligned(guard(t.numel(), dtype, DEV, fill=t, shape=tuple(t.shape)), t.shape[-1])


def gtab(t, dtype=F32):
    """A per-channel table (statistics, gamma, beta, chain, partial rows) inside guard bands; None stays None."""
    return None if t is None else guard(t.numel(), dtype, DEV, fill=t.contiguous())


def gout(C_, V, dtype=F32):
    return _aligned(guard_slice(C_, V, dtype, DEV), V)


def gvec(n, dtype=F32):
    return guard(n, dtype, DEV)


def ptr(g):
    return None if g is None else (g.payload if hasattr(g, "payload") else g).data_ptr()


def dt(io, bit):
    return BF if io & bit else F32


def side_tabs(s):
    return {k: gtab(s[k]) for k in ("mi", "gamma", "beta", "chain")}


# ---- dpi_join_bwd ------------------------------------------------------------------------------------------------------------------------
def launch_join(lib, p, what):
    """One dpi_join_bwd launch of the operands p (tensors on the CPU or on the device) into NaN-filled, guarded outputs: returns the
    payloads as join_cases.check_join takes them, after the guards, the exact-size workspace, coef and the untouched fork range of dxb
    have been checked."""
    L, row = lib.load(), p["row"]
    C_, V = p["xa"].shape
    lo, hi = p["fork"]["lo"], p["fork"]["hi"]
    fdt, gdt = dt(row.io, 1), dt(row.io, 2)
    top, A, B, fk = p["top"], p["A"], p["B"], p["fork"]
    xag, xbg, dyg, tg = gin(p["xa"], fdt), gin(p["xb"], fdt), gin(p["dy"], gdt), gin(p["t"], fdt)
    tt, ta, tb = side_tabs(dict(top, chain=None)), side_tabs(A), side_tabs(B)
    tf = {k: gtab(fk[k]) for k in ("mi", "gamma", "beta")}
    fwa, fwb = gtab(p["fwd_a"]), gtab(p["fwd_b"])
    n_ws = L.dpi_join_bwd_ws_doubles(C_, V)
    assert n_ws == E.stat_blocks(C_, V) * C_ * J.JOIN_SUMS
    wsg, coefg, dgbg = gvec(n_ws, F64), gvec(8 * C_), gvec(6 * C_)
    dgbfg = gvec(2 * (hi - lo)) if hi > lo else None
    dxag, dxbg = gout(C_, V, gdt), gout(C_, V, gdt)
    dxfg = gout(hi - lo, V, gdt) if hi > lo else None
    if lo == hi:
        assert tf["mi"] is None and dxfg is None and dgbfg is None                             # nothing of the fork may be dereferenced
    before = dxbg.bits()
    rc = L.dpi_join_bwd(ptr(dyg), ptr(tg), ptr(tt["mi"]), ptr(tt["gamma"]), ptr(tt["beta"]), sl(top["pre"]), C_, V,
                        ptr(xag), ptr(ta["mi"]), ptr(ta["gamma"]), ptr(ta["beta"]), ptr(ta["chain"]), sl(A["post"]),
                        ptr(xbg), ptr(tb["mi"]), ptr(tb["gamma"]), ptr(tb["beta"]), ptr(tb["chain"]), sl(B["post"]),
                        ptr(fwa), ptr(fwb), lo, hi, ptr(tf["mi"]), ptr(tf["gamma"]), ptr(tf["beta"]), sl(fk["post"]),
                        ptr(wsg), ptr(coefg), ptr(dxag), ptr(dxbg), ptr(dxfg), ptr(dgbg), ptr(dgbfg), row.io, lib.stream())
    _launch(lib, rc, "dpi_join_bwd")
    guards = [("dy", dyg), ("t", tg), ("xa", xag), ("xb", xbg), ("fwd_chain_a", fwa), ("fwd_chain_b", fwb), ("ws", wsg), ("coef", coefg),
              ("dxa", dxag), ("dxb", dxbg), ("dxf", dxfg), ("dgb", dgbg), ("dgb_f", dgbfg)]
    guards += [("%s.%s" % (n, k), g) for n, tabs in (("top", tt), ("a", ta), ("b", tb), ("fork", tf)) for k, g in tabs.items()]
    _check_guards(guards, what)
    J.written(wsg.payload, "ws"), J.written(coefg.payload, "coef")
    if hi > lo:                        # the fork channels of dxb keep their NaN pre-fill bit for bit
        assert torch.equal(dxbg.bits().view(C_, V)[lo:hi], before.view(C_, V)[lo:hi]), "%s: dxb was touched on the fork range" % what
    return {"dxa": dxag.payload, "dxb": dxbg.payload, "dxf": None if dxfg is None else dxfg.payload, "dgb": dgbg.payload.view(6, C_),
            "dgb_f": None if dgbfg is None else dgbfg.payload.view(2, hi - lo), "coef": coefg.payload.view(C_, 8)}


@pytest.mark.parametrize("row", J.JOIN_ROWS, ids=J.join_id)
def test_join_bwd(lib, row):
    """dxa, dxb (off the fork range only), dxf, dgb [6][C] and dgb_f [2][hi - lo] of one launch against join_cases.join_bwd64; with bf16
    tensors the nested sums describe unrounded intermediates, so the reference is float64 throughout.  coef's fork pair stays 0 off the
    fork range."""
    p = J.join_problem(row)
    what = "join_bwd " + J.join_id(row)
    got = launch_join(lib, p, what)
    lo, hi = row.fork
    worst = J.check_join(got, J.join_ref(p), lo, hi, row.V)
    off = [c for c in range(row.C) if not lo <= c < hi]
    assert bool((got["coef"][off, 6:] == 0).all())
    print("%s: tensors %.3g, vectors %.3g" % (what, worst[0], worst[1]))


def rel_dev(a, b):
    a, b = a.detach().double().reshape(-1), b.detach().double().reshape(-1)
    return float((a - b).norm() / (b.norm() + 1e-300))


def test_join_bwd_large(lib):
    """C = 1, V = 33570820, t = NULL, fork (0, 1): non-temporal loads and stores, 2048 capped blocks of 17 trips, the apply grid capped at
    4096 blocks with its grid-stride loop.  Operands drawn and nudged on the device, the float64 restatement evaluated there too.
    Measured on an MI355X: 0.4 s for the whole test (1033 of 67 M elements moved off a jump); dxa 7.8e-8, dxf 7.7e-8, vectors 2.1e-6."""
    t0 = time.time()
    row = J.LARGE_ROW
    gen = torch.Generator(device=DEV).manual_seed(79)
    draw = lambda scale, off: (torch.randn(row.V, generator=gen, device=DEV) * scale + off).view(1, row.V)
    p = J.build_join(row, draw(1.3, 0.7), draw(0.9, -0.4), draw(1.0, 0.0), torch.Generator().manual_seed(80))
    assert p["nudged"][-1] == 0 and p["t"] is None, p["nudged"]
    got = launch_join(lib, p, "join_bwd large")
    ref = J.join_ref(p)
    J.written(got["dxa"], "dxa"), J.written(got["dxf"], "dxf")
    ra, rf = rel_dev(got["dxa"], ref["dxa"]), rel_dev(got["dxf"], ref["dxf"])
    assert ra < J.DX_BAR and rf < J.DX_BAR, (ra, rf)
    assert bool(torch.isnan(got["dxb"]).all())
    wv = max(J.vectors_ok(got["dgb"], ref["dgb"], ref["mag_dgb"], row.V, "dgb"), J.vectors_ok(got["dgb_f"], ref["dgb_f"], ref["mag_dgb_f"], row.V, "dgb_f"))
    torch.cuda.synchronize()
    print("join_bwd large: dxa %.3g, dxf %.3g, vectors %.3g, %d elements moved off a jump, %.1f s" % (ra, rf, wv, p["nudged"][0], time.time() - t0))


# ---- dpi_bn_bwd_apply_fork ---------------------------------------------------------------------------------------------------------------
def _vectors(got, part, V, what):
    """dgamma / dbeta = float(total of the caller's partial rows): 2e-4 norm-wise, or against sum|row| with a handful of voxels."""
    for g, r, col, name in got:
        if g is not None:
            J.vectors_ok(g.payload.view(1, -1), r.view(1, -1), part[:, :, col].abs().sum(0).view(1, -1), V, "%s %s" % (what, name))


@pytest.mark.parametrize("row", J.FORK_ROWS, ids=J.fork_id)
def test_bn_bwd_apply_fork(lib, row):
    """dx, dgamma, dbeta from the caller's partial rows (the float64 rows of the restatement, or synthetic rows at a caller-given count:
    the one-wave stride-64 prologue of this kernel's own copy), and the {sum g, sum g xhat} rows the follow-up BatchNorms take of the
    STORED dx: A on xa (post 0.2), B on T_chain_b(xb) (post 0.2)."""
    L, p = lib.load(), J.fork_problem(row.V, row.io, row.form)
    C_, V, io = 3, row.V, row.io
    S, A, B = p["S"], p["A"], p["B"]
    what = "bn_bwd_apply_fork " + J.fork_id(row)
    nb = E.stat_blocks(C_, V)
    assert nb == L.dpi_stat_blocks(C_, V)
    if row.nblk is None:
        part = E.bn_bwd_partials64(p["dy"], p["x"], S["mi"], S["gamma"], S["beta"], S["chain"], S["pre"], S["post"])[0]
    else:
        part = E.synthetic_partials(row.nblk, C_, seed=3) * (0.2 * V)
    use_a, use_b = row.follow in ("both", "a"), row.follow in ("both", "b")
    fdt, gdt = dt(io, 1), dt(io, 2)
    xg, dyg, pg = gin(p["x"], fdt), gin(p["dy"], gdt), gtab(part, F64)
    xag, xbg = (gin(p["xa"], fdt) if use_a else None), (gin(p["xb"], fdt) if use_b else None)
    ts, ta, tb = side_tabs(S), side_tabs(A), side_tabs(B)
    pag, pbg = (gvec(nb * C_ * 2, F64) if use_a else None), (gvec(nb * C_ * 2, F64) if use_b else None)
    dxg = gout(C_, V, gdt)
    dgg, dbg = (None, None) if row.null_dgb else (gvec(C_), gvec(C_))
    rc = L.dpi_bn_bwd_apply_fork_io(ptr(dyg), ptr(xg), ptr(ts["mi"]), ptr(ts["gamma"]), ptr(ts["beta"]), ptr(ts["chain"]), sl(S["pre"]), sl(S["post"]),
                                    ptr(pg), part.shape[0], C_, V, ptr(dxg), ptr(dgg), ptr(dbg),
                                    ptr(xag), ptr(ta["mi"]), ptr(ta["gamma"]), ptr(ta["beta"]), None, sl(A["post"]), ptr(pag),
                                    ptr(xbg), ptr(tb["mi"]), ptr(tb["gamma"]), ptr(tb["beta"]), ptr(tb["chain"]), sl(B["post"]), ptr(pbg),
                                    io, lib.stream())
    _launch(lib, rc, "dpi_bn_bwd_apply_fork_io")
    guards = [("dy", dyg), ("x", xg), ("partials", pg), ("xa", xag), ("xb", xbg), ("partials_a", pag), ("partials_b", pbg), ("dx", dxg),
              ("dgamma", dgg), ("dbeta", dbg)]
    guards += [("%s.%s" % (n, k), g) for n, tabs in (("self", ts), ("a", ta), ("b", tb)) for k, g in tabs.items()]
    _check_guards(guards, what)
    dx, dg, db = J.fork64(p["dy"], p["x"], S["mi"], S["gamma"], S["beta"], S["chain"], S["pre"], S["post"], part.sum(0))
    J.stored_ok(dxg.payload, dx, what + " dx")
    _vectors([(dgg, dg, 1, "dgamma"), (dbg, db, 0, "dbeta")], part, V, what)
    stored = dxg.payload.float().cpu()
    for use, got, xs, s, name in ((use_a, pag, p["xa"], dict(A, chain=None), "partials_a"), (use_b, pbg, p["xb"], B, "partials_b")):
        if use:
            ref, mag = J.followup64(stored, xs, s["mi"], s["gamma"], s["beta"], s["chain"], s["post"])
            E.check_partials(got.payload.view(nb, C_, 2), ref, mag, K_FOLLOW, "%s %s" % (what, name))


# ---- dpi_bn_bwd_apply_dual ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", J.DUAL_ROWS, ids=J.dual_id)
def test_bn_bwd_apply_dual(lib, row):
    """dxa and dxb (every channel of both), the two (dgamma, dbeta) pairs from the caller's partial rows, and on [lo, hi) the fork's
    {sum g, sum g xhat} rows of the STORED dxb against the raw xb; lo == hi: f_partials and the fork's tables are NULL."""
    L, p = lib.load(), J.dual_problem(row.C, row.V, row.fork, row.form, row.io)
    C_, V, io = row.C, row.V, row.io
    lo, hi = row.fork
    A, B, fk = p["A"], p["B"], p["fork"]
    what = "bn_bwd_apply_dual " + J.dual_id(row)
    nb = E.stat_blocks(C_, V)
    if row.nblk is None:
        pa, pb = (E.bn_bwd_partials64(p["dy"], x, s["mi"], s["gamma"], s["beta"], s["chain"], 1.0, s["post"])[0] for x, s in ((p["xa"], A), (p["xb"], B)))
    else:
        pa, pb = (E.synthetic_partials(row.nblk, C_, seed=s) * (0.2 * V) for s in (3, 4))
    fdt, gdt = dt(io, 1), dt(io, 2)
    dyg, xag, xbg = gin(p["dy"], gdt), gin(p["xa"], fdt), gin(p["xb"], fdt)
    pag, pbg = gtab(pa, F64), gtab(pb, F64)
    ta, tb = side_tabs(A), side_tabs(B)
    tf = {k: gtab(fk[k]) for k in ("mi", "gamma", "beta")}
    fpg = gvec(nb * (hi - lo) * 2, F64) if hi > lo else None
    dxag, dxbg = gout(C_, V, gdt), gout(C_, V, gdt)
    vec = [gvec(C_) for _ in range(4)]
    rc = L.dpi_bn_bwd_apply_dual_io(ptr(dyg), pa.shape[0], C_, V,
                                    ptr(xag), ptr(ta["mi"]), ptr(ta["gamma"]), ptr(ta["beta"]), ptr(ta["chain"]), sl(A["post"]), ptr(pag), ptr(dxag), ptr(vec[0]), ptr(vec[1]),
                                    ptr(xbg), ptr(tb["mi"]), ptr(tb["gamma"]), ptr(tb["beta"]), ptr(tb["chain"]), sl(B["post"]), ptr(pbg), ptr(dxbg), ptr(vec[2]), ptr(vec[3]),
                                    lo, hi, ptr(tf["mi"]), ptr(tf["gamma"]), ptr(tf["beta"]), sl(fk["post"]), ptr(fpg), io, lib.stream())
    _launch(lib, rc, "dpi_bn_bwd_apply_dual_io")
    guards = [("dy", dyg), ("xa", xag), ("xb", xbg), ("partials_a", pag), ("partials_b", pbg), ("f_partials", fpg), ("dxa", dxag), ("dxb", dxbg)]
    guards += [("vector %d" % i, g) for i, g in enumerate(vec)]
    guards += [("%s.%s" % (n, k), g) for n, tabs in (("a", ta), ("b", tb), ("fork", tf)) for k, g in tabs.items()]
    _check_guards(guards, what)
    (dxa, dga, dba), (dxb, dgb, dbb) = J.dual64(p["dy"], A, p["xa"], pa.sum(0), B, p["xb"], pb.sum(0))
    J.stored_ok(dxag.payload, dxa, what + " dxa"), J.stored_ok(dxbg.payload, dxb, what + " dxb")
    _vectors([(vec[0], dga, 1, "dgamma_a"), (vec[1], dba, 0, "dbeta_a")], pa, V, what)
    _vectors([(vec[2], dgb, 1, "dgamma_b"), (vec[3], dbb, 0, "dbeta_b")], pb, V, what)
    if hi > lo:
        ref, mag = J.dual_fork_partials64(dxbg.payload.float().cpu(), p["xb"], fk)
        E.check_partials(fpg.payload.view(nb, hi - lo, 2), ref, mag, K_FOLLOW, what + " f_partials")


# ---- rejected arguments ------------------------------------------------------------------------------------------------------------------
def _refusals(L, g):
    """(entry point's name in the message, call) for every argument the three entry points refuse; g: dict of device addresses.
    C = 4, V = 8, fork (2, 4)."""
    x, q, d, y, v, st = g["x"], g["q"], g["d"], g["y"], g["v"], g["stream"]

    def join(**kw):
        a = dict(dy=x, t=x, mi=q, pre=0.2, C=4, V=8, xa=x, mi_a=q, xb=x, mi_b=q, fwa=q, fwb=q, lo=2, hi=4, f_mi=q, ws=d, coef=v, dxa=y, dxb=y, dxf=y,
                 dgb=v, dgb_f=v, io=0)
        a.update(kw)
        return lambda: L.dpi_join_bwd(a["dy"], a["t"], a["mi"], None, None, a["pre"], a["C"], a["V"], a["xa"], a["mi_a"], None, None, None, 0.2,
                                      a["xb"], a["mi_b"], None, None, None, 1.0, a["fwa"], a["fwb"], a["lo"], a["hi"], a["f_mi"], None, None, 0.2,
                                      a["ws"], a["coef"], a["dxa"], a["dxb"], a["dxf"], a["dgb"], a["dgb_f"], a["io"], st)

    def fork(**kw):
        a = dict(dy=x, x=x, mi=q, chain=None, pre=0.2, p=d, nblk=1, C=4, V=8, dx=y, xa=x, mi_a=q, pa=d, xb=x, mi_b=q, pb=d, io=0)
        a.update(kw)
        return lambda: L.dpi_bn_bwd_apply_fork_io(a["dy"], a["x"], a["mi"], None, None, a["chain"], a["pre"], 1.0, a["p"], a["nblk"], a["C"], a["V"], a["dx"],
                                                  None, None, a["xa"], a["mi_a"], None, None, None, 0.2, a["pa"], a["xb"], a["mi_b"], None, None, None, 0.2,
                                                  a["pb"], a["io"], st)

    def dual(**kw):
        a = dict(dy=x, nblk=1, C=4, V=8, xa=x, mi_a=q, pa=d, dxa=y, xb=x, mi_b=q, pb=d, dxb=y, lo=2, hi=4, f_mi=q, fp=d, io=0)
        a.update(kw)
        return lambda: L.dpi_bn_bwd_apply_dual_io(a["dy"], a["nblk"], a["C"], a["V"], a["xa"], a["mi_a"], None, None, None, 0.2, a["pa"], a["dxa"], None, None,
                                                  a["xb"], a["mi_b"], None, None, None, 1.0, a["pb"], a["dxb"], None, None, a["lo"], a["hi"], a["f_mi"], None,
                                                  None, 0.2, a["fp"], a["io"], st)
    out = [("join_bwd", join(lo=-1)), ("join_bwd", join(hi=5)), ("join_bwd", join(lo=3, hi=2)),
           ("join_bwd", join(f_mi=None)), ("join_bwd", join(dxf=None)), ("join_bwd", join(dgb_f=None)),
           ("join_bwd", join(t=None, fwa=None)), ("join_bwd", join(t=None, fwb=None)),
           ("join_bwd", join(io=4)), ("join_bwd", join(io=8)), ("join_bwd", join(C=0)), ("join_bwd", join(C=-1)), ("join_bwd", join(V=0))]
    out += [("join_bwd", join(**{k: None})) for k in ("dy", "mi", "xa", "xb", "mi_a", "mi_b", "ws", "coef", "dxa", "dxb", "dgb")]
    out += [("bn_bwd_apply_fork", fork(**{k: None})) for k in ("dy", "x", "mi", "p", "dx")]
    out += [("bn_bwd_apply_fork", fork(C=0)), ("bn_bwd_apply_fork", fork(V=0)), ("bn_bwd_apply_fork", fork(nblk=0)), ("bn_bwd_apply_fork", fork(io=4)),
            ("bn_bwd_apply_fork", fork(chain=q, pre=0.2)),                                                       # in_chain with pre != 1
            ("bn_bwd_apply_fork", fork(mi_a=None)), ("bn_bwd_apply_fork", fork(pa=None)),                        # incomplete follow-ups
            ("bn_bwd_apply_fork", fork(mi_b=None)), ("bn_bwd_apply_fork", fork(pb=None))]
    out += [("bn_bwd_apply_dual", dual(**{k: None})) for k in ("dy", "xa", "xb", "mi_a", "mi_b", "pa", "pb", "dxa", "dxb")]
    out += [("bn_bwd_apply_dual", dual(C=0)), ("bn_bwd_apply_dual", dual(V=0)), ("bn_bwd_apply_dual", dual(nblk=0)), ("bn_bwd_apply_dual", dual(io=4)),
            ("bn_bwd_apply_dual", dual(lo=-1)), ("bn_bwd_apply_dual", dual(hi=5)), ("bn_bwd_apply_dual", dual(lo=3, hi=2)), ("bn_bwd_apply_dual", dual(lo=2, hi=2)),
            ("bn_bwd_apply_dual", dual(f_mi=None))]
    return out


def test_refused_arguments_launch_nothing(lib):
    """Every DPI_REQUIRE of the three entry points, after the pattern of test_refused_alignments_launch_nothing: DPI_E_ARG, a message that
    names the entry point, and every buffer — the NaN outputs (tensor, vectors, double rows), the inputs, all bands — bit for bit as it
    was."""
    L = lib.load()
    xg, qg = gin(torch.randn(4, 8)), gtab(torch.rand(4, 5) + 0.5)
    yg, vg, dg = gout(4, 8), gvec(64), gvec(4 * 24, F64)
    g = {"x": ptr(xg), "q": ptr(qg), "y": ptr(yg), "v": ptr(vg), "d": ptr(dg), "stream": lib.stream()}
    bufs = (xg, qg, yg, vg, dg)
    before = [b.bits() for b in bufs]
    calls = _refusals(L, g)
    assert len(calls) == 56
    for name, call in calls:
        rc = call()
        msg = L.dpi_last_error().decode()
        assert rc == -1, (name, rc, msg)                                 # DPI_E_ARG
        assert msg.startswith(name + ":"), (name, msg)
    _check_guards([("x", xg), ("q", qg), ("y", yg), ("v", vg), ("d", dg)], "refused arguments")
    assert all(b.untouched(bits) for b, bits in zip(bufs, before)), "a refused launch wrote a buffer"
