"""The residual-join BatchNorm backward of csrc/elementwise.hip — dpi_join_bwd and its fallback pieces dpi_bn_bwd_apply_fork[_io] /
dpi_bn_bwd_apply_dual[_io] — as tests/test_gpu_join_contract.py launches them: the case rows, the operands, float64 restatements written
from include/dpi_hip.h (torch on the CPU, or wherever the operands live; the library is never called) and the checks the device test
applies to a launch's outputs.  A plain module: no fixtures, importable without a GPU.  tests/test_join_refs_host.py holds the
restatements against float64 autograd of the forward expressions and shows, restatement against restatement, that the checks catch a
wrong kernel (MUTATIONS).

The forms (reference architectures/mulresunet.py:85-96, 109-112), per channel:
   block     y = BN(act_pre(t)),  t = act(BN_a(xa)) + BN_b(T_CH(xb));  T_CH = the identity off the fork range [lo, hi) and act(BN_f(xb)) on
             it.  post_a = 0.2, post_b = 1, chain_b = T_CH, fwd_chain_b = the composition dpi_bn_finalize(in_chain = T_CH) makes.
   respath   y = BN(act_pre(t)),  t = act(BN_a(xa)) + act(BN_b(xb)): both posts 0.2, no chains, no fork.
 pre = 0.2 on every block row; pre = 1 runs on respath rows (with post_b = 1, pre = 1 makes dbeta_b = sum dt vanish identically: the top
 BatchNorm's input gradient has no mean).  The fork's |beta| is drawn from [0.3, ...): side B projects dxb off act(BN_f(xb)) and off 1, so
 on the fork range dgamma_f = -(beta_f / gamma_f) dbeta_f, and a beta_f near 0 leaves rounding residue where a gradient should be.

Why each row exists (span = stat_span(V, nblk), nblk = dpi_stat_blocks; join_bwd_sums_kernel takes two groups of four elements per thread
and trip, 2048 elements per block and trip):
 JOIN_V   1, 3, 4, 5   one thread or two, first group only; statistics HANDED (a BatchNorm's own statistics of a handful of voxels make
                        every gradient cancel, and nothing would be measured)
          1023          first group only, thread 255 has three elements
          1287          second group (`i0 + 1024`) for threads 0..65 only, thread 65 with a 3-element tail; every other thread takes
                        `if (i >= end) break`
          16384         one full block, eight trips, both groups everywhere
          16385, 16388  two blocks (scalar / vector path), span 8196: a fifth trip of one thread, first group only
          32772         three blocks, span 10924: sixth trip, second group for some threads only
          49153         four blocks, scalar path, span 12292
 LAYOUTS  (C, fork): (5, (3, 5)) Block3d's trailing slice; (5, (1, 2)) an interior single channel, the fork's constants indexed by c - lo;
          (3, (0, 3)) every channel forked, dxb receives nothing at all; (4, (0, 0)) no fork, null fork pointers, dxf, dgb_f;
          (4, (2, 2)) lo == hi != 0 with null fork pointers: must equal no fork
 KEY_V    1287, 16385, 16388: every layout, t stored and t = NULL, and the bf16 storage masks io = 1, 2, 3
 one row with gamma_b = beta_b = NULL (the kernels read 1, 0), one large row (C = 1, V = elementwise_cases.LARGE_V, t = NULL, fork (0, 1)):
 non-temporal loads and stores, 2048 capped blocks of 17 trips, the apply grid capped at 4096 blocks.

Operands.  The activation masks jump at t = 0, at BatchNorm output 0 of side A, side B and the fork, and inside a chain at its inner 0.
The statistics handed to the kernels are frozen first (fp32 statistics of the drawn tensors; handed ones at V <= 5); then every element of
xa / xb within relative margin 1e-5 of a jump is moved by 1e-3 (1 + |x|) (bf16 rows: 2^-6 (1 + |x|) and re-rounded, since 1e-3 is less
than half a bf16 spacing), until none is left.  tests/test_join_refs_host.py asserts, from the restatement's own expressions, that every
row has zero elements inside the margin."""
import functools
from collections import namedtuple

import torch

import elementwise_cases as E

F64, BF = torch.float64, torch.bfloat16
SLOPE = 0.2
MARGIN = 1e-5
SEED = 7000
JOIN_SUMS = 24                                      # doubles per block and channel of dpi_join_bwd's workspace
DX_BAR, VEC_BAR = 2e-5, 2e-4                        # test_join_bwd_two_pass...: dx tensors norm-wise, per-channel gradients

# What a wrong kernel would do, modelled in join_bwd64 (argument `mutation`)
MUTATIONS = ("group2_dropped", "fork_index_c", "fork_to_dxb")

JOIN_V = (1, 3, 4, 5, 1023, 1287, 16384, 16385, 16388, 32772, 49153)
KEY_V = (1287, 16385, 16388)
LAYOUTS = ((5, (3, 5)), (5, (1, 2)), (3, (0, 3)), (4, (0, 0)), (4, (2, 2)))

JoinRow = namedtuple("JoinRow", "C V fork form t_stored pre io null_gb")


def _join_rows():
    rows = []
    for vi, V in enumerate(JOIN_V):
        for li, (C, fork) in enumerate(LAYOUTS):
            if V not in KEY_V and li not in (vi % 5, (vi + 2) % 5):
                continue
            form = "respath" if fork == (0, 0) else "block"
            pre = 1.0 if form == "respath" and vi % 2 == 0 else SLOPE      # (block: post_b = 1, so pre = 1 would make dbeta_b = sum dt = 0 exactly)
            for t_stored in ((True, False) if V in KEY_V else ((vi + li) % 2 == 0,)):
                rows.append(JoinRow(C, V, fork, form, t_stored, pre, 0, False))
    for V in KEY_V:
        for io in (1, 2, 3):
            rows.append(JoinRow(5, V, (3, 5), "block", True, SLOPE, io, False))
            rows.append(JoinRow(3, V, (0, 3), "block", False, SLOPE, io, False))
            rows.append(JoinRow(4, V, (0, 0), "respath", io != 2, SLOPE, io, False))
    rows.append(JoinRow(5, 1287, (3, 5), "block", True, SLOPE, 0, True))
    return rows


JOIN_ROWS = _join_rows()
LARGE_ROW = JoinRow(1, E.LARGE_V, (0, 1), "block", False, SLOPE, 0, False)


def join_id(r):
    return "C%d-V%d-f%d_%d-%s-%s-pre%g-io%d%s" % (r.C, r.V, r.fork[0], r.fork[1], r.form, "t" if r.t_stored else "noT", r.pre, r.io,
                                                   "-nullgb" if r.null_gb else "")


# dpi_bn_bwd_apply_fork: (pre, post, in_chain) of the BatchNorm itself x which follow-up BatchNorms take their partial rows of dx
FORK_FORMS = ((SLOPE, 1.0, False), (1.0, SLOPE, False), (1.0, 1.0, True))
FORK_FOLLOW = ("both", "a", "b", "none")
ForkRow = namedtuple("ForkRow", "V io form follow nblk null_dgb")


def _fork_rows():
    rows = []
    for vi, V in enumerate(JOIN_V):
        if V in KEY_V:
            rows += [ForkRow(V, 0, f, fo, None, False) for f in range(3) for fo in FORK_FOLLOW]
            rows += [ForkRow(V, io, io % 3, FORK_FOLLOW[io % 2], None, False) for io in (1, 2, 3)]
        else:
            rows.append(ForkRow(V, 0, vi % 3, FORK_FOLLOW[vi % 4], None, False))
    rows.append(ForkRow(1287, 0, 0, "both", None, True))                                # dgamma = dbeta = NULL
    rows += [ForkRow(1287, 0, 0, "both", n, False) for n in E.APPLY_NBLK]               # caller-given row counts
    return rows


FORK_ROWS = _fork_rows()


def fork_id(r):
    return "V%d-io%d-form%d-%s%s%s" % (r.V, r.io, r.form, r.follow, "" if r.nblk is None else "-nblk%d" % r.nblk, "-nulldgb" if r.null_dgb else "")


DualRow = namedtuple("DualRow", "C V fork form io nblk")


def _dual_rows():
    rows = []
    for vi, V in enumerate(JOIN_V):
        for li, (C, fork) in enumerate(LAYOUTS):
            if V in KEY_V or li in (vi % 5, (vi + 2) % 5):
                rows.append(DualRow(C, V, fork, "respath" if (vi + li) % 2 else "block", 0, None))
    for V in KEY_V:
        rows += [DualRow(5, V, (3, 5), "block", io, None) for io in (1, 2, 3)]
    rows += [DualRow(5, 1287, (1, 2), "block", 0, n) for n in E.APPLY_NBLK]
    return rows


DUAL_ROWS = _dual_rows()


def dual_id(r):
    return "C%d-V%d-f%d_%d-%s-io%d%s" % (r.C, r.V, r.fork[0], r.fork[1], r.form, r.io, "" if r.nblk is None else "-nblk%d" % r.nblk)


# ---- sizes -------------------------------------------------------------------------------------------------------------------------------
def group_trips(V):
    """{(trip, group): number of threads that take it} of join_bwd_sums_kernel on the first (a longest) span of a channel."""
    beg, end = E.spans(V)[0]
    out = {}
    trip = 0
    while beg + trip * 2048 < end:
        for u in (0, 1):
            first = beg + trip * 2048 + u * 1024
            out[(trip, u)] = max(0, min(256, -(-(end - first) // 4)))
        trip += 1
    return out


def group2_keep(V, device="cpu"):
    """[1][V] float64: 0 on the elements the second group of a trip covers ([1024, 2048) mod 2048 of each span), 1 elsewhere."""
    keep = torch.ones(V, dtype=F64, device=device)
    for beg, end in E.spans(V):
        off = torch.arange(end - beg, device=device)
        keep[beg:end] = ((off % 2048) < 1024).to(F64)
    return keep.reshape(1, V)


# ---- chains as dpi_bn_finalize writes them (float32 arithmetic) ----------------------------------------------------------------------------
def _g32(gamma, C):
    return torch.ones(C) if gamma is None else gamma.float().cpu()


def _b32(beta, C):
    return torch.zeros(C) if beta is None else beta.float().cpu()


def bn_chain32(mi, gamma, beta, slope):
    """act_slope(BN(x)) as a chain: {a, beta - mean a, slope, 1, 0}, a = gamma invstd."""
    C = mi.shape[1]
    a = _g32(gamma, C) * mi[1]
    return torch.stack([a, _b32(beta, C) - mi[0] * a, torch.full((C,), float(slope)), torch.ones(C), torch.zeros(C)], 1).contiguous()


def compose32(in_chain, mi, gamma, beta):
    """BN(T_in(x)): {in.ps, in.pb, in.slope, a in.qs, a in.qb + (beta - mean a)}."""
    C = mi.shape[1]
    a = _g32(gamma, C) * mi[1]
    ic = in_chain.float()
    return torch.stack([ic[:, 0], ic[:, 1], ic[:, 2], a * ic[:, 3], a * ic[:, 4] + (_b32(beta, C) - mi[0] * a)], 1).contiguous()


def identity_chain(C):
    return torch.tensor([[1.0, 0.0, 1.0, 1.0, 0.0]] * C)


# ---- the jumps of the activation masks -----------------------------------------------------------------------------------------------------
def _col(v, x):
    return v.to(device=x.device, dtype=F64).reshape(-1, 1)


def out_edge(x, mi, gamma, beta, chain, margin=MARGIN):
    """Elements whose BatchNorm output a u + (beta - mean a), u = T_chain(x), lies within `margin` of 0 relative to its two terms
    (elementwise_cases.post_edge64's form, on whatever device x lives)."""
    C = x.shape[0]
    a32 = _g32(gamma, C) * mi[1].float().cpu()
    pb32 = _b32(beta, C) - mi[0].float().cpu() * a32
    au = _col(a32, x) * E.chain64(x, chain)
    return (au + _col(pb32, x)).abs() <= margin * (au.abs() + _col(pb32, x).abs())


def inner_edge(x, chain, margin=MARGIN):
    """Elements at the inner 0 of a chain: |ps x + pb| within `margin` of 0 relative to its two terms (identity channels have none)."""
    ch = chain.to(device=x.device, dtype=F64)
    px, pb = ch[:, 0:1] * x.to(F64), ch[:, 1:2]
    return ((px + pb).abs() <= margin * (px.abs() + pb.abs())) & (ch[:, 2:3] != 1.0)


def t_edge(xa, fwd_a, xb, fwd_b, margin=MARGIN):
    ta, tb = E.chain64(xa, fwd_a), E.chain64(xb, fwd_b)
    return (ta + tb).abs() <= margin * (ta.abs() + tb.abs())


def nudge(x, mask, bf16):
    """Move the masked elements off a jump: 1e-3 (1 + |x|); a bf16-representable tensor by 2^-6 (1 + |x|), re-rounded."""
    step = (2.0 ** -6 if bf16 else 1e-3) * (1.0 + x.abs())
    moved = x + step
    moved = moved.to(BF).float() if bf16 else moved
    return torch.where(mask, moved, x)


def join_edges(p):
    """(mask over xa, mask over xb): the elements within MARGIN of any jump of the join's activation masks."""
    xa, xb, A, B, fk = p["xa"], p["xb"], p["A"], p["B"], p["fork"]
    ma = t_edge(xa, p["fwd_a"], xb, p["fwd_b"])
    if A["post"] != 1.0:
        ma = ma | out_edge(xa, A["mi"], A["gamma"], A["beta"], A["chain"])
    mb = torch.zeros_like(ma)
    if B["post"] != 1.0:
        mb = mb | out_edge(xb, B["mi"], B["gamma"], B["beta"], B["chain"])
    if B["chain"] is not None:
        mb = mb | inner_edge(xb, B["chain"])
    lo, hi = fk["lo"], fk["hi"]
    if hi > lo and fk["mi"] is not None:
        mb[lo:hi] |= out_edge(xb[lo:hi], fk["mi"], fk["gamma"], fk["beta"], None)
    return ma, mb


# ---- operands ------------------------------------------------------------------------------------------------------------------------------
def _stats(u64, gen):
    """float32 [2][C]: the tensor's own statistics, or handed ones where a channel has a handful of voxels."""
    C, V = u64.shape
    if V > 5:
        return E.mean_invstd_of(u64).cpu()
    return torch.stack([torch.randn(C, generator=gen) * 0.2, torch.rand(C, generator=gen) + 0.5])


def _vecs(n, gen):
    return torch.rand(n, generator=gen) + 0.5, torch.randn(n, generator=gen) * 0.3


def build_join(row, xa, xb, dy, gen):
    """The operands of one dpi_join_bwd launch around given tensors (CPU or device): per-channel parameters, frozen statistics, chains,
    then xa / xb nudged off the jumps, then t.  Returns a dict; tensors [C][V], per-channel tables on the CPU."""
    C, V = xa.shape
    lo, hi = row.fork
    bf_fwd = bool(row.io & 1)
    top, A, B = ({"gamma": g, "beta": b} for g, b in [_vecs(C, gen) for _ in range(3)])
    # the fork's beta stays away from 0: side B projects dxb off act(BN_f(xb)) and off 1, so on the fork range dgamma_f = -(beta_f / gamma_f)
    # dbeta_f identically — with a small beta_f the fork's dgamma is a rounding residual of the statistics, not a gradient
    gf, bf_ = _vecs(max(hi - lo, 1), gen)
    bf_ = torch.where(bf_ < 0, -1.0, 1.0) * (0.3 + bf_.abs())
    if row.null_gb:
        B["gamma"] = B["beta"] = None
    A.update(mi=_stats(xa.to(F64), gen), chain=None, post=SLOPE)
    fork = {"lo": lo, "hi": hi, "mi": None, "gamma": None, "beta": None, "post": SLOPE}
    if row.form == "block":
        tch = identity_chain(C)
        if hi > lo:
            fork.update(mi=_stats(xb[lo:hi].to(F64), gen), gamma=gf[:hi - lo], beta=bf_[:hi - lo])
            tch[lo:hi] = bn_chain32(fork["mi"], fork["gamma"], fork["beta"], SLOPE)
        B.update(mi=_stats(E.chain64(xb, tch), gen), chain=tch, post=1.0)
        fwd_b = compose32(tch, B["mi"], B["gamma"], B["beta"])
    else:
        assert hi == lo, "the ResPath3d join has no fork"
        B.update(mi=_stats(xb.to(F64), gen), chain=None, post=SLOPE)
        fwd_b = bn_chain32(B["mi"], B["gamma"], B["beta"], SLOPE)
    fwd_a = bn_chain32(A["mi"], A["gamma"], A["beta"], SLOPE)
    top.update(mi=_stats(E.lrelu(E.chain_add64(xa, fwd_a, xb, fwd_b), row.pre), gen), pre=row.pre)
    p = {"row": row, "xa": xa, "xb": xb, "dy": dy, "top": top, "A": A, "B": B, "fork": fork, "fwd_a": fwd_a, "fwd_b": fwd_b, "nudged": []}
    for _ in range(8):
        ma, mb = join_edges(p)
        n = int(ma.sum()) + int(mb.sum())
        p["nudged"].append(n)
        if n == 0:
            break
        p["xa"], p["xb"] = nudge(p["xa"], ma, bf_fwd), nudge(p["xb"], mb, bf_fwd)
    t = E.chain_add64(p["xa"], fwd_a, p["xb"], fwd_b).float()
    p["t"] = (t.to(BF).float() if bf_fwd else t) if row.t_stored else None
    return p


@functools.lru_cache(maxsize=None)
def join_problem(row):
    """The operands of a row, drawn once on the CPU, shared by its tests and never modified."""
    gen = torch.Generator().manual_seed(SEED + row.V * 7 + row.C * 3 + row.fork[0] + 11 * row.io + int(row.t_stored))
    bf_f, bf_g = bool(row.io & 1), bool(row.io & 2)
    xa, xb = E.channel_data(row.C, row.V, gen, bf_f), E.channel_data(row.C, row.V, gen, bf_f).flip(0).contiguous()
    dy = torch.randn((row.C, row.V), generator=gen)
    return build_join(row, xa, xb, dy.to(BF).float() if bf_g else dy, gen)


# ---- the restatements ----------------------------------------------------------------------------------------------------------------------
def _stage64(g_in, mag_in, x, mi, gamma, beta, chain, pre, post, keep=None):
    """One BatchNorm backward from the header — reduce, then apply with those totals — on incoming gradient g_in [C][V], together with the
    magnitudes the fp32 rounding errors of its outputs scale with (mag_in >= |g_in|, the magnitudes of g_in's own terms):
    returns dx, mag_dx, dgamma, dbeta, mag_dgamma, mag_dbeta.  keep [1][V]: weights of the elements in the sums (a mutation's)."""
    C, V = x.shape
    u, xhat, g, mag_u = E.bn_bwd_terms64(g_in, x, mi, gamma, beta, chain, pre, post)
    mg = E.bn_bwd_terms64(mag_in, x, mi, gamma, beta, chain, pre, post)[2]
    mean, invstd = _col(mi[0], x), _col(mi[1], x)
    xh_mag = invstd * (mag_u + mean.abs())
    w = 1.0 if keep is None else keep
    tot = torch.stack([(g * w).sum(1), (g * xhat * w).sum(1)], 1)
    mtot = torch.stack([mg.sum(1), (mg * xh_mag).sum(1)], 1)
    dx, dgamma, dbeta = E.bn_bwd_apply64(g_in, x, mi, gamma, beta, chain, pre, post, tot)
    a = (_col(_g32(gamma, C), x) * invstd).abs()
    mag_dx = a * (mg + mtot[:, 0:1] / V + xh_mag * mtot[:, 1:2] / V)
    return dx, mag_dx, dgamma, dbeta, mtot[:, 1], mtot[:, 0]


def join_bwd64(dy, t, fwd, top, A, B, fork, xa, xb, mutation=None):
    """dpi_join_bwd as the header composes it: reduce + apply of the top BatchNorm on (dy, t) with `pre`, post = 1, giving dt; reduce + apply
    of sides A and B on dt; on [lo, hi) reduce + apply of the fork's BatchNorm on (dxb[lo:hi], raw xb[lo:hi]).  With the float32
    mean_invstd the kernel is handed; t = None: t = T_fwd_a(xa) + T_fwd_b(xb).
    Returns a dict of what the buffers hold after a launch into NaN-filled outputs: dxa [C][V]; dxb [C][V] with NaN on the fork channels
    (their result goes to dxf); dxf [hi - lo][V] or None; dgb [6][C]; dgb_f [2][hi - lo] or None; mag_dgb / mag_dgb_f: the sums of the
    magnitudes of the terms of each per-channel output."""
    C, V = xa.shape
    lo, hi = fork["lo"], fork["hi"]
    keep = group2_keep(V, xa.device) if mutation == "group2_dropped" else None
    t64 = t.to(F64) if t is not None else E.chain_add64(xa, fwd[0], xb, fwd[1])
    dy64 = dy.to(F64)
    dt, mdt, dg, db, mg, mb = _stage64(dy64, dy64.abs(), t64, top["mi"], top["gamma"], top["beta"], None, top["pre"], 1.0, keep)
    dxa, _, dga, dba, mga, mba = _stage64(dt, mdt, xa, A["mi"], A["gamma"], A["beta"], A["chain"], 1.0, A["post"], keep)
    dxb, mdxb, dgb_, dbb, mgb, mbb = _stage64(dt, mdt, xb, B["mi"], B["gamma"], B["beta"], B["chain"], 1.0, B["post"], keep)
    out = {"dxa": dxa, "dxf": None, "dgb_f": None, "mag_dgb_f": None,
           "dgb": torch.stack([dg, db, dga, dba, dgb_, dbb]).cpu(), "mag_dgb": torch.stack([mg, mb, mga, mba, mgb, mbb]).cpu()}
    if hi > lo:
        n = hi - lo
        mi_f, gam_f, bet_f = fork["mi"], fork["gamma"], fork["beta"]
        if mutation == "fork_index_c":         # the constants read at c, not c - lo: [mean | invstd] is one array; what lies behind an array is 1
            flat = torch.cat([mi_f.reshape(-1), torch.ones(2 * C)])
            idx = torch.arange(lo, hi)
            mi_f = torch.stack([flat[idx], flat[n + idx]])
            gam_f, bet_f = torch.cat([gam_f, torch.ones(C)])[idx], torch.cat([bet_f, torch.ones(C)])[idx]
        dxf, _, dgf, dbf, mgf, mbf = _stage64(dxb[lo:hi], mdxb[lo:hi], xb[lo:hi], mi_f, gam_f, bet_f, None, 1.0, fork["post"], keep)
        out.update(dgb_f=torch.stack([dgf, dbf]).cpu(), mag_dgb_f=torch.stack([mgf, mbf]).cpu())
        dxb = dxb.clone()
        if mutation == "fork_to_dxb":
            dxb[lo:hi] = dxf
            out["dxf"] = torch.full_like(dxf, float("nan"))
        else:
            dxb[lo:hi] = float("nan")
            out["dxf"] = dxf
    out["dxb"] = dxb
    return out


def join_ref(p, mutation=None):
    return join_bwd64(p["dy"], p["t"], (p["fwd_a"], p["fwd_b"]), p["top"], p["A"], p["B"], p["fork"], p["xa"], p["xb"], mutation)


def _terms(dy, x, mi, gamma, beta, chain, pre, post):
    u, xhat, g, mag_u = E.bn_bwd_terms64(dy, x, mi, gamma, beta, chain, pre, post)
    return xhat, g, _col(mi[1], x) * (mag_u + _col(mi[0], x).abs())


def fork64(dy, x, mi, gamma, beta, in_chain, pre, post, totals):
    """dpi_bn_bwd_apply_fork's own outputs from caller-given totals [C][2] = {sum g, sum g xhat}:
    dx = gamma invstd (g - sum_g / V - xhat sum_gxhat / V) act_pre'(x), dgamma = sum_gxhat, dbeta = sum_g."""
    C, V = x.shape
    xhat, g, _ = _terms(dy, x, mi, gamma, beta, in_chain, pre, post)
    tot = totals.to(device=x.device, dtype=F64)
    a = _col(_g32(gamma, C), x) * _col(mi[1], x)
    du = a * (g - tot[:, 0:1] / V - xhat * (tot[:, 1:2] / V))
    dx = torch.where(x.to(F64) > 0, du, du * pre) if in_chain is None and pre != 1.0 else du
    return dx, tot[:, 1].clone(), tot[:, 0].clone()


def followup64(dx, xs, mi, gamma, beta, chain, post, nblk=None):
    """The partial rows [nblk][C][2] = {sum g, sum g xhat} a follow-up BatchNorm (input xs, value-only chain, activation `post` behind it)
    takes of a GIVEN incoming gradient dx, span by span, and the magnitudes of their terms (for elementwise_cases.check_partials)."""
    xhat, g, xh_mag = _terms(dx, xs, mi, gamma, beta, chain, 1.0, post)
    ref = torch.stack([E.span_sums(g, nblk), E.span_sums(g * xhat, nblk)], 2)
    return ref, torch.stack([E.span_sums(g.abs(), nblk), E.span_sums(g.abs() * xh_mag, nblk)], 2)


def dual64(dy, A, xa, tot_a, B, xb, tot_b):
    """dpi_bn_bwd_apply_dual: phase 2 of the two sides on the shared incoming gradient (pre = 1, their chains value-only), from
    caller-given totals: (dxa, dgamma_a, dbeta_a), (dxb, dgamma_b, dbeta_b)."""
    return (fork64(dy, xa, A["mi"], A["gamma"], A["beta"], A["chain"], 1.0, A["post"], tot_a),
            fork64(dy, xb, B["mi"], B["gamma"], B["beta"], B["chain"], 1.0, B["post"], tot_b))


def dual_fork_partials64(dxb, xb, fork, nblk=None):
    """f_partials [nblk][hi - lo][2] of a GIVEN dxb against the raw xb on the fork range."""
    lo, hi = fork["lo"], fork["hi"]
    return followup64(dxb[lo:hi], xb[lo:hi], fork["mi"], fork["gamma"], fork["beta"], None, fork["post"], nblk)


# ---- float64 autograd of the forward expressions -------------------------------------------------------------------------------------------
def join_autograd64(p):
    """The gradients dpi_join_bwd returns, by float64 autograd of y = BN(act_pre(t)) built from torch primitives with each BatchNorm's own
    train-mode statistics (rows with genuine statistics only): dxa = dL/dxa, dxb = dL/d(T_CH(xb)), dxf = dL/dxb[lo:hi], dgb, dgb_f."""
    row, top, A, B, fk = p["row"], p["top"], p["A"], p["B"], p["fork"]
    C = row.C
    lo, hi = row.fork

    def bn(u, gamma, beta):
        m = u.mean(1, keepdim=True)
        v = ((u - m) ** 2).mean(1, keepdim=True)
        return (u - m) / torch.sqrt(v + E.EPS) * gamma[:, None] + beta[:, None]
    leaf = lambda v, n, fill: (torch.full((n,), fill, dtype=F64) if v is None else v.double()).requires_grad_()
    par = [leaf(d[k], C, f) for d in (top, A, B) for k, f in (("gamma", 1.0), ("beta", 0.0))]
    xa = p["xa"].double().requires_grad_()
    xb = p["xb"].double().requires_grad_()
    ub, gf, bf_ = xb, None, None
    if row.form == "block":
        if hi > lo:
            gf, bf_ = fk["gamma"].double().requires_grad_(), fk["beta"].double().requires_grad_()
            ub = torch.cat([xb[:lo], E.lrelu(bn(xb[lo:hi], gf, bf_), SLOPE), xb[hi:]], 0)
        ub = ub + 0.0
        ub.retain_grad()
        t = E.lrelu(bn(xa, par[2], par[3]), SLOPE) + bn(ub, par[4], par[5])
    else:
        t = E.lrelu(bn(xa, par[2], par[3]), SLOPE) + E.lrelu(bn(xb, par[4], par[5]), SLOPE)
    y = bn(E.lrelu(t, row.pre), par[0], par[1])
    (y * p["dy"].double()).sum().backward()
    dxb = (ub.grad if row.form == "block" else xb.grad).clone()
    out = {"dxa": xa.grad, "dxf": None, "dgb_f": None, "dgb": torch.stack([q.grad for q in par])}
    if hi > lo:
        dxb[lo:hi] = float("nan")
        out.update(dxf=xb.grad[lo:hi], dgb_f=torch.stack([gf.grad, bf_.grad]))
    out["dxb"] = dxb
    return out


# ---- the checks of the device test -----------------------------------------------------------------------------------------------------------
def written(t, what):
    bad = int((~torch.isfinite(t.float())).sum())
    assert bad == 0, "%s: %d elements were not written (NaN pre-fill left)" % (what, bad)


def stored_ok(got, ref64, what, bar=DX_BAR):
    """A stored tensor against the float64 restatement: `bar` norm-wise for fp32, half a bf16 ulp (slack 0.503) for a bf16 tensor.
    Returns the norm-wise figure (fp32)."""
    written(got, what)
    if got.dtype == BF:
        from test_gpu_bf16_storage import half_ulp_ok
        half_ulp_ok(got, ref64.reshape(got.shape), what)
        return 0.0
    r = E.rel(got, ref64)
    assert r < bar, "%s: off by %.3g norm-wise (bar %.3g)" % (what, r, bar)
    return r


def vectors_ok(got, ref, mag, V, what):
    """Per-channel gradients [rows][n]: each row (one gradient vector) at VEC_BAR norm-wise; with a handful of voxels (V <= 5, handed
    statistics) every element against the magnitudes of its terms: |got - ref| <= VEC_BAR sum|term|.  Returns the worst figure."""
    got, ref, mag = got.detach().cpu().to(F64), ref.detach().cpu().to(F64), mag.detach().cpu().to(F64)
    assert got.shape == ref.shape == mag.shape, (what, got.shape, ref.shape)
    written(got, what)
    worst = 0.0
    for i in range(ref.shape[0]):
        if V <= 5:
            ratio = float(((got[i] - ref[i]).abs() / (VEC_BAR * mag[i] + 1e-300)).max())
            assert ratio <= 1.0, "%s row %d: off by %.3g x (2e-4 sum|term|)" % (what, i, ratio)
            worst = max(worst, ratio * VEC_BAR)
        else:
            r = E.rel(got[i], ref[i])
            assert r < VEC_BAR, "%s row %d: off by %.3g norm-wise (bar %.3g)" % (what, i, r, VEC_BAR)
            worst = max(worst, r)
    return worst


def check_join(got, ref, lo, hi, V):
    """What the device test asserts of a dpi_join_bwd launch into NaN-filled outputs `got` (dxa, dxb, dxf, dgb [6][C], dgb_f), against the
    restatement's dict `ref`.  Returns the worst (tensor, vector) figures."""
    C = ref["dxa"].shape[0]
    worst_t = stored_ok(got["dxa"], ref["dxa"], "dxa")
    keep = [c for c in range(C) if not lo <= c < hi]
    if keep:
        worst_t = max(worst_t, stored_ok(got["dxb"][keep], ref["dxb"][keep], "dxb off the fork range"))
    if hi > lo:
        assert bool(torch.isnan(got["dxb"][lo:hi].float()).all()), "dxb was written on the fork range, whose result belongs in dxf"
        assert got["dxf"] is not None and got["dgb_f"] is not None
        worst_t = max(worst_t, stored_ok(got["dxf"], ref["dxf"], "dxf"))
    worst_v = vectors_ok(got["dgb"], ref["dgb"], ref["mag_dgb"], V, "dgb")
    if hi > lo:
        worst_v = max(worst_v, vectors_ok(got["dgb_f"], ref["dgb_f"], ref["mag_dgb_f"], V, "dgb_f"))
    return worst_t, worst_v


# ---- operands of the fork / dual launches ----------------------------------------------------------------------------------------------------
def fork_edges(p):
    S, A, B = p["S"], p["A"], p["B"]
    x = p["x"]
    mx = torch.zeros(x.shape, dtype=torch.bool)
    if S["post"] != 1.0:
        pre_chain = S["chain"] if S["chain"] is not None else torch.tensor([[1.0, 0.0, S["pre"], 1.0, 0.0]] * x.shape[0])
        mx = mx | out_edge(x, S["mi"], S["gamma"], S["beta"], pre_chain)
    if S["chain"] is not None:
        mx = mx | inner_edge(x, S["chain"])
    ma = out_edge(p["xa"], A["mi"], A["gamma"], A["beta"], None)
    mb = out_edge(p["xb"], B["mi"], B["gamma"], B["beta"], B["chain"]) | inner_edge(p["xb"], B["chain"])
    return mx, ma, mb


@functools.lru_cache(maxsize=None)
def fork_problem(V, io, form):
    """dpi_bn_bwd_apply_fork, C = 3: the BatchNorm itself on (dy, x) in one of FORK_FORMS and two follow-up BatchNorms, A on xa with
    post 0.2 and B on T_chain_b(xb) with post 0.2; frozen statistics, then x / xa / xb nudged off the jumps of the three masks."""
    C = 3
    gen = torch.Generator().manual_seed(9000 + V * 5 + io * 3 + form)
    bf_f, bf_g = bool(io & 1), bool(io & 2)
    pre, post, chained = FORK_FORMS[form]
    x, xa, xb = (E.channel_data(C, V, gen, bf_f) for _ in range(3))
    dy = torch.randn((C, V), generator=gen)
    dy = dy.to(BF).float() if bf_g else dy
    in_chain = E.chain_table(C, gen) if chained else None
    chain_b = E.chain_table(C, gen, identity=(0,))
    S, A, B = ({"gamma": g, "beta": b} for g, b in [_vecs(C, gen) for _ in range(3)])
    u = E.chain64(x, in_chain) if chained else E.lrelu(x.double(), pre)
    S.update(mi=_stats(u, gen), chain=in_chain, pre=pre, post=post)
    A.update(mi=_stats(xa.double(), gen), chain=None, post=SLOPE)
    B.update(mi=_stats(E.chain64(xb, chain_b), gen), chain=chain_b, post=SLOPE)
    p = {"x": x, "xa": xa, "xb": xb, "dy": dy, "S": S, "A": A, "B": B, "nudged": []}
    for _ in range(8):
        m = fork_edges(p)
        p["nudged"].append(sum(int(v.sum()) for v in m))
        if p["nudged"][-1] == 0:
            break
        p["x"], p["xa"], p["xb"] = [nudge(p[k], v, bf_f) for k, v in zip(("x", "xa", "xb"), m)]
    return p


@functools.lru_cache(maxsize=None)
def dual_problem(C, V, fork, form, io):
    """dpi_bn_bwd_apply_dual: the two sides of a join on a shared incoming gradient dy (= dt), built as a dpi_join_bwd row of the same
    layout is: posts (0.2, 1) with chain_b = T_CH (block) or (0.2, 0.2) without chains (respath).  A respath row keeps its fork range:
    BN_f then reads the raw xb as everywhere, its output just feeds nothing."""
    lo, hi = fork
    row = JoinRow(C, V, fork if form == "block" else (0, 0), form, True, SLOPE, io, False)
    gen = torch.Generator().manual_seed(11000 + V * 3 + C + lo + 7 * io)
    bf_f, bf_g = bool(io & 1), bool(io & 2)
    xa, xb = E.channel_data(C, V, gen, bf_f), E.channel_data(C, V, gen, bf_f).flip(0).contiguous()
    dy = torch.randn((C, V), generator=gen)
    p = build_join(row, xa, xb, dy.to(BF).float() if bf_g else dy, gen)
    if form != "block" and hi > lo:
        g, b = _vecs(hi - lo, gen)
        p["fork"] = {"lo": lo, "hi": hi, "mi": _stats(p["xb"][lo:hi].double(), gen), "gamma": g, "beta": b, "post": SLOPE}
        for _ in range(8):                       # the fork's own jump on the raw xb, and side B's again for what moved
            mb = join_edges(p)[1]
            p["nudged"].append(int(mb.sum()))
            if p["nudged"][-1] == 0:
                break
            p["xb"] = nudge(p["xb"], mb, bf_f)
    p["fork"] = dict(p["fork"], lo=lo, hi=hi)
    return p
