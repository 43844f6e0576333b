"""The launches of csrc/elementwise.hip whose contract tests/test_gpu_elementwise_contract.py checks on a device: the case rows, and float64
restatements of every entry point written from include/dpi_hip.h and the formulas in the kernels' comments (torch on the CPU or wherever the
operands live; the library is never called).  A plain module: no fixtures, importable without a GPU.  tests/test_elementwise_refs_host.py
holds every restatement against independent torch code and proves, restatement against restatement, that the checks below catch a wrong
kernel (MUTATIONS).

Why each row exists (span = stat_span(V, nblk) voxels per block, nblk = dpi_stat_blocks = min(ceil(V / 16384), 2048)):

 V_ROWS (C = 3; channel_stats, chain_apply, bn_bwd_reduce, bn_bwd_apply, chain_add_stats, chain_add_apply, channel_sum)
   1, 3        one block, one thread, scalar path: `i + k < end` with end < 4
   4           one float4: the smallest vector-path launch
   5           scalar path, a second thread with one element
   1023        scalar path, the last thread has 3 elements (the only size below 1024 that leaves thread 255 a partial group)
   1287        scalar path, second trip of the `i += 1024` loop with a 3-element tail (5 x 7 x 9 x ... odd voxel counts of the nets)
   16384       exactly one full block (what test_bn_large_offset reaches)
   16385       2 blocks, scalar path, span 8196: start of block 1, `end` clamp of the last span (8189 voxels), 1-element tail
   16388       2 blocks, vector path, span 8196, last span 8192
   32772       3 blocks, vector path, span 10924, partial last span
   49153       4 blocks, scalar path, span 12292 (a multiple of 4 although V is odd), 1-element tail
   bf16 rows   1287, 16385, 16388 through the _io entry points (forward and gradient tensors bf16)
 LARGE_V = 2048 * 16384 + 16388 (C = 1): C V >= 32 Mi floats takes the non-temporal loads and stores, the block count is capped at 2048 so a
   span (16396) exceeds 16384 and every thread makes 17 trips, and the apply kernels' grids are capped at 4096 blocks so their grid-stride
   loop runs; LARGE_V + 1 is the same on the scalar path.
 FINALIZE_NBLK (dpi_bn_finalize, 256 threads, `for (; b + 256 < nblk; b += 512)` + remainder)
   1, 2        remainder only;  63, 64, 65   around one wave;  255, 256, 257   first trip of the two-load loop starts at 257
   511, 512, 513   512: no remainder row at all, 513: second trip's remainder;  768, 769   remainder in the upper half
   2048        the cap of dpi_stat_blocks;  8192   what a convolution at 256 x 128 x 128 hands over
 APPLY_NBLK (dpi_bn_bwd_apply's one-wave prologue, stride 64): 1, 63, 64, 65, 2048
 UPSAMPLE_ROWS ((D, H, W) -> (Do, Ho, Wo); each row's `why` field says the same and the host test asserts it from the sizes)
   (3,4,5) -> (6,8,9)       cube kernel, crop along W only: the `2 w + 1 < Wo` store predicate
   (3,4,5) -> (5,7,9)       cube kernel, every axis cropped (`od >= Do`, `oh >= Ho`); bf16: packed pair store and its odd-offset fall-back
   (2,3,2) -> (4,6,4)       adjoint: row-pair W pass at n = 2, both neighbour taps clamped
   (1,4,6) -> (2,8,12)      D = 1 scaled: generic forward kernel, D pass of the adjoint with n = 1
   (3,1,5) -> (6,2,10)      H = 1: generic forward kernel;  (3,4,1) -> (6,8,2)   W = 1: generic forward kernel, one-element slabs
   (1,5,6) -> (1,10,12)     2-D: cube kernel without D taps, two-pass adjoint;  -> (1,9,11)   cropped, odd Wo (bf16 rows at odd offsets)
   (1,2,260) -> (1,4,520)   slabs of 260 (W pass, axis kernel) and 520 (H pass) elements: `per == 1`, several workgroups per slab
   (64,33,2) -> (128,66,4)  C = 4: 33792 rows, the `gy` halving loop and the slab stride of the W pass
   every row's adjoint runs with the workspace (separable passes), without (gather kernel) and with dy moved by one float (axis kernel
   instead of the row-pair kernel); nearest mode on rows 1, 2 and 4
 CROP_WINDOWS: a window flush with each of the six faces, an interior one, the whole tensor, one voxel (far corner, interior)
 FIR_K x FIR_T x FIR_S: K = 1 (no neighbours), 3, 9 with T = 1, 2 (K > T: every tap but one falls outside), 9, 40; S = 1, 7, 64 (rows of
   one element, odd rows, a row per wave)
 ACT_N: 1, 3 (scalar path), 4 (one float4), 5, 1027 (scalar, several blocks), 4096 (vector); also the n of add / axpy / lrelu_bwd

Precondition of every row (include/dpi_hip.h): the vector paths here are chosen from V % 4 (n % 4) alone, so a tensor with V % 4 == 0 is
handed over 16-byte aligned (bf16: 8-byte), as a channel slice of a 256-byte-aligned buffer is.  Element-aligned bases appear only with
V % 4 != 0.
"""
from collections import namedtuple

import torch
import torch.nn.functional as F

from oracle import dpi_oracle as O

F64 = torch.float64
STAT_SPAN, MAX_STAT_BLOCKS, NT_MIN_FLOATS, EW_MAX_BLOCKS = 16384, 2048, 32 << 20, 4096
U = 2.0 ** -24                                    # unit round-off of fp32
EPS, MOMENTUM = 1e-5, 0.1
ACT_ELU, ACT_TANH, ACT_SIGMOID = 1, 2, 3

# What a wrong kernel would do, modelled in the restatements (argument `mutation`); the host test shows that the device test's checks fail
# on the rows named for that edge.
MUTATIONS = ("span_start+4", "tail<=", "finalize_no_remainder", "no_w_crop", "fir_centre-1")


# ---- sizes -------------------------------------------------------------------------------------------------------------------------------
def stat_blocks(C, V):
    return 0 if C <= 0 or V == 0 else min(-(-V // STAT_SPAN), MAX_STAT_BLOCKS)


def stat_span(V, nblk):
    return (-(-V // nblk) + 3) & ~3


def spans(V, nblk=None, mutation=None):
    """[(beg, end)] of the nblk blocks of one channel."""
    nblk = stat_blocks(1, V) if nblk is None else nblk
    s = stat_span(V, nblk)
    out = []
    for b in range(nblk):
        beg, end = b * s, min(b * s + s, V)
        if mutation == "span_start+4" and b > 0:
            beg += 4
        out.append((min(beg, end), end))
    return out


def ew_blocks(n):
    return max(1, min(-(-n // 256), EW_MAX_BLOCKS))


VRow = namedtuple("VRow", "V nblk span last vec")      # last: voxels of the last span; vec: the float4 path
V_ROWS = [VRow(1, 1, 4, 1, False), VRow(3, 1, 4, 3, False), VRow(4, 1, 4, 4, True), VRow(5, 1, 8, 5, False), VRow(1023, 1, 1024, 1023, False),
          VRow(1287, 1, 1288, 1287, False), VRow(16384, 1, 16384, 16384, True), VRow(16385, 2, 8196, 8189, False),
          VRow(16388, 2, 8196, 8192, True), VRow(32772, 3, 10924, 10924, True), VRow(49153, 4, 12292, 12277, False)]
V_ROWS_BF16 = [r for r in V_ROWS if r.V in (1287, 16385, 16388)]
LARGE_V = 2048 * 16384 + 16388
FINALIZE_NBLK = (1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513, 768, 769, 2048, 8192)
APPLY_NBLK = (1, 63, 64, 65, 2048)

UpRow = namedtuple("UpRow", "C inp out nearest bf16 why")
UPSAMPLE_ROWS = [
    UpRow(2, (3, 4, 5), (6, 8, 9), True, False, "cube kernel, crop along W only: the `2 w + 1 < Wo` store predicate"),
    UpRow(2, (3, 4, 5), (5, 7, 9), True, True, "cube kernel, every axis cropped; bf16: packed pair and its odd-offset fall-back"),
    UpRow(2, (2, 3, 2), (4, 6, 4), False, False, "adjoint: row-pair W pass at n = 2 (both neighbours clamped)"),
    UpRow(2, (1, 4, 6), (2, 8, 12), True, False, "D = 1 scaled: generic forward kernel, D pass of the adjoint with n = 1"),
    UpRow(2, (3, 1, 5), (6, 2, 10), False, False, "H = 1: generic forward kernel, H pass with n = 1"),
    UpRow(2, (3, 4, 1), (6, 8, 2), False, False, "W = 1: generic forward kernel, W pass with n = 1 (slab of one element)"),
    UpRow(2, (1, 5, 6), (1, 10, 12), False, False, "2-D (D = Do = 1): cube kernel without the D taps, two-pass adjoint"),
    UpRow(2, (1, 5, 6), (1, 9, 11), False, True, "2-D cropped, odd Wo: bf16 rows start at odd element offsets"),
    UpRow(2, (1, 2, 260), (1, 4, 520), False, False, "W pass with a slab of 260 >= 256 elements: per == 1, two workgroups per slab"),
    UpRow(4, (64, 33, 2), (128, 66, 4), False, False, "33792 rows > 16384: the gy halving loop and the row stride of the W pass"),
]

CROP_SHAPE = (4, 5, 6)                                  # (D, H, W) of the source, C = 2
CROP_WINDOWS = [                                        # (od, oh, ow, Do, Ho, Wo)
    (0, 1, 1, 2, 3, 4), (2, 1, 1, 2, 3, 4),             # the two D faces
    (1, 0, 1, 2, 3, 4), (1, 2, 1, 2, 3, 4),             # the two H faces
    (1, 1, 0, 2, 3, 4), (1, 1, 2, 2, 3, 4),             # the two W faces
    (1, 1, 1, 2, 3, 4),                                 # interior
    (0, 0, 0, 4, 5, 6),                                 # the whole tensor
    (3, 4, 5, 1, 1, 1), (1, 2, 3, 1, 1, 1),             # one voxel: the far corner, the interior
]
FIR_K, FIR_T, FIR_S = (1, 3, 9), (1, 2, 9, 40), (1, 7, 64)
ACT_N = (1, 3, 4, 5, 1027, 4096)


# ---- operands ----------------------------------------------------------------------------------------------------------------------------
def chain_table(C, gen, identity=(1,)):
    """[C][5] = {ps, pb, slope, qs, qb}; the channels in `identity` carry the identity transform."""
    ch = torch.stack([torch.rand(C, generator=gen) + 0.5, torch.randn(C, generator=gen) * 0.3, torch.full((C,), 0.2),
                      torch.rand(C, generator=gen) + 0.5, torch.randn(C, generator=gen) * 0.1], 1)
    for c in identity:
        if c < C:
            ch[c] = torch.tensor([1.0, 0.0, 1.0, 1.0, 0.0])
    return ch.contiguous()


def channel_data(C, V, gen, bf16=False, device="cpu"):
    """[C][V] floats, channel c around offset_c with scale_c (|mean| / std up to 5, the regime of the nets' activations)."""
    off = torch.tensor([3.0, -1.5, 0.25, 0.0, -4.0])[:C].reshape(C, 1)
    scale = torch.tensor([1.0, 2.5, 0.6, 1.3, 0.8])[:C].reshape(C, 1)
    x = torch.randn((C, V), generator=gen, device=device) * scale.to(device) + off.to(device)
    return x.to(torch.bfloat16).float() if bf16 else x


def mean_invstd_of(u64):
    """float32 [2][C] of the float64 tensor the BatchNorm normalised: what dpi_bn_finalize hands the backward kernels."""
    m = u64.mean(1)
    v = ((u64 - m[:, None]) ** 2).mean(1)
    return torch.stack([m, 1.0 / torch.sqrt(v + EPS)]).float()


def act_inputs(n, gen):
    """[-100, 100] plus +-0 and values near 0 (expm1f is where ELU goes wrong), n values."""
    special = torch.tensor([0.0, -0.0, 1e-8, -1e-8, 1e-4, -1e-4, 100.0, -100.0, -1.0, 1.0, -20.0, 20.0, -88.0, 88.0, -0.5, 0.5])
    if n < 16:
        return special[[6, 7, 3, 1, 4][:n]].contiguous()
    body = torch.cat([(torch.rand(n, generator=gen) * 2 - 1) * 100, torch.randn(n, generator=gen), torch.randn(n, generator=gen) * 1e-3])
    x = torch.cat([special, body[torch.randperm(3 * n, generator=gen)][:n - 16]])
    return x[torch.randperm(n, generator=gen)].contiguous()


# ---- chains and statistics ---------------------------------------------------------------------------------------------------------------
def lrelu(v, slope):
    return torch.where(v > 0, v, v * slope)


def chain64(x, chain):
    """T(x) = qs act_slope(ps x + pb) + qb per channel of x [C][...]; chain None: the identity."""
    x = x.to(F64)
    if chain is None:
        return x
    ch = chain.to(device=x.device, dtype=F64).reshape((x.shape[0], 5) + (1,) * (x.ndim - 1))
    return ch[:, 3] * lrelu(ch[:, 0] * x + ch[:, 1], ch[:, 2]) + ch[:, 4]


def chain_mag64(x, chain):
    """|qs act(ps x + pb)| + |qb| >= |T(x)|: the magnitude the rounding errors of an fp32 evaluation of T scale with."""
    x = x.to(F64)
    if chain is None:
        return x.abs()
    ch = chain.to(device=x.device, dtype=F64).reshape((x.shape[0], 5) + (1,) * (x.ndim - 1))
    return (ch[:, 3] * lrelu(ch[:, 0] * x + ch[:, 1], ch[:, 2])).abs() + ch[:, 4].abs()


def span_sums(y, nblk=None, mutation=None, beyond=None):
    """[nblk][C] float64 sums of y [C][V] over the spans.  `tail<=` also takes the element behind a span that is no multiple of 4 long
    (`beyond` [C]: what lies behind the channel's last voxel — the next channel's first)."""
    C, V = y.shape
    nblk = stat_blocks(C, V) if nblk is None else nblk
    s = stat_span(V, nblk)
    if mutation is None:
        pad = torch.zeros((C, nblk * s - V), dtype=F64, device=y.device)
        return torch.cat([y.to(F64), pad], 1).reshape(C, nblk, s).sum(2).t().contiguous()
    out = torch.zeros((nblk, C), dtype=F64)
    for b, (beg, end) in enumerate(spans(V, nblk, mutation)):
        out[b] = y[:, beg:end].to(F64).sum(1)
        if mutation == "tail<=" and (end - beg) % 4 and beg < end:
            out[b] += y[:, end].to(F64) if end < V else beyond.to(F64)
    return out


def partials64(y, nblk=None, mutation=None, beyond=None):
    """[nblk][C][2] = {sum y, sum y^2} over the spans."""
    return torch.stack([span_sums(y, nblk, mutation, beyond), span_sums(y * y, nblk, mutation, None if beyond is None else beyond * beyond)], 2)


def check_partials(got, ref, mag, k, what, span_len=STAT_SPAN):
    """|got - ref| <= (k 2^-24 + n 2^-53) sum|term| for every partial: `mag` [nblk][C][2] are the float64 sums of the terms' magnitudes over
    the same spans, k counts the fp32 roundings a term passes (derived at each call), n 2^-53 covers the double accumulation."""
    got, ref, mag = got.detach().cpu().to(F64), ref.detach().cpu().to(F64), mag.detach().cpu().to(F64)
    assert got.shape == ref.shape == mag.shape, (what, got.shape, ref.shape, mag.shape)
    assert bool(torch.isfinite(got).all()), "%s: %d partials were not written" % (what, int((~torch.isfinite(got)).sum()))
    bound = (torch.as_tensor(k, dtype=F64) * U + span_len * 2.0 ** -53) * mag + 1e-300
    ratio = (got - ref).abs() / bound
    assert float(ratio.max()) <= 1.0, "%s: partial %s is off by %.3g x its bound (got %.17g, float64 %.17g)" % (
        what, tuple(int(i) for i in torch.nonzero(ratio == ratio.max())[0]), float(ratio.max()), float(got.flatten()[ratio.argmax()]),
        float(ref.flatten()[ratio.argmax()]))


def rel(a, b):
    a, b = a.detach().to(F64).cpu().reshape(-1), b.detach().to(F64).cpu().reshape(-1)
    return float((a - b).norm() / (b.norm() + 1e-300))


# ---- finalise ----------------------------------------------------------------------------------------------------------------------------
def synthetic_partials(nblk, C, seed=0):
    """[nblk][C][2] doubles in pairs of rows (m + d, -m), m in [1, 2) and different for every pair and channel: the totals stay small
    (sum d), so one dropped or doubled row moves a statistic by tens of percent, at every nblk."""
    b = torch.arange(nblk, dtype=F64).reshape(-1, 1, 1)
    j = torch.floor(b / 2) + 1
    c = torch.arange(C, dtype=F64).reshape(1, C, 1)
    k = torch.tensor([0.0, 1.0], dtype=F64).reshape(1, 1, 2)
    m = 1.0 + torch.frac(j * 0.6180339887 + c * 0.377 + k * 0.1931 + seed * 0.0917)
    d = torch.where(k == 0, 0.02 * (torch.frac(j * 0.7548776662 + c * 0.21) - 0.5), 0.01 + 0.02 * torch.frac(j * 0.5698402910 + c * 0.13))
    return torch.where(b % 2 == 0, m + d, -m).contiguous()


def finalize_totals(partials, mutation=None):
    """[C][2] totals of [nblk][C][2]; `finalize_no_remainder` drops the rows the kernel's remainder statement adds (256 threads, thread l
    takes rows l, l + 256 of every 512 while both exist, then one more)."""
    if mutation != "finalize_no_remainder":
        return partials.sum(0)
    nblk = partials.shape[0]
    keep = torch.zeros(nblk, dtype=torch.bool)
    for lane in range(256):
        b = lane
        while b + 256 < nblk:
            keep[b] = keep[b + 256] = True
            b += 512
    return partials[keep].sum(0)


def finalize64(partials, count, gamma, beta, eps=EPS, momentum=MOMENTUM, slope=1.0, act_first=0, in_chain=None, running_mean=None,
               running_var=None, nbt=None, mutation=None):
    """dpi_bn_finalize: mean, invstd (biased variance), running statistics (momentum, unbiased variance), num_batches_tracked + 1 and the
    three chain_out forms.  Returns a dict of float64 tensors."""
    tot = finalize_totals(partials.to(F64), mutation)
    C = tot.shape[0]
    mean = tot[:, 0] / count
    var = (tot[:, 1] / count - mean * mean).clamp_min(0.0)
    invstd = 1.0 / torch.sqrt(var + eps)
    out = {"mean_invstd": torch.stack([mean, invstd])}
    if running_mean is not None:
        out["running_mean"] = (1 - momentum) * running_mean.to(F64) + momentum * mean
    if running_var is not None:
        out["running_var"] = (1 - momentum) * running_var.to(F64) + momentum * (var * (count / (count - 1.0)) if count > 1 else var)
    if nbt is not None:
        out["nbt"] = int(nbt) + 1
    g = torch.ones(C, dtype=F64) if gamma is None else gamma.to(F64)
    bt = torch.zeros(C, dtype=F64) if beta is None else beta.to(F64)
    a, shift = g * invstd, bt - mean * g * invstd
    one, zero, sl = torch.ones(C, dtype=F64), torch.zeros(C, dtype=F64), torch.full((C,), slope, dtype=F64)
    if in_chain is not None:
        ic = in_chain.to(F64)
        out["chain_out"] = torch.stack([ic[:, 0], ic[:, 1], ic[:, 2], a * ic[:, 3], a * ic[:, 4] + shift], 1)
    elif act_first:
        out["chain_out"] = torch.stack([one, zero, sl, a, shift], 1)
    else:
        out["chain_out"] = torch.stack([a, shift, sl, one, zero], 1)
    return out


# ---- BatchNorm backward ------------------------------------------------------------------------------------------------------------------
def bn_bwd_terms64(dy, x, mi, gamma, beta, in_chain, pre, post):
    """Per element, from the header: u (what was normalised), xhat = (u - mean) invstd and g = dy act_post'(gamma xhat + beta), with the
    float32 mean / invstd the kernels are given.  The activation mask is taken from a u + (beta - mean a), a = gamma invstd formed in
    float32 as dpi_bn_finalize's chain forms it (the sign of an fp32 fma of those constants is the sign of this float64 expression).
    Also returns mag_u >= |u|, the magnitude u's fp32 rounding errors scale with."""
    C = x.shape[0]
    dev = x.device
    x64, dy64 = x.to(F64), dy.to(F64)
    mean, invstd = mi[0].to(dev).reshape(C, 1), mi[1].to(dev).reshape(C, 1)
    g32 = torch.ones(C) if gamma is None else gamma.float()
    b32 = torch.zeros(C) if beta is None else beta.float()
    a32 = g32.to(dev).reshape(C, 1) * invstd.float()
    pb32 = b32.to(dev).reshape(C, 1) - mean.float() * a32
    u = chain64(x64, in_chain) if in_chain is not None else lrelu(x64, pre)
    mag_u = chain_mag64(x64, in_chain) if in_chain is not None else u.abs()
    xhat = (u - mean.to(F64)) * invstd.to(F64)
    yv = a32.to(F64) * u + pb32.to(F64)
    g = dy64 if post == 1.0 else torch.where(yv > 0, dy64, dy64 * post)
    return u, xhat, g, mag_u


def post_edge64(x, mi, gamma, beta, in_chain, pre, margin=1e-5):
    """Mask of the elements whose BatchNorm output a u + (beta - mean a) lies within `margin` of 0, relative to |a u| + |beta - mean a|.
    act_post' jumps there, and the kernels are handed float32 statistics where float64 autograd forms its own: such an element may take
    either side (the statistics' rounding moves the output by about 1e-7 of those terms).  A test gives these elements dy = 0, which makes
    both sides agree without touching x or any statistic."""
    C = x.shape[0]
    mean, invstd = mi[0].reshape(C, 1).float(), mi[1].reshape(C, 1).float()
    a32 = (torch.ones(C) if gamma is None else gamma.float()).reshape(C, 1) * invstd
    pb32 = (torch.zeros(C) if beta is None else beta.float()).reshape(C, 1) - mean * a32
    u = chain64(x, in_chain) if in_chain is not None else lrelu(x.to(F64), pre)
    au = a32.to(F64) * u
    return (au + pb32.to(F64)).abs() <= margin * (au.abs() + pb32.to(F64).abs())


def bn_bwd_partials64(dy, x, mi, gamma, beta, in_chain, pre, post, nblk=None, mutation=None):
    """Phase 1: ([nblk][C][2] {sum g, sum g xhat}, the magnitudes of the terms for check_partials)."""
    u, xhat, g, mag_u = bn_bwd_terms64(dy, x, mi, gamma, beta, in_chain, pre, post)
    C = x.shape[0]
    invstd, mean = mi[1].to(x.device, F64).reshape(C, 1), mi[0].to(x.device, F64).reshape(C, 1)
    beyond = None
    if mutation == "tail<=":                 # what lies behind a channel: the next channel's first element (0 behind the last)
        beyond = (torch.cat([g[1:, 0], g.new_zeros(1)]), torch.cat([(g * xhat)[1:, 0], g.new_zeros(1)]))
    ref = torch.stack([span_sums(g, nblk, mutation, beyond and beyond[0]), span_sums(g * xhat, nblk, mutation, beyond and beyond[1])], 2)
    mag = torch.stack([span_sums(g.abs(), nblk), span_sums(g.abs() * invstd * (mag_u + mean.abs()), nblk)], 2)
    return ref, mag


def bn_bwd_apply64(dy, x, mi, gamma, beta, in_chain, pre, post, totals):
    """Phase 2 from the header: dx = gamma invstd (g - sum_g / V - xhat sum_gxhat / V) act_pre'(x), dgamma = sum_gxhat, dbeta = sum_g, with
    the caller's totals [C][2] (they need not be the sums of these very tensors)."""
    C, V = x.shape
    u, xhat, g, _ = bn_bwd_terms64(dy, x, mi, gamma, beta, in_chain, pre, post)
    ga = torch.ones(C, dtype=F64) if gamma is None else gamma.to(F64)
    a = (ga.to(x.device) * mi[1].to(x.device, F64)).reshape(C, 1)
    tot = totals.to(x.device, F64)
    du = a * (g - tot[:, 0:1] / V - xhat * tot[:, 1:2] / V)
    dx = du if pre == 1.0 else torch.where(x.to(F64) > 0, du, du * pre)
    return dx, tot[:, 1].clone(), tot[:, 0].clone()


def bn_bwd_autograd64(dy, x, gamma, beta, in_chain, pre, post, eps=EPS):
    """(dx, dgamma, dbeta) by float64 autograd of the forward expression y = act_post(BN(u)), u = T_in(x) (the gradient is then taken
    with respect to u) or u = act_pre(x) (with respect to x); train-mode statistics of u over the V voxels of each channel."""
    C = x.shape[0]
    ga = (torch.ones(C, dtype=F64) if gamma is None else gamma.to(F64)).to(x.device).requires_grad_()
    be = (torch.zeros(C, dtype=F64) if beta is None else beta.to(F64)).to(x.device).requires_grad_()
    if in_chain is not None:
        leaf = chain64(x, in_chain).detach().requires_grad_()
        u = leaf
    else:
        leaf = x.to(F64).detach().requires_grad_()
        u = lrelu(leaf, pre)
    m = u.mean(1, keepdim=True)
    v = ((u - m) ** 2).mean(1, keepdim=True)
    y = lrelu((u - m) / torch.sqrt(v + eps) * ga[:, None] + be[:, None], post)
    (y * dy.to(F64)).sum().backward()
    return leaf.grad, ga.grad, be.grad


# ---- residual join -----------------------------------------------------------------------------------------------------------------------
def chain_add64(a, chain_a, b, chain_b):
    return chain64(a, chain_a) + chain64(b, chain_b)


# ---- up-sampling -------------------------------------------------------------------------------------------------------------------------
def upsample_fwd64(x, chain, out, linear, mutation=None):
    """x [C][D][H][W] -> [C][Do][Ho][Wo]: x2 nearest / linear of T(x) (the oracle's upsample2x) cropped at the far ends; D = Do = 1 is the
    2-D form (D not scaled).  `no_w_crop`: the buffer a cube kernel without its W predicate leaves — every thread stores both outputs of
    its row pair, in input-voxel order — as (flat payload, what it stores behind the payload or None)."""
    C, D, H, W = x.shape
    Do, Ho, Wo = out
    t = chain64(x, chain)
    mode = "trilinear" if linear else "nearest"
    full = O.upsample2x(t[None, :, 0], mode)[0][:, None] if D == 1 and Do == 1 else O.upsample2x(t[None], mode)[0]
    y = full[:, :Do, :Ho, :Wo].contiguous()
    if mutation != "no_w_crop":
        return y
    flat = torch.cat([y.reshape(-1), torch.full((1,), float("nan"), dtype=F64)])
    for c in range(C):
        for d in range(D):
            for h in range(H):
                for w in range(W):
                    for od in ((d,) if D == 1 and Do == 1 else (2 * d, 2 * d + 1)):
                        for oh in (2 * h, 2 * h + 1):
                            if od < Do and oh < Ho:
                                o = ((c * Do + od) * Ho + oh) * Wo + 2 * w
                                flat[o], flat[o + 1] = full[c, od, oh, 2 * w], full[c, od, oh, 2 * w + 1]
    return flat[:-1].reshape(y.shape), (None if bool(torch.isnan(flat[-1])) else flat[-1])


def upsample_bwd64(dy, inp, linear):
    """The adjoint: autograd of upsample_fwd64 (no chain) at dy [C][Do][Ho][Wo] -> [C][D][H][W]."""
    x = torch.zeros((dy.shape[0],) + tuple(inp), dtype=F64, requires_grad=True)
    (upsample_fwd64(x, None, tuple(dy.shape[1:]), linear) * dy.to(F64)).sum().backward()
    return x.grad


# ---- crop, FIR, activations --------------------------------------------------------------------------------------------------------------
def crop64(x, win):
    od, oh, ow, Do, Ho, Wo = win
    return x[:, od:od + Do, oh:oh + Ho, ow:ow + Wo].contiguous()


def crop_bwd64(dy, shape, win):
    """x-shaped, zero outside the window."""
    od, oh, ow, Do, Ho, Wo = win
    dx = torch.zeros((dy.shape[0],) + tuple(shape), dtype=dy.dtype)
    dx[:, od:od + Do, oh:oh + Ho, ow:ow + Wo] = dy
    return dx


def fir64(x, taps, mutation=None):
    """y[c][t][s] = sum_k taps[k] x[c][t + K/2 - k][s], zero outside (a true convolution centred on K/2); x [C][T][S]."""
    C, T, S = x.shape
    K = taps.numel()
    p = K // 2 - (1 if mutation == "fir_centre-1" else 0)
    y = torch.zeros((C, T, S), dtype=F64)
    for k in range(K):
        for t in range(T):
            tt = t + p - k
            if 0 <= tt < T:
                y[:, t] += taps[k].to(F64) * x[:, tt].to(F64)
    return y


def act_fwd64(kind, x):
    x = x.to(F64)
    if kind == ACT_ELU:
        return torch.where(x > 0, x, torch.expm1(x))
    if kind == ACT_TANH:
        return torch.tanh(x)
    return 1.0 / (1.0 + torch.exp(-x))


def act_bwd64(kind, y, dy):
    """From the OUTPUT y: ELU' = y > 0 ? 1 : y + 1, tanh' = 1 - y^2, sigmoid' = y (1 - y)."""
    y, dy = y.to(F64), dy.to(F64)
    if kind == ACT_ELU:
        return torch.where(y > 0, dy, dy * (y + 1.0))
    if kind == ACT_TANH:
        return dy * (1.0 - y * y)
    return dy * (y * (1.0 - y))


def ulp_error(got, ref64):
    """max |got - ref| in units of the float32 spacing at ref (the spacing of the smallest normal below it)."""
    ref = ref64.detach().cpu().to(F64)
    e = torch.floor(torch.log2(ref.abs().clamp_min(2.0 ** -126)))
    return float(((got.detach().cpu().to(F64) - ref).abs() / 2.0 ** (e - 23)).max())


def lrelu_bwd_ref(dy, x, slope):
    """dx = x > 0 ? dy : dy * slope in float32 (one exact-or-rounded product: the float32 result IS the reference, bit for bit)."""
    return torch.where(x > 0, dy, dy * torch.tensor(slope, dtype=torch.float32))
