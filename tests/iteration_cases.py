"""The launches of csrc/loss_optim.hip that run in every iteration — dpi_adam_multi, dpi_masked_loss[_holdout], dpi_ema_loss, the Philox
input noise (dpi_fill_normal, dpi_noise_add*), dpi_loop_control, dpi_copy_if, dpi_overlap_add / dpi_overlap_normalize — as
tests/test_gpu_iteration_contract.py checks them on a device: the case rows, numpy restatements written from include/dpi_hip.h and the
kernels' comments (the library is never called), and the check functions.  A plain module: no fixtures, importable without a GPU.
tests/test_iteration_refs_host.py holds the restatements against independent code (torch.optim.Adam, the Random123 known answers, the
recorded scheduler traces, utils.EarlyStopping) and proves, restatement against restatement, that the checks catch a wrong kernel
(the `mutation` arguments).

Why each row exists:

 ADAM_SIZES (rows of ONE launch; the grid is 256 blocks x 256 threads x 4 elements = ADAM_PASS elements per pass and row)
   1, 3        one thread, `i + k < n` cuts its group;  4   one full group;  5   a second thread with one element
   1023, 1025  the last thread's group is cut / a second block with one element;  1024   exactly one block
   262144      exactly one pass;  262149   one pass and a tail of 5 (the first row to reach the grid-stride loop AND a cut group in it)
   524293      two full passes and a tail
 ADAM_MANY     300 rows of 1 + (i % 7) elements: blockIdx.y
 LOSS_N (grid = min(ceil(n / 2048), 1024) blocks of 256 threads; G = 256 x grid elements per pass)
   1, 255      one block, threads without an element;  2048   one block, 8 passes per thread;  2049   a second block with one element
   262147      129 blocks (128 full ones and 3 elements), below the cap;  2097152   1024 blocks: the cap reached exactly, 8 passes
   2359299     the cap exceeded: 9 full passes and a tail of 3 (the first row whose grid is cut by the cap)
 HOLDOUT_SHAPES [C][T][S]
   (3, 37, 2311)    G < TS: the carries `r >= TS` and `s >= S` both occur;  (40, 5, 1301)   G > TS: Gc = 5;  (2, 1000, 1)   S = 1
   (2, 48, 24960)   the cap: G = 262144
 NOISE_N (one thread per group of four, grid = min(ceil(n / 1024), 4096) blocks: NOISE_PASS = 4194304 elements per pass)
   1, 2, 3, 5  element path, one thread;  4   one float4;  1023, 1027   element path, cut last group;  1024   vector path
   4194304     one pass exactly;  4198404   a second pass on the vector path;  4198403   a second pass on the element path
   NOISE_NT = 33554432   n >= 32 Mi: the non-temporal stores
 COPY_N        1, 257, 1048579 (4096 blocks x 256 + 3: the cap, second pass)
 OVERLAP_CASES the suite's earlier case, windows that do not overlap, heavy overlap with stride 1, and ONE patch of 65 x 128 x 130 =
   1081600 > 4096 x 256 elements (the grid-stride loop), at the origin and flush with the far corner of a (66, 130, 133) volume

Precondition (include/dpi_hip.h): the noise kernels choose their float4 path from n % 4 alone, so a buffer with n % 4 == 0 is 16-byte
aligned (bf16: 8-byte) and element-aligned bases appear only with n % 4 != 0.  dpi_adam_multi uses scalar accesses only.
"""
import math

import numpy as np

F = np.float32
U = 2.0 ** -24                                    # unit round-off of fp32

ADAM_PASS = 256 * 256 * 4
ADAM_SIZES = (1, 3, 4, 5, 1023, 1024, 1025, 262144, 262149, 524293)
ADAM_OFFSET1 = (3, 1025, 262149)                  # rows whose four pointers all sit one element behind a 256-byte boundary
ADAM_MANY = tuple(1 + (i % 7) for i in range(300))
ADAM_DEFAULT, ADAM_OTHER = (0.9, 0.999, 1e-8), (0.8, 0.99, 1e-6)
# (betas + eps, step, lr) of every launch of the device test; test_iteration_refs_host.py asserts the tie condition for each
ADAM_LAUNCHES = ((ADAM_DEFAULT, 1, 1e-3), (ADAM_OTHER, 10, 1e-3), (ADAM_DEFAULT, 1000, 3e-4), (ADAM_DEFAULT, 2, 1e-3), (ADAM_DEFAULT, 3, 1e-3))

LOSS_BLOCKS, LOSS_PER_BLOCK = 1024, 2048
LOSS_N = (1, 255, 2048, 2049, 262147, 2097152, 2359299)
LOSS_FRACTIONAL_N = 262147
HOLDOUT_SHAPES = ((3, 37, 2311), (40, 5, 1301), (2, 1000, 1), (2, 48, 24960))

NOISE_MAX_BLOCKS = 4096
NOISE_PASS = NOISE_MAX_BLOCKS * 256 * 4
NOISE_N = (1, 2, 3, 4, 5, 1023, 1024, 1027, 4194304, 4198404, 4198403)
NOISE_NT = 32 << 20
FILL_STREAM = (0xFFFFFFFF << 32) | 3             # the stream id of the drivers' z fill: a non-zero high word
STEP_STREAM = (0x1234 << 32) | 7                 # *step_ptr of the perturbation, also with a high word

COPY_N = (1, 257, 4096 * 256 + 3)

OVERLAP_CASES = {                                 # name: (volume, patch, stride, origins or None for the whole window grid)
    "8x6x10-s4x4x6": ((20, 18, 22), (8, 6, 10), (4, 4, 6), None),
    "5x7x9-no-overlap": ((10, 14, 27), (5, 7, 9), (5, 7, 9), None),
    "3x4x5-s1x2x1": ((5, 8, 8), (3, 4, 5), (1, 2, 1), None),
    "65x128x130-one-patch": ((65, 128, 130), (65, 128, 130), (1, 1, 1), None),
    "65x128x130-far-corner": ((66, 130, 133), (65, 128, 130), (1, 2, 3), ((0, 0, 0), (1, 2, 3))),
}


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def check_bits(got, want, what):
    """Bit equality, zeros' signs and NaN payloads included; names the first differing element."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    bad = np.flatnonzero(bits(got).ravel() != bits(want).ravel())
    assert bad.size == 0, "%s: %d of %d elements differ, first at %d: got %r, want %r" % (
        what, bad.size, got.size, int(bad[0]), got.ravel()[bad[0]], want.ravel()[bad[0]])


# ---- Adam --------------------------------------------------------------------------------------------------------------------------------
def adam_scalars(step, lr, b1, b2, eps):
    """The launch's scalars as adam_kernel derives them: in double, then rounded to fp32; lr is the fp32 value of step_lr[1] widened.
    Returns (beta2, eps, omb1, omb2, step_size, bc2s) in fp32 and the doubles (step_size, bc2s) before their rounding."""
    lr = float(F(lr))
    step_size, bc2s = lr / (1.0 - b1 ** float(step)), math.sqrt(1.0 - b2 ** float(step))
    return (F(b2), F(eps), F(1.0 - b1), F(1.0 - b2), F(step_size), F(bc2s)), (step_size, bc2s)


def midpoint_margin(x):
    """Distance of the double x from the nearer of the two fp32 rounding boundaries around it, relative to |x|."""
    f = F(x)
    mids = [(float(f) + float(np.nextafter(f, F(s) * F(np.inf)))) / 2.0 for s in (-1, 1)]
    return min(abs(x - m) for m in mids) / abs(x)


def adam_np(p, g, m, v, step, lr, b1=0.9, b2=0.999, eps=1e-8, mutation=None):
    """One step of adam_kernel in float32 numpy, one correctly rounded operation per numpy call (the library is built with
    -ffp-contract=off).  Returns new (p, m, v).  mutation "no_tail": the last n % 4 elements stay as they were; "bc2s_before_sqrt"."""
    p, g, m0, v0 = (np.asarray(a, dtype=F) for a in (p, g, m, v))
    (beta2, eps32, omb1, omb2, step_size, bc2s), _ = adam_scalars(step, lr, b1, b2, eps)
    m1 = m0 + omb1 * (g - m0)
    v1 = beta2 * v0 + (omb2 * g) * g
    denom = (np.sqrt(v1 / bc2s) if mutation == "bc2s_before_sqrt" else np.sqrt(v1) / bc2s) + eps32
    p1 = p - step_size * (m1 / denom)
    assert p1.dtype == m1.dtype == v1.dtype == F
    if mutation == "no_tail":
        k = p.size - p.size % 4
        p1[k:], m1[k:], v1[k:] = p[k:], m0[k:], v0[k:]
    return p1, m1, v1


def adam_row(n, rng, zero_state=False):
    """(p, g, m0, v0) of one row: |g| over logspace(-9, 0) with random signs and exact zeros; v0 = 0 on half of those zeros (there
    denom == eps); m0 and v0 non-zero elsewhere unless zero_state."""
    p = (0.1 * rng.randn(n)).astype(F)
    g = (10.0 ** rng.uniform(-9, 0, n) * rng.choice([-1.0, 1.0], n)).astype(F)
    m0 = (1e-3 * rng.randn(n)).astype(F)
    v0 = (1e-6 * (0.1 + rng.rand(n))).astype(F)
    zero = np.arange(n) % 11 == (3 if n > 11 else 0)
    g[zero] = 0.0
    v0[zero & (np.arange(n) % 2 == (1 if n > 11 else 0))] = 0.0
    if zero_state:
        m0[:], v0[:] = 0.0, 0.0
    return p, g, m0, v0


def check_adam(got, want, what):
    """got, want: (p, m, v) — bit equality of all three."""
    for name, a, b in zip("pmv", got, want):
        check_bits(a, b, "%s: %s" % (what, name))


# ---- masked loss -------------------------------------------------------------------------------------------------------------------------
def loss_blocks(n):
    return max(1, min(-(-n // LOSS_PER_BLOCK), LOSS_BLOCKS))


def loss_inputs(n, seed, fractional=False):
    """(out, img, mask) float32 [n]: img = out + noise + offset, a 0/1 mask (or one in [0, 1))."""
    rng = np.random.RandomState(seed)
    o = rng.randn(n).astype(F)
    t = (o + 0.3 * rng.randn(n) + 0.1).astype(F)
    m = rng.rand(n).astype(F) if fractional else (rng.rand(n) > 0.4).astype(F)
    m[m >= 1.0] = 0.5
    return o, t, m


def loss_grad_np(o, t, m, kind, gscale):
    """dout in float32 numpy with the kernel's rounding points: d = o*m - t*m, inv_n = fp32(gscale) / fp32(n),
    MSE g = ((2 d) m) inv_n, L1 g = (sign(d) m) inv_n."""
    o, t, m = (np.asarray(a, dtype=F) for a in (o, t, m))
    d = o * m - t * m
    inv_n = F(gscale) / F(o.size)
    if kind == 1:
        return ((F(2.0) * d) * m) * inv_n
    sign = np.where(d > 0, F(1.0), np.where(d < 0, F(-1.0), F(0.0))).astype(F)
    return (sign * m) * inv_n


def loss_sums64(o, t, m, kind, keep=None):
    """float64 sums from the fp32 inputs, and the float64 sums of the terms' magnitudes the bounds scale with.  Order:
    {misfit (the numerator of result[0]), sum t^2, sum (t-o)^2, sum o, sum t, sum o^2, sum o t}.  The misfit's magnitude is
    |o m| + |t m| (squared for MSE): with a 0/1 mask that is >= |d|, with a fractional one the products round too.
    keep: a boolean mask of the elements that are summed (the mutations drop some)."""
    o, t, m = (np.asarray(a, dtype=F).astype(np.float64) for a in (o, t, m))
    if keep is not None:
        o, t, m = o[keep], t[keep], m[keep]
    d, e = o * m - t * m, t - o
    a = np.abs(o * m) + np.abs(t * m)
    ref = np.array([(d * d).sum() if kind == 1 else np.abs(d).sum(), (t * t).sum(), (e * e).sum(), o.sum(), t.sum(), (o * o).sum(), (o * t).sum()])
    mag = np.array([(a * a).sum() if kind == 1 else a.sum(), (t * t).sum(), (e * e).sum(), np.abs(o).sum(), np.abs(t).sum(), (o * o).sum(), np.abs(o * t).sum()])
    return ref, mag


def loss_k(kind, fractional):
    """fp32 roundings a term passes before the double accumulation, per sum of loss_sums64 (the last is not an output of its own).
    d = fl(fl(o m) - fl(t m)): a 0/1 mask makes the products exact, so |d| rounds once (L1: 1) and d^2, squared in double, twice the
    relative error (MSE: 2), against terms |d| = |o m - t m| <= |o m| + |t m|.  A fractional mask rounds both products and the
    difference: |fl(d) - d| < 2 u (|o m| + |t m|) (L1: 2), and d^2 moves by (|fl(d)| + |d|) times that < 4 u (|o m| + |t m|)^2 (MSE: 4).
    e = fl(t - o) is squared in double: 2.  t^2, o^2, o t are exact in double (48-bit products) and o, t are summed as they are: 0."""
    return np.array([(4.0 if fractional else 2.0) if kind == 1 else (2.0 if fractional else 1.0), 0.0, 2.0, 0.0, 0.0, 0.0, 0.0])


def sum_bound(k, n, mag):
    return (np.asarray(k, dtype=np.float64) * U + n * 2.0 ** -53) * np.asarray(mag, dtype=np.float64)


def check_sums(got, ref, mag, k, n, what):
    """|got - float64| <= (k 2^-24 + n 2^-53) sum|term| (elementwise_cases.check_partials' bound) for each sum."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert np.isfinite(got).all(), "%s: %s not written" % (what, np.flatnonzero(~np.isfinite(got)))
    ratio = np.abs(got - ref) / (sum_bound(k, n, mag) + 1e-300)
    assert ratio.max() <= 1.0, "%s: sum %d is off by %.3g x its bound (got %.17g, float64 %.17g)" % (
        what, int(ratio.argmax()), ratio.max(), got.ravel()[ratio.argmax()], ref.ravel()[ratio.argmax()])
    return float(ratio.max())


def snr_bound(num, den, num_err, den_err):
    """First-order propagation through 10 log10(num / den): |d| <= 10 / ln 10 (r_num / (1 - r_num) + r_den / (1 - r_den))."""
    rn, rd = num_err / num, den_err / den
    return 10.0 / math.log(10.0) * (rn / (1.0 - rn) + rd / (1.0 - rd))


def pcorr64(s, n):
    """PCORR from the float64 sums of loss_sums64: cov = S_ot - S_o S_t / n, v_t = S_t2 - S_t^2 / n, v_o likewise."""
    _, t2, _, so, st, o2, ot = s
    cov, vt, vo = ot - so * st / n, t2 - st * st / n, o2 - so * so / n
    return cov / (math.sqrt(vt) * math.sqrt(vo))


def pcorr_bound(ref, mag, n):
    """The bound of PCORR's error propagated from its five sums, all with k = 0: each is off by at most eps = n 2^-53 of the sum of its
    terms' magnitudes, which moves cov, v_t and v_o by eps (sum|o t| + 2 sum|o| sum|t| / n) and the like."""
    eps = (n + 8) * 2.0 ** -53                       # the sums, plus the handful of double operations of the finaliser
    _, t2, _, so, st, o2, ot = ref
    _, _, _, ao, at, _, aot = mag
    vt, vo = t2 - st * st / n, o2 - so * so / n
    dcov = eps * (aot + 2 * ao * at / n)
    dvt, dvo = eps * (t2 + 2 * at * at / n), eps * (o2 + 2 * ao * ao / n)
    p = abs(pcorr64(ref, n))
    return dcov / math.sqrt(vt * vo) + p * (dvt / vt + dvo / vo)


def loss_result64(o, t, m, kind, keep=None):
    """The eight doubles of loss_final from float64 sums (keep: loss_walk_keep of a mutation)."""
    n = float(np.asarray(o).size)
    s, _ = loss_sums64(o, t, m, kind, keep)
    with np.errstate(divide="ignore", invalid="ignore"):
        pc = np.float64(s[6] - s[3] * s[4] / n) / (np.sqrt(np.float64(s[1] - s[4] * s[4] / n)) * np.sqrt(np.float64(s[5] - s[3] * s[3] / n)))
        snr = 10.0 * np.log10(np.float64(s[1]) / np.float64(s[2]))
    return np.array([s[0] / n, snr, pc, s[1], s[2], s[3], s[4], s[5]])


def check_loss_result(res, o, t, m, kind, fractional, what):
    """The eight doubles of dpi_masked_loss against float64: the five sums result[3..7] and the numerator result[0] * n at check_sums'
    bound, SNR at 1e-6 dB and PCORR at 1e-8 (test_masked_loss_metrics' bars) — after asserting that the bounds propagated from the sums
    lie below those two figures, so that the existing ones are the ones that apply.  n == 1: PCORR is 0 / 0 = NaN by definition."""
    res = np.asarray(res, dtype=np.float64)
    n = np.asarray(o).size
    ref, mag = loss_sums64(o, t, m, kind)
    k = loss_k(kind, fractional)
    got = np.array([res[0] * n, res[3], res[4], res[5], res[6], res[7]])
    worst = check_sums(got, ref[:6], mag[:6], k[:6], n, what)
    snr = 10.0 * math.log10(ref[1] / ref[2])
    assert snr_bound(ref[1], ref[2], sum_bound(0, n, mag[1]), sum_bound(2, n, mag[2])) < 1e-6
    assert abs(res[1] - snr) < 1e-6, (what, "snr", res[1], snr)
    if n == 1:
        assert res[2] != res[2], (what, "pcorr of one sample", res[2])
    else:
        assert pcorr_bound(ref, mag, n) < 1e-8, (what, pcorr_bound(ref, mag, n))
        assert abs(res[2] - pcorr64(ref, n)) < 1e-8, (what, "pcorr", res[2], pcorr64(ref, n))
    return worst


def loss_walk_keep(n, mutation=None):
    """Which elements the grid-stride walk of loss_partial_kernel sums.  "drop_last_pass": every thread stops one trip early."""
    if mutation is None:
        return np.ones(n, dtype=bool)
    assert mutation == "drop_last_pass"
    G = 256 * loss_blocks(n)
    return np.arange(n) + G < n


# ---- held-out traces ---------------------------------------------------------------------------------------------------------------------
def holdout_inputs(shape, seed, sel_p=0.35):
    """(out, img, mask [C][T][S], sel [C][S]): known traces with a few dropped samples, sel a 0/1 subset of the known traces."""
    C, T, S = shape
    rng = np.random.RandomState(seed)
    o = rng.randn(C, T, S).astype(F)
    t = (o + 0.3 * rng.randn(C, T, S) + 0.1).astype(F)
    tr = rng.rand(C, 1, S) > 0.4
    if S == 1:
        tr[:] = True
    m = (tr & (rng.rand(C, T, S) > 0.05)).astype(F)
    sel = ((rng.rand(C, S) < sel_p) & tr[:, 0]).astype(F)
    if S == 1:
        sel[:] = np.array([1.0, 0.0] * C, dtype=F)[:C, None]
    assert 0 < sel.sum() < C * S
    return o, t, m, sel


def holdout_walk(shape, mutation=None):
    """The incremental index walk of loss_holdout_partial_kernel for every thread and pass: returns (c, s) [n] as the kernel forms them
    for element i (no division inside the loop).  mutation "no_r_carry": without `if (r >= TS) { r -= TS; ++c; }`."""
    C, T, S = shape
    n, TS = C * T * S, T * S
    G = 256 * loss_blocks(n)
    Gc, Gr, Gs = G // TS, G % TS, G % S
    i = np.arange(G, dtype=np.int64)
    c, r, s = i // TS, i % TS, i % S
    out_c, out_s = np.empty(n, dtype=np.int64), np.empty(n, dtype=np.int64)
    carries = {"r": 0, "s": 0}
    while i[0] < n:
        live = i < n
        out_c[i[live]], out_s[i[live]] = c[live], s[live]
        i, c, r, s = i + G, c + Gc, r + Gr, s + Gs
        cr, cs = r >= TS, s >= S
        carries["r"] += int(cr.sum())
        carries["s"] += int(cs.sum())
        if mutation != "no_r_carry":
            r, c = np.where(cr, r - TS, r), np.where(cr, c + 1, c)
        s = np.where(cs, s - S, s)
    return out_c, out_s, carries


def holdout_h(shape, sel, mutation=None):
    """h [C][T][S]: sel as the kernel's walk reads it (an index past the table, which only a mutation produces, reads 0)."""
    C, T, S = shape
    c, s, _ = holdout_walk(shape, mutation)
    flat = np.concatenate([np.asarray(sel, dtype=F).ravel(), np.zeros(1, dtype=F)])
    idx = c * S + s
    return flat[np.where(idx < C * S, idx, C * S)].reshape(shape)


def holdout_ref(o, t, m, h, kind):
    """float64 {sum |e m_ho| or (e m_ho)^2, sum (t m_ho)^2, sum (e m_ho)^2, N_ho} and the magnitudes of the first three."""
    o, t, m, h = (np.asarray(a, dtype=F).astype(np.float64) for a in (o, t, m, h))
    mh = m * h
    eh, th = (t - o) * mh, t * mh
    ref = np.array([(eh * eh).sum() if kind == 1 else np.abs(eh).sum(), (th * th).sum(), (eh * eh).sum()])
    return ref, ref.copy(), int((mh != 0).sum())


def check_holdout(res, o, t, m, h, kind, what):
    """result[8..10] of the held-out pass: the count exactly; val_loss x count and val_snr against float64.  m_ho is 0/1, so e m_ho and
    t m_ho are exact products of e = fl(t - o) and t: k = 1 (L1) or 2 (MSE) for the misfit, 0 for sum (t m_ho)^2, 2 for sum (e m_ho)^2;
    val_snr at the bound propagated from those two."""
    res = np.asarray(res, dtype=np.float64)
    n = np.asarray(o).size
    ref, mag, count = holdout_ref(o, t, m, h, kind)
    assert res[10] == count, (what, "N_ho", res[10], count)
    check_sums([res[8] * res[10]], ref[:1], mag[:1], [2.0 if kind == 1 else 1.0], n, what + " val_loss")
    bound = snr_bound(ref[1], ref[2], sum_bound(0, n, mag[1]), sum_bound(2, n, mag[2]))
    assert abs(res[9] - 10.0 * math.log10(ref[1] / ref[2])) <= bound, (what, "val_snr", res[9], 10.0 * math.log10(ref[1] / ref[2]), bound)


def ema_np(avg, out, beta, first):
    """avg <- out at iteration 0, else avg + w (out - avg) in fp32 with w = fp32(1 - double(fp32 beta))."""
    out = np.asarray(out, dtype=F)
    if first:
        return out.copy()
    w = F(1.0 - float(F(beta)))
    avg = np.asarray(avg, dtype=F)
    return avg + w * (out - avg)


# ---- Philox4x32-10 and Box-Muller --------------------------------------------------------------------------------------------------------
M32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(ctr, stream_id, seed, mutation=None):
    """Counter words {ctr lo, ctr hi, stream lo, stream hi}, key {seed lo, seed hi}; ctr: uint64 array.  Returns uint64 [len(ctr)][4] holding
    32-bit words.  mutation "swap_ctr_stream": the stream id in words 0, 1 and the counter in words 2, 3."""
    ctr = np.asarray(ctr, dtype=np.uint64)
    sid = np.full(ctr.shape, stream_id & 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)
    if mutation == "swap_ctr_stream":
        ctr, sid = sid, ctr
    c0, c1, c2, c3 = ctr & M32, ctr >> np.uint64(32), sid & M32, sid >> np.uint64(32)
    k0, k1 = np.uint64(seed & 0xFFFFFFFF), np.uint64((seed >> 32) & 0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2                # 32 x 32 -> 64 bits: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M32, (k1 + np.uint64(0xBB67AE85)) & M32
    return np.stack([c0, c1, c2, c3], 1)


def normals64(q0, q1, stream_id, seed, mutation=None):
    """The standard normals of counters q0 .. q1 - 1 (elements 4 q0 .. 4 q1 - 1) in float64 with the kernel's uniforms: radius from
    ((c >> 8) + 1) / 2^24, angle from (c >> 8) / 2^24, lanes r0 cos, r0 sin, r1 cos, r1 sin."""
    w = philox4x32_10(np.arange(q0, q1, dtype=np.uint64), stream_id, seed, mutation)
    u = (w >> np.uint64(8)).astype(np.float64)
    r0, r1 = np.sqrt(-2.0 * np.log((u[:, 0] + 1.0) / 2.0 ** 24)), np.sqrt(-2.0 * np.log((u[:, 2] + 1.0) / 2.0 ** 24))
    a0, a1 = 2.0 * np.pi * u[:, 1] / 2.0 ** 24, 2.0 * np.pi * u[:, 3] / 2.0 ** 24
    return np.stack([r0 * np.cos(a0), r0 * np.sin(a0), r1 * np.cos(a1), r1 * np.sin(a1)], 1).reshape(-1)


def noise_blocks(n):
    return max(1, min(-(-(-(-n // 4)) // 256), NOISE_MAX_BLOCKS))


def check_normals(got, base64, z64, std, bf16, what):
    """|out - (base + std z64)| <= 1e-3 std + half an fp32 ulp of the value (+ half a bf16 ulp for a bf16 out).  A wrong counter, key,
    stream word or lane order moves a sample by O(std); 1e-3 std separates that from the device intrinsics' error and is no accuracy
    claim.  Returns the largest |out - ref| / std over the elements."""
    got = np.asarray(got, dtype=np.float64)
    ref = np.asarray(base64, dtype=np.float64) + float(F(std)) * np.asarray(z64, dtype=np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.isfinite(got).all(), "%s: %d elements were not written" % (what, int((~np.isfinite(got)).sum()))
    ulp = np.spacing(np.abs(ref).astype(F)).astype(np.float64)
    bound = 1e-3 * abs(std) + 0.5 * ulp
    if bf16:
        bound = bound + 0.5 * 2.0 ** (np.floor(np.log2(np.maximum(np.abs(ref), 2.0 ** -126))) - 7)
    err = np.abs(got - ref)
    bad = np.flatnonzero(err > bound)
    assert bad.size == 0, "%s: %d of %d elements outside the bar, first at %d: got %.9g, want %.9g" % (
        what, bad.size, got.size, int(bad[0]), got[bad[0]], ref[bad[0]])
    return float((err / abs(std)).max())


# ---- loop control ------------------------------------------------------------------------------------------------------------------------
LoopCfg = dict(use_plateau=0, factor=0.9, threshold=1e-5, patience=100, min_lr=0.0, lr_eps=1e-8, es_patience=0, es_min_delta=1.0)


def loop_cfg(**kw):
    return dict(LoopCfg, **kw)


LOOP_VARIANTS = {"plain": (0, 0), "holdout": (1, 0), "ema": (0, 1), "ema-holdout": (1, 1)}      # name: (held-out part, running average)


def loop_layout(variant):
    """(state doubles, history columns): state {iter, loss_min, plateau_best, plateau_bad, es_best, es_bad, es_has_best, reserved} of the
    plain entry point, + {val_min, best_iter} with a held-out part, + {q_min, reserved} with a running average (which has slots 8 and 9
    with or without a held-out part); rows {loss, snr, pcorr, lr[, val_loss, val_snr][, ema_loss, ema_snr[, ema_val_loss, ema_val_snr]]}."""
    ho, ema = LOOP_VARIANTS[variant]
    return (12 if ema else 10 if ho else 8), 4 + 2 * ho + ema * (2 + 2 * ho)


def new_loop_state(variant="plain"):
    st = np.zeros(loop_layout(variant)[0])
    st[2] = np.inf
    return st


def loop_control_step(metrics, state, hist, max_iters, step_lr, active, cfg, mutation=None, variant="plain", ema=None):
    """One call of dpi_loop_control (plain), dpi_loop_control_holdout or dpi_loop_control_ema on host copies: metrics [>= 3] doubles ([>= 10]
    with a held-out part), ema the average's doubles, state and hist as loop_layout says, step_lr [2] fp32, active int.  Everything is
    updated in place; returns (improved, active).  The selection misfit q — loss; val_loss = metrics[8] with a held-out part; the
    average's ema[0], or ema[8] with a held-out part — drives *improved, best_iter, early stopping and the NaN stop; its minimum lives in
    state[1], state[8] (which is the raw val_min as well) or state[10].  ReduceLROnPlateau follows the raw training loss.
    mutation "improved<": `<` in place of `<=` in the selection."""
    if not active:
        return 0, 0
    ho, has_ema = LOOP_VARIANTS[variant]
    improved = 0
    it = int(state[0])
    loss = float(metrics[0])
    lr = float(step_lr[1])
    row = [loss, metrics[1], metrics[2], lr] + ([metrics[8], metrics[9]] if ho else [])
    if has_ema:
        row += [ema[0], ema[1]] + ([ema[8], ema[9]] if ho else [])
    if it < max_iters:
        hist[len(row) * it:len(row) * (it + 1)] = row
    better = lambda x, best: it == 0 or (x < best if mutation == "improved<" else x <= best)
    if has_ema:                                                  # raw minima, then the selection on the average's misfit
        if it == 0 or loss <= state[1]:
            state[1] = loss
        if ho and (it == 0 or metrics[8] <= state[8]):
            state[8] = metrics[8]
        q = float(ema[8] if ho else ema[0])
        if better(q, state[10]):
            state[10], state[9], improved = q, float(it), 1
    elif ho:
        if it == 0 or loss <= state[1]:
            state[1] = loss
        q = float(metrics[8])
        if better(q, state[8]):
            state[8], state[9], improved = q, float(it), 1
    else:
        q = loss
        if better(q, state[1]):
            state[1], improved = loss, 1
    if cfg["use_plateau"]:
        if loss < state[2] * (1.0 - cfg["threshold"]):
            state[2], state[3] = loss, 0.0
        else:
            state[3] += 1.0
        if state[3] > float(cfg["patience"]):
            nl = max(lr * cfg["factor"], cfg["min_lr"])
            if lr - nl > cfg["lr_eps"]:
                step_lr[1] = F(nl)
            state[3] = 0.0
    if cfg["es_patience"] != 0:
        if state[6] == 0.0:
            state[4], state[6] = q, 1.0
        elif q != q:
            active = 0
        else:
            if q < state[4] - state[4] * cfg["es_min_delta"] / 100.0:
                state[5], state[4] = 0.0, q
            else:
                state[5] += 1.0
            if state[5] >= float(cfg["es_patience"]):
                active = 0
    state[0] = float(it + 1)
    return improved, active


def loop_inputs(variant, it, loss, q=None):
    """(metrics, ema doubles or None) of call `it`: snr = 10 + it, pcorr = 0.5; with a held-out part val_snr = 20 + it and val_loss = q,
    or 3 + it under a running average, whose own doubles carry q where the selection reads it and a decoy that would select differently
    in the other misfit slot."""
    ho, has_ema = LOOP_VARIANTS[variant]
    if not ho and not has_ema:
        return loop_metrics(it, loss), None
    m = np.zeros(11)
    m[[0, 1, 2, 8, 9]] = [loss, 10.0 + it, 0.5, 3.0 + it if has_ema else q, 20.0 + it]
    if not has_ema:
        return m, None
    e = np.zeros(11)
    e[[0, 1, 8, 9]] = [5.0 + it, 30.0 + it, q, 40.0 + it] if ho else [q, 30.0 + it, 5.0 - it, 40.0 + it]
    return m, e


def loop_control_run(losses, lr0, max_iters, cfg, mutation=None, variant="plain", qs=None):
    """The model over a loss sequence (and, for the other variants, the sequence qs of selection misfits), inputs as loop_inputs builds
    them.  Returns a list of per-call records (improved, active, lr after the call, a copy of the state) and the history; stops calling
    once *active is 0, as a driver does."""
    state, hist = new_loop_state(variant), np.full(loop_layout(variant)[1] * max_iters, np.nan)
    step_lr, active, log = np.array([1.0, lr0], dtype=F), 1, []
    for it, loss in enumerate(losses):
        metrics, ema = loop_inputs(variant, it, loss, None if qs is None else qs[it])
        improved, active = loop_control_step(metrics, state, hist, max_iters, step_lr, active, cfg, mutation, variant, ema)
        log.append((improved, active, float(step_lr[1]), state.copy()))
        if not active:
            break
    return log, hist


def check_loop_log(got, want, what):
    """Per call: *improved, *active, the bits of step_lr[1] and every state double (a NaN equals a NaN)."""
    assert len(got) == len(want), (what, len(got), len(want))
    for it, (g, w) in enumerate(zip(got, want)):
        assert (g[0], g[1]) == (w[0], w[1]), "%s: call %d: (improved, active) = %s, model %s" % (what, it, g[:2], w[:2])
        assert bits(F(g[2])) == bits(F(w[2])), "%s: call %d: lr %r, model %r" % (what, it, g[2], w[2])
        assert np.asarray(g[3]).shape == np.asarray(w[3]).shape, (what, it)
        np.testing.assert_array_equal(np.asarray(g[3]), np.asarray(w[3]), err_msg="%s: state after call %d" % (what, it))


def loop_metrics(it, loss):
    return np.array([loss, 10.0 + it, 0.5, 0.0, 0.0, 0.0, 0.0, 0.0])


NAN = float("nan")
LOOP_SCRIPTS = {                                  # name: (losses, cfg, max_iters or None for len(losses))
    "ties": ([1.0, 0.9, 0.9, 0.95, 0.9, 0.8, 0.8], loop_cfg(), None),                       # the later iterate wins a tie
    "nan-first": ([NAN, 0.9, 0.8, 0.7, 0.6, 0.5], loop_cfg(es_patience=3), None),           # NaN becomes es_best: every later call is bad
    "nan-first-no-es": ([NAN, 0.9, 0.8], loop_cfg(), None),                                 # ... and never improves on loss_min = NaN
    "nan-later": ([1.0, 0.9, NAN, 0.7, 0.6], loop_cfg(es_patience=5), None),                # the NaN stop
    "nan-later-no-es": ([1.0, 0.9, NAN, 0.7, 0.6], loop_cfg(), None),                       # no early stopping: a NaN only fails to improve
    "rising": ([1.0, 0.9, 0.95, 1.1, 1.2, 1.3, 0.1], loop_cfg(es_patience=3), None),
    "lr-eps": ([1.0] * 8, loop_cfg(use_plateau=1, factor=0.5, threshold=0.1, patience=1, lr_eps=1e-3), None),          # cut suppressed
    "min-lr": ([1.0] * 12, loop_cfg(use_plateau=1, factor=0.5, threshold=0.1, patience=1, min_lr=3e-4), None),         # clamped, then no cut
    "no-plateau": ([1.0] * 8, loop_cfg(use_plateau=0, factor=0.5, threshold=0.1, patience=1), None),
    "past-max-iters": ([1.0, 0.9, 0.8, 0.8, 0.8, 0.7], loop_cfg(use_plateau=1, factor=0.5, threshold=0.1, patience=1), 3),
}

# Scripts of the other variants, shared by the host and the device tests.  name: (rows, ReduceLROnPlateau (factor, threshold, patience) or
# None, EarlyStopping (patience, min_delta %)).  --holdout: rows of (training loss, val_loss)
HOLDOUT_SCRIPTS = {
    "ties": ([(1.0, 1.0), (0.9, 1.0), (0.8, 0.7), (0.85, 0.7), (0.7, 0.75), (0.6, 0.7)], None, (0, 1.0)),
    "rising": ([(1.0, 1.0), (0.9, 0.95), (0.8, 1.1), (0.7, 1.2), (0.6, 1.3), (0.5, 1.4), (0.4, 0.1)], None, (3, 1.0)),
    "nan": ([(1.0, 1.0), (0.9, 0.8), (0.8, NAN), (0.7, 0.5), (0.6, 0.4)], None, (5, 1.0)),
    "plateau": ([(1.0, 1.0 - 0.05 * k) for k in range(12)], (0.5, 0.1, 1), (4, 1.0)),        # flat training loss, falling val_loss
}
# --out_ema: rows of (raw training loss, the average's selection misfit)
EMA_SCRIPTS = {
    "ties": ([(1.0, 1.0), (0.9, 1.0), (0.8, 0.7), (0.85, 0.7), (0.7, 0.75), (0.6, 0.7)], None, (0, 1.0)),
    "rising": ([(1.0, 1.0), (0.9, 0.95), (0.8, 1.1), (0.7, 1.2), (0.6, 1.3), (0.5, 1.4), (0.4, 0.1)], None, (3, 1.0)),      # stops on q while the raw loss falls
    "nan": ([(1.0, 1.0), (0.9, 0.8), (0.8, NAN), (0.7, 0.5), (0.6, 0.4)], None, (5, 1.0)),
    "nan_raw": ([(1.0, 1.0), (NAN, 0.8), (0.8, 0.7), (0.7, 0.9)], None, (5, 1.0)),                                        # a NaN raw loss does not stop the loop
    "plateau": ([(1.0, 1.0 - 0.05 * k) for k in range(12)], (0.5, 0.1, 1), (4, 1.0)),        # flat raw loss: lr cuts; falling q: no stop
}


def script_cfg(plateau, es):
    """The loop_cfg of a row of HOLDOUT_SCRIPTS / EMA_SCRIPTS, with the constants their device tests pass (min_lr 0, lr_eps 1e-8)."""
    factor, threshold, patience = plateau if plateau else (0.9, 1e-5, 100)
    return loop_cfg(use_plateau=int(plateau is not None), factor=factor, threshold=threshold, patience=patience, es_patience=es[0],
                    es_min_delta=es[1])


def eager_loop_model(rows, lr0, plateau, es):
    """The eager loop's rules over rows of (training loss, selection misfit q): best on q (utils.select_latest_min: <=, the later iterate
    wins), utils.EarlyStopping on q, the ReduceLROnPlateau arithmetic on the training loss.  Per call (improved, lr used, best_iter)."""
    from deep_prior_interpolation_amd import utils as u
    stopper = u.EarlyStopping(patience=es[0], min_delta=es[1], percentage=True)
    best, bad, lr = float("inf"), 0, np.float32(lr0)
    qmin, best_iter, log = None, None, []
    for it, (loss, q) in enumerate(rows):
        improved, qmin, best_iter = u.select_latest_min(it, q, qmin, best_iter)
        lr_used = lr
        if plateau is not None:
            factor, thr, pat = plateau
            if loss < best * (1.0 - thr):
                best, bad = loss, 0
            else:
                bad += 1
            if bad > pat:
                nl = max(float(lr) * factor, 0.0)
                if float(lr) - nl > 1e-8:
                    lr = np.float32(nl)
                bad = 0
        stop = stopper.step(q)
        log.append((int(improved), float(lr_used), best_iter))
        if stop:
            break
    return log


def variant_scripts(variant):
    """name: (losses, qs or None, cfg, max_iters) — LOOP_SCRIPTS for the plain variant, for the others the table they belong to and the
    past-the-end case (six calls on a history of three rows; q falls, rises and ties while the flat loss cuts the lr)."""
    if variant == "plain":
        return {k: (losses, None, cfg, n or len(losses)) for k, (losses, cfg, n) in LOOP_SCRIPTS.items()}
    table = HOLDOUT_SCRIPTS if variant == "holdout" else EMA_SCRIPTS
    out = {k: ([r[0] for r in rows], [r[1] for r in rows], script_cfg(plateau, es), len(rows)) for k, (rows, plateau, es) in table.items()}
    out["past-max-iters"] = ([1.0] * 6, [1.0, 0.9, 0.95, 0.9, 0.8, 0.85], LOOP_SCRIPTS["past-max-iters"][1], 3)
    return out


# ---- overlap-add -------------------------------------------------------------------------------------------------------------------------
def window_origins(volume, patch, stride):
    ax = [range(0, N - p + 1, s) for N, p, s in zip(volume, patch, stride)]
    return [(a, b, c) for a in ax[0] for b in ax[1] for c in ax[2]]


def hits(N, p, s, mutation=None):
    """Number of windows {k s : 0 <= k s <= N - p} covering each coordinate 0 .. N - 1, as the kernel counts them.
    mutation "kmax-1": the last window is forgotten."""
    x = np.arange(N)
    kmax = (N - p) // s - (1 if mutation == "kmax-1" else 0)
    lo = x - p + 1
    lo = np.where(lo <= 0, 0, (lo + s - 1) // s)
    hi = np.minimum(x // s, kmax)
    return np.where(hi >= lo, hi - lo + 1, 0)


def overlap_add_np(volume, patch_shape, patches, origins):
    """acc [D][H][W] float32: the patches added in launch order, one fp32 addition each."""
    acc = np.zeros(volume, dtype=F)
    pd, ph, pw = patch_shape
    for p, (od, oh, ow) in zip(patches, origins):
        acc[od:od + pd, oh:oh + ph, ow:ow + pw] += np.asarray(p, dtype=F).reshape(patch_shape)
    return acc


def overlap_normalize_np(acc, patch, stride, gain, mutation=None):
    """acc / (fp32(count) * gain): one fp32 product, one fp32 division.  A sample no window covers has count 0 and gets x / 0."""
    D, H, W = acc.shape
    c = (hits(D, patch[0], stride[0], mutation)[:, None, None] * hits(H, patch[1], stride[1], mutation)[None, :, None]
         * hits(W, patch[2], stride[2], mutation)[None, None, :])
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.asarray(acc, dtype=F) / (c.astype(F) * F(gain))


def overlap_patches(name, seed=0):
    volume, patch, stride, origins = OVERLAP_CASES[name]
    origins = window_origins(volume, patch, stride) if origins is None else list(origins)
    rng = np.random.RandomState(seed)
    return [rng.randn(*patch).astype(F) for _ in origins], origins
