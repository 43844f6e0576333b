/*
 * dpi_hip.h — C ABI of libdpi_hip.so: the MI355X (gfx950) kernels behind the deep-prior
 * interpolation hot path (MulResUnet3D / MulResUnet / Skip3D forward + backward, masked loss,
 * metrics, Adam, overlap-add reassembly).
 *
 * The reference (polimi-ispl/deep_prior_interpolation) has NO native/FFI interface: its hot path
 * sits behind `architectures.get_net(args, outchannel) -> torch.nn.Module`
 * (architectures/__init__.py:10) and delegates all arithmetic to torch's aten kernels.  Each entry
 * point below therefore cites the torch call site in the reference whose work it takes over; the
 * Python binding a maintainer adds is shown in INTEGRATION.md.
 *
 * Conventions
 *  - All pointers are DEVICE pointers owned by the caller (PyTorch caching allocator), fp32 unless
 *    stated, batch N = 1 (the reference optimises one patch at a time, main.py:131-135), layout
 *    channel-planar [C][D][H][W] with W contiguous.  2-D tensors use D = 1 and kd = 1.
 *    A channel slice [c0:c1] of such a tensor is itself a valid tensor (zero-copy concat).
 *  - `stream` is a hipStream_t passed as void*; every call only enqueues work on it (graph-capturable:
 *    no allocation, no synchronisation, no host read-back).
 *  - Return value: 0 on success, negative DPI_E_* otherwise; dpi_last_error() gives the message of
 *    the calling thread's last failure.  No exceptions cross the ABI.
 *  - "chain": optional per-channel input transform applied while a tensor is LOADED, 5 floats per
 *    channel {ps, pb, slope, qs, qb}:  T(x) = qs * act(ps*x + pb) + qb,  act(v) = v>0 ? v : slope*v.
 *    It lets BatchNorm-apply + LeakyReLU be fused into the consumer instead of a separate pass.
 *    NULL = identity.
 *  - "stat partials": double[nblk][C][2] = per-block {sum, sum of squares}; reduced in fixed order by
 *    dpi_bn_finalize (deterministic, double precision).
 *  - Alignment and extent (what tests/test_gpu_conv_contract.py holds every convolution launch to, inside guard bands):
 *    a tensor is a channel slice of an allocation whose base is 16-byte aligned.  With a voxel count that is no multiple of 4 such a
 *    slice has the alignment of its ELEMENT only — 4 bytes for fp32, 2 bytes for a bf16 tensor (dpi_conv_desc.io) — and every entry
 *    point takes such a slice.  A view moved off the alignment its slice would have is served only by the kernels listed next, and is
 *    neither served nor refused by the others (gating those on the address as well is open work).  Launch variants that need more (16-byte staging loads, 8-byte / dword stores of two elements) are chosen from the
 *    addresses of the call as well as from the shape, and have an element-wise twin; results of the variants agree to rounding.
 *    Chosen that way, so that a view moved off its natural alignment (by any number of elements) is served too: every kernel of
 *    dpi_conv_bwd_weight, the 3x3(x3) MFMA kernels of dpi_conv_fwd / dpi_conv_bwd_data (fp32 arithmetic, both strides, the 4x4x1
 *    kernel included), stride-2 dpi_conv_bwd_data, dpi_upsample2x_bwd and dpi_hale_sections.  The other kernels (1x1x1 and VALU
 *    forward / backward-data, the element-wise operators) vectorise where the voxel count (the output row, for the VALU stencil) is a
 *    multiple of 4 and rely on what a channel slice then has: 16 bytes for fp32, 8 bytes for bf16.
 *    Refused with DPI_E_ARG, before anything that touches the caller's buffers is launched ("... the bf16 input tensor <name> must be
 *    8-byte aligned", <name> = x, dy or dy1): a bf16 INPUT (x of dpi_conv_fwd, dy / dy3 / dy1 of dpi_conv_bwd_data / _dual) that is not
 *    8-byte aligned when the launch belongs to the bf16 stencil kernels, i.e. precision >= 1, 3x3(x3), stride 1 with W % 4 == 0, or
 *    precision 1, 3x3x3, stride 2, bf16 x and y with W % 4 == 0.  Workspaces, weights, chains and statistic partials are the caller's own
 *    allocations: 16-byte aligned (any allocator's base address is).
 *    A launch writes its output tensor and nothing else of the caller's: `stat_partials` receives exactly
 *    dpi_conv_fwd_stat_blocks(d) rows of Cout x 2 doubles, every one of them written; a workspace is used up to at most the floats its
 *    sizing query names (dpi_conv_*_ws_floats), for every chain / alignment a launch of that descriptor can have.
 */
#ifndef DPI_HIP_H
#define DPI_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DPI_OK 0
#define DPI_E_ARG (-1)      /* invalid argument / unsupported shape */
#define DPI_E_LAUNCH (-2)   /* HIP launch or runtime error */
#define DPI_E_WORKSPACE (-3)/* workspace too small */

#define DPI_CHAIN_STRIDE 5

const char* dpi_last_error(void);
/* ABI version (406 = dpi_masked_loss_holdout / dpi_loop_control_holdout: held-out traces, --holdout; 405 = dpi_hale_sections / dpi_structure_tensor_sections: the anti-aliasing add-on on 3-D patches; 404 = round 6: the ten
 * dpi_set_* tuning functions left the ABI for dpi_set_option): 300 = round 3 (dpi_conv_desc carries its own size as first field), 301 adds dpi_conv_fwd_ws / dpi_conv_bwd_data_ws /
 * dpi_conv_bwd_data_dual, 401 = dpi_pack_scratch_bytes / dpi_pack_release, 402 = dpi_pack_forget (round 5), 403 = dpi_join_bwd (round 5), 400 = round 4: dpi_conv_desc grows the `io` field (bf16 storage of activations) and the elementwise entry
 * points get `_io` twins that take the storage types of their tensors.  A binding checks `>=` the version it was written against and
 * dpi_conv_desc_size() == its own struct size. */
int dpi_version(void);
/* Number of devices / properties as HIP sees them (no torch involved). */
int dpi_device_info(int device, int* cus, int* lds_bytes, size_t* hbm_bytes, char* name, int name_len);
/* Profiling aid (no reference counterpart): an empty kernel `dpi_marker_kernel` launched with `id` workgroups of one wave.
 * rocprofv3's kernel trace records launch grids but not kernel arguments, so tools/rocpd_stats.py uses these markers to
 * attribute the dispatches that follow (in host launch order) to the layer the caller tagged; id = 1 ends a scope. */
int dpi_profile_marker(int id, void* stream);
/* ABI 404.  The ONE process-global switchboard of the library, for tests, tools and A/B experiments only — the product path (ops.py, main.py,
 * parallel.py, bench.py's timed region) never calls it: what a launch computes is a function of its descriptor and arguments alone (SURVEY §8(b):
 * "no hidden global state").  Every key selects between launch PLANS or kernel VARIANTS that compute the same result (or, for the *_debug keys,
 * skips phases for timing experiments and says so); none changes the arithmetic contract of an entry point.  Returns DPI_OK, or DPI_E_ARG for
 * an unknown key / a value out of range.  Keys (defaults in brackets; the environment variable that sets the initial value, if any):
 *   "splitk"                   [1]  0: no input-channel split of coarse-level launches (DPI_SPLITK)
 *   "dual_bwd_data"            [1]  0: dpi_conv_bwd_data_dual always runs two launches (DPI_NO_DUAL)
 *   "bw_pair"                  [2]  backward-weight, two 4-channel groups per workgroup: 0 off, 1 every layer with >= 2 full groups, 2 the long
 *                                   group loops of the finest level only (DPI_BW_PAIR)
 *   "bw_workgroups"            [-]  workgroups the backward-weight MFMA launch plan aims at (> 0)
 *   "bw_xcd_order"             [1]  XCD-aware workgroup order of that plan (0 / 1)
 *   "mfma_min_cout"            [8]  3x3(x3) stride-1 forward / backward-data with at least this many output channels run the fp32-MFMA stencil
 *   "bwd_weight_mfma_min_cout" [8]  ... the same threshold of the backward-weight dispatch
 *   "fewco_mfma"               [1]  0: forward 3x3x3 with Cout <= 4 back on the VALU kernel
 *   "q4"                       [1]  4x4x1-MFMA kernel for <= 8 output channels: 0 off, 1 where it pays, 2 wherever it can run (tests)
 *   "q4_ck"                    [0]  its chunk variant: 2 planar, 4 channel-interleaved, 0 by shape
 *   "q4_debug"                 [0]  its phase-skipping bits (timing experiments, WRONG results): 0 no input loads after the first chunk, 1 no LDS
 *                                   stores after it, 2 no MFMAs, 3 no output stores, 5 no barriers; bits 8-15 = KiB of extra dynamic LDS
 *   "bf16_debug"               [0]  bf16 stencil kernel: bits 0-2 skip phases (WRONG results), bit 3 routes EVERY 3x3(x3) stride-1 convolution of
 *                                   a precision = 1 descriptor through it (default: only the shapes where it beats the fp32 kernels)
 * (the per-knob functions behind the keys live in csrc/dpi_hip_internal.h and are not exported). */
int dpi_set_option(const char* key, int value);

/* ---------------------------------------------------------------- convolution ------------------
 * Replaces nn.Conv3d / nn.Conv2d built at architectures/base.py:123,176 (k in {1,3}, stride in {1,2},
 * zero padding (k-1)/2) and their autograd backward (aten convolution_backward).
 * x: [Cin][D][H][W]   w: [Cout][Cin][kd][k][k]   y: [Cout][Do][Ho][Wo],  Xo = (X + 2*pad - k)/stride + 1.
 * kd = k for 3-D, kd = 1 for 2-D (D must be 1).
 */
typedef struct {
  /* = sizeof(dpi_conv_desc) of the header the CALLER was built against (dpi_conv_desc_size() gives the library's).  Every entry
   * point that takes a descriptor rejects a mismatch with DPI_E_ARG instead of reading fields past a shorter struct: the
   * descriptor grew a `precision` field in round 2 and a binding with the old 8-int layout read it from adjacent memory. */
  int size;
  int Cin, Cout;
  int D, H, W;      /* input spatial size */
  int k, kd;        /* kernel extent in H/W and in D */
  int stride;       /* 1 or 2 (applies to D only when kd > 1) */
  /* 0 (default): fp32 operands, the reference's arithmetic.  1: mixed precision of BASELINE configs[4] — the operands of 3x3(x3)
   * stride-1 convolutions (forward, backward-data, backward-weight) are rounded to bf16 on their way into the matrix cores
   * (v_mfma_f32_16x16x32_bf16, fp32 accumulate); tensors in HBM, master weights, BatchNorm statistics and Adam stay fp32.
   * 2: "split" mode — forward / backward-data operands are split exactly into three bf16 terms and six partial products are
   * accumulated in fp32: fp32-class accuracy (same tolerance as precision 0 against the fp64 oracle) on the bf16 matrix cores. */
  int precision;
  /* ABI 400: storage type of the ACTIVATION tensors of this layer in HBM, a mask of DPI_IO_*: bit set = that tensor is bf16
   * (2 bytes per element, same [C][D][H][W] layout), clear = fp32.  The pointer arguments keep their `float*` spelling; with a bit
   * set the library reads / writes that tensor as bf16: widened exactly on load, rounded to nearest-even on store, all arithmetic
   * and accumulation in fp32 (BASELINE configs[4]: "bf16 activations + fp32 Adam master weights").  Weights, biases, weight
   * gradients, chains and statistic partials are always fp32 / double.  BatchNorm partials emitted by dpi_conv_fwd describe the
   * stored (rounded) output.  0 = every tensor fp32 (the reference's storage, main.py:112). */
  int io;
} dpi_conv_desc;
#define DPI_IO_X_BF16 1   /* x: input of dpi_conv_fwd / dpi_conv_bwd_weight */
#define DPI_IO_Y_BF16 2   /* y: output of dpi_conv_fwd */
#define DPI_IO_DY_BF16 4  /* dy: input of dpi_conv_bwd_data / dpi_conv_bwd_weight */
#define DPI_IO_DX_BF16 8  /* dx: output (and, with accumulate, input) of dpi_conv_bwd_data */
/* sizeof(dpi_conv_desc) as the library was compiled; a binding asserts it equals its own struct size at load time. */
int dpi_conv_desc_size(void);

/* number of stat-partial blocks dpi_conv_fwd writes for this problem (0 if desc invalid) */
int dpi_conv_fwd_stat_blocks(const dpi_conv_desc* d);
/* y = conv(T(x), w) + bias.  bias may be NULL.  stat_partials (may be NULL): double[nblk][Cout][2]. */
int dpi_conv_fwd(const dpi_conv_desc* d, const float* x, const float* x_chain, const float* w,
                 const float* bias, float* y, double* stat_partials, void* stream);
/* dx (+)= conv_transpose(dy, w):  dx [Cin][D][H][W], dy [Cout][Do][Ho][Wo].  accumulate != 0 adds. */
int dpi_conv_bwd_data(const dpi_conv_desc* d, const float* dy, const float* w, float* dx,
                      int accumulate, void* stream);
/* The same two operations with a caller-owned workspace (ABI 301).  At the coarse levels of the U-Net a convolution is a few
 * dozen output tiles with hundreds of input channels: the library then splits the input-channel loop over more workgroups, writes
 * partial outputs into `ws` and sums them in a fixed order (deterministic).  dpi_conv_*_ws_floats(d) = floats wanted (0: the
 * problem is not split and ws may be NULL); with ws == NULL these are exactly dpi_conv_fwd / dpi_conv_bwd_data.  Results of the
 * split and the unsplit launch differ by fp32 rounding of the partial sums only. */
size_t dpi_conv_fwd_ws_floats(const dpi_conv_desc* d);
size_t dpi_conv_bwd_data_ws_floats(const dpi_conv_desc* d);
int dpi_conv_fwd_ws(const dpi_conv_desc* d, const float* x, const float* x_chain, const float* w,
                    const float* bias, float* y, double* stat_partials, float* ws, size_t ws_floats, void* stream);
int dpi_conv_bwd_data_ws(const dpi_conv_desc* d, const float* dy, const float* w, float* dx,
                         int accumulate, float* ws, size_t ws_floats, void* stream);
/* dx (+)= conv_transpose(dy3, w3) + conv_transpose(dy1, w1) for a 3x3(x3) stride-1 layer d3 and a 1x1(x1) layer d1 that read the SAME
 * tensor (equal Cin, D, H, W): Block3d.conv1 + shortcut (mulresunet.py:72-96) and ResPath3d.conv3x3 + conv1x1 (mulresunet.py:99-113),
 * whose input gradient is the sum of the two transposed convolutions.  Where the fp32-MFMA stencil kernel serves d3, the 1x1x1 term is
 * accumulated in the same pass (dx written once instead of written by one launch and read-modified-written by the next); every other
 * case runs the two launches.  ws / ws_floats: dpi_conv_bwd_data_ws_floats(d3) (may be NULL / 0). */
int dpi_conv_bwd_data_dual(const dpi_conv_desc* d3, const float* dy3, const float* w3,
                           const dpi_conv_desc* d1, const float* dy1, const float* w1,
                           float* dx, int accumulate, float* ws, size_t ws_floats, void* stream);
/* dw[Cout][Cin][kd][k][k] = sum_p dy[co][p] * T(x)[ci][p*stride + tap - pad].
 * workspace: float[dpi_conv_bwd_weight_ws_floats(d)].  */
size_t dpi_conv_bwd_weight_ws_floats(const dpi_conv_desc* d);
int dpi_conv_bwd_weight(const dpi_conv_desc* d, const float* x, const float* x_chain, const float* dy,
                        float* dw, float* ws, size_t ws_floats, void* stream);


/* ---------------------------------------------------------------- BatchNorm / activations -------
 * Replaces nn.BatchNorm3d/2d in training mode (base.py:164,214; mulresunet.py:80-81,104,225) and
 * LeakyReLU(0.2) (base.py:102), plus their backward.
 *
 * Precondition of every entry point of this section and of the element-wise ones further down (dpi_chain_add_*, dpi_join_bwd, the *_io
 * twins, dpi_add, dpi_lrelu_bwd, dpi_act_*, dpi_axpy): the float4 / packed-bf16 paths are chosen from V % 4 (n % 4) ALONE, the base
 * addresses are not consulted (unlike the convolution files, which ask dpi_vec4_base).  A tensor with V % 4 == 0 must therefore be
 * 16-byte aligned (8-byte for a bf16 tensor) — what a channel slice of a 16-byte-aligned allocation is; an element-aligned base is served
 * only with V % 4 != 0, where the element-wise path runs.  A base that is off 16 bytes while V % 4 == 0 is neither served nor refused.
 * dpi_upsample2x_fwd_io with a bf16 y stores pairs of outputs as one dword where the element offset into y is even: y itself must then
 * be 4-byte aligned.  tests/test_gpu_elementwise_contract.py launches inside this precondition only, and asserts it of its buffers.
 * The streaming reductions cut a channel into dpi_stat_blocks(C, V) = min(ceil(V / 16384), 2048) spans of ceil(V / nblk) voxels rounded
 * up to a multiple of 4; every one of the nblk partial rows is written.
 */
int dpi_stat_blocks(int C, size_t V);
/* partials[nblk][C][2] of T(x) over the V voxels of each channel */
int dpi_channel_stats(const float* x, const float* chain, int C, size_t V, double* partials, void* stream);
/* Reduce partials -> mean, invstd (biased var, eps); update running stats (momentum, unbiased var);
 * write chain_out[c] = {gamma*invstd, beta - mean*gamma*invstd, slope, 1, 0}  (BN-apply followed by act with
 * `slope`; slope = 1 means no activation) or, with act_first != 0, {1, 0, slope, gamma*invstd, beta - mean*...}
 * (BN of act(x), the partials then being statistics of act(x)).  running_* / nbt / chain_out may be NULL.
 * in_chain != NULL (requires slope == 1, act_first == 0): the partials are statistics of T_in(x) and chain_out is the
 * composition BN(T_in(x)) = {in.ps, in.pb, in.slope, a*in.qs, a*in.qb + shift} — bn1 over the never-materialised
 * concat of Block3d (mulresunet.py:90-91).
 * mean_invstd: float[2][C]. */
int dpi_bn_finalize(const double* partials, int nblk, int C, size_t count, const float* gamma,
                    const float* beta, float eps, float momentum, float slope, int act_first,
                    const float* in_chain, float* running_mean, float* running_var, int64_t* num_batches_tracked,
                    float* mean_invstd, float* chain_out, void* stream);
/* y = T(x) elementwise */
int dpi_chain_apply(const float* x, const float* chain, int C, size_t V, float* y, void* stream);
/* BatchNorm backward, two-phase, with the surrounding LeakyReLU folded in (slope 1 = none):
 *   pre_slope  (act -> BN, mulresunet.py:93-94,110-111): u = act(x) was normalised; dx = du * act'(x)
 *   post_slope (BN -> act, base.py:214-215):            dy is w.r.t. act(BN(x)); g = dy * act'(gamma*xhat + beta)
 * phase 1: partials[nblk][C][2] = {sum g, sum g*xhat}, xhat = (act_pre(x) - mean) * invstd
 * phase 2: dx = gamma*invstd*(g - sum_g/V - xhat*sum_gxhat/V) * act_pre'(x); dgamma = sum_gxhat; dbeta = sum_g
 * in_chain != NULL (requires pre_slope == 1): the normalised tensor was u = T_in(x) (value only) and dx is the
 * gradient w.r.t. u, not x. */
int dpi_bn_bwd_reduce(const float* dy, const float* x, const float* mean_invstd, const float* gamma,
                      const float* beta, const float* in_chain, float pre_slope, float post_slope, int C,
                      size_t V, double* partials, void* stream);
int dpi_bn_bwd_apply(const float* dy, const float* x, const float* mean_invstd, const float* gamma,
                     const float* beta, const float* in_chain, float pre_slope, float post_slope,
                     const double* partials, int nblk, int C, size_t V, float* dx, float* dgamma,
                     float* dbeta, void* stream);
/* dpi_bn_bwd_apply fused with phase 1 (dpi_bn_bwd_reduce) of up to two BatchNorms whose incoming gradient is this dx
 * (the residual joins of Block3d / ResPath3d, mulresunet.py:92-94,109-111): partials_a/b[dpi_stat_blocks][C][2] receive
 * {sum g, sum g*xhat} of dx against (xa, mi_a, gamma_a, beta_a, chain_a, post_a) resp. (xb, ...); xa / xb may be NULL.
 * Rows: `partials` is read as nblk rows [nblk][C][2], whatever wrote them (nblk is the caller's, not dpi_stat_blocks); partials_a / _b are
 * WRITTEN as dpi_stat_blocks(C, V) rows each, every row, and only where that side's x is given; they describe the dx the launch stored (the
 * bf16-rounded one with DPI_STORE_GRAD_BF16).  dgamma / dbeta may be NULL.  tests/test_gpu_join_contract.py holds all of this. */
int dpi_bn_bwd_apply_fork(const float* dy, const float* x, const float* mean_invstd, const float* gamma,
                          const float* beta, const float* in_chain, float pre_slope, float post_slope,
                          const double* partials, int nblk, int C, size_t V, float* dx, float* dgamma,
                          float* dbeta, const float* xa, const float* mi_a, const float* gamma_a,
                          const float* beta_a, const float* chain_a, float post_a, double* partials_a,
                          const float* xb, const float* mi_b, const float* gamma_b, const float* beta_b,
                          const float* chain_b, float post_b, double* partials_b, void* stream);
/* Phase 2 of TWO BatchNorm backward passes that share the incoming gradient dy (the two branches of a residual join), from
 * their phase-1 partials, in one pass; optionally phase 1 of one more BatchNorm whose incoming gradient is dxb on the
 * channels [f_lo, f_hi) and whose input is xb itself (raw): f_partials[dpi_stat_blocks][f_hi - f_lo][2].
 * Rows: partials_a / partials_b are read as nblk rows [nblk][C][2] each (the caller's count); f_partials is WRITTEN as
 * dpi_stat_blocks(C, V) rows of f_hi - f_lo channels, every row, and describes the stored dxb.  dxa and dxb are written on every channel,
 * the fork range of dxb included.  f_partials == NULL: no fork, f_lo / f_hi and the f_* tables are not looked at; f_partials != NULL
 * requires 0 <= f_lo < f_hi <= C and f_mi. */
int dpi_bn_bwd_apply_dual(const float* dy, int nblk, int C, size_t V, const float* xa, const float* mi_a,
                          const float* gamma_a, const float* beta_a, const float* chain_a, float post_a,
                          const double* partials_a, float* dxa, float* dgamma_a, float* dbeta_a, const float* xb,
                          const float* mi_b, const float* gamma_b, const float* beta_b, const float* chain_b,
                          float post_b, const double* partials_b, float* dxb, float* dgamma_b, float* dbeta_b,
                          int f_lo, int f_hi, const float* f_mi, const float* f_gamma, const float* f_beta,
                          float f_post, double* f_partials, void* stream);
/* t = T_a(a) + T_b(b);  partials[nblk][C][2] = {sum, sum^2} of act(t) with LeakyReLU(slope): the residual join
 * followed by act -> BatchNorm of Block3d / ResPath3d (mulresunet.py:92-94,109-111) in one pass. */
int dpi_chain_add_stats(const float* a, const float* chain_a, const float* b, const float* chain_b, int C,
                        size_t V, float slope, float* t, double* partials, void* stream);
/* dx = dy * act'(x) with act(v) = v>0 ? v : slope*v  (x = the activation INPUT or OUTPUT: same sign) */
int dpi_lrelu_bwd(const float* dy, const float* x, float slope, size_t n, float* dx, void* stream);
/* The other activations of the reference's get_activation (architectures/base.py:97-114): ELU (alpha = 1), Tanh, Sigmoid.
 * Backward takes the activation OUTPUT y. */
#define DPI_ACT_ELU 1
#define DPI_ACT_TANH 2
#define DPI_ACT_SIGMOID 3
int dpi_act_fwd(const float* x, size_t n, int kind, float* y, void* stream);
int dpi_act_bwd(const float* dy, const float* y, size_t n, int kind, float* dx, void* stream);
/* y = a + b */
int dpi_add(const float* a, const float* b, size_t n, float* y, void* stream);
/* per-channel sum: out[c] = sum_v x[c][v]   (bias gradients) ; ws: double[dpi_stat_blocks*C*2] */
int dpi_channel_sum(const float* x, int C, size_t V, double* ws, float* out, void* stream);

/* ---------------------------------------------------------------- bf16 storage of activations (ABI 400) ---------
 * `_io` twins of the entry points above that read or write activation tensors.  `io` says how those tensors live in HBM:
 *   DPI_STORE_FWD_BF16   the FORWARD tensors of the call (activations: conv outputs, join results, block outputs) are bf16
 *   DPI_STORE_GRAD_BF16  the GRADIENT tensors of the call (dy, dx: gradients of such activations) are bf16
 * Per call, [F] / [G] below mark which arguments each bit covers.  Everything else — chains, mean / invstd, gamma / beta and their
 * gradients, statistic partials (double), workspaces — keeps its type.  Arithmetic is fp32 (double for the reductions); a bf16 element
 * is widened exactly on load and a result is rounded to nearest-even on store; statistics emitted together with a stored tensor
 * describe the ROUNDED values.  io = 0 is the fp32 entry point.  Unknown bits are rejected (DPI_E_ARG). */
#define DPI_STORE_FWD_BF16 1u
#define DPI_STORE_GRAD_BF16 2u
int dpi_channel_stats_io(const float* x /*F*/, const float* chain, int C, size_t V, double* partials, unsigned io, void* stream);
int dpi_chain_apply_io(const float* x /*F*/, const float* chain, int C, size_t V, float* y /*F*/, unsigned io, void* stream);
int dpi_chain_add_stats_io(const float* a /*F*/, const float* chain_a, const float* b /*F*/, const float* chain_b, int C, size_t V,
                           float slope, float* t /*F*/, double* partials, unsigned io, void* stream);
int dpi_bn_bwd_reduce_io(const float* dy /*G*/, const float* x /*F*/, const float* mean_invstd, const float* gamma, const float* beta,
                         const float* in_chain, float pre_slope, float post_slope, int C, size_t V, double* partials, unsigned io,
                         void* stream);
int dpi_bn_bwd_apply_io(const float* dy /*G*/, const float* x /*F*/, const float* mean_invstd, const float* gamma, const float* beta,
                        const float* in_chain, float pre_slope, float post_slope, const double* partials, int nblk, int C, size_t V,
                        float* dx /*G*/, float* dgamma, float* dbeta, unsigned io, void* stream);
int dpi_bn_bwd_apply_fork_io(const float* dy /*G*/, const float* x /*F*/, const float* mean_invstd, const float* gamma, const float* beta,
                             const float* in_chain, float pre_slope, float post_slope, const double* partials, int nblk, int C,
                             size_t V, float* dx /*G*/, float* dgamma, float* dbeta, const float* xa /*F*/, const float* mi_a,
                             const float* gamma_a, const float* beta_a, const float* chain_a, float post_a, double* partials_a,
                             const float* xb /*F*/, const float* mi_b, const float* gamma_b, const float* beta_b, const float* chain_b,
                             float post_b, double* partials_b, unsigned io, void* stream);
int dpi_bn_bwd_apply_dual_io(const float* dy /*G*/, int nblk, int C, size_t V, const float* xa /*F*/, const float* mi_a,
                             const float* gamma_a, const float* beta_a, const float* chain_a, float post_a,
                             const double* partials_a, float* dxa /*G*/, float* dgamma_a, float* dbeta_a, const float* xb /*F*/,
                             const float* mi_b, const float* gamma_b, const float* beta_b, const float* chain_b,
                             float post_b, const double* partials_b, float* dxb /*G*/, float* dgamma_b, float* dbeta_b,
                             int f_lo, int f_hi, const float* f_mi, const float* f_gamma, const float* f_beta,
                             float f_post, double* f_partials, unsigned io, void* stream);
int dpi_upsample2x_fwd_io(const float* x /*F*/, const float* chain, int C, int D, int H, int W, int Do, int Ho, int Wo, int linear,
                          float* y /*F*/, unsigned io, void* stream);
/* ws (fp32, dpi_upsample2x_bwd_ws_floats) keeps its type */
int dpi_upsample2x_bwd_io(const float* dy /*G*/, int C, int D, int H, int W, int Do, int Ho, int Wo, int linear, float* dx /*G*/,
                          float* ws, unsigned io, void* stream);
/* z stays fp32 (it is the fixed network input of main.py:62-64); out [F] is the perturbed input the first layers read */
int dpi_noise_add_io(const float* z, size_t n, float std, uint64_t seed, const uint64_t* step_ptr, float* out /*F*/, unsigned io,
                     void* stream);

/* ---------------------------------------------------------------- up-sampling / concat ----------
 * Replaces nn.Upsample(scale_factor=2, mode=nearest|bilinear|trilinear, align_corners=False)
 * (mulresunet.py:168,242; skip.py:128,231) fused with the centre-crop of Concat/Concat3D
 * (base.py:297-319,333-359): the output may be cropped to (Do,Ho,Wo) <= 2*(D,H,W), offset 0.
 * 2-D: D = Do = 1 (no scaling along D when D == Do == 1).
 */
int dpi_upsample2x_fwd(const float* x, const float* chain, int C, int D, int H, int W, int Do, int Ho,
                       int Wo, int linear, float* y, void* stream);
/* ws (optional, linear only): dpi_upsample2x_bwd_ws_floats floats; with it the adjoint runs as three separable,
 * coalesced passes (W, H, D) instead of a 64-tap gather per voxel.  NULL = gather. */
size_t dpi_upsample2x_bwd_ws_floats(int C, int D, int H, int W, int Do, int Ho, int Wo, int linear);
int dpi_upsample2x_bwd(const float* dy, int C, int D, int H, int W, int Do, int Ho, int Wo, int linear,
                       float* dx, float* ws, void* stream);
/* centre-crop copy [C][D][H][W] -> [C][Do][Ho][Wo] starting at (od,oh,ow); and its adjoint (zero-fill) */
int dpi_crop_copy(const float* x, int C, int D, int H, int W, int od, int oh, int ow, int Do, int Ho,
                  int Wo, float* y, void* stream);
int dpi_crop_copy_bwd(const float* dy, int C, int D, int H, int W, int od, int oh, int ow, int Do,
                      int Ho, int Wo, float* dx, void* stream);

/* ---------------------------------------------------------------- attention gate ----------------
 * Replaces the tail of GridAttentionBlock.forward, `psi = Upsample(2, bilinear)(Sigmoid(q)); return x * psi` (attention.py:107-113), for the
 * skip tensor x [C][Do][Ho][Wo] and the one-channel map q [D][H][W] on the coarse grid: Ho = 2 H, Wo = 2 W, Do = scale_d ? 2 D : D
 * (D = 1, scale_d = 0: the reference's 2-D case; scale_d = 1: the 3-D net).  Up-sampling as dpi_upsample2x_fwd with linear = 1
 * (align_corners=False, taps .25 / .75, edge-clamped).  fp32 tensors only.  x, y, dy, dx may be views at any element offset (y a channel
 * slice of the concatenated tensor): 16-, 8- or 4-byte accesses are chosen from the addresses of the call and give bit-identical results.
 * No atomics: every result is bitwise reproducible.
 *   y[c][v] = x[c][v] * a[v],  a = upsample2x(s),  s = sigmoid(q);  s_out [D][H][W] receives s for the backward. */
int dpi_attn_gate_fwd(const float* x, const float* q, int C, int D, int H, int W, int scale_d, float* s_out, float* y, void* stream);
/* Backward of attention.py:107-113 in two launches: dx[c][v] = dy[c][v] * a[v] with t[v] = sum_c dy[c][v] * x[c][v] into ws, then
 * dq = (adjoint up-sampling of t) * s * (1 - s) as a gather on the coarse grid.  ws: dpi_attn_gate_bwd_ws_floats floats (0 = bad geometry). */
size_t dpi_attn_gate_bwd_ws_floats(int C, int D, int H, int W, int scale_d);
int dpi_attn_gate_bwd(const float* dy, const float* x, const float* s, int C, int D, int H, int W, int scale_d, float* dx, float* dq,
                      float* ws, void* stream);

/* ---------------------------------------------------------------- partial convolution ------------
 * Replaces everything around the convolution in Partial2DConv / Partial3DConv.forward (partial_unet.py:42-70, 119-147) for one patch:
 *   xm = x * m;  c = conv3x3(x3)(xm, W) without bias (dpi_conv_fwd);  S[v] = sum over the channels and the zero-padded 3x3(x3) window of m
 *   (the all-ones mask_conv, one value per voxel);  y[o][v] = S[v] == 0 ? 0 : c[o][v] / S[v] + b[o];  new_mask[v] = S[v] == 0 ? 0 : 1.
 * x [Cin][V], m [Cm][V] with Cm = Cin or 1 (broadcast), V = D H W voxels (D = 1: 2-D, the window is 3 x 3).  S is not differentiated
 * (partial_unet.py:47-49 computes it under no_grad).  fp32 tensors only.  Tensors may be views at any element offset and V any count:
 * 16-, 8- or 4-byte accesses are chosen from the addresses of the call and from V and give bit-identical results.  No atomics: every
 * result, the bias gradient included, is bitwise reproducible.
 *   partial_unet.py:44,121 `input_x * mask` and the channel sum of the mask: xm [Cin][V], msum[v] = sum_c m[c][v] (Cm = 1: Cin * m[v]) */
int dpi_pconv_mask_fwd(const float* x, const float* m, int Cin, int Cm, size_t V, float* xm, float* msum, void* stream);
/* partial_unet.py:47-70, 124-147: S = box sum of msum (27 additions in the order d, h, w, a tap outside adding 0), y (may be c itself),
 * the ONE-channel new_mask [V] (the reference stores Cout identical channels) and S [V] for the backward.  bias [Cout] or NULL. */
int dpi_pconv_norm_fwd(const float* c, const float* msum, const float* bias, int Cout, int D, int H, int W, float* y, float* new_mask,
                       float* S, void* stream);
/* Backward of partial_unet.py:65-66, 142-143: dc[o][v] = S[v] == 0 ? 0 : dy[o][v] / S[v]; dbias[o] = sum over S[v] != 0 of dy[o][v] (NULL:
 * not computed) as one partial per 256 voxels in ws, then a fixed-order finaliser.  ws: dpi_pconv_norm_bwd_ws_floats floats (0 = bad
 * geometry), needed only with dbias. */
size_t dpi_pconv_norm_bwd_ws_floats(int Cout, size_t V);
int dpi_pconv_norm_bwd(const float* dy, const float* S, int Cout, size_t V, float* dc, float* dbias, float* ws, void* stream);
/* Backward of partial_unet.py:44,121 `input_x * mask`: dx[c][v] = dxm[c][v] * m[c][v] (dx may be dxm itself); dm (NULL: not computed)
 * [Cm][V]: dm[c][v] = dxm[c][v] * x[c][v] for Cm = Cin, dm[v] = sum_c dxm[c][v] * x[c][v] for Cm = 1.  x may be NULL without dm. */
int dpi_pconv_mask_bwd(const float* dxm, const float* x, const float* m, int Cin, int Cm, size_t V, float* dx, float* dm, void* stream);

/* ---------------------------------------------------------------- plain 2-D UNet extras ----------
 * Replaces nn.MaxPool2d(2, 2) (unet.py:42) and nn.ConvTranspose2d(Cin, Cout, 4, stride=2, padding=1) (unet.py:59) with
 * their backward passes.  x: [C][H][W]; pooled / transposed outputs are [C][H/2][W/2] and [Cout][2H][2W];
 * deconv weight layout is torch's [Cin][Cout][4][4].  bias [Cout] or NULL; H, W >= 1 for the transposed convolution, >= 2 for the pool.
 * The pool takes the first maximum of a window in (kh, kw) scan order, like aten: a later tap replaces the running maximum only if it
 * is greater, so of equal taps (0.0 and -0.0 included) the first is returned and receives dy, and a NaN is never selected unless it is
 * tap (0, 0).  dpi_maxpool2x2_bwd writes all of dx: 0 at the other taps and in the trailing row / column of an odd H / W. */
int dpi_maxpool2x2_fwd(const float* x, int C, int H, int W, float* y, void* stream);
int dpi_maxpool2x2_bwd(const float* dy, const float* x, int C, int H, int W, float* dx, void* stream);
int dpi_deconv4x4s2_fwd(const float* x, const float* w, const float* bias, int Cin, int Cout, int H, int W,
                        float* y, void* stream);
int dpi_deconv4x4s2_bwd_data(const float* dy, const float* w, int Cin, int Cout, int H, int W, float* dx,
                             void* stream);
int dpi_deconv4x4s2_bwd_weight(const float* x, const float* dy, int Cin, int Cout, int H, int W, float* dw,
                               void* stream);

/* ---------------------------------------------------------------- plain 3-D UNet extras ----------
 * nn.MaxPool3d(2, 2) and nn.ConvTranspose3d(Cin, Cout, 4, stride=2, padding=1) with their backward passes, for UNet3D (ours: the
 * reference has no 3-D form of its plain UNet).  fp32 in every --precision mode.  x: [C][D][H][W]; pooled / transposed outputs are
 * [C][D/2][H/2][W/2] (floor) and [Cout][2D][2H][2W]; deconv weight layout is torch's [Cin][Cout][4][4][4]; bias [Cout] or NULL.
 * D, H, W >= 1 for the transposed convolution, >= 2 for the pool.  Tensors may be views at any element offset.
 * Pool: y[c][od][oh][ow] = the first maximum of x[c][2od + kd][2oh + kh][2ow + kw] in (kd, kh, kw) scan order, like aten: a later tap
 * replaces the running maximum only if it is greater, so of equal taps (0.0 and -0.0 included) the first is returned and receives dy,
 * and a NaN is never selected unless it is tap (0, 0, 0).  dpi_maxpool2x2x2_bwd writes all of dx: 0 at the other taps and in the
 * trailing plane / row / column of an odd D / H / W.
 * Transposed convolution: y[co][od][oh][ow] = bias[co] + sum over ci and the taps with o = 2 i - 1 + k on every axis of
 * x[ci][id][ih][iw] w[ci][co][kd][kh][kw] (at most 2 x 2 x 2 taps reach an output);  dx[ci][i] = sum over co and the 4 x 4 x 4 taps of
 * dy[co][2 i - 1 + k] w[ci][co][k] (outputs outside the tensor add 0);  dw[ci][co][k] = sum over i of x[ci][i] dy[co][2 i - 1 + k].
 * With Cin and Cout multiples of 16 the three run as GEMMs over the eight output-parity classes on v_mfma_f32_16x16x4_f32 (operands
 * staged in LDS, fp32 accumulation); other channel counts take one-thread-per-output VALU kernels.  Either way the summation order is
 * fixed and there are no atomics: two launches on the same data give the same bits.  ws of dpi_deconv4x4x4s2_bwd_weight:
 * dpi_deconv4x4x4s2_bwd_weight_ws_floats floats (0 = bad geometry, never 0 otherwise).
 * Refused with DPI_E_ARG before any launch: a NULL pointer (bias excepted), an output that is one of the inputs, a non-positive size,
 * and a tensor of the call with more than 2^31 - 1 elements. */
int dpi_maxpool2x2x2_fwd(const float* x, int C, int D, int H, int W, float* y, void* stream);
int dpi_maxpool2x2x2_bwd(const float* dy, const float* x, int C, int D, int H, int W, float* dx, void* stream);
int dpi_deconv4x4x4s2_fwd(const float* x, const float* w, const float* bias, int Cin, int Cout, int D, int H, int W,
                          float* y, void* stream);
int dpi_deconv4x4x4s2_bwd_data(const float* dy, const float* w, int Cin, int Cout, int D, int H, int W, float* dx,
                               void* stream);
size_t dpi_deconv4x4x4s2_bwd_weight_ws_floats(int Cin, int Cout, int D, int H, int W);
int dpi_deconv4x4x4s2_bwd_weight(const float* x, const float* dy, int Cin, int Cout, int D, int H, int W, float* dw,
                                 float* ws, void* stream);

/* ---------------------------------------------------------------- loss + metrics ----------------
 * Replaces main.py:161-167: loss = mean(|out*m - img*m|) (kind 0, L1) or mean((.)^2) (kind 1, MSE)
 * over all n elements; dout = dloss/dout * grad_scale; plus the sums for snr/pcorr
 * (utils/metrics.py:15,32-36).  ws: double[dpi_loss_ws_doubles(n)].
 * result (device, double[8]): {loss, snr_dB, pcorr, sum_t2, sum_(t-o)^2, sum_o, sum_t, sum_o2}; all eight are written.
 * Extents (tests/test_gpu_iteration_contract.py holds every launch to them, inside guard bands): dpi_loss_ws_doubles(n) = 8 * 1024 for
 * every n — the grid is min(ceil(n / 2048), 1024) blocks and block b writes ws[8 b .. 8 b + 6] only; nothing is read or written past
 * result[7].  Per element, in fp32: d = out*mask - img*mask, inv_n = grad_scale / (float)n, dout = ((2 d) mask) inv_n (MSE) or
 * (sign(d) mask) inv_n (L1); dout may be NULL (no gradient is stored, the result is the same bit for bit).  The sums are accumulated in
 * double in a fixed order: two launches on the same data give the same bits.
 */
size_t dpi_loss_ws_doubles(size_t n);
int dpi_masked_loss(const float* out, const float* img, const float* mask, size_t n, int kind,
                    float grad_scale, float* dout, double* ws, double* result, void* stream);
/* ABI 406.  The same pass with held-out traces (--holdout).  The tensors are [C][T][S] (n = C*T*S: the device layout (1, C, T, S...)
 * of a patch, one trace per (c, s)); sel (device, float[C][S]) is 1 on the held-out traces and 0 elsewhere.  With m_tr = mask * (1 - sel)
 * and m_ho = mask * sel per sample, dout and result[0..7] are bit for bit those of dpi_masked_loss(out, img, m_tr, n, ...) — same grid, walk
 * and accumulation order; neither mask is materialised — and the pass adds, with e = t - o:
 *   result[8] = val_loss = sum |e m_ho| (kind 0) or sum (e m_ho)^2 (kind 1), divided by N_ho;
 *   result[9] = val_snr  = 10 log10(sum (t m_ho)^2 / sum (e m_ho)^2);   result[10] = N_ho = number of samples with m_ho != 0.
 * result: double[11], all written.  ws: double[2 * dpi_loss_ws_doubles(n)] (block b writes ws[16 b .. 16 b + 11]). */
int dpi_masked_loss_holdout(const float* out, const float* img, const float* mask, const float* sel, int C, int T, size_t S,
                            int kind, float grad_scale, float* dout, double* ws, double* result, void* stream);

/* Running average of the network output (--out_ema; the out_avg of the deep-image-prior method, which the reference dropped) with the
 * metrics of the average in the same pass.  Tensors as dpi_masked_loss_holdout ([C][T][S], n = C*T*S); sel may be NULL (no held-out part).
 * it = (int)step_lr[0]: called BEFORE the optimiser step of an iteration it is the 0-based iteration index (dpi_moments_update).
 *   *active == 0 (active may be NULL): avg and result stay untouched.
 *   it == 0:  avg = out, whatever avg held (it is not read: NaNs of a fresh buffer do not leak);
 *   else      avg = avg + w * (out - avg) in fp32, w = (float)(1.0 - (double)beta), beta in [0, 1).
 * result has the layout and the meaning of dpi_masked_loss_holdout evaluated on the stored avg (double[11]: training part on
 * mask * (1 - sel), held-out part in [8..10]); with sel == NULL only result[0..7] are written, as dpi_masked_loss(avg, img, mask) writes
 * them.  Grid, walk and summation order are those of the loss pass (double partials, fixed order, no atomics), so the numbers are bit for
 * bit what that pass gives on avg.  There is no gradient: the iterate's own dpi_masked_loss[_holdout] call stays as it is.
 * ws: double[2 * dpi_loss_ws_doubles(n)].  Traffic: out, avg, img, mask read, avg written: 20 B per sample. */
int dpi_ema_loss(const float* out, float* avg, const float* img, const float* mask, const float* sel, int C, int T, size_t S,
                 int kind, float beta, const float* step_lr, const int* active, double* ws, double* result, void* stream);

/* ---------------------------------------------------------------- optimiser ---------------------
 * Replaces torch.optim.Adam(lr, betas=(0.9,0.999), eps=1e-8).step() (main.py:200,213) for a list of
 * tensors in ONE launch.  ptrs: device array of {p, g, m, v} pointers per tensor; sizes: element counts;
 * step_lr (device, float[2]): {step count as float (already incremented), lr}.  `active` (device int,
 * may be NULL): when *active == 0 the update is skipped (device-side early stop).  Betas/eps are doubles so that
 * 1-beta and the bias corrections are derived in double and then rounded, exactly as torch does on the host.
 * Rounding points (the library is built with -ffp-contract=off; tests/iteration_cases.py adam_np restates them and
 * tests/test_gpu_iteration_contract.py holds p, m and v to that restatement bit for bit):
 *   omb1 = (float)(1 - beta1), omb2 = (float)(1 - beta2), step_size = (float)(lr / (1 - beta1^step)), bc2s = (float)sqrt(1 - beta2^step),
 *   with lr the fp32 step_lr[1] widened to double, and beta2, eps rounded to fp32; then per element, every operation in fp32:
 *   m = m + omb1 * (g - m);   v = beta2 * v + (omb2 * g) * g;   p = p - step_size * (m / (sqrt(v) / bc2s + eps)).
 * torch's CPU kernels fuse the multiply-adds of lerp_ / addcmul_ and form (step_size * m) / denom: against torch.optim.Adam one step
 * differs by at most 1 ulp in m and v and 5 ulp of max(|p|, |update|) in p (measured, tests/test_iteration_refs_host.py).
 * ntensors must lie in [1, 65535] (it is a grid dimension).  Accesses are scalar: a row may start at any element offset.  g is only read.
 */
typedef struct { float* p; const float* g; float* m; float* v; } dpi_adam_tensor;
int dpi_adam_multi(const dpi_adam_tensor* tensors, const int64_t* sizes, int ntensors,
                   const float* step_lr, double beta1, double beta2, double eps, const int* active,
                   void* stream);
/* Langevin samplers in one launch for all tensors.  Replaces architectures/optimizers.py:79-106 (SGLD.step, momentum 0) and :144-181
 * (pSGLD.step, not centred), which the reference ships without a caller.  Table, sizes, step_lr {step already incremented, lr}, `active`
 * and the grid are those of dpi_adam_multi; the `m` slot is unused, pSGLD keeps V in the `v` slot.  With d = g + weight_decay * p (only
 * when weight_decay != 0):
 *   kind 0 (SGLD):   p -= lr * d;  p += sqrt(noise_scale) * sqrt(temperature) * xi
 *   kind 1 (pSGLD):  V = beta * V + (1 - beta) * d * d;  G = sqrt(V) + lambda;  p -= lr * d / G;  p += sqrt(2 * lr / G) * sqrt(temperature) * xi
 * in the operation order and with the rounding points of the torch CPU calls the reference makes (csrc/loss_optim.hip); sqrt(temperature)
 * is a separate fp32 factor, so temperature 1 is the reference's rule.  xi (device array of `ntensors` device pointers, row order of the
 * table) holds the standard normals; xi == NULL draws them in the kernel: Philox4x32-10 with key `seed`, stream id
 * (0xFFFFFFFE << 32) | step (read from step_lr[0] on the device: a replayed graph draws fresh noise) and counter (row << 40) | q, q the
 * group of four consecutive elements of the tensor — the normals dpi_fill_normal(mean 0, std 1) writes for that stream on row 0. */
int dpi_langevin_multi(const dpi_adam_tensor* tensors, const int64_t* sizes, int ntensors, const float* step_lr, int kind,
                       double weight_decay, double beta, double lambda, double noise_scale, double temperature, uint64_t seed,
                       const float* const* xi, const int* active, void* stream);
/* Posterior moments of the network output over the sampled iterations (the iterate averaging of the Bayesian deep-image-prior use of
 * optimizers.py; the reference has no caller).  it = (int)step_lr[0]: called BEFORE the optimiser step of an iteration it is the 0-based
 * iteration index.  Nothing happens when *active == 0 (active may be NULL), it < burn_in or (it - burn_in) % thin != 0; otherwise, with
 * k = (it - burn_in) / thin + 1 (Welford):  delta = out - mean;  mean += delta / k;  m2 += delta * (out - mean).
 * out, mean, m2: device float[n]. */
int dpi_moments_update(const float* out, float* mean, float* m2, size_t n, const float* step_lr, int burn_in, int thin,
                       const int* active, void* stream);

/* ---------------------------------------------------------------- device-resident loop control --
 * Replaces the host-side bookkeeping of main.py:165-182,214-217 so that a captured hipGraph of one iteration can be
 * replayed without host synchronisation: appends {loss, snr, pcorr, lr} to hist[iter], raises *improved when
 * loss <= loss_min (best-output tracking), runs ReduceLROnPlateau(mode=min, rel threshold) on step_lr[1] and
 * EarlyStopping(percentage) / NaN stop on *active.  state: double[8], zero-initialised except state[2] = +inf.
 * hist: double[4 * max_iters]; a call with state[0] >= max_iters writes no row and still advances state[0].  *active == 0 on entry:
 * state, hist and step_lr stay bit for bit as they were and *improved is set to 0.  A tie (loss == loss_min) improves: the later
 * iterate wins.  A NaN loss never improves; it stops the run only with es_patience != 0 and from the second call on (the first call's
 * loss becomes es_best unexamined, as in utils/torch.py).
 * dpi_copy_if copies src -> dst only when *flag != 0 (keeps out_best on the device). */
int dpi_loop_control(const double* metrics, double* state, double* hist, int max_iters, float* step_lr,
                     int* active, int* improved, int use_plateau, double factor, double threshold,
                     int patience, double min_lr, double lr_eps, int es_patience, double es_min_delta,
                     void* stream);
/* ABI 406.  dpi_loop_control for a run with held-out traces: metrics = the 11 doubles of dpi_masked_loss_holdout, hist rows of six
 * {loss, snr, pcorr, lr, val_loss, val_snr}.  *improved (best output) when val_loss <= val_min (the later iterate wins a tie) and
 * EarlyStopping(percentage) / NaN stop follow val_loss; ReduceLROnPlateau follows the training loss metrics[0].
 * state: double[10] {iter, loss_min (training), plateau_best, plateau_bad, es_best, es_bad, es_has_best, reserved, val_min, best_iter},
 * zero-initialised except state[2] = +inf. */
int dpi_loop_control_holdout(const double* metrics, double* state, double* hist, int max_iters, float* step_lr,
                             int* active, int* improved, int use_plateau, double factor, double threshold,
                             int patience, double min_lr, double lr_eps, int es_patience, double es_min_delta,
                             void* stream);
/* dpi_loop_control for a run with --out_ema, with (has_holdout != 0) or without held-out traces.  metrics = the doubles of the raw iterate
 * (dpi_masked_loss: 8, dpi_masked_loss_holdout: 11), ema_metrics = those of the stored average (dpi_ema_loss).  hist rows: the 4 raw columns
 * {loss, snr, pcorr, lr} (6 with a holdout: + {val_loss, val_snr}), then {ema_loss, ema_snr} and, with a holdout, {ema_val_loss, ema_val_snr}:
 * 6 or 10 doubles per iteration.  *improved and best_iter follow the average's selection misfit q = ema_val_loss with a holdout, else
 * ema_loss (q <= q_min: the later iterate wins a tie; a NaN never improves); EarlyStopping(percentage) / the NaN stop follow q too;
 * ReduceLROnPlateau follows the raw training loss metrics[0].  The caller keeps the selected average with dpi_copy_if(improved, avg, best).
 * state: double[12], zero-initialised except state[2] = +inf:
 *   [0] iter   [1] loss_min (raw training)   [2] plateau_best   [3] plateau_bad   [4] es_best   [5] es_bad   [6] es_has_best   [7] reserved
 *   [8] val_min (raw held-out misfit; holdout only)   [9] best_iter   [10] q_min   [11] reserved */
int dpi_loop_control_ema(const double* metrics, const double* ema_metrics, int has_holdout, double* state, double* hist,
                         int max_iters, float* step_lr, int* active, int* improved, int use_plateau, double factor,
                         double threshold, int patience, double min_lr, double lr_eps, int es_patience, double es_min_delta,
                         void* stream);
int dpi_copy_if(const int* flag, const float* src, float* dst, size_t n, void* stream);

/* ---------------------------------------------------------------- input perturbation ------------
 * Replaces main.py:148-150: out = z + std * N(0,1), Philox4x32-10 + Box-Muller, counter = element index,
 * key = (seed, *step_ptr) so that every replay of a captured graph draws fresh noise.
 * step_ptr (device, uint64) may be NULL (then step = 0).
 * The stream, as tests/iteration_cases.py restates it on the host: elements 4q .. 4q+3 come from ONE Philox4x32-10 block with counter
 * words {q lo, q hi, stream lo, stream hi} (stream = *step_ptr, or stream_id for dpi_fill_normal) and key {seed lo, seed hi}; Box-Muller
 * on the four output words c0..c3: r0 = sqrt(-2 ln(((c0 >> 8) + 1) / 2^24)), a0 = 2 pi (c1 >> 8) / 2^24, likewise r1, a1 from c2, c3;
 * the four normals are r0 cos a0, r0 sin a0, r1 cos a1, r1 sin a1, and out = fma(std, normal, z or mean).  n % 4 != 0 and n % 4 == 0
 * draw the same values.  The float4 path is chosen from n % 4 alone (the precondition above dpi_bn_*).
 */
int dpi_noise_add(const float* z, size_t n, float std, uint64_t seed, const uint64_t* step_ptr,
                  float* out, void* stream);
int dpi_fill_normal(float* out, size_t n, float mean, float std, uint64_t seed, uint64_t stream_id,
                    void* stream);
/* dpi_noise_add for a z that IS such a fill (z = dpi_fill_normal(mean 0, z_std, z_seed, z_stream_id), untouched since): the kernel re-draws z
 * from its Philox stream instead of reading it — out = z + std * N(0,1) with the same bits as dpi_noise_add_io(z, ...), minus the HBM read of
 * z (64 channels at full resolution, every iteration).  io: DPI_STORE_FWD_BF16 = out is bf16. */
int dpi_noise_add_regen_io(size_t n, float z_std, uint64_t z_seed, uint64_t z_stream_id, float std, uint64_t seed,
                           const uint64_t* step_ptr, float* out /*F*/, unsigned io, void* stream);
/* Replaces utils/processing.py:34-67 (ConvolveKernel_1d: grouped conv_transposeNd with a 1-D kernel along the time
 * axis, used by --filter_noise_with_wavelet / --lowpass_*): y[c][t][s] = sum_k taps[k] * x[c][t + K/2 - k][s],
 * x: [C][T][S] with S = product of the remaining spatial axes; K odd; taps on the device. */
int dpi_fir_axis0(const float* x, const float* taps, int K, int C, int T, size_t S, float* y, void* stream);
/* y += a * x  (data-forgetting term of main.py:153-154) */
int dpi_axpy(float a, const float* x, size_t n, float* y, void* stream);

/* ---------------------------------------------------------------- patch reassembly --------------
 * Replaces PatchExtractor.reconstruct (utils/patch_extractor.py:395-428): overlap-add of one patch
 * (pd,ph,pw) at origin (od,oh,ow) into acc[D][H][W]; dpi_overlap_normalize divides by the analytic hit
 * count of the regular window grid and by `gain` (data.py:116).
 * dpi_overlap_add: acc += patch, one fp32 addition per sample, in launch order on one stream; a patch reaching outside the volume is
 * refused.  dpi_overlap_normalize: acc = acc / ((float)count * gain) with count the number of windows {k * stride : 0 <= k * stride <=
 * N - p} per axis that cover the sample, multiplied over the axes; gain == 0 and a stride <= 0 are refused.  A sample that no window
 * covers — the far end of an axis with (N - p) % stride != 0 — has count 0 and gets acc / 0: +-inf, or NaN where acc is 0.  The callers
 * use window grids that cover the volume; the weighted pair below writes 0 there instead.
 */
int dpi_overlap_add(const float* patch, int pd, int ph, int pw, int od, int oh, int ow, float* acc,
                    int D, int H, int W, void* stream);
int dpi_overlap_normalize(float* acc, int D, int H, int W, int pd, int ph, int pw, int sd, int sh,
                          int sw, float gain, void* stream);
/* Weighted overlap-add (ours: --reassembly cover, --blend taper, the std volume of a sampler run; utils/patch_extractor.py `reassemble`
 * defines the arithmetic).  acc is ONE stacked buffer [K][D][H][W], zeroed by the caller: plane 0 += w, plane 1 += w * mean, plane 2 +=
 * w * std^2; K = 3 exactly when std (a patch of per-sample standard deviations, same shape as mean) is given, else 2.
 * w = (w_d * w_h) * w_w in fp32; along an axis of p samples with a ramp table of l <= p/2 floats on the device (may be null when l = 0) the
 * weight of sample i is ramp[i] for i < l where the low face tapers, ramp[p-1-i] for i >= p - l where the high face does, 1 elsewhere.
 * sides: bit 0 / 1 = low / high face of the D axis, bits 2 / 3 of H, bits 4 / 5 of W; a face on the volume's edge is left out by the caller.
 * One pass, a thread per four consecutive samples along W; 16-byte accesses when pw, ow and W are multiples of 4 and mean, std and acc sit
 * on 16 bytes, one sample at a time otherwise.  No atomics: calls that add into one acc go to one stream (or are ordered by events). */
int dpi_overlap_add_weighted(const float* mean, const float* std /*nullable*/, int pd, int ph, int pw, int od, int oh, int ow,
                             const float* ramp_d, int ld, const float* ramp_h, int lh, const float* ramp_w, int lw, unsigned sides,
                             float* acc, int K, int D, int H, int W, void* stream);
/* out_mean = plane 1 / plane 0 / gain; out_std (nullable; needs K = 3) = sqrt(plane 2 / plane 0) / |gain|: the window-weighted mean of the
 * per-patch variances, i.e. the spread WITHIN the windows, not the disagreement between overlapping patches.  A sample of weight 0 gives 0.
 * out_mean and out_std are [D][H][W] buffers of their own (not planes of acc). */
int dpi_overlap_finalize_weighted(const float* acc, int K, int D, int H, int W, float gain, float* out_mean, float* out_std /*nullable*/,
                                  void* stream);

/* ---------------------------------------------------------------- anti-aliasing operators -------
 * Linear operators of the anti-aliasing add-on (BASELINE configs[3]); `adjoint` != 0 applies the exact transpose, which is
 * what the backward of a loss term built on the operator needs (reference operators/base.py:53-67 `dottest` is the unit test).
 *
 * dpi_diff_axis replaces utils/processing.py:139-181 first_derivative (stencil 0 forward, 1 backward, 2 centered) and
 * second_derivative (stencil 3) along the middle axis of a contiguous [outer][n][inner] view, and with stencil 0, spacing 1 on the
 * H axis of BCHW it is operators/derivative.py:8-21 VerticalGrad.forward / .adjoint.   x != y.
 * The differences are followed by ONE fp32 division by the spacing, like the reference, so the three first derivatives are the reference's
 * bits.  The second derivative divides by the fp32 product spacing * spacing of the fp32 argument, where the reference rounds the double
 * spacing ** 2 once: the two divisors can be one ulp apart (0.7: they are), the quotients two. */
int dpi_diff_axis(const float* x, size_t outer, int n, size_t inner, int stencil, float spacing, int adjoint, float* y,
                  void* stream);
/* Replaces utils/slopes.py:51-105 directional_laplacian / Hale2D.forward on [N][H][W] planes with coefficient planes
 * a = cos^2, b = -cos sin, c = sin^2 of the dips (same shape as x):  y = -(Dh(a Dv x + b Dh x) + Dv(b Dv x + c Dh x)). */
int dpi_hale2d(const float* x, const float* a, const float* b, const float* c, size_t N, int H, int W, int adjoint, float* y,
               void* stream);
/* Replaces utils/slopes.py:19-22 (forward-difference gradients and their products) and :35-46 (eigen-analysis: dip angle phi
 * with NaN -> 0, anisotropy 1 - l2/l1); the Gaussian smoothing in between (:25-32) is dpi_fir_axis0 along H and W.
 * dpi_dips evaluates t1 = (gvv + ghh) / 2, t2 = sqrt((gvv - ghh)^2 + 4 gvh^2) / 2, l1 = t1 + t2, l2 = t1 - t2 in fp32, one rounding per
 * operation, and leaves the special cases as IEEE gives them: with gvh = 0 the ratio (l1 - gvv) / gvh is 0 / 0 where l1 == gvv (a
 * diagonal tensor with gvv >= ghh, e.g. (3, 0, 1)), which gives phi = 0, and +-inf otherwise ((1, 0, 3): phi = +pi/2); the zero tensor has
 * phi = 0 and the anisotropy NaN. */
int dpi_structure_tensor(const float* x, size_t N, int H, int W, float dv, float dh, float* gvv, float* gvh, float* ghh,
                         void* stream);
int dpi_dips(const float* gvv, const float* gvh, const float* ghh, size_t n, float* phi, float* anisotropy, void* stream);
/* ABI 405.  The same operator on both families of vertical sections of a [C][T][X][Y] patch (Y contiguous): the (t,x) sections
 * (v = t, h = x) and the (t,y) sections (v = t, h = y).  coef: six [C][T][X][Y] fields a, b, c of the (t,x) family, then of the (t,y)
 * family.  Forward: y = [2][C][T][X][Y], the (t,x) result then the (t,y) result.  Adjoint: x is that [2][...] tensor and
 * y = L_tx^T x[0] + L_ty^T x[1].  Per sample the same arithmetic as dpi_hale2d on the section.  C*T*X*Y < 2^31; x != y. */
int dpi_hale_sections(const float* x, const float* coef, int C, int T, int X, int Y, int adjoint, float* y, void* stream);
/* ABI 405.  dpi_structure_tensor for both section families of a [C][T][X][Y] patch in one pass: forward-difference gradients gt, gx,
 * gy (spacings dt, dx, dy) and the five products gtt (shared), gtx, gxx (t,x) and gty, gyy (t,y).  The smoothing is dpi_fir_axis0
 * along the two axes of each family, the angles dpi_dips. */
int dpi_structure_tensor_sections(const float* x, int C, int T, int X, int Y, float dt, float dx, float dy, float* gtt, float* gtx,
                                  float* gxx, float* gty, float* gyy, void* stream);

/* ---------------------------------------------------------------- AVO modelling (--avo_theta) -------
 * Replaces operators/avo.py:67-95 AVOLinearModelling.forward / .adjoint: the linearised amplitude-versus-angle operator that maps three
 * elastic-parameter sections to ntheta angle sections, y[a][t][s] = sum_k G[a][k][t] * x[k][t][s] (dpi_avo_fwd), and its exact transpose
 * x[k][t][s] = sum_a G[a][k][t] * y[a][t][s] (dpi_avo_adj: the backward of the forward call and the reference's .adjoint).
 * x = [3][T][S], y = [ntheta][T][S], G = [ntheta][3][T] (the reference's G (ntheta, 3, nt0, 1[, 1]) without its unit axes), all fp32 and
 * contiguous; S = the product of the spatial sizes behind t.  Any ntheta, T, S >= 1 and any 4-byte aligned x / y (16-byte accesses only
 * on the rows that start on 16 bytes in both); no atomics: the sums run in a fixed order (k = 0, 1, 2; a = 0 .. ntheta-1), so a result
 * does not depend on the launch shape.  Input and output must not alias.  ABI version stays: a stale library fails on the unresolved
 * symbols. */
int dpi_avo_fwd(const float* x, const float* G, int ntheta, int T, size_t S, float* y, void* stream);
int dpi_avo_adj(const float* y, const float* G, int ntheta, int T, size_t S, float* x, void* stream);

/* ---------------------------------------------------------------- Convolutional modelling (--wavelet) --
 * Replaces operators/signal.py:8-45 (VerticalConv: every trace convolved with a wavelet along t) behind operators/derivative.py:8-21
 * (VerticalGrad: the forward difference along t, last row zero) in one launch each way: the convolutional model of seismic data,
 * d = w * r on a reflectivity section (diff = 0) and d = (w / 2) * D ln(AI) on a log-impedance section (diff = 1, taps = w / 2).
 * Tensors [C][T][S] fp32, contiguous, S = X or X * Y: one layout for (1, C, T, X) and (1, C, T, X, Y).  taps: K floats on the device.
 *     dpi_wavelet_fwd:  d[c][t][s] = sum_k taps[k] * u[c][t + K/2 - k][s], zero outside [0, T): a true convolution centred on K/2, the
 *                       arithmetic of dpi_fir_axis0.  diff = 0: u = m.  diff = 1: u[t] = m[t + 1] - m[t] for t < T - 1, u[T - 1] = 0.
 *     dpi_wavelet_adj:  the exact transpose: g[t] = sum_k taps[k] * d[t - K/2 + k]; diff = 0: m = g; diff = 1:
 *                       m[t] = -g[t] [t < T - 1] + g[t - 1] [t >= 1].
 * Every sum is one fmaf chain from 0 over the taps in ascending k (the adjoint: over its reversed taps), whatever the tile or the
 * length of the wavelet; the difference is rounded once.  K odd, 1 <= K <= 255; T < K/2 is fine (a wavelet longer than the trace).
 * Any 4-byte aligned tensors: the input is read 16 bytes at a time when S % 4 == 0 and it starts on 16 bytes, one element at a time
 * otherwise, with the same bits either way.  Null or aliased pointers, an even K or one out of range, diff other than 0 / 1 and
 * C, T, S < 1 return an error before any launch.  ABI version stays: a stale library fails on the unresolved symbols. */
int dpi_wavelet_fwd(const float* m, const float* taps, int K, int diff, int C, int T, size_t S, float* d, void* stream);
int dpi_wavelet_adj(const float* d, const float* taps, int K, int diff, int C, int T, size_t S, float* m, void* stream);

/* ---------------------------------------------------------------- Moveout along t (--moveout) --
 * Ours (the reference warps no axis): d = L m reads every recorded sample from a fractional row of its own trace column of the model m,
 * the flattened gather the network writes.  Tensors [C][T][S] fp32, contiguous, S = X or X * Y: one layout for (1, C, T, X) and
 * (1, C, T, X, Y).  tau: [T][S] fp32 on the device, shared by the channels; a sample is live when 0 <= tau <= T - 1 and muted otherwise.
 *     interp 0, linear: i0 = floor(tau), f = tau - i0, rows i0, i0 + 1 with the weights 1 - f, f.
 *     interp 1, cubic:  Keys, a = -1/2, rows i0 - 1 .. i0 + 2 with ((-.5f+1)f-.5)f, (1.5f-2.5)f^2+1, ((-1.5f+2)f+.5)f, (.5f-.5)f^2.
 * Row indices clamp to [0, T - 1] and every clamped tap counts.
 *     dpi_moveout_fwd:  d[c][t][s] = sum_k w_k(tau[t][s]) * m[c][row_k][s] in ascending k from the first product; 0 where muted.
 *     dpi_moveout_adj:  the exact transpose as a gather without atomics: m[c][i][s] = the sum, in ascending t then k, of w_k d[c][t][s]
 *                       over the live samples range[0][i][s] <= t < range[1][i][s] of column s whose tap k lands on row i (rows 0 and
 *                       T - 1 collect the clamped taps).  range: [2][T][S] int32 on the device; any range that holds every live sample
 *                       touching row i gives the same bits (for a table whose live values do not decrease along t those samples are
 *                       contiguous among the live ones: operators/moveout.py builds the tightest range).  The bounds are clamped to
 *                       [0, T] and every tap is checked against i: no table or range reads or writes out of bounds.
 * The weights come from the same fp32 expressions both ways; f = 0 gives 1, 0 / 0, 1, 0, 0 exactly, so the identity table is the identity
 * bit for bit.  Null or aliased pointers, interp other than 0 / 1, C, T, S < 1 and T > 2^24 return an error before any launch.  ABI version
 * stays: a stale library fails on the unresolved symbols. */
int dpi_moveout_fwd(const float* m, const float* tau, int interp, int C, int T, size_t S, float* d, void* stream);
int dpi_moveout_adj(const float* d, const float* tau, const int* range, int interp, int C, int T, size_t S, float* m, void* stream);

/* ---------------------------------------------------------------- Penalty on the model (--model_reg) --
 * Ours (the reference has no prior on what the network writes): plain L1 or anisotropic total variation of m = [C][n0][n1][n2] fp32,
 * contiguous, N = C n0 n1 n2, value and gradient in one launch.  Bit k of `axes` asks for the differences along n_k; channels are
 * never differenced; axes = 0 is plain L1.
 *     res[0]  = (1/N) sum_{a in axes} sum_i |m[i + e_a] - m[i]| over the pairs inside      (axes = 0: (1/N) sum_i |m[i]|)
 *     grad[i] = (float)k[i] / (float)N with the INTEGER k[i] = sum_a ( sgn(m[i] - m[i - e_a]) [i_a >= 1] - sgn(m[i + e_a] - m[i])
 *               [i_a < n_a - 1] ), axes = 0: sgn(m[i]); sgn from comparisons, sgn(0) = 0: one rounding, the same bits as any restatement.
 * Every |a - b| is formed in fp32 and summed in double: per workgroup into ws (dpi_model_reg_ws_doubles(N) doubles), then by a second
 * launch of one wave in a fixed order (the scheme of dpi_masked_loss).  No atomics, one thread per output: repeated launches give the
 * same bits of grad and res.  An axis of extent 1 contributes nothing.  Any 4-byte aligned tensors: 16-byte accesses along n2 when
 * n2 % 4 == 0 and m and grad both start on 16 bytes, four 4-byte accesses per lane otherwise, with the same bits either way.  A 4-D
 * device tensor (1, C, a, b) is passed as n0 = 1, n1 = a, n2 = b with the bits shifted to match.  Null or aliased pointers, C or an
 * extent < 1, axes outside [0, 7] and a tensor of 2^32 or more groups of four along n2 return an error before any launch.  ABI version
 * stays: a stale library fails on the unresolved symbols. */
size_t dpi_model_reg_ws_doubles(size_t n);
int dpi_model_reg(const float* m, int C, size_t n0, size_t n1, size_t n2, int axes /* bit k: differences along n_k; 0 = plain L1 */,
                  float* grad, double* ws, double* res /* [1]: R */, void* stream);

/* ---------------------------------------------------------------- Semblance velocity scan (--moveout_offset) --
 * Ours (the reference estimates no velocity): the three sums behind a semblance panel, over the known traces of a gather along the
 * hyperbola of every trial velocity.  d, mask: [T][S] fp32 on the device (mask: non-zero = known), any 4-byte aligned address;
 * offset: [S] float64 in cells; vel: [NV] float64 in cells per sample, > 0; stretch: float64, <= 0 = no stretch mute.  Trace k of
 * gather g is column g * group_stride + k * trace_stride, g < n_groups, k < n_traces.  On a (T, X, Y) volume, S = X Y:
 *     the whole cube one gather:               (n_groups, group_stride, n_traces, trace_stride) = (1, 0, S, 1)
 *     every y index a gather of its X traces:  (Y, 1, X, Y)
 *     every x index a gather of its Y traces:  (X, Y, Y, 1)
 * For gather g, velocity v, zero-offset row tau and trace s of that gather, everything in float64:
 *     t = sqrt(tau^2 + (offset[s] / vel[v])^2)
 *     live iff t <= T - 1 and (stretch <= 0 or t <= stretch * tau) and both tap rows i, i + 1 of column s are known
 *     i = min(floor(t), T - 2), f = t - i, a = (1 - f) d[i][s] + f d[i + 1][s]       (T = 1: i = 0, row 0 alone, a = d[0][s])
 *     num[g][v][tau] = sum a, den[g][v][tau] = sum a^2, cnt[g][v][tau] = the number of live traces        (float64, float64, int32)
 * A lane adds its traces in ascending order, a wave is folded by shuffles, the waves that share a row are added in ascending order through
 * LDS: no atomics, repeated launches give the same bits.  A sample that is not live reads nothing and a live one has 0 <= i <= T - 2: no
 * offset, velocity or mask (NaN included: not live) sends a load out of bounds.  The inputs are read only and may share memory.  A null
 * pointer, an output that shares memory with an input or another output, T, S, NV, n_groups or n_traces < 1, a geometry whose last
 * column (n_groups - 1) group_stride + (n_traces - 1) trace_stride is not below S and T > 2^24 return an error before any launch.  ABI
 * version stays: a stale library fails on the unresolved symbol. */
int dpi_semblance_sums(const float* d, const float* mask, const double* offset, const double* vel, int NV, double stretch, int T, size_t S,
                       int n_groups, size_t group_stride, int n_traces, size_t trace_stride, double* num, double* den, int* cnt, void* stream);

/* ---------------------------------------------------------------- NMO table of sampled laws (--moveout_table device) --
 * Ours: operators.nmo_table for laws given at tau = 0 .. T - 1, statement by statement and in its order of operations, all gathers in one
 * launch.  law: [n_groups][T] float64 on the device, cells per sample, finite and > 0; offset: [S] float64 in cells; stretch: the stretch
 * mute, 0 = none; table: [T][S] float64.  The geometry is that of dpi_semblance_sums: trace k of gather g is column g * group_stride +
 * k * trace_stride, and every (g, k) must be a column of its own (the three layouts above name every column once; a column no (g, k)
 * names is left untouched).  For the trace in column s of gather g, v = law[g], off = offset[s], everything in float64:
 *     g[j] = sqrt(j^2 + (off / v[j])^2); jmin = the last index of its minimum; env[j] = max(g[jmin .. j]), -inf below jmin
 *     j(t) = (the number of env <= t) - 1 clipped to [0, T - 2], for the recorded sample t = 0 .. T - 1
 *     live iff j >= jmin, env[j] == g[j], env[j + 1] == g[j + 1], g[j + 1] > g[j], g[j] <= t <= g[j + 1] and (stretch == 0 or
 *          1 / (g[j + 1] - g[j]) <= stretch)
 *     56 bisection steps of [j, j + 1] on travel(x) = sqrt(x^2 + (off / vel(x))^2) <= t with vel(x) = v[j] at x == j, v[j + 1] at
 *          x == j + 1, else (v[j + 1] - v[j]) * (x - j) + v[j]
 *     table[t][s] = hi if travel(hi) == t else lo, clipped to [0, T - 1]; -1 (muted) where not live.  T = 1: 0 where off == 0, else -1.
 * No fused multiply-add: the table can differ from the host's only through the rounding of the fp64 square root and division.  One
 * workgroup per trace, g and env in LDS (16 T bytes), no atomics, one thread per output: repeated launches give the same bits.  No law
 * or offset (NaN included: the sample is muted) reads or writes out of bounds.  A null pointer, table sharing memory with an input, T, S,
 * n_groups or n_traces < 1, a negative or non-finite stretch, a stride < 1 where there is more than one gather / trace, a geometry
 * whose last column is not below S and T > 4096 return an error before any launch.  ABI version stays: a stale library fails on the
 * unresolved symbol. */
int dpi_nmo_table(const double* law, const double* offset, double stretch, int T, int S, int n_groups, int group_stride, int n_traces,
                  int trace_stride, double* table, void* stream);

/* ---------------------------------------------------------------- Trace sampling (--trace_offsets) --
 * Ours (the reference takes every known trace to sit on a grid node): R samples a regular-grid tensor at the recorded trace positions,
 * bilinear in (x, y), the same for every t and every channel.  Tensor [C][T][X][Y] fp32 (a 2-D patch is Y = 1); offsets off = [2][X][Y]
 * fp32, plane 0 dx, plane 1 dy: the recorded position minus the bin centre in units of the grid spacing, |d| <= 0.5.  Per axis, from d
 * alone (no x + d in floating point): d >= 0 -> taps i and i + 1 with weights 1 - d and d; d < 0 -> taps i - 1 and i with weights -d and
 * 1 + d.  Tap indices are clamped to [0, n - 1] (nearest-edge extrapolation); two taps that clamp onto the same node both count, so the
 * weights of a trace always sum to 1.
 *     dpi_trace_sample_fwd:  y[c][t][x][y] = sum over the 2 x 2 taps of wx * wy * in[c][t][tap_x][tap_y]
 *     dpi_trace_sample_adj:  the exact transpose as a gather: grid node (x', y') collects from the 3 x 3 traces around it the weights of
 *                            their clamped taps that are (x', y').  No atomics, sums in a fixed order: deterministic.
 * Zero offsets make both the identity bit for bit.  The tap indices never depend on the size of d, so offsets out of range or not finite
 * cannot address out of bounds (the Python operator refuses them).  Null pointers, in == out, a non-positive size and more than 2^60
 * elements return an error before any launch.  ABI version stays: a stale library fails on the unresolved symbols. */
int dpi_trace_sample_fwd(const float* x, const float* off, int C, int T, int X, int Y, float* y, void* stream);
int dpi_trace_sample_adj(const float* y, const float* off, int C, int T, int X, int Y, float* x, void* stream);

/* ---------------------------------------------------------------- Trace sampling with K x K taps (--trace_interp) --
 * Ours.  The bilinear R above is a low-pass filter whose strength depends on the offset (a zero at the spatial Nyquist wavenumber for
 * d = 0.5); these entry points apply R from a table of per-trace weights with K taps per axis.  Kinds 0 / 1 / 2 = linear / cubic /
 * sinc8, K = 2 / 4 / 8 (dpi_trace_interp_taps; -1 for an unknown kind).
 * Tap geometry, per axis of n nodes, trace on node i with offset d: the first tap is i - K/2 + 1 when d >= 0, else i - K/2; tap k in
 * [0, K) sits at clamp(first + k, 0, n - 1); taps that clamp onto one node all count.  Tap indices never depend on the size of d (the
 * offsets are read for their sign only), and K = 2 is exactly the geometry of dpi_trace_sample_*.
 * Weights w(u) at u = (first + k) - (i + d), in float64 from the fp32 offset, rounded to fp32 once:
 *     linear  1 - |u|
 *     cubic   Keys, a = -1/2: 1.5|u|^3 - 2.5|u|^2 + 1 for |u| <= 1, -0.5|u|^3 + 2.5|u|^2 - 4|u| + 2 for 1 < |u| < 2
 *             (d = 0.5: -1/16, 9/16, 9/16, -1/16; reproduces polynomials up to degree 2 away from the edges)
 *     sinc8   sinc(u) * I0(beta * sqrt(1 - (u/4)^2)) / I0(beta), beta = 6, divided by the sum of the eight values (weights sum to 1)
 * d == 0 gives the unit weight on the trace's own node and exact zeros elsewhere for every kind, and w(-d)[k] = w(d)[K - 1 - k] exactly.
 *     dpi_trace_interp_weights: host pointers; off = [2][X][Y] (plane 0 dx, plane 1 dy) -> w = [2][K][X][Y]: axis, then tap, then trace.
 *                               DPI_E_ARG for null pointers, non-positive sizes or an unknown kind.
 *     dpi_trace_resample_fwd:   y[c][t][x][y] = sum_kx w[0][kx][x][y] * (sum_ky w[1][ky][x][y] * in[c][t][tap_x][tap_y]) in fp32, ky
 *                               ascending inside, kx ascending outside.  For Y = 1 every y tap is the one node and the inner sum is
 *                               taken as (w[1][0] + ... + w[1][K-1]) * in: K taps, not K^2 (the factor is 1 exactly for dy = 0).
 *     dpi_trace_resample_adj:   the exact transpose as a gather: node (x', y') collects from the (K + 1) x (K + 1) traces around it those
 *                               of their clamped taps that land on it.  No atomics, sums in a fixed order: deterministic, and
 *                               independent of the launch shape.
 * Device tensors [C][T][X][Y] fp32 as for dpi_trace_sample_*, w and off on the device, any 4-byte aligned pointers.  K is 2, 4 or 8;
 * another K, null pointers, in == out, a non-positive size and more than 2^60 elements return an error before any launch.  Zero
 * offsets make both the identity bit for bit.  ABI version stays: a stale library fails on the unresolved symbols. */
int dpi_trace_interp_taps(int kind);
int dpi_trace_interp_weights(const float* off, int kind, int X, int Y, float* w);
int dpi_trace_resample_fwd(const float* x, const float* w, const float* off, int K, int C, int T, int X, int Y, float* y, void* stream);
int dpi_trace_resample_adj(const float* y, const float* w, const float* off, int K, int C, int T, int X, int Y, float* x, void* stream);

/* ---------------------------------------------------------------- POCS regulariser --------------
 * Replaces utils/pocs.py:5-19 (threshold / compute_threshold: out = max(x) * scale with scale = perc/100, kept on the device;
 * y = x * ((x > th) + (x < -th)) on the real view of the spectrum) and :80-84 (y = weighted_data + weighted_mask * x).
 * The transform between them (reference: torch.rfft / irfft, main_pocs.py:156-157) is the rocFFT library call.
 * dpi_scaled_max: ws = dpi_max_ws_floats(n) floats, out = one float = fp32(max x) * scale.  The maximum is taken with fmaxf, which ignores
 * a NaN where torch.max would return it; a tensor of NaN only gives -inf * scale.  dpi_threshold reads *thresh on the device; the two
 * flags are added as floats like the reference's, so the inequalities are strict (x == th and x == -th give 0) and a negative th, for
 * which both hold on |x| < -th, gives 2 x there. */
size_t dpi_max_ws_floats(size_t n);
int dpi_scaled_max(const float* x, size_t n, float scale, float* ws, float* out, void* stream);
int dpi_threshold(const float* x, size_t n, const float* thresh, float* y, void* stream);
int dpi_pocs_project(const float* x, const float* wdata, const float* wmask, size_t n, float* y, void* stream);

/* ---------------------------------------------------------------- BatchNorm backward of a residual join in two passes (ABI 403) -----
 * Replaces autograd's chain through the tail of Block3d / ResPath3d (reference architectures/mulresunet.py:85-96, 109-112):
 *     y = BN(act_pre(t)),   t = act_a(BN_a(T_a(xa))) + act_b(BN_b(T_b(xb)))      [per channel; T_* optional value-only input chains]
 * and, on the channel range [f_lo, f_hi) of side B, one more BatchNorm BN_f whose OUTPUT (after act_f) is xb's chain input there and whose
 * input is the raw xb (Block3d: the third 3x3x3 layer's BatchNorm under bn1).  Given dy = dL/dy it writes dxa = dL/d(T_a(xa)),
 * dxb = dL/d(T_b(xb)) on the channels outside the fork range, dxf [f_hi - f_lo][V] = dL/d(xb) through BN_f on the fork range, and the
 * (dgamma, dbeta) pairs of BN, BN_a, BN_b as dgb [6][C] = rows {dgamma, dbeta, dgamma_a, dbeta_a, dgamma_b, dbeta_b} and of BN_f as dgb_f
 * [2][f_hi - f_lo] (every row a contiguous gradient vector).  The same per-element expressions as dpi_bn_bwd_reduce / _apply_fork / _apply_dual / _apply in sequence (13.6 tensor
 * passes); the nested per-channel sums are expanded so that ONE reduction pass (24 sums per channel, double precision) and ONE apply
 * pass suffice (10.5 passes, the intermediate gradient dL/dt is never stored).  io (DPI_STORE_FWD_BF16: t, xa, xb; DPI_STORE_GRAD_BF16: dy, dxa,
 * dxb, dxf): a bf16 element is widened on load, results are rounded on store; the nested sums describe the UNROUNDED intermediate gradients
 * (the rounds 1-4 sequence took them of the bf16-rounded stored ones), so with bf16 tensors the outputs equal round_bf16 of what the fp32
 * call computes on the widened operands.
 * ws: dpi_join_bwd_ws_doubles(C, V) doubles; coef: C x 8 floats of scratch (the per-channel constants the apply pass reads).
 * mi* = {mean[C], invstd[C]} as dpi_bn_finalize wrote them; post_* = slope of the activation BEHIND that BatchNorm (1 = none);
 * pre = slope of the activation in FRONT of the top BatchNorm.  t may be NULL (see dpi_chain_add_apply below).
 * What a launch writes (tests/test_gpu_join_contract.py): every element of dxa, of dxf [f_hi - f_lo][V], of coef [C][8] (the fork's pair
 * {f1, f2} = 0 off the fork range), of dgb [6][C] and of dgb_f [2][f_hi - f_lo]; dxb on the channels OUTSIDE [f_lo, f_hi) only — the fork
 * channels of dxb are not touched, their result is dxf; ws up to dpi_join_bwd_ws_doubles(C, V) = dpi_stat_blocks(C, V) * C * 24 doubles and
 * not beyond.  gamma / beta of any of the four BatchNorms may be NULL (= 1, 0).  f_lo == f_hi (0 <= f_lo <= C): no fork, and f_mi, f_gamma,
 * f_beta, dxf, dgb_f are not dereferenced (may be NULL).  Refused (DPI_E_ARG): f_lo < 0, f_hi > C, f_lo > f_hi, a non-empty fork without
 * f_mi / dxf / dgb_f, t == NULL without both forward chains, unknown io bits, C <= 0, V == 0, any other pointer NULL. */
size_t dpi_join_bwd_ws_doubles(int C, size_t V);
int dpi_join_bwd(const float* dy, const float* t, const float* mi, const float* gamma, const float* beta, float pre, int C, size_t V,
                 const float* xa, const float* mi_a, const float* gamma_a, const float* beta_a, const float* chain_a, float post_a,
                 const float* xb, const float* mi_b, const float* gamma_b, const float* beta_b, const float* chain_b, float post_b,
                 const float* fwd_chain_a, const float* fwd_chain_b,
                 int f_lo, int f_hi, const float* f_mi, const float* f_gamma, const float* f_beta, float f_post,
                 double* ws, float* coef, float* dxa, float* dxb, float* dxf, float* dgb, float* dgb_f, unsigned io, void* stream);
/* The join itself without a stored t (ABI 403): dpi_chain_add_stats(.., t = NULL, ..) takes the statistics of act(T_a(a) + T_b(b)) only,
 * dpi_chain_add_apply writes y = T_out(T_a(a) + T_b(b)) (T_out = the BatchNorm dpi_bn_finalize made of those statistics), and dpi_join_bwd
 * with t = NULL recomputes t from xa, xb through fwd_chain_a / fwd_chain_b (= chain_a / chain_b of the forward calls): the three form the
 * sum with the same expression, so all of them see the same fp32 values.  Saves one tensor write forward and two reads backward per join. */
int dpi_chain_add_apply(const float* a, const float* chain_a, const float* b, const float* chain_b, const float* chain_out, int C, size_t V,
                        float* y, unsigned io, void* stream);

/* ---------------------------------------------------------------- packed-weight scratch (ABI 401) --------------------------------
 * No reference counterpart (torch's convolutions own their workspaces the same way).  In the bf16 arithmetic modes the 3x3(x3) stride-1
 * stencil kernel reads its weights from a bf16 copy in MFMA-fragment order that a small kernel writes in front of EVERY launch, on the
 * launch's stream, into the layer's slot of a library-owned scratch: one slot per (weight pointer, shape, direction), carved from 64 MB
 * hipMalloc chunks at the layer's first launch and kept.  Consequences for a caller:
 *   - the weight tensor itself is never cached: whatever wrote it before the launch is what the launch uses;
 *   - a layer's FIRST launch must not happen inside a stream capture unless a chunk with room already exists (hipMalloc is not
 *     capturable): run one eager iteration before capturing, as for any captured workload;
 *   - the scratch grows with the number of distinct (device, weight pointer, shape) triples seen, up to 4 GB per device; beyond that
 *     launches fail with DPI_E_LAUNCH until slots are handed back.  A caller that builds a new network per patch (reference
 *     main.py:286: 343 patches per configs[2] volume) calls dpi_pack_forget() for the weight tensors of the network it drops.
 * dpi_pack_scratch_bytes(): bytes currently held, all devices.
 * dpi_pack_forget(w) (ABI 402): the slots of weight tensor `w` go to a per-device free list, from which the next layer that needs a slot of
 *     the same size takes it; returns the number of slots handed back.  The caller guarantees that no launch that reads them is in flight or
 *     sits in a captured graph that will still be replayed (deep_prior_interpolation_amd.main.Interpolator calls it when a synchronised
 *     patch's network is replaced).
 * dpi_pack_release(): synchronises every device that owns a chunk, then frees every chunk and forgets every slot; the caller guarantees
 *     that no graph captured before the call is launched after it (its kernels hold slot addresses). */
size_t dpi_pack_scratch_bytes(void);
size_t dpi_pack_slot_count(void);      /* ABI 402: live (device, weight tensor, shape) slots — what dpi_pack_forget() brings down */
int dpi_pack_forget(const void* w);
int dpi_pack_release(void);

#ifdef __cplusplus
}
#endif
#endif /* DPI_HIP_H */
