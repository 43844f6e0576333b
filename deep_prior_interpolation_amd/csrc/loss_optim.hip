// Masked L1/MSE loss with fused gradient and SNR/PCORR sums, the running average of the output (--out_ema), multi-tensor Adam, Philox input noise,
// overlap-add patch reassembly.
#include "common.h"
#include "loop_rule.h"

namespace {

constexpr int kLossBlocks = 1024;

// partial layout per block: {sum|d| or d^2, sum t^2, sum (t-o)^2, sum o, sum t, sum o^2, sum o*t, unused}
__global__ __launch_bounds__(256) void loss_partial_kernel(const float* __restrict__ out, const float* __restrict__ img,
                                                           const float* __restrict__ mask, size_t n, int kind, float gscale,
                                                           float* __restrict__ dout, double* __restrict__ ws) {
  double acc[7] = {0, 0, 0, 0, 0, 0, 0};
  const float inv_n = gscale / (float)n;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    const float o = out[i], t = img[i], m = mask[i];
    const float d = o * m - t * m;
    float g;
    if (kind == 1) { acc[0] += (double)d * d; g = 2.f * d * m * inv_n; }
    else { acc[0] += fabsf(d); g = (d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f)) * m * inv_n; }
    if (dout) dout[i] = g;
    const float e = t - o;
    acc[1] += (double)t * t; acc[2] += (double)e * e; acc[3] += o; acc[4] += t;
    acc[5] += (double)o * o; acc[6] += (double)o * t;
  }
  __shared__ double sh[4];
#pragma unroll
  for (int k = 0; k < 7; ++k) {
    const double r = block_sum(acc[k], sh);
    if (threadIdx.x == 0) ws[(size_t)blockIdx.x * 8 + k] = r;
  }
}

// the body of loss_final_kernel (one wave of 64); dpi_ema_loss finalises with it too
__device__ __forceinline__ void loss_final(const double* __restrict__ ws, int nblk, double n, double* __restrict__ res) {
  double acc[7];
#pragma unroll
  for (int k = 0; k < 7; ++k) {
    double s = 0.0;
    for (int b = threadIdx.x; b < nblk; b += 64) s += ws[(size_t)b * 8 + k];
    acc[k] = wave_sum(s);
  }
  if (threadIdx.x == 0) {
    const double loss = acc[0] / n;
    const double snr = 10.0 * log10(acc[1] / acc[2]);
    const double mo = acc[3] / n, mt = acc[4] / n;
    const double cov = acc[6] - n * mo * mt;
    const double vt = acc[1] - n * mt * mt, vo = acc[5] - n * mo * mo;
    res[0] = loss; res[1] = snr; res[2] = cov / (sqrt(vt) * sqrt(vo));
    res[3] = acc[1]; res[4] = acc[2]; res[5] = acc[3]; res[6] = acc[4]; res[7] = acc[5];
  }
}
__global__ __launch_bounds__(64) void loss_final_kernel(const double* __restrict__ ws, int nblk, double n, double* __restrict__ res) {
  loss_final(ws, nblk, n, res);
}

// ---- masked loss with held-out traces (--holdout) ------------------------------------------------------------------
// The walk, the grid and the first seven sums of loss_partial_kernel with m_tr = m * (1 - h) in place of m, so that the training part is
// bit for bit dpi_masked_loss on a materialised m_tr; the same pass adds the misfit on m_ho = m * h.  h is one float per trace
// (sel[c * S + s] of the layout [C][T][S]); its index follows i incrementally, no division inside the loop.
// partial layout per block (stride 16): {the seven sums of loss_partial_kernel, unused, sum |e| or e^2 on m_ho, sum (t m_ho)^2,
// sum (e m_ho)^2, number of held samples} with e = t - o
__global__ __launch_bounds__(256) void loss_holdout_partial_kernel(const float* __restrict__ out, const float* __restrict__ img,
                                                                   const float* __restrict__ mask, const float* __restrict__ sel,
                                                                   uint32_t TS, uint32_t S, size_t n, int kind, float gscale,
                                                                   float* __restrict__ dout, double* __restrict__ ws) {
  double acc[11] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  const float inv_n = gscale / (float)n;
  const size_t G = (size_t)gridDim.x * 256;
  const uint32_t Gc = (uint32_t)(G / TS), Gr = (uint32_t)(G % TS), Gs = (uint32_t)(G % S);
  size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  uint32_t c = (uint32_t)(i / TS), r = (uint32_t)(i % TS), s = (uint32_t)(i % S);      // i = c * TS + r, s = i mod S (n < 2^32)
  for (; i < n; i += G) {
    const float o = out[i], t = img[i], m0 = mask[i], h = sel[(size_t)c * S + s];
    const float m = m0 * (1.f - h);
    const float d = o * m - t * m;
    float g;
    if (kind == 1) { acc[0] += (double)d * d; g = 2.f * d * m * inv_n; }
    else { acc[0] += fabsf(d); g = (d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f)) * m * inv_n; }
    if (dout) dout[i] = g;
    const float e = t - o;
    acc[1] += (double)t * t; acc[2] += (double)e * e; acc[3] += o; acc[4] += t;
    acc[5] += (double)o * o; acc[6] += (double)o * t;
    const float mh = m0 * h;
    const float eh = e * mh, th = t * mh;
    acc[7] += kind == 1 ? (double)eh * eh : (double)fabsf(eh);
    acc[8] += (double)th * th; acc[9] += (double)eh * eh; acc[10] += mh != 0.f ? 1.0 : 0.0;
    c += Gc; r += Gr; s += Gs;
    if (r >= TS) { r -= TS; ++c; }
    if (s >= S) s -= S;
  }
  __shared__ double sh[4];
#pragma unroll
  for (int k = 0; k < 11; ++k) {
    const double v = block_sum(acc[k], sh);
    if (threadIdx.x == 0) ws[(size_t)blockIdx.x * 16 + (k < 7 ? k : k + 1)] = v;
  }
}

__device__ __forceinline__ void loss_holdout_final(const double* __restrict__ ws, int nblk, double n, double* __restrict__ res) {
  double acc[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (int b = threadIdx.x; b < nblk; b += 64) {          // per k the order of loss_final_kernel; the 12 loads of a row issue together
#pragma unroll
    for (int k = 0; k < 12; ++k)
      if (k != 7) acc[k] += ws[(size_t)b * 16 + k];
  }
#pragma unroll
  for (int k = 0; k < 12; ++k) acc[k] = wave_sum(acc[k]);
  if (threadIdx.x == 0) {                                  // res[0..7] exactly as loss_final_kernel
    const double loss = acc[0] / n;
    const double snr = 10.0 * log10(acc[1] / acc[2]);
    const double mo = acc[3] / n, mt = acc[4] / n;
    const double cov = acc[6] - n * mo * mt;
    const double vt = acc[1] - n * mt * mt, vo = acc[5] - n * mo * mo;
    res[0] = loss; res[1] = snr; res[2] = cov / (sqrt(vt) * sqrt(vo));
    res[3] = acc[1]; res[4] = acc[2]; res[5] = acc[3]; res[6] = acc[4]; res[7] = acc[5];
    res[8] = acc[8] / acc[11]; res[9] = 10.0 * log10(acc[9] / acc[10]); res[10] = acc[11];
  }
}
__global__ __launch_bounds__(64) void loss_holdout_final_kernel(const double* __restrict__ ws, int nblk, double n, double* __restrict__ res) {
  loss_holdout_final(ws, nblk, n, res);
}

// ---- running average of the net output (--out_ema) -------------------------------------------------------------
// avg <- out at iteration 0 (whatever avg held: it is not read), else avg + w * (out - avg) with w = fp32(1 - beta); in the same pass the
// sums of loss_partial_kernel (HO = false: grid, walk, partial layout and order of dpi_masked_loss) or of loss_holdout_partial_kernel
// (HO = true) on the value just stored, so the finalisers below give the metrics of the stored average bit for bit as the loss pass would
// on it.  No gradient: the deep-image-prior out_avg only selects and reports.  avg is read and written once, by one thread per element.
template <bool HO>
__global__ __launch_bounds__(256) void ema_loss_partial_kernel(const float* __restrict__ out, float* __restrict__ avg,
                                                               const float* __restrict__ img, const float* __restrict__ mask,
                                                               const float* __restrict__ sel, uint32_t TS, uint32_t S, size_t n, int kind,
                                                               float w, const float* __restrict__ step_lr, const int* __restrict__ active,
                                                               double* __restrict__ ws) {
  if (active && *active == 0) return;
  const bool first = (int)step_lr[0] == 0;
  double acc[11] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  const size_t G = (size_t)gridDim.x * 256;
  size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  uint32_t Gc = 0, Gr = 0, Gs = 0, c = 0, r = 0, s = 0;
  if (HO) {
    Gc = (uint32_t)(G / TS); Gr = (uint32_t)(G % TS); Gs = (uint32_t)(G % S);
    c = (uint32_t)(i / TS); r = (uint32_t)(i % TS); s = (uint32_t)(i % S);               // i = c * TS + r, s = i mod S (n < 2^32)
  }
  for (; i < n; i += G) {
    const float x = out[i];
    float o = x;
    if (!first) { const float p = avg[i]; o = p + w * (x - p); }
    avg[i] = o;
    const float t = img[i], m0 = mask[i];
    const float h = HO ? sel[(size_t)c * S + s] : 0.f;
    const float m = HO ? m0 * (1.f - h) : m0;
    const float d = o * m - t * m;
    if (kind == 1) acc[0] += (double)d * d;
    else acc[0] += fabsf(d);
    const float e = t - o;
    acc[1] += (double)t * t; acc[2] += (double)e * e; acc[3] += o; acc[4] += t;
    acc[5] += (double)o * o; acc[6] += (double)o * t;
    if (HO) {
      const float mh = m0 * h;
      const float eh = e * mh, th = t * mh;
      acc[7] += kind == 1 ? (double)eh * eh : (double)fabsf(eh);
      acc[8] += (double)th * th; acc[9] += (double)eh * eh; acc[10] += mh != 0.f ? 1.0 : 0.0;
      c += Gc; r += Gr; s += Gs;
      if (r >= TS) { r -= TS; ++c; }
      if (s >= S) s -= S;
    }
  }
  __shared__ double sh[4];
#pragma unroll
  for (int k = 0; k < (HO ? 11 : 7); ++k) {
    const double v = block_sum(acc[k], sh);
    if (threadIdx.x == 0) ws[(size_t)blockIdx.x * (HO ? 16 : 8) + (k < 7 ? k : k + 1)] = v;
  }
}

__global__ __launch_bounds__(64) void ema_final_kernel(const double* __restrict__ ws, int nblk, double n, int ho, const int* __restrict__ active,
                                                       double* __restrict__ res) {
  if (active && *active == 0) return;                      // the partials are stale: result stays
  if (ho) loss_holdout_final(ws, nblk, n, res);
  else loss_final(ws, nblk, n, res);
}

// ---- Adam -----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void adam_kernel(const dpi_adam_tensor* __restrict__ tensors, const int64_t* __restrict__ sizes,
                                                   const float* __restrict__ step_lr, double beta1d, double beta2d, double epsd,
                                                   const int* __restrict__ active) {
  if (active && *active == 0) return;
  const dpi_adam_tensor t = tensors[blockIdx.y];
  const size_t n = (size_t)sizes[blockIdx.y];
  const size_t i0 = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;
  if (i0 >= n) return;
  // scalars exactly as torch.optim.Adam derives them: in double on the "host side", then rounded to fp32
  const double step = (double)step_lr[0], lr = (double)step_lr[1];
  const float beta2 = (float)beta2d, eps = (float)epsd;
  const float omb1 = (float)(1.0 - beta1d), omb2 = (float)(1.0 - beta2d);
  const float step_size = (float)(lr / (1.0 - pow(beta1d, step)));
  const float bc2s = (float)sqrt(1.0 - pow(beta2d, step));
  for (size_t i = i0; i < n; i += (size_t)gridDim.x * 1024) {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (i + k < n) {
        const float g = t.g[i + k];
        const float m0 = t.m[i + k];
        const float m = m0 + omb1 * (g - m0);                   // exp_avg.lerp_(grad, 1-beta1)
        const float v = beta2 * t.v[i + k] + (omb2 * g) * g;    // mul_(beta2).addcmul_(g, g, value=1-beta2)
        t.m[i + k] = m;
        t.v[i + k] = v;
        const float denom = sqrtf(v) / bc2s + eps;
        t.p[i + k] -= step_size * (m / denom);
      }
  }
}

// ---- Philox4x32-10 ---------------------------------------------------------------------------------------------
__device__ __forceinline__ void philox_round(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
  const uint64_t p0 = (uint64_t)0xD2511F53u * c[0], p1 = (uint64_t)0xCD9E8D57u * c[2];
  const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0, n1 = (uint32_t)p1;
  const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1, n3 = (uint32_t)p0;
  c[0] = n0; c[1] = n1; c[2] = n2; c[3] = n3;
}
__device__ __forceinline__ void philox4(uint64_t ctr, uint64_t stream_id, uint64_t seed, float (&z)[4]) {
  uint32_t c[4] = {(uint32_t)ctr, (uint32_t)(ctr >> 32), (uint32_t)stream_id, (uint32_t)(stream_id >> 32)};
  uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    philox_round(c, k0, k1);
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  // Box-Muller on two pairs of uniforms in (0,1]
  const float u0 = ((c[0] >> 8) + 1) * (1.f / 16777216.f), u1 = (c[1] >> 8) * (1.f / 16777216.f);
  const float u2 = ((c[2] >> 8) + 1) * (1.f / 16777216.f), u3 = (c[3] >> 8) * (1.f / 16777216.f);
  const float r0 = sqrtf(-2.f * __logf(u0)), r1 = sqrtf(-2.f * __logf(u2));
  float s0, c0, s1, c1;
  __sincosf(6.283185307179586f * u1, &s0, &c0);
  __sincosf(6.283185307179586f * u3, &s1, &c1);
  z[0] = r0 * c0; z[1] = r0 * s0; z[2] = r1 * c1; z[3] = r1 * s1;
}

// zregen: instead of READING z (zin) the kernel re-draws it — z = zstd * N(0,1) of the Philox stream (zseed, zstream), exactly the values
// dpi_fill_normal(mean 0) wrote — so the fixed network input never has to be streamed from HBM again (1.07 GB per iteration at the bench patch).
struct ZRegen { int on; float zstd; uint64_t zseed, zstream; };
__global__ __launch_bounds__(256) void noise_kernel(const float* __restrict__ zin, size_t n, float mean, float std, uint64_t seed,
                                                    const uint64_t* __restrict__ step_ptr, uint64_t stream_id,
                                                    float* __restrict__ out, bool ob = false, ZRegen zr = ZRegen{0, 0.f, 0, 0}) {        // ob: `out` is stored as bf16
  typedef float nz_f32x4 __attribute__((ext_vector_type(4)));
  const uint64_t sid = step_ptr ? *step_ptr : stream_id;
  const bool vec = (n & 3) == 0;
  const bool nt = n >= ((size_t)32 << 20);          // streaming tensors beyond the Infinity Cache: non-temporal accesses (elementwise.hip)
  for (size_t q = (size_t)blockIdx.x * 256 + threadIdx.x; q * 4 < n; q += (size_t)gridDim.x * 256) {
    float z[4];
    philox4(q, sid, seed, z);
    const size_t i = q * 4;
    if (vec) {
      float4 b = make_float4(mean, mean, mean, mean);
      if (zr.on) {
        float zz[4];
        philox4(q, zr.zstream, zr.zseed, zz);
        b = make_float4(fmaf(zr.zstd, zz[0], 0.f), fmaf(zr.zstd, zz[1], 0.f), fmaf(zr.zstd, zz[2], 0.f), fmaf(zr.zstd, zz[3], 0.f));   // bit for bit what fill_normal stored
      } else if (zin) {
        if (nt) { const nz_f32x4 v = __builtin_nontemporal_load(reinterpret_cast<const nz_f32x4*>(zin + i)); b = make_float4(v[0], v[1], v[2], v[3]); }
        else b = *reinterpret_cast<const float4*>(zin + i);
      }
      b.x = fmaf(std, z[0], b.x); b.y = fmaf(std, z[1], b.y); b.z = fmaf(std, z[2], b.z); b.w = fmaf(std, z[3], b.w);
      dpi_st4(out, i, b, ob, nt);
    } else {
      float zz[4] = {0.f, 0.f, 0.f, 0.f};
      if (zr.on) philox4(q, zr.zstream, zr.zseed, zz);
      for (int k = 0; k < 4 && i + k < n; ++k) dpi_st(out, i + k, fmaf(std, z[k], zr.on ? fmaf(zr.zstd, zz[k], 0.f) : (zin ? zin[i + k] : mean)), ob);
    }
  }
}

// ---- Langevin samplers (--optimizer sgld | psgld) ---------------------------------------------------------------
// One element of the reference's SGLD.step (optimizers.py:79-106, momentum 0) / pSGLD.step (optimizers.py:144-181, not centred), with
// the rounding points of the torch CPU calls it makes: Tensor.add_(alpha, other) is ONE fused multiply-add (other * alpha + self),
// addcmul_(value, a, b) is fma(value * a, b, self), addcdiv_(value, a, b) is self + (value * a) / b, and `2*lr / G` is
// G.reciprocal() * (2*lr).  The library is built with -ffp-contract=off: only the fmaf() below fuse.  sqrt_temp = sqrt(temperature)
// multiplies last (xi itself for SGLD, whose noise add is the fused one), so temperature 1 multiplies by exactly 1.
struct LangevinScalars { int kind, has_wd; float wd, neg_lr, beta, omb, lam, two_lr, sqrt_ns, sqrt_temp; };
__device__ __forceinline__ void langevin_element(const LangevinScalars& s, float& p, float g, float& V, float xi) {
  const float d = s.has_wd ? fmaf(p, s.wd, g) : g;                 // weight decay: an add with alpha (fused)
  if (s.kind == 0) {
    p = fmaf(d, s.neg_lr, p);                                      // drift: an add with alpha = -lr (fused)
    p = fmaf(xi * s.sqrt_temp, s.sqrt_ns, p);                      // noise: an add with alpha = sqrt(noise_scale) (fused)
  } else {
    V = fmaf(s.omb * d, d, V * s.beta);                            // mul by beta, then addcmul with value 1 - beta
    const float G = sqrtf(V) + s.lam;                              // sqrt, then add Lambda
    p = p + (s.neg_lr * d) / G;                                    // drift: addcdiv with value -lr
    const float ns = sqrtf((1.f / G) * s.two_lr);                  // noise std: reciprocal of G times 2 lr, then sqrt
    p = p + (xi * ns) * s.sqrt_temp;                               // noise: product first, then a plain add
  }
}

// Grid, table and step_lr as adam_kernel.  xi == NULL: the normals come from Philox — key `seed`, stream id (0xFFFFFFFE << 32) | step,
// counter (row << 40) | q with q the group of four elements inside the tensor; else xi[row] holds them (parity mode).
// 16-byte accesses only on rows whose pointers are all 16-byte aligned (the state slices start at arbitrary element offsets).
__global__ __launch_bounds__(256) void langevin_kernel(const dpi_adam_tensor* __restrict__ tensors, const int64_t* __restrict__ sizes,
                                                       const float* __restrict__ step_lr, int kind, double wdd, double betad, double lambdad,
                                                       double noise_scaled, float sqrt_temp, uint64_t seed, const float* const* __restrict__ xi,
                                                       const int* __restrict__ active) {
  if (active && *active == 0) return;
  const dpi_adam_tensor t = tensors[blockIdx.y];
  const size_t n = (size_t)sizes[blockIdx.y];
  const size_t i0 = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;
  if (i0 >= n) return;
  // scalars as the reference's Python derives them: in double, then rounded to fp32 where torch takes them as the alpha / value of an op
  const float lr = step_lr[1];
  LangevinScalars s;
  s.kind = kind; s.has_wd = wdd != 0.0; s.wd = (float)wdd; s.neg_lr = -lr;
  s.beta = (float)betad; s.omb = (float)(1.0 - betad); s.lam = (float)lambdad; s.two_lr = 2.f * lr;
  s.sqrt_ns = (float)sqrt(noise_scaled); s.sqrt_temp = sqrt_temp;
  const uint64_t sid = (0xFFFFFFFEull << 32) | (uint64_t)(uint32_t)step_lr[0];
  const uint64_t row = (uint64_t)blockIdx.y << 40;
  const float* __restrict__ x = xi ? xi[blockIdx.y] : nullptr;
  const bool vec = dpi_vec4_base(t.p, false) && dpi_vec4_base(t.g, false) && (kind == 0 || dpi_vec4_base(t.v, false)) &&
                   (!x || dpi_vec4_base(x, false));
  for (size_t i = i0; i < n; i += (size_t)gridDim.x * 1024) {
    float z[4];
    if (!x) philox4(row | (uint64_t)(i >> 2), sid, seed, z);
    if (vec && i + 4 <= n) {
      float4 p4 = dpi_ld4(t.p, i, false, false);
      const float4 g4 = dpi_ld4(t.g, i, false, false);
      float4 v4 = kind == 1 ? dpi_ld4(t.v, i, false, false) : make_float4(0.f, 0.f, 0.f, 0.f);
      if (x) { const float4 x4 = dpi_ld4(x, i, false, false); z[0] = x4.x; z[1] = x4.y; z[2] = x4.z; z[3] = x4.w; }
      langevin_element(s, p4.x, g4.x, v4.x, z[0]);
      langevin_element(s, p4.y, g4.y, v4.y, z[1]);
      langevin_element(s, p4.z, g4.z, v4.z, z[2]);
      langevin_element(s, p4.w, g4.w, v4.w, z[3]);
      if (kind == 1) dpi_st4(t.v, i, v4, false, false);
      dpi_st4(t.p, i, p4, false, false);
    } else {
      for (int k = 0; k < 4 && i + k < n; ++k) {
        float p = t.p[i + k], V = kind == 1 ? t.v[i + k] : 0.f;
        langevin_element(s, p, t.g[i + k], V, x ? x[i + k] : z[k]);
        if (kind == 1) t.v[i + k] = V;
        t.p[i + k] = p;
      }
    }
  }
}

// ---- posterior moments: Welford running mean and sum of squared deviations of the net output over the sampled iterations -----------
// it = step_lr[0] = the 0-based iteration index when launched before the optimiser step.  Every element is owned by one thread and the
// sample number k is a pure function of `it`: no block reads what another wrote.
__global__ __launch_bounds__(256) void moments_kernel(const float* __restrict__ out, float* __restrict__ mean, float* __restrict__ m2,
                                                      size_t n, const float* __restrict__ step_lr, int burn_in, int thin,
                                                      const int* __restrict__ active) {
  if (active && *active == 0) return;
  const int it = (int)step_lr[0];
  if (it < burn_in || (it - burn_in) % thin != 0) return;
  const float k = (float)((it - burn_in) / thin + 1);
  const bool vec = (n & 3) == 0 && dpi_vec4_base(out, false) && dpi_vec4_base(mean, false) && dpi_vec4_base(m2, false);
  const bool nt = n >= ((size_t)32 << 20);          // streaming tensors beyond the Infinity Cache: non-temporal accesses (noise_kernel)
  if (vec) {
    for (size_t i = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4; i < n; i += (size_t)gridDim.x * 1024) {
      const float4 x = dpi_ld4(out, i, false, nt);
      float4 m = dpi_ld4(mean, i, false, nt), q = dpi_ld4(m2, i, false, nt);
      float d;
      d = x.x - m.x; m.x += d / k; q.x += d * (x.x - m.x);
      d = x.y - m.y; m.y += d / k; q.y += d * (x.y - m.y);
      d = x.z - m.z; m.z += d / k; q.z += d * (x.z - m.z);
      d = x.w - m.w; m.w += d / k; q.w += d * (x.w - m.w);
      dpi_st4(mean, i, m, false, nt);
      dpi_st4(m2, i, q, false, nt);
    }
  } else {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
      const float x = out[i];
      float m = mean[i];
      const float d = x - m;
      m += d / k;
      mean[i] = m;
      m2[i] += d * (x - m);
    }
  }
}

// ---- overlap-add -------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void overlap_add_kernel(const float* __restrict__ patch, int pd, int ph, int pw, int od, int oh, int ow,
                                                          float* __restrict__ acc, int D, int H, int W) {
  const size_t n = (size_t)pd * ph * pw;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    const int w = i % pw, h = (i / pw) % ph, d = i / ((size_t)pw * ph);
    acc[((size_t)(od + d) * H + oh + h) * W + ow + w] += patch[i];
  }
}

// number of windows {k*s : 0 <= k*s <= N-p} covering coordinate x
__device__ __forceinline__ int hits(int x, int N, int p, int s) {
  const int kmax = (N - p) / s;
  int lo = x - p + 1; lo = lo <= 0 ? 0 : (lo + s - 1) / s;
  int hi = x / s; if (hi > kmax) hi = kmax;
  return hi >= lo ? hi - lo + 1 : 0;
}

__global__ __launch_bounds__(256) void overlap_norm_kernel(float* __restrict__ acc, int D, int H, int W, int pd, int ph, int pw, int sd,
                                                           int sh, int sw, float gain) {
  const size_t n = (size_t)D * H * W;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    const int w = i % W, h = (i / W) % H, d = i / ((size_t)W * H);
    const int c = hits(d, D, pd, sd) * hits(h, H, ph, sh) * hits(w, W, pw, sw);
    acc[i] = acc[i] / ((float)c * gain);
  }
}

// ---- weighted overlap-add (--reassembly cover / --blend taper / the std volume of a sampler run) ------------------------------------
// Axis weight of sample i of a p-sample window: ramp[i] over the first l samples where the low side tapers, ramp[p-1-i] over the last l
// where the high side does, 1 elsewhere (l <= p/2: the two never meet).
struct BlendAxis {
  const float* ramp;
  int l, lo, hi;
};
__device__ __forceinline__ float blend_weight(const BlendAxis& a, int i, int p) {
  if (a.lo && i < a.l) return a.ramp[i];
  if (a.hi && i >= p - a.l) return a.ramp[p - 1 - i];
  return 1.f;
}

// One pass over the patch, a thread per four consecutive samples of a row (W is the contiguous axis): plane 0 += w, plane 1 += w * mean,
// plane 2 += w * std^2 (K = 3).  16-byte accesses where rows, origin and every base allow them (wave-uniform), else the same four
// samples one by one.  Every accumulator element is read and written by one thread: plain stores, launches of one stream serialise.
__global__ __launch_bounds__(256) void overlap_add_weighted_kernel(const float* __restrict__ mean, const float* __restrict__ sd, int pd, int ph,
                                                                   int pw, int od, int oh, int ow, BlendAxis ad, BlendAxis ah, BlendAxis aw,
                                                                   float* __restrict__ acc, int D, int H, int W) {
  const int qpr = (pw + 3) >> 2;                               // quads per row
  const size_t nq = (size_t)pd * ph * qpr, plane = (size_t)D * H * W;
  const bool vec = (pw & 3) == 0 && (ow & 3) == 0 && (W & 3) == 0 && dpi_vec4_base(mean, false) && dpi_vec4_base(acc, false) &&
                   (!sd || dpi_vec4_base(sd, false));
  for (size_t t = (size_t)blockIdx.x * 256 + threadIdx.x; t < nq; t += (size_t)gridDim.x * 256) {
    const int q = (int)(t % qpr);
    const size_t row = t / qpr;
    const int h = (int)(row % ph), d = (int)(row / ph), w0 = q * 4;
    const float wdh = blend_weight(ad, d, pd) * blend_weight(ah, h, ph);
    const size_t src = row * pw + w0;
    const size_t dst = ((size_t)(od + d) * H + (oh + h)) * W + ow + w0;
    if (vec) {
      const float4 m = dpi_ld4(mean, src, false, false);
      const float4 wt = make_float4(wdh * blend_weight(aw, w0, pw), wdh * blend_weight(aw, w0 + 1, pw), wdh * blend_weight(aw, w0 + 2, pw),
                                    wdh * blend_weight(aw, w0 + 3, pw));
      float4 a0 = dpi_ld4(acc, dst, false, false), a1 = dpi_ld4(acc, plane + dst, false, false);
      a0.x += wt.x; a0.y += wt.y; a0.z += wt.z; a0.w += wt.w;
      a1.x += wt.x * m.x; a1.y += wt.y * m.y; a1.z += wt.z * m.z; a1.w += wt.w * m.w;
      dpi_st4(acc, dst, a0, false, false);
      dpi_st4(acc, plane + dst, a1, false, false);
      if (sd) {
        const float4 s = dpi_ld4(sd, src, false, false);
        float4 a2 = dpi_ld4(acc, 2 * plane + dst, false, false);
        a2.x += wt.x * (s.x * s.x); a2.y += wt.y * (s.y * s.y); a2.z += wt.z * (s.z * s.z); a2.w += wt.w * (s.w * s.w);
        dpi_st4(acc, 2 * plane + dst, a2, false, false);
      }
    } else {
      for (int k = 0; k < 4 && w0 + k < pw; ++k) {
        const float wt = wdh * blend_weight(aw, w0 + k, pw);
        acc[dst + k] += wt;
        acc[plane + dst + k] += wt * mean[src + k];
        if (sd) { const float s = sd[src + k]; acc[2 * plane + dst + k] += wt * (s * s); }
      }
    }
  }
}

// mean = plane 1 / plane 0 / gain, std = sqrt(plane 2 / plane 0) / |gain|; a sample no window reached (weight 0) gives 0.
__device__ __forceinline__ void blend_finalize_element(float w, float a1, float a2, float gain, float& m, float& s) {
  m = w > 0.f ? a1 / w / gain : 0.f;
  s = w > 0.f ? sqrtf(a2 / w) / fabsf(gain) : 0.f;
}
__global__ __launch_bounds__(256) void overlap_finalize_weighted_kernel(const float* __restrict__ acc, int K, size_t n, float gain,
                                                                        float* __restrict__ out_mean, float* __restrict__ out_std) {
  const bool vec = (n & 3) == 0 && dpi_vec4_base(acc, false) && dpi_vec4_base(out_mean, false) && (!out_std || dpi_vec4_base(out_std, false));
  const bool sq = K == 3 && out_std;
  if (vec) {
    for (size_t i = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4; i < n; i += (size_t)gridDim.x * 1024) {
      const float4 w = dpi_ld4(acc, i, false, false), a1 = dpi_ld4(acc, n + i, false, false);
      const float4 a2 = sq ? dpi_ld4(acc, 2 * n + i, false, false) : make_float4(0.f, 0.f, 0.f, 0.f);
      float4 m, s;
      blend_finalize_element(w.x, a1.x, a2.x, gain, m.x, s.x);
      blend_finalize_element(w.y, a1.y, a2.y, gain, m.y, s.y);
      blend_finalize_element(w.z, a1.z, a2.z, gain, m.z, s.z);
      blend_finalize_element(w.w, a1.w, a2.w, gain, m.w, s.w);
      dpi_st4(out_mean, i, m, false, false);
      if (sq) dpi_st4(out_std, i, s, false, false);
    }
  } else {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
      float m, s;
      blend_finalize_element(acc[i], acc[n + i], sq ? acc[2 * n + i] : 0.f, gain, m, s);
      out_mean[i] = m;
      if (sq) out_std[i] = s;
    }
  }
}

// ---- device-resident loop control (one thread): history row, best-output flag, ReduceLROnPlateau, EarlyStopping ---------
// The rule, the state slots and the history rows of the three variants are those of loop_rule.h (dpi_loop_rule).
__global__ void loop_control_kernel(const double* __restrict__ metrics, double* __restrict__ state, double* __restrict__ hist, int max_iters,
                                    float* __restrict__ step_lr, int* __restrict__ active, int* __restrict__ improved, dpi_loop_rules r) {
  if (threadIdx.x == 0 && blockIdx.x == 0) dpi_loop_rule(metrics, nullptr, false, state, hist, max_iters, step_lr, active, improved, r);
}
__global__ void loop_control_holdout_kernel(const double* __restrict__ metrics, double* __restrict__ state, double* __restrict__ hist, int max_iters,
                                            float* __restrict__ step_lr, int* __restrict__ active, int* __restrict__ improved, dpi_loop_rules r) {
  if (threadIdx.x == 0 && blockIdx.x == 0) dpi_loop_rule(metrics, nullptr, true, state, hist, max_iters, step_lr, active, improved, r);
}
__global__ void loop_control_ema_kernel(const double* __restrict__ metrics, const double* __restrict__ ema, int ho, double* __restrict__ state,
                                        double* __restrict__ hist, int max_iters, float* __restrict__ step_lr, int* __restrict__ active,
                                        int* __restrict__ improved, dpi_loop_rules r) {
  if (threadIdx.x == 0 && blockIdx.x == 0) dpi_loop_rule(metrics, ema, ho != 0, state, hist, max_iters, step_lr, active, improved, r);
}

__global__ __launch_bounds__(256) void copy_if_kernel(const int* __restrict__ flag, const float* __restrict__ src, float* __restrict__ dst,
                                                      size_t n) {
  if (*flag == 0) return;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) dst[i] = src[i];
}

inline unsigned nblocks(size_t n) {
  size_t b = cdivz(n, 256);
  if (b > 4096) b = 4096;
  if (b < 1) b = 1;
  return (unsigned)b;
}

}  // namespace

extern "C" size_t dpi_loss_ws_doubles(size_t n) { (void)n; return (size_t)kLossBlocks * 8; }

extern "C" int dpi_masked_loss(const float* out, const float* img, const float* mask, size_t n, int kind, float grad_scale,
                               float* dout, double* ws, double* result, void* stream) {
  DPI_REQUIRE(out && img && mask && ws && result && n > 0, "masked_loss: bad argument");
  DPI_REQUIRE(kind == 0 || kind == 1, "masked_loss: kind must be 0 (L1) or 1 (MSE)");
  size_t nb = cdivz(n, 256 * 8);
  if (nb > kLossBlocks) nb = kLossBlocks;
  if (nb < 1) nb = 1;
  loss_partial_kernel<<<(unsigned)nb, 256, 0, (hipStream_t)stream>>>(out, img, mask, n, kind, grad_scale, dout, ws);
  if (int e = dpi_check_launch("loss_partial")) return e;
  loss_final_kernel<<<1, 64, 0, (hipStream_t)stream>>>(ws, (int)nb, (double)n, result);
  return dpi_check_launch("loss_final");
}

extern "C" int dpi_masked_loss_holdout(const float* out, const float* img, const float* mask, const float* sel, int C, int T, size_t S,
                                       int kind, float grad_scale, float* dout, double* ws, double* result, void* stream) {
  DPI_REQUIRE(out && img && mask && sel && ws && result && C > 0 && T > 0 && S > 0, "masked_loss_holdout: bad argument");
  DPI_REQUIRE(kind == 0 || kind == 1, "masked_loss_holdout: kind must be 0 (L1) or 1 (MSE)");
  const size_t n = (size_t)C * T * S;
  // the trace index is 32-bit: r + (G mod TS) < TS + G and s + (G mod S) < S + G must not wrap, G = grid * 256 <= kLossBlocks * 256
  DPI_REQUIRE(n <= (size_t)0xFFFFFFFFu - (size_t)kLossBlocks * 256, "masked_loss_holdout: %zu samples: the trace index is 32-bit", n);
  size_t nb = cdivz(n, 256 * 8);                           // the grid of dpi_masked_loss
  if (nb > kLossBlocks) nb = kLossBlocks;
  if (nb < 1) nb = 1;
  loss_holdout_partial_kernel<<<(unsigned)nb, 256, 0, (hipStream_t)stream>>>(out, img, mask, sel, (uint32_t)((size_t)T * S), (uint32_t)S, n, kind,
                                                                             grad_scale, dout, ws);
  if (int e = dpi_check_launch("loss_holdout_partial")) return e;
  loss_holdout_final_kernel<<<1, 64, 0, (hipStream_t)stream>>>(ws, (int)nb, (double)n, result);
  return dpi_check_launch("loss_holdout_final");
}

extern "C" int dpi_ema_loss(const float* out, float* avg, const float* img, const float* mask, const float* sel, int C, int T, size_t S,
                            int kind, float beta, const float* step_lr, const int* active, double* ws, double* result, void* stream) {
  DPI_REQUIRE(out && avg && img && mask && step_lr && ws && result && C > 0 && T > 0 && S > 0, "ema_loss: bad argument");
  DPI_REQUIRE(kind == 0 || kind == 1, "ema_loss: kind must be 0 (L1) or 1 (MSE)");
  DPI_REQUIRE(beta >= 0.f && beta < 1.f, "ema_loss: beta = %g must lie in [0, 1)", (double)beta);
  const size_t n = (size_t)C * T * S;
  // the trace index is 32-bit (dpi_masked_loss_holdout)
  DPI_REQUIRE(!sel || n <= (size_t)0xFFFFFFFFu - (size_t)kLossBlocks * 256, "ema_loss: %zu samples: the trace index is 32-bit", n);
  size_t nb = cdivz(n, 256 * 8);                           // the grid of dpi_masked_loss
  if (nb > kLossBlocks) nb = kLossBlocks;
  if (nb < 1) nb = 1;
  const float w = (float)(1.0 - (double)beta);
  if (sel)
    ema_loss_partial_kernel<true><<<(unsigned)nb, 256, 0, (hipStream_t)stream>>>(out, avg, img, mask, sel, (uint32_t)((size_t)T * S), (uint32_t)S, n,
                                                                               kind, w, step_lr, active, ws);
  else
    ema_loss_partial_kernel<false><<<(unsigned)nb, 256, 0, (hipStream_t)stream>>>(out, avg, img, mask, nullptr, 0u, 0u, n, kind, w, step_lr, active,
                                                                                ws);
  if (int e = dpi_check_launch("ema_loss_partial")) return e;
  ema_final_kernel<<<1, 64, 0, (hipStream_t)stream>>>(ws, (int)nb, (double)n, sel != nullptr, active, result);
  return dpi_check_launch("ema_final");
}

extern "C" int dpi_adam_multi(const dpi_adam_tensor* tensors, const int64_t* sizes, int ntensors, const float* step_lr,
                              double beta1, double beta2, double eps, const int* active, void* stream) {
  DPI_REQUIRE(tensors && sizes && step_lr && ntensors > 0 && ntensors <= 65535, "adam_multi: bad argument");
  // grid.x is sized for the largest tensor by the caller-independent cap below; blocks past a tensor's end exit.
  adam_kernel<<<dim3(256, ntensors), 256, 0, (hipStream_t)stream>>>(tensors, sizes, step_lr, beta1, beta2, eps, active);
  return dpi_check_launch("adam_multi");
}

extern "C" int dpi_langevin_multi(const dpi_adam_tensor* tensors, const int64_t* sizes, int ntensors, const float* step_lr, int kind,
                                  double weight_decay, double beta, double lambda, double noise_scale, double temperature, uint64_t seed,
                                  const float* const* xi, const int* active, void* stream) {
  DPI_REQUIRE(tensors && sizes && step_lr && ntensors > 0 && ntensors <= 65535, "langevin_multi: bad argument");
  DPI_REQUIRE(kind == 0 || kind == 1, "langevin_multi: kind must be 0 (SGLD) or 1 (pSGLD)");
  DPI_REQUIRE(temperature >= 0.0 && noise_scale >= 0.0 && lambda >= 0.0 && weight_decay >= 0.0,
              "langevin_multi: temperature, noise_scale, lambda and weight_decay must be >= 0");
  langevin_kernel<<<dim3(256, ntensors), 256, 0, (hipStream_t)stream>>>(tensors, sizes, step_lr, kind, weight_decay, beta, lambda, noise_scale,
                                                                        (float)sqrt(temperature), seed, xi, active);
  return dpi_check_launch("langevin_multi");
}

extern "C" int dpi_moments_update(const float* out, float* mean, float* m2, size_t n, const float* step_lr, int burn_in, int thin,
                                  const int* active, void* stream) {
  DPI_REQUIRE(out && mean && m2 && step_lr && n > 0, "moments_update: bad argument");
  DPI_REQUIRE(thin >= 1 && burn_in >= 0, "moments_update: burn_in must be >= 0 and thin >= 1");
  moments_kernel<<<nblocks(cdivz(n, 4)), 256, 0, (hipStream_t)stream>>>(out, mean, m2, n, step_lr, burn_in, thin, active);
  return dpi_check_launch("moments_update");
}

extern "C" int dpi_noise_add_io(const float* z, size_t n, float std, uint64_t seed, const uint64_t* step_ptr, float* out, unsigned io,
                                void* stream) {
  DPI_REQUIRE(z && out && n > 0, "noise_add: bad argument");
  DPI_REQUIRE((io & ~3u) == 0, "noise_add: unknown storage-type bits in io = %u", io);
  noise_kernel<<<nblocks(cdivz(n, 4)), 256, 0, (hipStream_t)stream>>>(z, n, 0.f, std, seed, step_ptr, 0, out, (io & DPI_STORE_FWD_BF16) != 0);
  return dpi_check_launch("noise_add");
}
extern "C" int dpi_noise_add_regen_io(size_t n, float z_std, uint64_t z_seed, uint64_t z_stream_id, float std, uint64_t seed,
                                      const uint64_t* step_ptr, float* out, unsigned io, void* stream) {
  DPI_REQUIRE(out && n > 0, "noise_add_regen: bad argument");
  DPI_REQUIRE((io & ~3u) == 0, "noise_add_regen: unknown storage-type bits in io = %u", io);
  noise_kernel<<<nblocks(cdivz(n, 4)), 256, 0, (hipStream_t)stream>>>(nullptr, n, 0.f, std, seed, step_ptr, 0, out, (io & DPI_STORE_FWD_BF16) != 0,
                                                                      ZRegen{1, z_std, z_seed, z_stream_id});
  return dpi_check_launch("noise_add_regen");
}
extern "C" int dpi_noise_add(const float* z, size_t n, float std, uint64_t seed, const uint64_t* step_ptr, float* out,
                             void* stream) {
  return dpi_noise_add_io(z, n, std, seed, step_ptr, out, 0, stream);
}

extern "C" int dpi_fill_normal(float* out, size_t n, float mean, float std, uint64_t seed, uint64_t stream_id, void* stream) {
  DPI_REQUIRE(out && n > 0, "fill_normal: bad argument");
  noise_kernel<<<nblocks(cdivz(n, 4)), 256, 0, (hipStream_t)stream>>>(nullptr, n, mean, std, seed, nullptr, stream_id, out);
  return dpi_check_launch("fill_normal");
}

extern "C" int dpi_overlap_add(const float* patch, int pd, int ph, int pw, int od, int oh, int ow, float* acc, int D, int H, int W,
                               void* stream) {
  DPI_REQUIRE(patch && acc && od >= 0 && oh >= 0 && ow >= 0 && od + pd <= D && oh + ph <= H && ow + pw <= W,
              "overlap_add: patch (%d,%d,%d)@(%d,%d,%d) outside volume (%d,%d,%d)", pd, ph, pw, od, oh, ow, D, H, W);
  overlap_add_kernel<<<nblocks((size_t)pd * ph * pw), 256, 0, (hipStream_t)stream>>>(patch, pd, ph, pw, od, oh, ow, acc, D, H, W);
  return dpi_check_launch("overlap_add");
}

extern "C" int dpi_overlap_normalize(float* acc, int D, int H, int W, int pd, int ph, int pw, int sd, int sh, int sw, float gain,
                                     void* stream) {
  DPI_REQUIRE(acc && pd <= D && ph <= H && pw <= W && sd > 0 && sh > 0 && sw > 0 && gain != 0.f, "overlap_normalize: bad argument");
  overlap_norm_kernel<<<nblocks((size_t)D * H * W), 256, 0, (hipStream_t)stream>>>(acc, D, H, W, pd, ph, pw, sd, sh, sw, gain);
  return dpi_check_launch("overlap_normalize");
}

extern "C" int dpi_overlap_add_weighted(const float* mean, const float* std, int pd, int ph, int pw, int od, int oh, int ow,
                                        const float* ramp_d, int ld, const float* ramp_h, int lh, const float* ramp_w, int lw, unsigned sides,
                                        float* acc, int K, int D, int H, int W, void* stream) {
  DPI_REQUIRE(mean && acc && pd > 0 && ph > 0 && pw > 0, "overlap_add_weighted: bad argument");
  DPI_REQUIRE(od >= 0 && oh >= 0 && ow >= 0 && od <= D - pd && oh <= H - ph && ow <= W - pw,
              "overlap_add_weighted: patch (%d,%d,%d)@(%d,%d,%d) outside volume (%d,%d,%d)", pd, ph, pw, od, oh, ow, D, H, W);
  DPI_REQUIRE(K == (std ? 3 : 2), "overlap_add_weighted: K = %d planes %s a std patch (2 = weight, mean; 3 = weight, mean, variance with one)", K,
              std ? "with" : "without");
  DPI_REQUIRE(ld >= 0 && lh >= 0 && lw >= 0 && ld <= pd / 2 && lh <= ph / 2 && lw <= pw / 2,
              "overlap_add_weighted: ramp lengths (%d,%d,%d) must lie in [0, half the patch (%d,%d,%d)]", ld, lh, lw, pd, ph, pw);
  DPI_REQUIRE((sides & ~63u) == 0, "overlap_add_weighted: sides = %u has bits beyond the six faces", sides);
  DPI_REQUIRE((ld == 0 || ramp_d) && (lh == 0 || ramp_h) && (lw == 0 || ramp_w), "overlap_add_weighted: a ramp of non-zero length needs its table");
  const BlendAxis ad = {ramp_d, ld, ld > 0 && (sides & 1u), ld > 0 && (sides & 2u)};
  const BlendAxis ah = {ramp_h, lh, lh > 0 && (sides & 4u), lh > 0 && (sides & 8u)};
  const BlendAxis aw = {ramp_w, lw, lw > 0 && (sides & 16u), lw > 0 && (sides & 32u)};
  overlap_add_weighted_kernel<<<nblocks((size_t)pd * ph * cdivz(pw, 4)), 256, 0, (hipStream_t)stream>>>(mean, std, pd, ph, pw, od, oh, ow, ad, ah, aw,
                                                                                                      acc, D, H, W);
  return dpi_check_launch("overlap_add_weighted");
}

extern "C" int dpi_overlap_finalize_weighted(const float* acc, int K, int D, int H, int W, float gain, float* out_mean, float* out_std,
                                             void* stream) {
  DPI_REQUIRE(acc && out_mean && D > 0 && H > 0 && W > 0, "overlap_finalize_weighted: bad argument");
  DPI_REQUIRE(K == 2 || K == 3, "overlap_finalize_weighted: K = %d planes (2 = weight, mean; 3 = weight, mean, variance)", K);
  DPI_REQUIRE(!out_std || K == 3, "overlap_finalize_weighted: a std volume needs the variance plane (K = 3), got K = %d", K);
  DPI_REQUIRE(gain != 0.f && gain == gain, "overlap_finalize_weighted: gain must be a non-zero number");
  const size_t n = (size_t)D * H * W;
  overlap_finalize_weighted_kernel<<<nblocks(cdivz(n, 4)), 256, 0, (hipStream_t)stream>>>(acc, K, n, gain, out_mean, out_std);
  return dpi_check_launch("overlap_finalize_weighted");
}

extern "C" int dpi_loop_control(const double* metrics, double* state, double* hist, int max_iters, float* step_lr, int* active,
                                int* improved, int use_plateau, double factor, double threshold, int patience, double min_lr,
                                double lr_eps, int es_patience, double es_min_delta, void* stream) {
  DPI_REQUIRE(metrics && state && hist && step_lr && active && improved && max_iters > 0, "loop_control: bad argument");
  loop_control_kernel<<<1, 64, 0, (hipStream_t)stream>>>(metrics, state, hist, max_iters, step_lr, active, improved, {use_plateau, factor,
                                                        threshold, patience, min_lr, lr_eps, es_patience, es_min_delta});
  return dpi_check_launch("loop_control");
}

extern "C" int dpi_loop_control_holdout(const double* metrics, double* state, double* hist, int max_iters, float* step_lr, int* active,
                                        int* improved, int use_plateau, double factor, double threshold, int patience, double min_lr,
                                        double lr_eps, int es_patience, double es_min_delta, void* stream) {
  DPI_REQUIRE(metrics && state && hist && step_lr && active && improved && max_iters > 0, "loop_control_holdout: bad argument");
  loop_control_holdout_kernel<<<1, 64, 0, (hipStream_t)stream>>>(metrics, state, hist, max_iters, step_lr, active, improved, {use_plateau,
                                                                factor, threshold, patience, min_lr, lr_eps, es_patience, es_min_delta});
  return dpi_check_launch("loop_control_holdout");
}

extern "C" int dpi_loop_control_ema(const double* metrics, const double* ema_metrics, int has_holdout, double* state, double* hist,
                                    int max_iters, float* step_lr, int* active, int* improved, int use_plateau, double factor,
                                    double threshold, int patience, double min_lr, double lr_eps, int es_patience, double es_min_delta,
                                    void* stream) {
  DPI_REQUIRE(metrics && ema_metrics && state && hist && step_lr && active && improved && max_iters > 0, "loop_control_ema: bad argument");
  loop_control_ema_kernel<<<1, 64, 0, (hipStream_t)stream>>>(metrics, ema_metrics, has_holdout != 0, state, hist, max_iters, step_lr, active,
                                                            improved, {use_plateau, factor, threshold, patience, min_lr, lr_eps, es_patience,
                                                            es_min_delta});
  return dpi_check_launch("loop_control_ema");
}

extern "C" int dpi_copy_if(const int* flag, const float* src, float* dst, size_t n, void* stream) {
  DPI_REQUIRE(flag && src && dst && n > 0, "copy_if: bad argument");
  copy_if_kernel<<<nblocks(n), 256, 0, (hipStream_t)stream>>>(flag, src, dst, n);
  return dpi_check_launch("copy_if");
}
