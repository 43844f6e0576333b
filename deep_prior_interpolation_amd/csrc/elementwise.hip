// HBM-bound elementwise / reduction kernels of the hot path: BatchNorm statistics + finalize + apply,
// BatchNorm backward, LeakyReLU backward, residual add, x2 up-sampling (nearest / linear, with the
// Concat centre-crop folded in), crop copy.  All reductions are two-stage in double precision with a
// fixed summation order (deterministic run to run).
#include "common.h"
#include <stdlib.h>

namespace {

constexpr int kStatSpan = 16384;   // voxels per block and channel in the streaming reductions
constexpr int kMaxStatBlocks = 2048;

__host__ __device__ inline size_t stat_span(size_t V, int nblk) {
  size_t s = (V + nblk - 1) / nblk;
  return (s + 3) & ~(size_t)3;   // keep float4 alignment of every span start
}

// Streaming accesses.  Tensors far larger than the 256 MB Infinity Cache are read once and written once per pass; marking those
// accesses non-temporal (`global_load/store_dwordx4 ... nt`) measured +8-9 % on a plain streaming pass (tools/ubench/stream_nt:
// 5.5-6.1 -> 6.1-6.6 TB/s read + write).  Smaller tensors (the coarse levels) keep the default policy: the next kernel may still find
// them in cache.  `nt` is wave-uniform (decided from the tensor size at the top of a kernel).
typedef float ew_f32x4 __attribute__((ext_vector_type(4)));
constexpr size_t kNtMinFloats = (size_t)32 << 20;          // 128 MB
__device__ __forceinline__ float4 ld4(const float* p, bool nt) {
  if (nt) { const ew_f32x4 v = __builtin_nontemporal_load(reinterpret_cast<const ew_f32x4*>(p)); return make_float4(v[0], v[1], v[2], v[3]); }
  return *reinterpret_cast<const float4*>(p);
}
__device__ __forceinline__ void st4(float* p, float4 v, bool nt) {
  if (nt) __builtin_nontemporal_store((ew_f32x4){v.x, v.y, v.z, v.w}, reinterpret_cast<ew_f32x4*>(p));
  else *reinterpret_cast<float4*>(p) = v;
}

// ---- per-channel {sum, sum^2} of T(x) ------------------------------------------------------------------
// (storage types are TEMPLATE parameters in this file: with a run-time flag every load sits in its own `if (bf16)` and, because the bf16
//  side widens what it loads, waits for its data inside that branch — the two or three streams of a pass then load one after the other)
template <bool xb = false>
__global__ __launch_bounds__(256) void channel_stats_kernel(const float* __restrict__ x, const float* __restrict__ chain,
                                                            int C, size_t V, int nblk, double* __restrict__ partials) {
  const bool nt = (size_t)gridDim.y * V >= kNtMinFloats;
  const int c = blockIdx.y, b = blockIdx.x;
  const size_t span = stat_span(V, nblk);
  const size_t beg = (size_t)b * span, end = beg + span < V ? beg + span : V;
  const float* __restrict__ xc = dpi_at(x, (size_t)c * V, xb);
  const Chain t = load_chain(chain, c);
  double s = 0.0, q = 0.0;
  const bool vec = (V & 3) == 0;
  for (size_t i = beg + (size_t)threadIdx.x * 4; i < end; i += 1024) {
    float v[4];
    if (vec) {
      const float4 f = dpi_ld4(xc, i, xb, nt);
      v[0] = f.x; v[1] = f.y; v[2] = f.z; v[3] = f.w;
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) v[k] = i + k < end ? dpi_ld(xc, i + k, xb) : 0.f;
    }
    float ls = 0.f;
    double lq = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (i + k < end) {
        const float y = apply_chain(t, v[k]);
        ls += y;
        lq += (double)y * y;
      }
    s += ls; q += lq;
  }
  __shared__ double sh[8];
  const double S = block_sum(s, sh);
  const double Q = block_sum(q, sh + 4);
  if (threadIdx.x == 0) {
    partials[((size_t)b * C + c) * 2 + 0] = S;
    partials[((size_t)b * C + c) * 2 + 1] = Q;
  }
}

// ---- finalize: one workgroup per channel, fixed-order reduction of the block partials ------------------------
// (a convolution at 256x128x128 hands over 8192 tile partials per channel: with one wave per channel the 128 dependent
// iterations of the loop below were 10 us of pure latency, 70 times per iteration)
__global__ __launch_bounds__(256) void bn_finalize_kernel(const double* __restrict__ partials, int nblk, int C, double count,
                                                         const float* __restrict__ gamma, const float* __restrict__ beta,
                                                         float eps, float momentum, float slope, int act_first,
                                                         const float* __restrict__ in_chain, float* running_mean, float* running_var, int64_t* nbt,
                                                         float* __restrict__ mean_invstd, float* __restrict__ chain_out) {
  const int c = blockIdx.x, lane = threadIdx.x;
  double s = 0.0, q = 0.0;
  {
    double s1 = 0.0, q1 = 0.0;
    int b = lane;
    for (; b + 256 < nblk; b += 512) {                         // two independent loads in flight per thread
      const double2 u = *reinterpret_cast<const double2*>(partials + ((size_t)b * C + c) * 2);
      const double2 v = *reinterpret_cast<const double2*>(partials + ((size_t)(b + 256) * C + c) * 2);
      s += u.x; q += u.y; s1 += v.x; q1 += v.y;
    }
    if (b < nblk) {
      const double2 u = *reinterpret_cast<const double2*>(partials + ((size_t)b * C + c) * 2);
      s += u.x; q += u.y;
    }
    s += s1; q += q1;
  }
  __shared__ double sh[8];
  s = block_sum(s, sh);
  q = block_sum(q, sh + 4);
  if (lane == 0) {
    const double mean = s / count;
    double var = q / count - mean * mean;
    if (var < 0.0) var = 0.0;
    const float invstd = (float)(1.0 / sqrt(var + (double)eps));
    const float meanf = (float)mean;
    if (mean_invstd) { mean_invstd[c] = meanf; mean_invstd[C + c] = invstd; }
    if (running_mean) running_mean[c] = (1.f - momentum) * running_mean[c] + momentum * meanf;
    if (running_var) {
      const double unb = count > 1.0 ? var * (count / (count - 1.0)) : var;
      running_var[c] = (1.f - momentum) * running_var[c] + momentum * (float)unb;
    }
    if (nbt && c == 0) *nbt += 1;
    if (chain_out) {
      const float g = gamma ? gamma[c] : 1.f, bt = beta ? beta[c] : 0.f;
      const float a = g * invstd;
      float* o = chain_out + (size_t)c * DPI_CHAIN_STRIDE;
      if (in_chain) {   // BN of T_in(x) (no activation after): compose the affine part into T_in's output stage
        const float* ic = in_chain + (size_t)c * DPI_CHAIN_STRIDE;
        o[0] = ic[0]; o[1] = ic[1]; o[2] = ic[2]; o[3] = a * ic[3]; o[4] = fmaf(a, ic[4], bt - meanf * a);
      } else if (act_first) { o[0] = 1.f; o[1] = 0.f; o[2] = slope; o[3] = a; o[4] = bt - meanf * a; }   // BN(act(x))
      else { o[0] = a; o[1] = bt - meanf * a; o[2] = slope; o[3] = 1.f; o[4] = 0.f; }           // act(BN(x))
    }
  }
}

template <bool xb = false, bool yb = false>
__global__ __launch_bounds__(256) void chain_apply_kernel(const float* __restrict__ x, const float* __restrict__ chain, size_t V,
                                                          float* __restrict__ y) {
  const bool nt = (size_t)gridDim.y * V >= kNtMinFloats;
  const int c = blockIdx.y;
  const Chain t = load_chain(chain, c);
  const float* __restrict__ xc = dpi_at(x, (size_t)c * V, xb);
  float* __restrict__ yc = dpi_at(y, (size_t)c * V, yb);
  const bool vec = (V & 3) == 0;
  for (size_t i = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4; i < V; i += (size_t)gridDim.x * 1024) {
    if (vec) {
      float4 f = dpi_ld4(xc, i, xb, nt);
      f.x = apply_chain(t, f.x); f.y = apply_chain(t, f.y); f.z = apply_chain(t, f.z); f.w = apply_chain(t, f.w);
      dpi_st4(yc, i, f, yb, nt);
    } else {
      for (int k = 0; k < 4 && i + k < V; ++k) dpi_st(yc, i + k, apply_chain(t, dpi_ld(xc, i + k, xb)), yb);
    }
  }
}

// ---- BatchNorm backward ------------------------------------------------------------------------------------
// Generalised to the two fused forms the networks use (slopes of 1 disable them):
//   pre_slope  (act -> BN):  u = act_pre(x) is what was normalised;  dx = du * act_pre'(x)
//   post_slope (BN -> act):  the incoming gradient is w.r.t. act_post(BN(x));  g = dy * act_post'(gamma*xhat + beta)
// so neither the activation output nor an intermediate gradient tensor is ever materialised.
struct BnBwd {
  float mean, invstd, a, pb, pre, post;
  bool chained;
  Chain in;   // value-only input transform: the BN input is u = T_in(x) and dx is the gradient w.r.t. u
};
__device__ __forceinline__ BnBwd bn_bwd_consts(const float* __restrict__ mean_invstd, const float* __restrict__ gamma,
                                               const float* __restrict__ beta, const float* __restrict__ in_chain, float pre,
                                               float post, int C, int c) {
  BnBwd k;
  k.chained = in_chain != nullptr;
  k.in = load_chain(in_chain, c);
  k.mean = mean_invstd[c]; k.invstd = mean_invstd[C + c];
  k.a = (gamma ? gamma[c] : 1.f) * k.invstd;
  k.pb = (beta ? beta[c] : 0.f) - k.mean * k.a;   // same expression as bn_finalize's chain shift: identical activation mask
  k.pre = pre; k.post = post;
  return k;
}
// returns xhat and the gradient w.r.t. the BN output proper
__device__ __forceinline__ void bn_bwd_elem(const BnBwd& k, float x, float dy, float& xhat, float& g) {
  if (k.chained) x = apply_chain(k.in, x);
  const float u = x > 0.f ? x : x * k.pre;
  xhat = (u - k.mean) * k.invstd;
  const float yv = fmaf(k.a, u, k.pb);
  g = (k.post == 1.f || yv > 0.f) ? dy : dy * k.post;
}

template <bool fb = false, bool gb = false>
__global__ __launch_bounds__(256) void bn_bwd_reduce_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                            const float* __restrict__ mean_invstd, const float* __restrict__ gamma,
                                                            const float* __restrict__ beta, const float* __restrict__ in_chain,
                                                            float pre, float post, int C, size_t V, int nblk,
                                                            double* __restrict__ partials) {
  // fb: the forward tensor x is bf16; gb: the gradient tensor dy is bf16 (all BatchNorm-backward kernels below alike)
  const bool nt = (size_t)gridDim.y * V >= kNtMinFloats;
  const int c = blockIdx.y, b = blockIdx.x;
  const size_t span = stat_span(V, nblk);
  const size_t beg = (size_t)b * span, end = beg + span < V ? beg + span : V;
  const BnBwd k = bn_bwd_consts(mean_invstd, gamma, beta, in_chain, pre, post, C, c);
  const float* __restrict__ xc = dpi_at(x, (size_t)c * V, fb);
  const float* __restrict__ gc = dpi_at(dy, (size_t)c * V, gb);
  double s = 0.0, q = 0.0;
  const bool vec = (V & 3) == 0;
  for (size_t i = beg + (size_t)threadIdx.x * 4; i < end; i += 1024) {
    float xv[4], gv[4];
    if (vec) {
      const float4 f = dpi_ld4(xc, i, fb, nt);
      const float4 g = dpi_ld4(gc, i, gb, nt);
      xv[0] = f.x; xv[1] = f.y; xv[2] = f.z; xv[3] = f.w;
      gv[0] = g.x; gv[1] = g.y; gv[2] = g.z; gv[3] = g.w;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) { xv[j] = i + j < end ? dpi_ld(xc, i + j, fb) : 0.f; gv[j] = i + j < end ? dpi_ld(gc, i + j, gb) : 0.f; }
    }
    float ls = 0.f, lq = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (i + j < end) {
        float xh, g;
        bn_bwd_elem(k, xv[j], gv[j], xh, g);
        ls += g; lq = fmaf(g, xh, lq);
      }
    s += ls; q += lq;
  }
  __shared__ double sh[8];
  const double S = block_sum(s, sh);
  const double Q = block_sum(q, sh + 4);
  if (threadIdx.x == 0) {
    partials[((size_t)b * C + c) * 2 + 0] = S;
    partials[((size_t)b * C + c) * 2 + 1] = Q;
  }
}

template <bool fb = false, bool gb = false>
__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                           const float* __restrict__ mean_invstd, const float* __restrict__ gamma,
                                                           const float* __restrict__ beta, const float* __restrict__ in_chain,
                                                           float pre, float post, const double* __restrict__ partials, int nblk, int C, size_t V,
                                                           float* __restrict__ dx, float* __restrict__ dgamma,
                                                           float* __restrict__ dbeta) {
  const bool nt = (size_t)gridDim.y * V >= kNtMinFloats;
  const int c = blockIdx.y;
  __shared__ double tot[2];
  if (threadIdx.x < 64) {
    double s = 0.0, q = 0.0;
    for (int b = threadIdx.x; b < nblk; b += 64) {
      s += partials[((size_t)b * C + c) * 2 + 0];
      q += partials[((size_t)b * C + c) * 2 + 1];
    }
    s = wave_sum(s);
    q = wave_sum(q);
    if (threadIdx.x == 0) { tot[0] = s; tot[1] = q; }
  }
  __syncthreads();
  const BnBwd k = bn_bwd_consts(mean_invstd, gamma, beta, in_chain, pre, post, C, c);
  const float k1 = (float)(tot[0] / (double)V), k2 = (float)(tot[1] / (double)V);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    if (dgamma) dgamma[c] = (float)tot[1];
    if (dbeta) dbeta[c] = (float)tot[0];
  }
  const float* __restrict__ xc = dpi_at(x, (size_t)c * V, fb);
  const float* __restrict__ gc = dpi_at(dy, (size_t)c * V, gb);
  float* __restrict__ oc = dpi_at(dx, (size_t)c * V, gb);
  const bool vec = (V & 3) == 0;
  auto one = [&](float xv, float gv) {
    float xh, g;
    bn_bwd_elem(k, xv, gv, xh, g);
    const float du = k.a * (g - k1 - xh * k2);
    return (k.pre == 1.f || xv > 0.f) ? du : du * k.pre;
  };
  for (size_t i = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4; i < V; i += (size_t)gridDim.x * 1024) {
    if (vec) {
      const float4 f = dpi_ld4(xc, i, fb, nt);
      const float4 g = dpi_ld4(gc, i, gb, nt);
      dpi_st4(oc, i, make_float4(one(f.x, g.x), one(f.y, g.y), one(f.z, g.z), one(f.w, g.w)), gb, nt);
    } else {
      for (int j = 0; j < 4 && i + j < V; ++j) dpi_st(oc, i + j, one(dpi_ld(xc, i + j, fb), dpi_ld(gc, i + j, gb)), gb);
    }
  }
}

// ---- t = T_a(a) + T_b(b), and {sum, sum^2} of act(t): the residual join of Block3d / ResPath3d in one pass -----------
template <bool fb = false>
__global__ __launch_bounds__(256) void chain_add_stats_kernel(const float* __restrict__ a, const float* __restrict__ chain_a,
                                                              const float* __restrict__ b, const float* __restrict__ chain_b, int C,
                                                              size_t V, int nblk, float slope, float* __restrict__ t,
                                                              double* __restrict__ partials) {
  const bool nt = (size_t)gridDim.y * V >= kNtMinFloats;
  const int c = blockIdx.y, blk = blockIdx.x;
  const size_t span = stat_span(V, nblk);
  const size_t beg = (size_t)blk * span, end = beg + span < V ? beg + span : V;
  const Chain ta = load_chain(chain_a, c), tb = load_chain(chain_b, c);
  const float* __restrict__ ac = dpi_at(a, (size_t)c * V, fb);
  const float* __restrict__ bc = dpi_at(b, (size_t)c * V, fb);
  float* __restrict__ tc = dpi_at(t, (size_t)c * V, fb);
  double s = 0.0, q = 0.0;
  const bool vec = (V & 3) == 0;
  for (size_t i = beg + (size_t)threadIdx.x * 4; i < end; i += 1024) {
    float av[4], bv[4], tv[4];
    if (vec) {
      const float4 f = dpi_ld4(ac, i, fb, nt);
      const float4 g = dpi_ld4(bc, i, fb, nt);
      av[0] = f.x; av[1] = f.y; av[2] = f.z; av[3] = f.w;
      bv[0] = g.x; bv[1] = g.y; bv[2] = g.z; bv[3] = g.w;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) { av[j] = i + j < end ? dpi_ld(ac, i + j, fb) : 0.f; bv[j] = i + j < end ? dpi_ld(bc, i + j, fb) : 0.f; }
    }
    float ls = 0.f;
    double lq = 0.0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      tv[j] = dpi_stored(apply_chain(ta, av[j]) + apply_chain(tb, bv[j]), fb && t != nullptr);    // the statistics describe the stored t (not stored: the fp32 sum its consumers re-form)
      if (i + j < end) {
        const float y = tv[j] > 0.f ? tv[j] : tv[j] * slope;
        ls += y;
        lq += (double)y * y;
      }
    }
    if (t != nullptr) {          // (NULL: statistics only — the consumers recompute t from a and b, round 5)
      if (vec) dpi_st4(tc, i, make_float4(tv[0], tv[1], tv[2], tv[3]), fb, nt);
      else
        for (int j = 0; j < 4 && i + j < end; ++j) dpi_st(tc, i + j, tv[j], fb);
    }
    s += ls; q += lq;
  }
  __shared__ double sh[8];
  const double S = block_sum(s, sh);
  const double Q = block_sum(q, sh + 4);
  if (threadIdx.x == 0) {
    partials[((size_t)blk * C + c) * 2 + 0] = S;
    partials[((size_t)blk * C + c) * 2 + 1] = Q;
  }
}

// ---- BN backward phase 2 fused with phase 1 of the BatchNorms the result feeds ------------------------------------------
// dx of this BatchNorm is the incoming gradient of up to two other BatchNorm backward passes (the residual join of
// Block3d / ResPath3d: d t -> shortcut-BN and bn1 / the two conv-BNs).  Their {sum g, sum g*xhat} partials are taken
// while dx is still in registers, which removes their separate reduction passes (2 reads each).
struct BnFork {
  const float* x;            // that BatchNorm's input (raw), NULL = unused
  const float* mean_invstd;
  const float* gamma;
  const float* beta;
  const float* in_chain;
  float post;
  double* partials;          // [nblk][C][2]
};
template <bool tb = false, bool gb = false>       // tb: forward tensors (x, fa.x, fb.x) bf16; gb: dy, dx bf16
__global__ __launch_bounds__(256) void bn_bwd_apply_fork_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                                const float* __restrict__ mean_invstd, const float* __restrict__ gamma,
                                                                const float* __restrict__ beta, const float* __restrict__ in_chain,
                                                                float pre, float post, const double* __restrict__ partials, int nblk_in,
                                                                int C, size_t V, int nblk, float* __restrict__ dx,
                                                                float* __restrict__ dgamma, float* __restrict__ dbeta, BnFork fa, BnFork fb) {
  const bool nt = (size_t)gridDim.y * V >= kNtMinFloats;
  const int c = blockIdx.y, b = blockIdx.x;
  __shared__ double tot[2];
  if (threadIdx.x < 64) {
    double s = 0.0, q = 0.0;
    for (int i = threadIdx.x; i < nblk_in; i += 64) {
      s += partials[((size_t)i * C + c) * 2 + 0];
      q += partials[((size_t)i * C + c) * 2 + 1];
    }
    s = wave_sum(s);
    q = wave_sum(q);
    if (threadIdx.x == 0) { tot[0] = s; tot[1] = q; }
  }
  __syncthreads();
  const BnBwd k = bn_bwd_consts(mean_invstd, gamma, beta, in_chain, pre, post, C, c);
  const float k1 = (float)(tot[0] / (double)V), k2 = (float)(tot[1] / (double)V);
  if (b == 0 && threadIdx.x == 0) {
    if (dgamma) dgamma[c] = (float)tot[1];
    if (dbeta) dbeta[c] = (float)tot[0];
  }
  const BnBwd ka = fa.x ? bn_bwd_consts(fa.mean_invstd, fa.gamma, fa.beta, fa.in_chain, 1.f, fa.post, C, c) : k;
  const BnBwd kb = fb.x ? bn_bwd_consts(fb.mean_invstd, fb.gamma, fb.beta, fb.in_chain, 1.f, fb.post, C, c) : k;
  const size_t span = stat_span(V, nblk);
  const size_t beg = (size_t)b * span, end = beg + span < V ? beg + span : V;
  const float* __restrict__ xc = dpi_at(x, (size_t)c * V, tb);
  const float* __restrict__ gc = dpi_at(dy, (size_t)c * V, gb);
  const float* __restrict__ xa = fa.x ? dpi_at(fa.x, (size_t)c * V, tb) : xc;
  const float* __restrict__ xb = fb.x ? dpi_at(fb.x, (size_t)c * V, tb) : xc;
  float* __restrict__ oc = dpi_at(dx, (size_t)c * V, gb);
  double sa = 0.0, qa = 0.0, sb = 0.0, qb = 0.0;
  const bool vec = (V & 3) == 0;
  for (size_t i = beg + (size_t)threadIdx.x * 4; i < end; i += 1024) {
    float xv[4], gv[4], av[4], bv[4], o[4];
    if (vec) {
      const float4 f = dpi_ld4(xc, i, tb, nt);
      const float4 g = dpi_ld4(gc, i, gb, nt);
      xv[0] = f.x; xv[1] = f.y; xv[2] = f.z; xv[3] = f.w;
      gv[0] = g.x; gv[1] = g.y; gv[2] = g.z; gv[3] = g.w;
      if (fa.x) { const float4 t = dpi_ld4(xa, i, tb, nt); av[0] = t.x; av[1] = t.y; av[2] = t.z; av[3] = t.w; }
      if (fb.x) { const float4 t = dpi_ld4(xb, i, tb, nt); bv[0] = t.x; bv[1] = t.y; bv[2] = t.z; bv[3] = t.w; }
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const bool in = i + j < end;
        xv[j] = in ? dpi_ld(xc, i + j, tb) : 0.f; gv[j] = in ? dpi_ld(gc, i + j, gb) : 0.f;
        av[j] = (in && fa.x) ? dpi_ld(xa, i + j, tb) : 0.f; bv[j] = (in && fb.x) ? dpi_ld(xb, i + j, tb) : 0.f;
      }
    }
    float lsa = 0.f, lqa = 0.f, lsb = 0.f, lqb = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float xh, g;
      bn_bwd_elem(k, xv[j], gv[j], xh, g);
      const float du = k.a * (g - k1 - xh * k2);
      o[j] = dpi_stored((k.pre == 1.f || xv[j] > 0.f) ? du : du * k.pre, gb);     // the follow-up partials describe the stored dx
      if (i + j < end) {
        if (fa.x) { float h, ga_; bn_bwd_elem(ka, av[j], o[j], h, ga_); lsa += ga_; lqa = fmaf(ga_, h, lqa); }
        if (fb.x) { float h, gb_; bn_bwd_elem(kb, bv[j], o[j], h, gb_); lsb += gb_; lqb = fmaf(gb_, h, lqb); }
      }
    }
    if (vec) dpi_st4(oc, i, make_float4(o[0], o[1], o[2], o[3]), gb, nt);
    else
      for (int j = 0; j < 4 && i + j < end; ++j) dpi_st(oc, i + j, o[j], gb);
    sa += lsa; qa += lqa; sb += lsb; qb += lqb;
  }
  __shared__ double sh[16];
  const double SA = block_sum(sa, sh), QA = block_sum(qa, sh + 4), SB = block_sum(sb, sh + 8), QB = block_sum(qb, sh + 12);
  if (threadIdx.x == 0) {
    if (fa.x) { fa.partials[((size_t)b * C + c) * 2 + 0] = SA; fa.partials[((size_t)b * C + c) * 2 + 1] = QA; }
    if (fb.x) { fb.partials[((size_t)b * C + c) * 2 + 0] = SB; fb.partials[((size_t)b * C + c) * 2 + 1] = QB; }
  }
}

// ---- two BatchNorm backward phase-2 passes that share their incoming gradient, in one pass ------------------------------
// (the two branches of a residual join: shortcut-BN and bn1 of Block3d, the two conv-BNs of ResPath3d).  Optionally the
// phase-1 partials of ONE more BatchNorm fed by dxb on the channel range [f_lo, f_hi) are taken on the fly (the third
// conv-BN of Block3d: its input gradient is exactly bn1's dx on those channels, nothing accumulates into it later).
struct BnSide {
  const float* x;
  const float* mean_invstd;
  const float* gamma;
  const float* beta;
  const float* in_chain;
  float post;
  const double* partials;    // phase-1 partials of this BatchNorm, [nblk_in][C][2]
  float* dx;
  float* dgamma;
  float* dbeta;
};
template <bool tb = false, bool gb = false>
__global__ __launch_bounds__(256) void bn_bwd_apply_dual_kernel(const float* __restrict__ dy, BnSide A, BnSide B, int nblk_in, int C, size_t V,
                                                                int nblk, int f_lo, int f_hi, const float* __restrict__ f_mi,
                                                                const float* __restrict__ f_gamma, const float* __restrict__ f_beta,
                                                                float f_post, double* __restrict__ f_partials) {
  const bool nt = (size_t)gridDim.y * V >= kNtMinFloats;
  const int c = blockIdx.y, b = blockIdx.x;
  __shared__ double tot[4];
  if (threadIdx.x < 64) {
    double sa = 0.0, qa = 0.0, sb = 0.0, qb = 0.0;
    for (int i = threadIdx.x; i < nblk_in; i += 64) {
      sa += A.partials[((size_t)i * C + c) * 2 + 0]; qa += A.partials[((size_t)i * C + c) * 2 + 1];
      sb += B.partials[((size_t)i * C + c) * 2 + 0]; qb += B.partials[((size_t)i * C + c) * 2 + 1];
    }
    sa = wave_sum(sa); qa = wave_sum(qa); sb = wave_sum(sb); qb = wave_sum(qb);
    if (threadIdx.x == 0) { tot[0] = sa; tot[1] = qa; tot[2] = sb; tot[3] = qb; }
  }
  __syncthreads();
  const BnBwd ka = bn_bwd_consts(A.mean_invstd, A.gamma, A.beta, A.in_chain, 1.f, A.post, C, c);
  const BnBwd kb = bn_bwd_consts(B.mean_invstd, B.gamma, B.beta, B.in_chain, 1.f, B.post, C, c);
  const float a1 = (float)(tot[0] / (double)V), a2 = (float)(tot[1] / (double)V);
  const float b1 = (float)(tot[2] / (double)V), b2 = (float)(tot[3] / (double)V);
  if (b == 0 && threadIdx.x == 0) {
    if (A.dgamma) A.dgamma[c] = (float)tot[1];
    if (A.dbeta) A.dbeta[c] = (float)tot[0];
    if (B.dgamma) B.dgamma[c] = (float)tot[3];
    if (B.dbeta) B.dbeta[c] = (float)tot[2];
  }
  const bool forked = f_partials && c >= f_lo && c < f_hi;
  const int fc = forked ? c - f_lo : 0, fC = f_hi - f_lo;
  const BnBwd kf = forked ? bn_bwd_consts(f_mi, f_gamma, f_beta, nullptr, 1.f, f_post, fC, fc) : ka;
  const size_t span = stat_span(V, nblk);
  const size_t beg = (size_t)b * span, end = beg + span < V ? beg + span : V;
  const float* __restrict__ gc = dpi_at(dy, (size_t)c * V, gb);
  const float* __restrict__ xa = dpi_at(A.x, (size_t)c * V, tb);
  const float* __restrict__ xb = dpi_at(B.x, (size_t)c * V, tb);
  float* __restrict__ oa = dpi_at(A.dx, (size_t)c * V, gb);
  float* __restrict__ ob = dpi_at(B.dx, (size_t)c * V, gb);
  double sf = 0.0, qf = 0.0;
  const bool vec = (V & 3) == 0;
  for (size_t i = beg + (size_t)threadIdx.x * 4; i < end; i += 1024) {
    float gv[4], av[4], bv[4], ra[4], rb[4];
    if (vec) {
      const float4 g = dpi_ld4(gc, i, gb, nt);
      const float4 t = dpi_ld4(xa, i, tb, nt);
      const float4 u = dpi_ld4(xb, i, tb, nt);
      gv[0] = g.x; gv[1] = g.y; gv[2] = g.z; gv[3] = g.w;
      av[0] = t.x; av[1] = t.y; av[2] = t.z; av[3] = t.w;
      bv[0] = u.x; bv[1] = u.y; bv[2] = u.z; bv[3] = u.w;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const bool in = i + j < end;
        gv[j] = in ? dpi_ld(gc, i + j, gb) : 0.f; av[j] = in ? dpi_ld(xa, i + j, tb) : 0.f; bv[j] = in ? dpi_ld(xb, i + j, tb) : 0.f;
      }
    }
    float lsf = 0.f, lqf = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float xh, g;
      bn_bwd_elem(ka, av[j], gv[j], xh, g);
      ra[j] = ka.a * (g - a1 - xh * a2);
      bn_bwd_elem(kb, bv[j], gv[j], xh, g);
      rb[j] = dpi_stored(kb.a * (g - b1 - xh * b2), gb);          // the fork's partials describe the stored dxb
      if (forked && i + j < end) { float h, gf_; bn_bwd_elem(kf, bv[j], rb[j], h, gf_); lsf += gf_; lqf = fmaf(gf_, h, lqf); }
    }
    if (vec) {
      dpi_st4(oa, i, make_float4(ra[0], ra[1], ra[2], ra[3]), gb, nt);
      dpi_st4(ob, i, make_float4(rb[0], rb[1], rb[2], rb[3]), gb, nt);
    } else {
      for (int j = 0; j < 4 && i + j < end; ++j) { dpi_st(oa, i + j, ra[j], gb); dpi_st(ob, i + j, rb[j], gb); }
    }
    sf += lsf; qf += lqf;
  }
  if (f_partials && f_hi > f_lo) {
    __shared__ double sh[8];
    const double SF = block_sum(sf, sh), QF = block_sum(qf, sh + 4);
    if (threadIdx.x == 0 && forked) {
      f_partials[((size_t)b * fC + fc) * 2 + 0] = SF;
      f_partials[((size_t)b * fC + fc) * 2 + 1] = QF;
    }
  }
}

// ---- y = T_out(T_a(a) + T_b(b)): the residual join and the BatchNorm behind it in one pass, t itself never stored (round 5; fp32) ----
template <bool fb = false>       // fb: a, b, y are bf16 (the sum itself is formed in fp32 from the widened operands and never rounded: it is not stored)
__global__ __launch_bounds__(256) void chain_add_apply_kernel(const float* __restrict__ a, const float* __restrict__ chain_a,
                                                              const float* __restrict__ b, const float* __restrict__ chain_b,
                                                              const float* __restrict__ chain_out, size_t V, float* __restrict__ y) {
  const bool nt = (size_t)gridDim.y * V >= kNtMinFloats;
  const int c = blockIdx.y;
  const Chain ta = load_chain(chain_a, c), tb = load_chain(chain_b, c), to = load_chain(chain_out, c);
  const float* __restrict__ ac = dpi_at(a, (size_t)c * V, fb);
  const float* __restrict__ bc = dpi_at(b, (size_t)c * V, fb);
  float* __restrict__ yc = dpi_at(y, (size_t)c * V, fb);
  const bool vec = (V & 3) == 0;
  // (the sum is formed exactly as chain_add_stats_kernel forms it: the statistics in chain_out describe these very values)
  for (size_t i = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4; i < V; i += (size_t)gridDim.x * 1024) {
    if (vec) {
      const float4 f = dpi_ld4(ac, i, fb, nt), g = dpi_ld4(bc, i, fb, nt);
      float4 o;
      o.x = apply_chain(to, apply_chain(ta, f.x) + apply_chain(tb, g.x)); o.y = apply_chain(to, apply_chain(ta, f.y) + apply_chain(tb, g.y));
      o.z = apply_chain(to, apply_chain(ta, f.z) + apply_chain(tb, g.z)); o.w = apply_chain(to, apply_chain(ta, f.w) + apply_chain(tb, g.w));
      dpi_st4(yc, i, o, fb, nt);
    } else {
      for (int j = 0; j < 4 && i + j < V; ++j)
        dpi_st(yc, i + j, apply_chain(to, apply_chain(ta, dpi_ld(ac, i + j, fb)) + apply_chain(tb, dpi_ld(bc, i + j, fb))), fb);
    }
  }
}

// ---- the whole BatchNorm backward of a residual join in TWO passes (round 5; fp32 tensors) -------------------------------------------
// Block3d:   y = bn2(act(t)),  t = act(bnS(S)) + bn1(T_CH(R))   [+ on the last channel slice: R3 -> bn3 -> act feeds bn1's input]
// ResPath3d: y = bn(act(t)),   t = act(bn3(r3)) + act(bn1(r1))
// Backward needs three NESTED sets of per-channel sums: {sum dy, sum dy xhat} of the top BatchNorm; then, of dt = the top BatchNorm's
// input gradient, {sum g, sum g xhat} of the two branch BatchNorms; then (Block3d, fork range) the same of dxb for the third conv's
// BatchNorm.  Rounds 1-4 took them in sequence — reduce (2 reads), apply + fork partials (4 reads, 1 write: dt), dual apply + fork
// partials (3 reads, 2 writes), apply on the fork range — 13.6 tensor passes per block.  But dt = P (dy - k1 - X k2) is LINEAR in (k1, k2),
// so every nested sum expands into sums that do not depend on the outer constants:
//     sum m dt f = sum m P dy f - k1 sum m P f - k2 sum m P X f                  (P = gamma invstd act'(t), X = xhat of the top BatchNorm)
// and likewise one level further for the fork.  ONE pass over (dy, t, xa, xb) accumulates the 24 expanded sums per channel in double
// precision (join_bwd_sums_kernel), a one-wave-per-channel kernel turns them into the eight constants {k1, k2, a1, a2, b1, b2, f1, f2} and
// the four (dgamma, dbeta) pairs (join_bwd_coef_kernel), and ONE pass recomputes dt in registers and writes dxa, dxb and — on the fork
// range — the third BatchNorm's input gradient directly (join_bwd_apply_kernel): 10.5 tensor passes, dt is never stored.
// Per element the apply pass evaluates exactly the expressions of bn_bwd_apply_fork / _dual / bn_bwd_apply; only the constants come from
// the expanded sums (fp32 products and four-element partial sums, double accumulation: the arithmetic of bn_bwd_reduce_kernel).
constexpr int kJoinSums = 24;
constexpr int kJoinGroups = 2;      // groups of four elements per thread between two double-precision accumulations
struct JoinSide {
  const float* x;
  const float* mean_invstd;
  const float* gamma;
  const float* beta;
  const float* in_chain;
  float post;
  const float* fwd_chain;       // t == NULL: this side's term of t = T_fwd_a(xa) + T_fwd_b(xb), recomputed exactly as the forward pass formed it
};
struct JoinFork {
  int lo, hi;                   // channel range of side B that feeds one more BatchNorm (lo == hi: none)
  const float* mean_invstd;     // [2 (hi - lo)]
  const float* gamma;
  const float* beta;
  float post;
};
template <bool fb = false, bool gb = false>      // fb: t, xa, xb bf16; gb: dy (and the apply pass's outputs) bf16
__global__ __launch_bounds__(256) void join_bwd_sums_kernel(const float* __restrict__ dy, const float* __restrict__ t,
                                                            const float* __restrict__ mean_invstd, const float* __restrict__ gamma,
                                                            const float* __restrict__ beta, float pre, JoinSide A, JoinSide B, JoinFork F,
                                                            int C, size_t V, int nblk, double* __restrict__ partials) {
  const bool nt = (size_t)gridDim.y * V >= kNtMinFloats;
  const int c = blockIdx.y, b = blockIdx.x;
  const BnBwd k = bn_bwd_consts(mean_invstd, gamma, beta, nullptr, pre, 1.f, C, c);
  const BnBwd ka = bn_bwd_consts(A.mean_invstd, A.gamma, A.beta, A.in_chain, 1.f, A.post, C, c);
  const BnBwd kb = bn_bwd_consts(B.mean_invstd, B.gamma, B.beta, B.in_chain, 1.f, B.post, C, c);
  const bool forked = c >= F.lo && c < F.hi;
  const int fC = F.hi - F.lo, fc = forked ? c - F.lo : 0;
  const BnBwd kf = forked ? bn_bwd_consts(F.mean_invstd, F.gamma, F.beta, nullptr, 1.f, F.post, fC, fc) : ka;
  const size_t span = stat_span(V, nblk);
  const size_t beg = (size_t)b * span, end = beg + span < V ? beg + span : V;
  const float* __restrict__ gc = dpi_at(dy, (size_t)c * V, gb);
  const float* __restrict__ tc = t ? dpi_at(t, (size_t)c * V, fb) : nullptr;
  const float* __restrict__ xa = dpi_at(A.x, (size_t)c * V, fb);
  const float* __restrict__ xb = dpi_at(B.x, (size_t)c * V, fb);
  const Chain fwa = load_chain(A.fwd_chain, c), fwb = load_chain(B.fwd_chain, c);
  double s[kJoinSums];
#pragma unroll
  for (int i = 0; i < kJoinSums; ++i) s[i] = 0.0;
  const bool vec = (V & 3) == 0;
  for (size_t i0 = beg + (size_t)threadIdx.x * 4; i0 < end; i0 += 1024 * kJoinGroups) {
   float l[kJoinSums];
#pragma unroll
   for (int q = 0; q < kJoinSums; ++q) l[q] = 0.f;
#pragma unroll
   for (int u = 0; u < kJoinGroups; ++u) {
    const size_t i = i0 + (size_t)u * 1024;
    if (i >= end) break;
    float gv[4], tv[4], av[4], bv[4];
    if (vec) {
      const float4 g = dpi_ld4(gc, i, gb, nt), p = dpi_ld4(xa, i, fb, nt), q = dpi_ld4(xb, i, fb, nt);
      gv[0] = g.x; gv[1] = g.y; gv[2] = g.z; gv[3] = g.w;
      av[0] = p.x; av[1] = p.y; av[2] = p.z; av[3] = p.w;
      bv[0] = q.x; bv[1] = q.y; bv[2] = q.z; bv[3] = q.w;
      if (tc) { const float4 u = dpi_ld4(tc, i, fb, nt); tv[0] = u.x; tv[1] = u.y; tv[2] = u.z; tv[3] = u.w; }
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const bool in = i + j < end;
        gv[j] = in ? dpi_ld(gc, i + j, gb) : 0.f; tv[j] = (in && tc) ? dpi_ld(tc, i + j, fb) : 0.f;
        av[j] = in ? dpi_ld(xa, i + j, fb) : 0.f; bv[j] = in ? dpi_ld(xb, i + j, fb) : 0.f;
      }
    }
    if (!tc) {
#pragma unroll
      for (int j = 0; j < 4; ++j) tv[j] = apply_chain(fwa, av[j]) + apply_chain(fwb, bv[j]);
    }
    // fp32 products, fp32 partial sums over the thread's eight elements (two groups of four: 333 -> 317 us at full resolution with fp32 tensors,
    // 301 -> 274 us with bf16 tensors; four groups: no further gain), ONE double-precision add per sum and trip — the arithmetic of
    // bn_bwd_reduce_kernel (`ls += g; lq = fmaf(g, xh, lq)` ... `s += ls`).  (The first version formed every product and sum in double: 45
    // DP operations per element made the pass ALU-bound — 1.23 ms per iteration with bf16 tensors, where its bytes take 0.5 ms.)
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (i + j < end) {
        float X, D, Xa, ma, Xb, mb;
        bn_bwd_elem(k, tv[j], gv[j], X, D);                       // post = 1: D = dy
        bn_bwd_elem(ka, av[j], 1.f, Xa, ma);                      // m = act_post'(BN(x)): 1 or the slope
        bn_bwd_elem(kb, bv[j], 1.f, Xb, mb);
        const float P = (k.pre == 1.f || tv[j] > 0.f) ? k.a : k.a * k.pre;
        l[0] += D; l[1] = fmaf(D, X, l[1]);
        const float wa = ma * P, wb = mb * P;
        const float waD = wa * D, waX = wa * X, wbD = wb * D, wbX = wb * X;
        l[2] += waD; l[3] += wa; l[4] += waX;
        l[5] = fmaf(waD, Xa, l[5]); l[6] = fmaf(wa, Xa, l[6]); l[7] = fmaf(waX, Xa, l[7]);
        l[8] += wbD; l[9] += wb; l[10] += wbX;
        l[11] = fmaf(wbD, Xb, l[11]); l[12] = fmaf(wb, Xb, l[12]); l[13] = fmaf(wbX, Xb, l[13]);
        if (forked) {
          // the fork's BatchNorm reads the RAW side-B tensor (its own conv output); its incoming gradient is dxb
          float Xf, mf;
          bn_bwd_elem(kf, bv[j], 1.f, Xf, mf);
          const float wf = mf * wb, wfD = wf * D, wfX = wf * X, mfXf = mf * Xf;
          l[14] += wfD; l[15] += wf; l[16] += wfX; l[17] += mf; l[18] = fmaf(mf, Xb, l[18]);
          l[19] = fmaf(wfD, Xf, l[19]); l[20] = fmaf(wf, Xf, l[20]); l[21] = fmaf(wfX, Xf, l[21]); l[22] += mfXf; l[23] = fmaf(mfXf, Xb, l[23]);
        }
      }
   }
#pragma unroll
   for (int q = 0; q < kJoinSums; ++q) s[q] += (double)l[q];
  }
  __shared__ double sh[4][kJoinSums];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < kJoinSums; ++i) {
    const double v = wave_sum(s[i]);
    if (lane == 0) sh[wid][i] = v;
  }
  __syncthreads();
  if (threadIdx.x < kJoinSums) {
    const int i = threadIdx.x;
    partials[((size_t)b * C + c) * kJoinSums + i] = (sh[0][i] + sh[1][i]) + (sh[2][i] + sh[3][i]);
  }
}

// one wave per channel: fixed-order reduction of the block partials, then the constants.  coef [C][8] = {k1, k2, a1, a2, b1, b2, f1, f2};
// dgb [6][C] = rows {dgamma, dbeta} x {top, A, B}; the fork's pair goes to dgb_f [2][hi - lo].
__global__ __launch_bounds__(64) void join_bwd_coef_kernel(const double* __restrict__ partials, int nblk, int C, double V,
                                                          const float* __restrict__ mi_b, const float* __restrict__ gamma_b, int f_lo, int f_hi,
                                                          float* __restrict__ coef, float* __restrict__ dgb, float* __restrict__ dgb_f) {
  const int c = blockIdx.x, lane = threadIdx.x;
  double s[kJoinSums];
#pragma unroll
  for (int i = 0; i < kJoinSums; ++i) s[i] = 0.0;
  for (int b = lane; b < nblk; b += 64) {
    const double* __restrict__ p = partials + ((size_t)b * C + c) * kJoinSums;
#pragma unroll
    for (int i = 0; i < kJoinSums; ++i) s[i] += p[i];
  }
#pragma unroll
  for (int i = 0; i < kJoinSums; ++i) s[i] = wave_sum(s[i]);
  if (lane != 0) return;
  const double k1 = s[0] / V, k2 = s[1] / V;
  const double Ga = s[2] - k1 * s[3] - k2 * s[4], Ha = s[5] - k1 * s[6] - k2 * s[7];
  const double Gb = s[8] - k1 * s[9] - k2 * s[10], Hb = s[11] - k1 * s[12] - k2 * s[13];
  // the apply pass uses the constants as floats (as bn_bwd_apply does): the fork's sums are taken with the ROUNDED b1, b2 it will use
  const float k1f = (float)k1, k2f = (float)k2, a1f = (float)(Ga / V), a2f = (float)(Ha / V), b1f = (float)(Gb / V), b2f = (float)(Hb / V);
  float f1f = 0.f, f2f = 0.f;
  if (c >= f_lo && c < f_hi) {
    const double ab = (double)((gamma_b ? gamma_b[c] : 1.f) * mi_b[C + c]);          // gamma invstd of side B, the float product the apply pass uses
    const double T1 = s[14] - k1 * s[15] - k2 * s[16], TX = s[19] - k1 * s[20] - k2 * s[21];
    const double Gf = ab * (T1 - (double)b1f * s[17] - (double)b2f * s[18]);
    const double Hf = ab * (TX - (double)b1f * s[22] - (double)b2f * s[23]);
    f1f = (float)(Gf / V); f2f = (float)(Hf / V);
    dgb_f[c - f_lo] = (float)Hf;                      // [2][hi - lo]: row 0 dgamma, row 1 dbeta (each row a contiguous gradient tensor)
    dgb_f[(f_hi - f_lo) + c - f_lo] = (float)Gf;
  }
  float* o = coef + (size_t)c * 8;
  o[0] = k1f; o[1] = k2f; o[2] = a1f; o[3] = a2f; o[4] = b1f; o[5] = b2f; o[6] = f1f; o[7] = f2f;
  dgb[c] = (float)s[1]; dgb[C + c] = (float)s[0]; dgb[2 * C + c] = (float)Ha; dgb[3 * C + c] = (float)Ga;      // [6][C]
  dgb[4 * C + c] = (float)Hb; dgb[5 * C + c] = (float)Gb;
}

template <bool fb = false, bool gb = false>
__global__ __launch_bounds__(256) void join_bwd_apply_kernel(const float* __restrict__ dy, const float* __restrict__ t,
                                                             const float* __restrict__ mean_invstd, const float* __restrict__ gamma,
                                                             const float* __restrict__ beta, float pre, JoinSide A, JoinSide B, JoinFork F,
                                                             const float* __restrict__ coef, int C, size_t V, float* __restrict__ dxa,
                                                             float* __restrict__ dxb, float* __restrict__ dxf) {
  const bool nt = (size_t)gridDim.y * V >= kNtMinFloats;
  const int c = blockIdx.y;
  const BnBwd k = bn_bwd_consts(mean_invstd, gamma, beta, nullptr, pre, 1.f, C, c);
  const BnBwd ka = bn_bwd_consts(A.mean_invstd, A.gamma, A.beta, A.in_chain, 1.f, A.post, C, c);
  const BnBwd kb = bn_bwd_consts(B.mean_invstd, B.gamma, B.beta, B.in_chain, 1.f, B.post, C, c);
  const bool forked = c >= F.lo && c < F.hi;
  const int fC = F.hi - F.lo, fc = forked ? c - F.lo : 0;
  const BnBwd kf = forked ? bn_bwd_consts(F.mean_invstd, F.gamma, F.beta, nullptr, 1.f, F.post, fC, fc) : ka;
  const float* __restrict__ q = coef + (size_t)c * 8;
  const float k1 = q[0], k2 = q[1], a1 = q[2], a2 = q[3], b1 = q[4], b2 = q[5], f1 = q[6], f2 = q[7];
  const float* __restrict__ gc = dpi_at(dy, (size_t)c * V, gb);
  const float* __restrict__ tc = t ? dpi_at(t, (size_t)c * V, fb) : nullptr;
  const float* __restrict__ xa = dpi_at(A.x, (size_t)c * V, fb);
  const float* __restrict__ xb = dpi_at(B.x, (size_t)c * V, fb);
  const Chain fwa = load_chain(A.fwd_chain, c), fwb = load_chain(B.fwd_chain, c);
  float* __restrict__ oa = dpi_at(dxa, (size_t)c * V, gb);
  float* __restrict__ ob = forked ? dpi_at(dxf, (size_t)fc * V, gb) : dpi_at(dxb, (size_t)c * V, gb);        // fork range: the third BatchNorm's input gradient instead of dxb
  const bool vec = (V & 3) == 0;
  auto one = [&](float gv, float tv, float av, float bv, float& ra, float& rb) {
    float X, g, xh, gg;
    bn_bwd_elem(k, tv, gv, X, g);
    const float du = k.a * (g - k1 - X * k2);
    const float dt = (k.pre == 1.f || tv > 0.f) ? du : du * k.pre;              // bn_bwd_apply_fork's dx, kept in a register
    bn_bwd_elem(ka, av, dt, xh, gg);
    ra = ka.a * (gg - a1 - xh * a2);
    bn_bwd_elem(kb, bv, dt, xh, gg);
    rb = kb.a * (gg - b1 - xh * b2);
    if (forked) {
      bn_bwd_elem(kf, bv, rb, xh, gg);
      rb = kf.a * (gg - f1 - xh * f2);                                            // bn_bwd_apply of the fork's BatchNorm (pre = 1)
    }
  };
  for (size_t i = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4; i < V; i += (size_t)gridDim.x * 1024) {
    if (vec) {
      const float4 g = dpi_ld4(gc, i, gb, nt), p = dpi_ld4(xa, i, fb, nt), r = dpi_ld4(xb, i, fb, nt);
      float4 u;
      if (tc) u = dpi_ld4(tc, i, fb, nt);
      else u = make_float4(apply_chain(fwa, p.x) + apply_chain(fwb, r.x), apply_chain(fwa, p.y) + apply_chain(fwb, r.y),
                           apply_chain(fwa, p.z) + apply_chain(fwb, r.z), apply_chain(fwa, p.w) + apply_chain(fwb, r.w));
      float4 ya, yb;
      one(g.x, u.x, p.x, r.x, ya.x, yb.x); one(g.y, u.y, p.y, r.y, ya.y, yb.y);
      one(g.z, u.z, p.z, r.z, ya.z, yb.z); one(g.w, u.w, p.w, r.w, ya.w, yb.w);
      dpi_st4(oa, i, ya, gb, nt);
      dpi_st4(ob, i, yb, gb, nt);
    } else {
      for (int j = 0; j < 4 && i + j < V; ++j) {
        float ra, rb;
        const float av = dpi_ld(xa, i + j, fb), bv = dpi_ld(xb, i + j, fb);
        one(dpi_ld(gc, i + j, gb), tc ? dpi_ld(tc, i + j, fb) : apply_chain(fwa, av) + apply_chain(fwb, bv), av, bv, ra, rb);
        dpi_st(oa, i + j, ra, gb); dpi_st(ob, i + j, rb, gb);
      }
    }
  }
}

__global__ __launch_bounds__(256) void lrelu_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ x, float slope,
                                                        size_t n, float* __restrict__ dx) {
  const bool nt = n >= kNtMinFloats;
  const bool vec = (n & 3) == 0;
  for (size_t i = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4; i < n; i += (size_t)gridDim.x * 1024) {
    if (vec) {
      const float4 f = ld4(x + i, nt);
      float4 g = ld4(dy + i, nt);
      g.x = f.x > 0.f ? g.x : g.x * slope; g.y = f.y > 0.f ? g.y : g.y * slope;
      g.z = f.z > 0.f ? g.z : g.z * slope; g.w = f.w > 0.f ? g.w : g.w * slope;
      st4(dx + i, g, nt);
    } else {
      for (int k = 0; k < 4 && i + k < n; ++k) dx[i + k] = x[i + k] > 0.f ? dy[i + k] : dy[i + k] * slope;
    }
  }
}

// ---- the other activations of get_activation (reference base.py:97-114): ELU(alpha = 1), Tanh, Sigmoid --------------------
// forward y = f(x); backward from the OUTPUT y (what autograd keeps): ELU' = y > 0 ? 1 : y + 1, tanh' = 1 - y^2,
// sigmoid' = y (1 - y).  (LeakyReLU / ReLU never come here: they are chains fused into their neighbours.)
__device__ __forceinline__ float act_fwd_one(int kind, float x) {
  if (kind == DPI_ACT_ELU) return x > 0.f ? x : expm1f(x);
  if (kind == DPI_ACT_TANH) return tanhf(x);
  // below -87 the sum 1 + e^-x is e^-x in fp32, and e^-x overflows from 88.73 on: 1 / (1 + inf) returned 0 where sigmoid(x) = e^x is
  // still a (subnormal) float.  Above -87 the expression is unchanged.
  if (x < -87.f) return expf(x);
  return 1.f / (1.f + expf(-x));
}
__device__ __forceinline__ float act_bwd_one(int kind, float y, float dy) {
  if (kind == DPI_ACT_ELU) return y > 0.f ? dy : dy * (y + 1.f);
  if (kind == DPI_ACT_TANH) return dy * (1.f - y * y);
  return dy * (y * (1.f - y));
}
__global__ __launch_bounds__(256) void act_fwd_kernel(const float* __restrict__ x, size_t n, int kind, float* __restrict__ y) {
  const bool vec = (n & 3) == 0;
  for (size_t i = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4; i < n; i += (size_t)gridDim.x * 1024) {
    if (vec) {
      float4 f = *reinterpret_cast<const float4*>(x + i);
      f.x = act_fwd_one(kind, f.x); f.y = act_fwd_one(kind, f.y); f.z = act_fwd_one(kind, f.z); f.w = act_fwd_one(kind, f.w);
      *reinterpret_cast<float4*>(y + i) = f;
    } else {
      for (int k = 0; k < 4 && i + k < n; ++k) y[i + k] = act_fwd_one(kind, x[i + k]);
    }
  }
}
__global__ __launch_bounds__(256) void act_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ y, size_t n, int kind,
                                                      float* __restrict__ dx) {
  const bool vec = (n & 3) == 0;
  for (size_t i = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4; i < n; i += (size_t)gridDim.x * 1024) {
    if (vec) {
      const float4 f = *reinterpret_cast<const float4*>(y + i);
      float4 g = *reinterpret_cast<const float4*>(dy + i);
      g.x = act_bwd_one(kind, f.x, g.x); g.y = act_bwd_one(kind, f.y, g.y); g.z = act_bwd_one(kind, f.z, g.z); g.w = act_bwd_one(kind, f.w, g.w);
      *reinterpret_cast<float4*>(dx + i) = g;
    } else {
      for (int k = 0; k < 4 && i + k < n; ++k) dx[i + k] = act_bwd_one(kind, y[i + k], dy[i + k]);
    }
  }
}

__global__ __launch_bounds__(256) void add_kernel(const float* __restrict__ a, const float* __restrict__ b, size_t n,
                                                  float* __restrict__ y) {
  const bool nt = n >= kNtMinFloats;
  const bool vec = (n & 3) == 0;
  for (size_t i = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4; i < n; i += (size_t)gridDim.x * 1024) {
    if (vec) {
      const float4 f = ld4(a + i, nt);
      const float4 g = ld4(b + i, nt);
      st4(y + i, make_float4(f.x + g.x, f.y + g.y, f.z + g.z, f.w + g.w), nt);
    } else {
      for (int k = 0; k < 4 && i + k < n; ++k) y[i + k] = a[i + k] + b[i + k];
    }
  }
}

__global__ __launch_bounds__(64) void channel_sum_final_kernel(const double* __restrict__ partials, int nblk, int C,
                                                               float* __restrict__ out) {
  const int c = blockIdx.x;
  double s = 0.0;
  for (int b = threadIdx.x; b < nblk; b += 64) s += partials[((size_t)b * C + c) * 2];
  s = wave_sum(s);
  if (threadIdx.x == 0) out[c] = (float)s;
}

// ---- x2 up-sampling (lin_src / lin_bwd_taps: common.h) -------------------------------------------------------

template <bool xb = false, bool yb = false>
__global__ __launch_bounds__(256) void upsample_fwd_kernel(const float* __restrict__ x, const float* __restrict__ chain, int D, int H,
                                                           int W, int Do, int Ho, int Wo, int linear, int scale_d,
                                                           float* __restrict__ y) {
  const int c = blockIdx.y;
  const size_t Vo = (size_t)Do * Ho * Wo, V = (size_t)D * H * W;
  const Chain t = load_chain(chain, c);
  const float* __restrict__ xc = dpi_at(x, (size_t)c * V, xb);
  float* __restrict__ yc = dpi_at(y, (size_t)c * Vo, yb);
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < Vo; i += (size_t)gridDim.x * 256) {
    const int ow = i % Wo, oh = (i / Wo) % Ho, od = i / ((size_t)Wo * Ho);
    float r;
    if (!linear) {
      const int id = scale_d ? od >> 1 : od;
      r = apply_chain(t, dpi_ld(xc, ((size_t)id * H + (oh >> 1)) * W + (ow >> 1), xb));
    } else {
      int d0, d1, h0, h1, w0, w1;
      float a0, a1, b0, b1, c0, c1;
      if (scale_d) lin_src(od, D, d0, d1, a0, a1); else { d0 = d1 = od; a0 = 1.f; a1 = 0.f; }
      lin_src(oh, H, h0, h1, b0, b1);
      lin_src(ow, W, w0, w1, c0, c1);
      auto at = [&](int d, int h, int w) { return apply_chain(t, dpi_ld(xc, ((size_t)d * H + h) * W + w, xb)); };
      const float p0 = b0 * (c0 * at(d0, h0, w0) + c1 * at(d0, h0, w1)) + b1 * (c0 * at(d0, h1, w0) + c1 * at(d0, h1, w1));
      r = a0 * p0;
      if (scale_d)
        r += a1 * (b0 * (c0 * at(d1, h0, w0) + c1 * at(d1, h0, w1)) + b1 * (c0 * at(d1, h1, w0) + c1 * at(d1, h1, w1)));
    }
    dpi_st(yc, i, r, yb);
  }
}

// weight with which output index o reads input index i along one axis of length n
__device__ __forceinline__ float lin_wt(int o, int i, int n) {
  int i0, i1; float w0, w1;
  lin_src(o, n, i0, i1, w0, w1);
  return (i0 == i ? w0 : 0.f) + (i1 == i ? w1 : 0.f);
}

template <bool gb = false>
__global__ __launch_bounds__(256) void upsample_bwd_kernel(const float* __restrict__ dy, int D, int H, int W, int Do, int Ho, int Wo,
                                                           int linear, int scale_d, float* __restrict__ dx) {
  const int c = blockIdx.y;
  const size_t Vo = (size_t)Do * Ho * Wo, V = (size_t)D * H * W;
  const float* __restrict__ gc = dpi_at(dy, (size_t)c * Vo, gb);
  float* __restrict__ oc = dpi_at(dx, (size_t)c * V, gb);
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < V; i += (size_t)gridDim.x * 256) {
    const int iw = i % W, ih = (i / W) % H, id = i / ((size_t)W * H);
    float acc = 0.f;
    if (!linear) {
      const int dlo = scale_d ? 2 * id : id, dhi = scale_d ? 2 * id + 1 : id;
      for (int od = dlo; od <= dhi && od < Do; ++od)
        for (int oh = 2 * ih; oh <= 2 * ih + 1 && oh < Ho; ++oh)
          for (int ow = 2 * iw; ow <= 2 * iw + 1 && ow < Wo; ++ow) acc += dpi_ld(gc, ((size_t)od * Ho + oh) * Wo + ow, gb);
    } else {
      const int dlo = scale_d ? max(2 * id - 1, 0) : id, dhi = scale_d ? min(2 * id + 2, Do - 1) : id;
      for (int od = dlo; od <= dhi; ++od) {
        const float wd = scale_d ? lin_wt(od, id, D) : 1.f;
        if (wd == 0.f) continue;
        for (int oh = max(2 * ih - 1, 0); oh <= min(2 * ih + 2, Ho - 1); ++oh) {
          const float wh = lin_wt(oh, ih, H);
          if (wh == 0.f) continue;
          for (int ow = max(2 * iw - 1, 0); ow <= min(2 * iw + 2, Wo - 1); ++ow) {
            const float ww = lin_wt(ow, iw, W);
            if (ww != 0.f) acc = fmaf(wd * wh * ww, dpi_ld(gc, ((size_t)od * Ho + oh) * Wo + ow, gb), acc);
          }
        }
      }
    }
    dpi_st(oc, i, acc, gb);
  }
}

// ---- x2 linear up-sampling, fast 3-D / 2-D paths ------------------------------------------------------------------------
// forward: one thread per INPUT voxel produces its 2x2x2 output cube from the 3x3x3 (edge-clamped) neighbourhood:
//   out[2i] = .25 in[i-1] + .75 in[i],  out[2i+1] = .75 in[i] + .25 in[i+1]   per axis (27 loads for 8 outputs)
template <bool SCALE_D, bool xb = false, bool yb = false>
__global__ __launch_bounds__(256) void upsample_lin_fwd_cube_kernel(const float* __restrict__ x, const float* __restrict__ chain, int D, int H,
                                                                    int W, int Do, int Ho, int Wo, float* __restrict__ y) {
  const int c = blockIdx.y;
  const size_t V = (size_t)D * H * W, Vo = (size_t)Do * Ho * Wo;
  const Chain t = load_chain(chain, c);
  const float* __restrict__ xc = dpi_at(x, (size_t)c * V, xb);
  float* __restrict__ yc = dpi_at(y, (size_t)c * Vo, yb);
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < V; i += (size_t)gridDim.x * 256) {
    const int w = i % W, h = (i / W) % H, d = i / ((size_t)W * H);
    const int wm = max(w - 1, 0), wp = min(w + 1, W - 1), hm = max(h - 1, 0), hp = min(h + 1, H - 1);
    const int dm = SCALE_D ? max(d - 1, 0) : d, dp = SCALE_D ? min(d + 1, D - 1) : d;
    const int ds_[3] = {dm, d, dp}, hs_[3] = {hm, h, hp}, ws_[3] = {wm, w, wp};
    // reduce along w first: for each (dz, hy) the two w-outputs
    float lo[3][3], hi[3][3];
#pragma unroll
    for (int a = 0; a < (SCALE_D ? 3 : 1); ++a)
#pragma unroll
      for (int b = 0; b < 3; ++b) {
        const size_t row = ((size_t)ds_[SCALE_D ? a : 1] * H + hs_[b]) * W;
        const float v0 = apply_chain(t, dpi_ld(xc, row + ws_[0], xb)), v1 = apply_chain(t, dpi_ld(xc, row + ws_[1], xb)),
                    v2 = apply_chain(t, dpi_ld(xc, row + ws_[2], xb));
        lo[a][b] = .25f * v0 + .75f * v1;
        hi[a][b] = .75f * v1 + .25f * v2;
      }
#pragma unroll
    for (int od_ = 0; od_ < (SCALE_D ? 2 : 1); ++od_) {
      const int od = SCALE_D ? 2 * d + od_ : d;
      if (od >= Do) continue;
#pragma unroll
      for (int oh_ = 0; oh_ < 2; ++oh_) {
        const int oh = 2 * h + oh_;
        if (oh >= Ho) continue;
        float r0, r1;
        auto hcomb = [&](int a, float& l, float& u) {
          l = oh_ == 0 ? .25f * lo[a][0] + .75f * lo[a][1] : .75f * lo[a][1] + .25f * lo[a][2];
          u = oh_ == 0 ? .25f * hi[a][0] + .75f * hi[a][1] : .75f * hi[a][1] + .25f * hi[a][2];
        };
        if (SCALE_D) {
          float l0, u0, l1, u1, l2, u2;
          hcomb(0, l0, u0); hcomb(1, l1, u1); hcomb(2, l2, u2);
          r0 = od_ == 0 ? .25f * l0 + .75f * l1 : .75f * l1 + .25f * l2;
          r1 = od_ == 0 ? .25f * u0 + .75f * u1 : .75f * u1 + .25f * u2;
        } else {
          hcomb(0, r0, r1);
        }
        const size_t o = ((size_t)od * Ho + oh) * Wo + 2 * w;
        if (yb && 2 * w + 1 < Wo && !((o + (size_t)c * Vo) & 1)) {       // bf16 pair in one aligned 4-byte store (a torch allocation is >= 4-byte aligned)
          reinterpret_cast<unsigned*>(reinterpret_cast<unsigned short*>(yc) + o)[0] = dpi_pack_bf16(r0, r1);
        } else {
          if (2 * w < Wo) dpi_st(yc, o, r0, yb);
          if (2 * w + 1 < Wo) dpi_st(yc, o + 1, r1, yb);
        }
      }
    }
  }
}

// backward: one thread per INPUT voxel gathers its 4x4x4 (3-D) / 4x4 (2-D) output neighbourhood with the per-axis weights of lin_bwd_taps

template <bool SCALE_D, bool gb = false>
__global__ __launch_bounds__(256) void upsample_lin_bwd_gather_kernel(const float* __restrict__ dy, int D, int H, int W, int Do, int Ho,
                                                                      int Wo, float* __restrict__ dx) {
  const int c = blockIdx.y;
  const size_t V = (size_t)D * H * W, Vo = (size_t)Do * Ho * Wo;
  const float* __restrict__ gc = dpi_at(dy, (size_t)c * Vo, gb);
  float* __restrict__ oc = dpi_at(dx, (size_t)c * V, gb);
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < V; i += (size_t)gridDim.x * 256) {
    const int w = i % W, h = (i / W) % H, d = i / ((size_t)W * H);
    int ow[4], oh[4], od[4];
    float ww[4], wh[4], wd[4];
    lin_bwd_taps(w, W, Wo, ow, ww);
    lin_bwd_taps(h, H, Ho, oh, wh);
    if (SCALE_D) lin_bwd_taps(d, D, Do, od, wd);
    float acc = 0.f;
#pragma unroll
    for (int a = 0; a < (SCALE_D ? 4 : 1); ++a) {
      const int od_ = SCALE_D ? od[a] : d;
      const float wa = SCALE_D ? wd[a] : 1.f;
      float accd = 0.f;
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const size_t row = ((size_t)od_ * Ho + oh[b]) * Wo;
        const float rsum = ww[0] * dpi_ld(gc, row + ow[0], gb) + ww[1] * dpi_ld(gc, row + ow[1], gb) + ww[2] * dpi_ld(gc, row + ow[2], gb)
                           + ww[3] * dpi_ld(gc, row + ow[3], gb);
        accd = fmaf(wh[b], rsum, accd);
      }
      acc = fmaf(wa, accd, acc);
    }
    dpi_st(oc, i, acc, gb);
  }
}

// Separable adjoint, one axis per pass: in [outer][no][inner] -> out [outer][n][inner],
//   out[i] = .25 in[2i-1] + .75 in[2i] + .75 in[2i+1] + .25 in[2i+2]   (edge weights 1 at i = 0 / n-1, taps >= no dropped).
// Three coalesced passes (W, H, D) move 2.6x the gradient once instead of gathering 64 strided values per voxel
// (8 L1 requests per voxel): 0.95 -> ~0.5 ms for the 51-channel full-resolution tensor.
template <bool ib = false, bool ob = false>
__global__ __launch_bounds__(256) void upsample_lin_bwd_axis_kernel(const float* __restrict__ in, float* __restrict__ out, unsigned outer,
                                                                    int n, int no, unsigned inner) {
  // blockIdx.x walks one [n][inner] slab (32-bit index math only), blockIdx.y strides over the outer slabs; a slab shorter
  // than the workgroup (the W pass: one row) shares it with its neighbours
  const unsigned slab = (unsigned)n * inner;
  const unsigned per = slab < 256 ? 256 / slab : 1;
  const unsigned sub = per > 1 ? threadIdx.x / slab : 0;
  const unsigned e = per > 1 ? threadIdx.x - sub * slab : blockIdx.x * 256 + threadIdx.x;
  if (e >= slab || sub >= per) return;
  const unsigned i = e / inner, in_i = e - i * inner;
  int oo[4];
  float wt[4];
  lin_bwd_taps((int)i, n, no, oo, wt);
  const unsigned o0 = oo[0] * inner + in_i, o1 = oo[1] * inner + in_i, o2 = oo[2] * inner + in_i, o3 = oo[3] * inner + in_i;
  for (unsigned o = blockIdx.y * per + sub; o < outer; o += gridDim.y * per) {
    const float* __restrict__ p = dpi_at(in, (size_t)o * no * inner, ib);
    dpi_st(out, (size_t)o * slab + e, (wt[0] * dpi_ld(p, o0, ib) + wt[1] * dpi_ld(p, o1, ib)) + (wt[2] * dpi_ld(p, o2, ib) + wt[3] * dpi_ld(p, o3, ib)), ob);
  }
}

// The W pass of the separable adjoint (inner = 1: rows of `no` = 2 n floats -> rows of n) with a thread per PAIR of outputs: one aligned float4
// (in[2i .. 2i+3], i even) + the two neighbours in[2i-1], in[2i+4] instead of eight scalar loads, one 8-byte store; the same taps, weights and
// summation order as upsample_lin_bwd_axis_kernel, so the two are bit-identical (round 5: the scalar pass ran at 3.6 TB/s where the H and D
// passes reach 5.4-5.8).  fp32 rows of whole float4 without a crop (no = 2 n, n even); everything else takes the generic kernel.
__global__ __launch_bounds__(256) void upsample_lin_bwd_w2_kernel(const float* __restrict__ in, float* __restrict__ out, size_t rows, int n) {
  const int half = n >> 1, no = 2 * n;
  const size_t total = rows * (size_t)half;
  for (size_t p = (size_t)blockIdx.x * 256 + threadIdx.x; p < total; p += (size_t)gridDim.x * 256) {
    const size_t r = p / half;
    const int i = 2 * (int)(p - r * half);
    const float* __restrict__ row = in + r * no;
    const float4 v = *reinterpret_cast<const float4*>(row + 2 * i);          // in[2i], in[2i+1], in[2i+2], in[2i+3]
    const float lo = row[i > 0 ? 2 * i - 1 : 0], hi = row[i + 1 < n - 1 ? 2 * i + 4 : 0];
    int o[4];
    float w0[4], w1[4];
    lin_bwd_taps(i, n, no, o, w0);
    lin_bwd_taps(i + 1, n, no, o, w1);
    float2 y;
    y.x = (w0[0] * lo + w0[1] * v.x) + (w0[2] * v.y + w0[3] * v.z);
    y.y = (w1[0] * v.y + w1[1] * v.z) + (w1[2] * v.w + w1[3] * hi);
    *reinterpret_cast<float2*>(out + r * n + i) = y;
  }
}

__global__ __launch_bounds__(256) void crop_copy_kernel(const float* __restrict__ x, int D, int H, int W, int od, int oh, int ow,
                                                        int Do, int Ho, int Wo, float* __restrict__ y, int adjoint) {
  // forward: y[c][Do][Ho][Wo] = x[c][od+.., oh+.., ow+..]; adjoint: x-shaped output, zero outside the window
  const int c = blockIdx.y;
  const size_t V = (size_t)D * H * W, Vo = (size_t)Do * Ho * Wo;
  if (!adjoint) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < Vo; i += (size_t)gridDim.x * 256) {
      const int w = i % Wo, h = (i / Wo) % Ho, d = i / ((size_t)Wo * Ho);
      y[(size_t)c * Vo + i] = x[(size_t)c * V + ((size_t)(d + od) * H + h + oh) * W + w + ow];
    }
  } else {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < V; i += (size_t)gridDim.x * 256) {
      const int w = i % W, h = (i / W) % H, d = i / ((size_t)W * H);
      const int cd = d - od, ch = h - oh, cw = w - ow;
      const bool in = cd >= 0 && cd < Do && ch >= 0 && ch < Ho && cw >= 0 && cw < Wo;
      y[(size_t)c * V + i] = in ? x[(size_t)c * Vo + ((size_t)cd * Ho + ch) * Wo + cw] : 0.f;
    }
  }
}

// y[c][t][s] = sum_k taps[k] * x[c][t + K/2 - k][s]  (zero outside): the grouped conv_transposeNd the reference uses to
// filter the input noise along the time axis (utils/processing.py:34-67) is a true convolution centred on K/2
__global__ __launch_bounds__(256) void fir_axis0_kernel(const float* __restrict__ x, const float* __restrict__ taps, int K, int T, size_t S,
                                                        float* __restrict__ y) {
  const int c = blockIdx.y, p = K / 2;
  const size_t n = (size_t)T * S;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    const int t = (int)(i / S);
    const size_t s_ = i % S;
    float acc = 0.f;
    for (int k = 0; k < K; ++k) {
      const int tt = t + p - k;
      if (tt >= 0 && tt < T) acc = fmaf(taps[k], x[(size_t)c * n + (size_t)tt * S + s_], acc);
    }
    y[(size_t)c * n + i] = acc;
  }
}

__global__ __launch_bounds__(256) void axpy_kernel(float a, const float* __restrict__ x, size_t n, float* __restrict__ y) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) y[i] = fmaf(a, x[i], y[i]);
}

inline unsigned ew_blocks(size_t n_vec4_threads) {
  size_t b = cdivz(n_vec4_threads, 256);
  if (b > 4096) b = 4096;
  if (b < 1) b = 1;
  return (unsigned)b;
}

}  // namespace

extern "C" int dpi_stat_blocks(int C, size_t V) {
  if (C <= 0 || V == 0) return 0;
  size_t n = cdivz(V, kStatSpan);
  if (n > kMaxStatBlocks) n = kMaxStatBlocks;
  return (int)n;
}

// launch KERNEL<forward tensors bf16, gradient tensors bf16> for the two bits of an `io` mask
#define DPI_LAUNCH_FG(io, KERNEL, GRID, ST, ...)                                          \
  do {                                                                                    \
    if (DPI_FB(io)) {                                                                     \
      if (DPI_GB(io)) KERNEL<true, true><<<GRID, 256, 0, ST>>>(__VA_ARGS__);              \
      else KERNEL<true, false><<<GRID, 256, 0, ST>>>(__VA_ARGS__);                        \
    } else {                                                                              \
      if (DPI_GB(io)) KERNEL<false, true><<<GRID, 256, 0, ST>>>(__VA_ARGS__);             \
      else KERNEL<false, false><<<GRID, 256, 0, ST>>>(__VA_ARGS__);                       \
    }                                                                                     \
  } while (0)
#define DPI_FB(io) (((io) & DPI_STORE_FWD_BF16) != 0)
#define DPI_GB(io) (((io) & DPI_STORE_GRAD_BF16) != 0)
#define DPI_REQUIRE_IO(io, what) DPI_REQUIRE(((io) & ~3u) == 0, what ": unknown storage-type bits in io = %u", (unsigned)(io))

extern "C" int dpi_channel_stats_io(const float* x, const float* chain, int C, size_t V, double* partials, unsigned io, void* stream) {
  DPI_REQUIRE(x && partials && C > 0 && V > 0, "channel_stats: bad argument");
  DPI_REQUIRE_IO(io, "channel_stats");
  const int nblk = dpi_stat_blocks(C, V);
  if (DPI_FB(io)) channel_stats_kernel<true><<<dim3(nblk, C), 256, 0, (hipStream_t)stream>>>(x, chain, C, V, nblk, partials);
  else channel_stats_kernel<false><<<dim3(nblk, C), 256, 0, (hipStream_t)stream>>>(x, chain, C, V, nblk, partials);
  return dpi_check_launch("channel_stats");
}
extern "C" int dpi_channel_stats(const float* x, const float* chain, int C, size_t V, double* partials, void* stream) {
  return dpi_channel_stats_io(x, chain, C, V, partials, 0, stream);
}

extern "C" int dpi_bn_finalize(const double* partials, int nblk, int C, size_t count, const float* gamma, const float* beta,
                               float eps, float momentum, float slope, int act_first, const float* in_chain, float* running_mean,
                               float* running_var, int64_t* num_batches_tracked, float* mean_invstd, float* chain_out,
                               void* stream) {
  DPI_REQUIRE(partials && nblk > 0 && C > 0 && count > 0, "bn_finalize: bad argument");
  DPI_REQUIRE(!in_chain || (slope == 1.f && !act_first), "bn_finalize: a composed input chain excludes a fused activation");
  bn_finalize_kernel<<<C, 256, 0, (hipStream_t)stream>>>(partials, nblk, C, (double)count, gamma, beta, eps, momentum, slope, act_first,
                                                        in_chain, running_mean, running_var, num_batches_tracked, mean_invstd, chain_out);
  return dpi_check_launch("bn_finalize");
}

extern "C" int dpi_chain_apply_io(const float* x, const float* chain, int C, size_t V, float* y, unsigned io, void* stream) {
  DPI_REQUIRE(x && y && C > 0 && V > 0, "chain_apply: bad argument");
  DPI_REQUIRE_IO(io, "chain_apply");
  if (DPI_FB(io)) chain_apply_kernel<true, true><<<dim3(ew_blocks(cdivz(V, 4)), C), 256, 0, (hipStream_t)stream>>>(x, chain, V, y);
  else chain_apply_kernel<false, false><<<dim3(ew_blocks(cdivz(V, 4)), C), 256, 0, (hipStream_t)stream>>>(x, chain, V, y);
  return dpi_check_launch("chain_apply");
}
extern "C" int dpi_chain_apply(const float* x, const float* chain, int C, size_t V, float* y, void* stream) {
  return dpi_chain_apply_io(x, chain, C, V, y, 0, stream);
}

extern "C" int dpi_bn_bwd_reduce(const float* dy, const float* x, const float* mean_invstd, const float* gamma, const float* beta,
                                 const float* in_chain, float pre_slope, float post_slope, int C, size_t V, double* partials,
                                 void* stream) {
  return dpi_bn_bwd_reduce_io(dy, x, mean_invstd, gamma, beta, in_chain, pre_slope, post_slope, C, V, partials, 0, stream);
}
extern "C" int dpi_bn_bwd_reduce_io(const float* dy, const float* x, const float* mean_invstd, const float* gamma, const float* beta,
                                    const float* in_chain, float pre_slope, float post_slope, int C, size_t V, double* partials,
                                    unsigned io, void* stream) {
  DPI_REQUIRE(dy && x && mean_invstd && partials && C > 0 && V > 0, "bn_bwd_reduce: bad argument");
  DPI_REQUIRE_IO(io, "bn_bwd_reduce");
  DPI_REQUIRE(!in_chain || pre_slope == 1.f, "bn_bwd_reduce: in_chain excludes pre_slope");
  const int nblk = dpi_stat_blocks(C, V);
  DPI_LAUNCH_FG(io, bn_bwd_reduce_kernel, dim3(nblk, C), (hipStream_t)stream, dy, x, mean_invstd, gamma, beta, in_chain, pre_slope, post_slope, C, V,
                nblk, partials);
  return dpi_check_launch("bn_bwd_reduce");
}

extern "C" int dpi_bn_bwd_apply(const float* dy, const float* x, const float* mean_invstd, const float* gamma, const float* beta,
                                const float* in_chain, float pre_slope, float post_slope, const double* partials, int nblk, int C,
                                size_t V, float* dx, float* dgamma, float* dbeta, void* stream) {
  return dpi_bn_bwd_apply_io(dy, x, mean_invstd, gamma, beta, in_chain, pre_slope, post_slope, partials, nblk, C, V, dx, dgamma, dbeta, 0, stream);
}
extern "C" int dpi_bn_bwd_apply_io(const float* dy, const float* x, const float* mean_invstd, const float* gamma, const float* beta,
                                   const float* in_chain, float pre_slope, float post_slope, const double* partials, int nblk, int C,
                                   size_t V, float* dx, float* dgamma, float* dbeta, unsigned io, void* stream) {
  DPI_REQUIRE(dy && x && mean_invstd && partials && dx && C > 0 && V > 0 && nblk > 0, "bn_bwd_apply: bad argument");
  DPI_REQUIRE_IO(io, "bn_bwd_apply");
  DPI_REQUIRE(!in_chain || pre_slope == 1.f, "bn_bwd_apply: in_chain excludes pre_slope");
  // every workgroup first re-reduces the phase-1 partials of its channel (nblk double pairs): keep >= 8 float4 per thread
  // behind that prologue instead of one
  unsigned gx = ew_blocks(cdivz(V, 4 * 8));
  DPI_LAUNCH_FG(io, bn_bwd_apply_kernel, dim3(gx, C), (hipStream_t)stream, dy, x, mean_invstd, gamma, beta, in_chain, pre_slope, post_slope, partials, nblk,
                C, V, dx, dgamma, dbeta);
  return dpi_check_launch("bn_bwd_apply");
}

extern "C" int dpi_bn_bwd_apply_fork(const float* dy, const float* x, const float* mean_invstd, const float* gamma, const float* beta,
                                     const float* in_chain, float pre_slope, float post_slope, const double* partials, int nblk, int C,
                                     size_t V, float* dx, float* dgamma, float* dbeta, const float* xa, const float* mi_a,
                                     const float* gamma_a, const float* beta_a, const float* chain_a, float post_a, double* partials_a,
                                     const float* xb, const float* mi_b, const float* gamma_b, const float* beta_b, const float* chain_b,
                                     float post_b, double* partials_b, void* stream) {
  return dpi_bn_bwd_apply_fork_io(dy, x, mean_invstd, gamma, beta, in_chain, pre_slope, post_slope, partials, nblk, C, V, dx, dgamma, dbeta,
                                  xa, mi_a, gamma_a, beta_a, chain_a, post_a, partials_a, xb, mi_b, gamma_b, beta_b, chain_b, post_b, partials_b, 0,
                                  stream);
}
extern "C" int dpi_bn_bwd_apply_fork_io(const float* dy, const float* x, const float* mean_invstd, const float* gamma, const float* beta,
                                        const float* in_chain, float pre_slope, float post_slope, const double* partials, int nblk, int C,
                                        size_t V, float* dx, float* dgamma, float* dbeta, const float* xa, const float* mi_a,
                                        const float* gamma_a, const float* beta_a, const float* chain_a, float post_a, double* partials_a,
                                        const float* xb, const float* mi_b, const float* gamma_b, const float* beta_b, const float* chain_b,
                                        float post_b, double* partials_b, unsigned io, void* stream) {
  DPI_REQUIRE(dy && x && mean_invstd && partials && dx && C > 0 && V > 0 && nblk > 0, "bn_bwd_apply_fork: bad argument");
  DPI_REQUIRE_IO(io, "bn_bwd_apply_fork");
  DPI_REQUIRE(!in_chain || pre_slope == 1.f, "bn_bwd_apply_fork: in_chain excludes pre_slope");
  DPI_REQUIRE((!xa || (mi_a && partials_a)) && (!xb || (mi_b && partials_b)), "bn_bwd_apply_fork: incomplete follow-up BatchNorm");
  const int nb = dpi_stat_blocks(C, V);
  const BnFork fa{xa, mi_a, gamma_a, beta_a, chain_a, post_a, partials_a}, fb{xb, mi_b, gamma_b, beta_b, chain_b, post_b, partials_b};
  DPI_LAUNCH_FG(io, bn_bwd_apply_fork_kernel, dim3(nb, C), (hipStream_t)stream, dy, x, mean_invstd, gamma, beta, in_chain, pre_slope, post_slope,
                partials, nblk, C, V, nb, dx, dgamma, dbeta, fa, fb);
  return dpi_check_launch("bn_bwd_apply_fork");
}

extern "C" int dpi_bn_bwd_apply_dual(const float* dy, int nblk, int C, size_t V, const float* xa, const float* mi_a, const float* gamma_a,
                                     const float* beta_a, const float* chain_a, float post_a, const double* partials_a, float* dxa,
                                     float* dgamma_a, float* dbeta_a, const float* xb, const float* mi_b, const float* gamma_b,
                                     const float* beta_b, const float* chain_b, float post_b, const double* partials_b, float* dxb,
                                     float* dgamma_b, float* dbeta_b, int f_lo, int f_hi, const float* f_mi, const float* f_gamma,
                                     const float* f_beta, float f_post, double* f_partials, void* stream) {
  return dpi_bn_bwd_apply_dual_io(dy, nblk, C, V, xa, mi_a, gamma_a, beta_a, chain_a, post_a, partials_a, dxa, dgamma_a, dbeta_a, xb, mi_b, gamma_b,
                                  beta_b, chain_b, post_b, partials_b, dxb, dgamma_b, dbeta_b, f_lo, f_hi, f_mi, f_gamma, f_beta, f_post, f_partials, 0,
                                  stream);
}
extern "C" int dpi_bn_bwd_apply_dual_io(const float* dy, int nblk, int C, size_t V, const float* xa, const float* mi_a, const float* gamma_a,
                                        const float* beta_a, const float* chain_a, float post_a, const double* partials_a, float* dxa,
                                        float* dgamma_a, float* dbeta_a, const float* xb, const float* mi_b, const float* gamma_b,
                                        const float* beta_b, const float* chain_b, float post_b, const double* partials_b, float* dxb,
                                        float* dgamma_b, float* dbeta_b, int f_lo, int f_hi, const float* f_mi, const float* f_gamma,
                                        const float* f_beta, float f_post, double* f_partials, unsigned io, void* stream) {
  DPI_REQUIRE(dy && xa && xb && mi_a && mi_b && partials_a && partials_b && dxa && dxb && C > 0 && V > 0 && nblk > 0,
              "bn_bwd_apply_dual: bad argument");
  DPI_REQUIRE_IO(io, "bn_bwd_apply_dual");
  DPI_REQUIRE(!f_partials || (f_mi && f_lo >= 0 && f_hi <= C && f_lo < f_hi), "bn_bwd_apply_dual: bad fork range");
  const int nb = dpi_stat_blocks(C, V);
  const BnSide A{xa, mi_a, gamma_a, beta_a, chain_a, post_a, partials_a, dxa, dgamma_a, dbeta_a};
  const BnSide B{xb, mi_b, gamma_b, beta_b, chain_b, post_b, partials_b, dxb, dgamma_b, dbeta_b};
  DPI_LAUNCH_FG(io, bn_bwd_apply_dual_kernel, dim3(nb, C), (hipStream_t)stream, dy, A, B, nblk, C, V, nb, f_lo, f_hi, f_mi, f_gamma, f_beta, f_post,
                f_partials);
  return dpi_check_launch("bn_bwd_apply_dual");
}

// ---- the residual join's BatchNorm backward in two passes (ABI 403; fp32 tensors) ---------------------------------------------------
// (blocks per channel: dpi_stat_blocks, as the two-sum passes.  Fewer, four times longer blocks — to amortise the 24-value reduction at a
//  block's end — measured SLOWER: 94.5 -> 99.8 us per launch on average.)
static int join_blocks(int C, size_t V) { return dpi_stat_blocks(C, V); }
extern "C" size_t dpi_join_bwd_ws_doubles(int C, size_t V) { return (size_t)join_blocks(C, V) * (size_t)C * kJoinSums; }
extern "C" int dpi_join_bwd(const float* dy, const float* t, const float* mi, const float* gamma, const float* beta, float pre, int C, size_t V,
                            const float* xa, const float* mi_a, const float* gamma_a, const float* beta_a, const float* chain_a, float post_a,
                            const float* xb, const float* mi_b, const float* gamma_b, const float* beta_b, const float* chain_b, float post_b,
                            const float* fwd_chain_a, const float* fwd_chain_b,
                            int f_lo, int f_hi, const float* f_mi, const float* f_gamma, const float* f_beta, float f_post,
                            double* ws, float* coef, float* dxa, float* dxb, float* dxf, float* dgb, float* dgb_f, unsigned io, void* stream) {
  DPI_REQUIRE(dy && mi && xa && xb && mi_a && mi_b && ws && coef && dxa && dxb && dgb && C > 0 && V > 0, "join_bwd: bad argument");
  DPI_REQUIRE_IO(io, "join_bwd");
  DPI_REQUIRE(t || (fwd_chain_a && fwd_chain_b), "join_bwd: without t the two forward chains that form it are needed");
  DPI_REQUIRE(f_lo >= 0 && f_hi <= C && f_lo <= f_hi, "join_bwd: bad fork range");
  DPI_REQUIRE(f_lo == f_hi || (f_mi && dxf && dgb_f), "join_bwd: the fork range needs its BatchNorm's statistics and outputs");
  const int nblk = join_blocks(C, V);
  const JoinSide A{xa, mi_a, gamma_a, beta_a, chain_a, post_a, fwd_chain_a}, B{xb, mi_b, gamma_b, beta_b, chain_b, post_b, fwd_chain_b};
  const JoinFork F{f_lo, f_hi, f_mi, f_gamma, f_beta, f_post};
  hipStream_t st = (hipStream_t)stream;
  DPI_LAUNCH_FG(io, join_bwd_sums_kernel, dim3(nblk, C), st, dy, t, mi, gamma, beta, pre, A, B, F, C, V, nblk, ws);
  join_bwd_coef_kernel<<<C, 64, 0, st>>>(ws, nblk, C, (double)V, mi_b, gamma_b, f_lo, f_hi, coef, dgb, dgb_f);
  DPI_LAUNCH_FG(io, join_bwd_apply_kernel, dim3(ew_blocks(cdivz(V, 4 * 8)), C), st, dy, t, mi, gamma, beta, pre, A, B, F, coef, C, V, dxa, dxb, dxf);   // (8 float4 per thread, as bn_bwd_apply)
  return dpi_check_launch("join_bwd");
}

extern "C" int dpi_chain_add_stats(const float* a, const float* chain_a, const float* b, const float* chain_b, int C, size_t V,
                                   float slope, float* t, double* partials, void* stream) {
  return dpi_chain_add_stats_io(a, chain_a, b, chain_b, C, V, slope, t, partials, 0, stream);
}
extern "C" int dpi_chain_add_stats_io(const float* a, const float* chain_a, const float* b, const float* chain_b, int C, size_t V,
                                      float slope, float* t, double* partials, unsigned io, void* stream) {
  DPI_REQUIRE(a && b && partials && C > 0 && V > 0, "chain_add_stats: bad argument");      // t == NULL: statistics only (ABI 403)
  DPI_REQUIRE_IO(io, "chain_add_stats");
  const int nblk = dpi_stat_blocks(C, V);
  if (DPI_FB(io)) chain_add_stats_kernel<true><<<dim3(nblk, C), 256, 0, (hipStream_t)stream>>>(a, chain_a, b, chain_b, C, V, nblk, slope, t, partials);
  else chain_add_stats_kernel<false><<<dim3(nblk, C), 256, 0, (hipStream_t)stream>>>(a, chain_a, b, chain_b, C, V, nblk, slope, t, partials);
  return dpi_check_launch("chain_add_stats");
}

extern "C" int dpi_chain_add_apply(const float* a, const float* chain_a, const float* b, const float* chain_b, const float* chain_out, int C,
                                   size_t V, float* y, unsigned io, void* stream) {
  DPI_REQUIRE(a && b && y && C > 0 && V > 0, "chain_add_apply: bad argument");
  DPI_REQUIRE_IO(io, "chain_add_apply");
  if (DPI_FB(io)) chain_add_apply_kernel<true><<<dim3(ew_blocks(cdivz(V, 4)), C), 256, 0, (hipStream_t)stream>>>(a, chain_a, b, chain_b, chain_out, V, y);
  else chain_add_apply_kernel<false><<<dim3(ew_blocks(cdivz(V, 4)), C), 256, 0, (hipStream_t)stream>>>(a, chain_a, b, chain_b, chain_out, V, y);
  return dpi_check_launch("chain_add_apply");
}

extern "C" int dpi_lrelu_bwd(const float* dy, const float* x, float slope, size_t n, float* dx, void* stream) {
  DPI_REQUIRE(dy && x && dx && n > 0, "lrelu_bwd: bad argument");
  lrelu_bwd_kernel<<<ew_blocks(cdivz(n, 4)), 256, 0, (hipStream_t)stream>>>(dy, x, slope, n, dx);
  return dpi_check_launch("lrelu_bwd");
}

extern "C" int dpi_act_fwd(const float* x, size_t n, int kind, float* y, void* stream) {
  DPI_REQUIRE(x && y && n > 0 && kind >= DPI_ACT_ELU && kind <= DPI_ACT_SIGMOID, "act_fwd: bad argument");
  act_fwd_kernel<<<ew_blocks(cdivz(n, 4)), 256, 0, (hipStream_t)stream>>>(x, n, kind, y);
  return dpi_check_launch("act_fwd");
}

extern "C" int dpi_act_bwd(const float* dy, const float* y, size_t n, int kind, float* dx, void* stream) {
  DPI_REQUIRE(dy && y && dx && n > 0 && kind >= DPI_ACT_ELU && kind <= DPI_ACT_SIGMOID, "act_bwd: bad argument");
  act_bwd_kernel<<<ew_blocks(cdivz(n, 4)), 256, 0, (hipStream_t)stream>>>(dy, y, n, kind, dx);
  return dpi_check_launch("act_bwd");
}

extern "C" int dpi_add(const float* a, const float* b, size_t n, float* y, void* stream) {
  DPI_REQUIRE(a && b && y && n > 0, "add: bad argument");
  add_kernel<<<ew_blocks(cdivz(n, 4)), 256, 0, (hipStream_t)stream>>>(a, b, n, y);
  return dpi_check_launch("add");
}

extern "C" int dpi_channel_sum(const float* x, int C, size_t V, double* ws, float* out, void* stream) {
  DPI_REQUIRE(x && ws && out && C > 0 && V > 0, "channel_sum: bad argument");
  const int nblk = dpi_stat_blocks(C, V);
  channel_stats_kernel<false><<<dim3(nblk, C), 256, 0, (hipStream_t)stream>>>(x, nullptr, C, V, nblk, ws);
  if (int e = dpi_check_launch("channel_sum.stats")) return e;
  channel_sum_final_kernel<<<C, 64, 0, (hipStream_t)stream>>>(ws, nblk, C, out);
  return dpi_check_launch("channel_sum.final");
}

extern "C" int dpi_upsample2x_fwd(const float* x, const float* chain, int C, int D, int H, int W, int Do, int Ho, int Wo,
                                  int linear, float* y, void* stream) {
  return dpi_upsample2x_fwd_io(x, chain, C, D, H, W, Do, Ho, Wo, linear, y, 0, stream);
}
extern "C" int dpi_upsample2x_fwd_io(const float* x, const float* chain, int C, int D, int H, int W, int Do, int Ho, int Wo,
                                     int linear, float* y, unsigned io, void* stream) {
  DPI_REQUIRE(x && y && C > 0 && D > 0 && H > 0 && W > 0, "upsample_fwd: bad argument");
  DPI_REQUIRE_IO(io, "upsample_fwd");
  const bool fb = DPI_FB(io);
  const int scale_d = !(D == 1 && Do == 1);
  DPI_REQUIRE(Do >= 1 && Ho >= 1 && Wo >= 1 && Do <= (scale_d ? 2 * D : 1) && Ho <= 2 * H && Wo <= 2 * W,
              "upsample_fwd: output (%d,%d,%d) exceeds 2x input (%d,%d,%d)", Do, Ho, Wo, D, H, W);
  const size_t Vo = (size_t)Do * Ho * Wo, V = (size_t)D * H * W;
  if (linear && H > 1 && W > 1 && (!scale_d || D > 1)) {
    if (scale_d) {
      if (fb) upsample_lin_fwd_cube_kernel<true, true, true><<<dim3(ew_blocks(V), C), 256, 0, (hipStream_t)stream>>>(x, chain, D, H, W, Do, Ho, Wo, y);
      else upsample_lin_fwd_cube_kernel<true, false, false><<<dim3(ew_blocks(V), C), 256, 0, (hipStream_t)stream>>>(x, chain, D, H, W, Do, Ho, Wo, y);
    } else {
      if (fb) upsample_lin_fwd_cube_kernel<false, true, true><<<dim3(ew_blocks(V), C), 256, 0, (hipStream_t)stream>>>(x, chain, D, H, W, Do, Ho, Wo, y);
      else upsample_lin_fwd_cube_kernel<false, false, false><<<dim3(ew_blocks(V), C), 256, 0, (hipStream_t)stream>>>(x, chain, D, H, W, Do, Ho, Wo, y);
    }
    return dpi_check_launch("upsample_lin_fwd_cube");
  }
  if (fb) upsample_fwd_kernel<true, true><<<dim3(ew_blocks(Vo), C), 256, 0, (hipStream_t)stream>>>(x, chain, D, H, W, Do, Ho, Wo, linear, scale_d, y);
  else upsample_fwd_kernel<false, false><<<dim3(ew_blocks(Vo), C), 256, 0, (hipStream_t)stream>>>(x, chain, D, H, W, Do, Ho, Wo, linear, scale_d, y);
  return dpi_check_launch("upsample_fwd");
}

extern "C" size_t dpi_upsample2x_bwd_ws_floats(int C, int D, int H, int W, int Do, int Ho, int Wo, int linear) {
  if (!linear || C <= 0) return 0;
  const int scale_d = !(D == 1 && Do == 1);
  return (size_t)C * Do * Ho * W + (scale_d ? (size_t)C * Do * H * W : 0);
}

extern "C" int dpi_upsample2x_bwd(const float* dy, int C, int D, int H, int W, int Do, int Ho, int Wo, int linear, float* dx,
                                  float* ws, void* stream) {
  return dpi_upsample2x_bwd_io(dy, C, D, H, W, Do, Ho, Wo, linear, dx, ws, 0, stream);
}
extern "C" int dpi_upsample2x_bwd_io(const float* dy, int C, int D, int H, int W, int Do, int Ho, int Wo, int linear, float* dx,
                                     float* ws, unsigned io, void* stream) {
  DPI_REQUIRE(dy && dx && C > 0 && D > 0 && H > 0 && W > 0, "upsample_bwd: bad argument");
  DPI_REQUIRE_IO(io, "upsample_bwd");
  const bool gb = DPI_GB(io);        // dy and dx; the workspace of the separable passes stays fp32
  const int scale_d = !(D == 1 && Do == 1);
  const size_t V = (size_t)D * H * W;
  if (linear && ws) {                                   // separable passes through the caller's workspace
    hipStream_t st = (hipStream_t)stream;
    float* t1 = ws;                                     // [C][Do][Ho][W]
    float* t2 = ws + (size_t)C * Do * Ho * W;           // [C][Do][H][W]
    // the axis kernel indexes one [n][inner] (output) / [no][inner] (input) slab and the slab count with 32 bits
    DPI_REQUIRE((size_t)C * Do * Ho < (1ull << 32) && (size_t)Do * Ho * Wo < (1ull << 31) && (size_t)Do * H * W < (1ull << 31),
                "upsample_bwd: %d x %d x %d x %d exceeds the 32-bit slab indexing of the separable adjoint", C, Do, Ho, Wo);
    auto launch = [&](const float* src, float* dst, size_t outer, int n, int no, size_t inner, bool ib, bool ob) {
      const unsigned gx = (unsigned)cdivz((size_t)n * inner, 256);
      // enough slabs per launch to fill the chip, each workgroup then strides over the rest
      size_t gy = outer < 65535 ? outer : 65535;
      while (gy > 1 && (size_t)gx * gy > 16384) gy = (gy + 1) / 2;
      const dim3 g(gx, (unsigned)gy);
      if (ib && ob) upsample_lin_bwd_axis_kernel<true, true><<<g, 256, 0, st>>>(src, dst, (unsigned)outer, n, no, (unsigned)inner);
      else if (ib) upsample_lin_bwd_axis_kernel<true, false><<<g, 256, 0, st>>>(src, dst, (unsigned)outer, n, no, (unsigned)inner);
      else if (ob) upsample_lin_bwd_axis_kernel<false, true><<<g, 256, 0, st>>>(src, dst, (unsigned)outer, n, no, (unsigned)inner);
      else upsample_lin_bwd_axis_kernel<false, false><<<g, 256, 0, st>>>(src, dst, (unsigned)outer, n, no, (unsigned)inner);
    };
    static const bool w2 = getenv("DPI_NO_UPW2") == nullptr;
    if (w2 && !gb && Wo == 2 * W && (W & 1) == 0 && (Wo & 3) == 0 && (((uintptr_t)dy | (uintptr_t)t1) & 15) == 0) {
      const size_t rows = (size_t)C * Do * Ho, pairs = rows * (size_t)(W / 2);
      upsample_lin_bwd_w2_kernel<<<ew_blocks(cdivz(pairs, 1)), 256, 0, st>>>(dy, t1, rows, W);
    } else
    launch(dy, t1, (size_t)C * Do * Ho, W, Wo, 1, gb, false);
    launch(t1, scale_d ? t2 : dx, (size_t)C * Do, H, Ho, W, false, scale_d ? false : gb);
    if (scale_d) launch(t2, dx, C, D, Do, (size_t)H * W, false, gb);
    return dpi_check_launch("upsample_lin_bwd_axis");
  }
  if (linear) {
    if (scale_d) {
      if (gb) upsample_lin_bwd_gather_kernel<true, true><<<dim3(ew_blocks(V), C), 256, 0, (hipStream_t)stream>>>(dy, D, H, W, Do, Ho, Wo, dx);
      else upsample_lin_bwd_gather_kernel<true, false><<<dim3(ew_blocks(V), C), 256, 0, (hipStream_t)stream>>>(dy, D, H, W, Do, Ho, Wo, dx);
    } else {
      if (gb) upsample_lin_bwd_gather_kernel<false, true><<<dim3(ew_blocks(V), C), 256, 0, (hipStream_t)stream>>>(dy, D, H, W, Do, Ho, Wo, dx);
      else upsample_lin_bwd_gather_kernel<false, false><<<dim3(ew_blocks(V), C), 256, 0, (hipStream_t)stream>>>(dy, D, H, W, Do, Ho, Wo, dx);
    }
    return dpi_check_launch("upsample_lin_bwd_gather");
  }
  if (gb) upsample_bwd_kernel<true><<<dim3(ew_blocks(V), C), 256, 0, (hipStream_t)stream>>>(dy, D, H, W, Do, Ho, Wo, linear, scale_d, dx);
  else upsample_bwd_kernel<false><<<dim3(ew_blocks(V), C), 256, 0, (hipStream_t)stream>>>(dy, D, H, W, Do, Ho, Wo, linear, scale_d, dx);
  return dpi_check_launch("upsample_bwd");
}

extern "C" int dpi_crop_copy(const float* x, int C, int D, int H, int W, int od, int oh, int ow, int Do, int Ho, int Wo, float* y,
                             void* stream) {
  DPI_REQUIRE(x && y && od >= 0 && oh >= 0 && ow >= 0 && od + Do <= D && oh + Ho <= H && ow + Wo <= W, "crop_copy: bad window");
  crop_copy_kernel<<<dim3(ew_blocks((size_t)Do * Ho * Wo), C), 256, 0, (hipStream_t)stream>>>(x, D, H, W, od, oh, ow, Do, Ho, Wo,
                                                                                            y, 0);
  return dpi_check_launch("crop_copy");
}

extern "C" int dpi_crop_copy_bwd(const float* dy, int C, int D, int H, int W, int od, int oh, int ow, int Do, int Ho, int Wo,
                                 float* dx, void* stream) {
  DPI_REQUIRE(dy && dx && od >= 0 && oh >= 0 && ow >= 0 && od + Do <= D && oh + Ho <= H && ow + Wo <= W, "crop_copy_bwd: bad window");
  crop_copy_kernel<<<dim3(ew_blocks((size_t)D * H * W), C), 256, 0, (hipStream_t)stream>>>(dy, D, H, W, od, oh, ow, Do, Ho, Wo, dx,
                                                                                         1);
  return dpi_check_launch("crop_copy_bwd");
}

extern "C" int dpi_fir_axis0(const float* x, const float* taps, int K, int C, int T, size_t S, float* y, void* stream) {
  DPI_REQUIRE(x && taps && y && K > 0 && (K & 1) && C > 0 && T > 0 && S > 0, "fir_axis0: bad argument (odd tap count required)");
  fir_axis0_kernel<<<dim3(ew_blocks((size_t)T * S), C), 256, 0, (hipStream_t)stream>>>(x, taps, K, T, S, y);
  return dpi_check_launch("fir_axis0");
}

extern "C" int dpi_axpy(float a, const float* x, size_t n, float* y, void* stream) {
  DPI_REQUIRE(x && y && n > 0, "axpy: bad argument");
  axpy_kernel<<<ew_blocks(n), 256, 0, (hipStream_t)stream>>>(a, x, n, y);
  return dpi_check_launch("axpy");
}
