// Grid-attention gate of the attention MultiRes-UNet (reference architectures/attention.py:107-113):
//   y[c][v] = x[c][v] * a[v],   a = upsample2x_linear(sigmoid(q)),   q one channel on the coarse grid (D, H, W).
// H and W are doubled, D only with scale_d (D = 1, scale_d = 0 is the 2-D case).  The C-channel gate tensor is never formed: a thread owns
// VW consecutive fine voxels, builds their gate values in registers from the coarse sigmoid and walks the channels with them.
//   forward     x read once, y written once                                                   (2 C V floats)
//   backward i  dy, x read once, dx = dy * a written once, t[v] = sum_c dy[c][v] * x[c][v]     (3 C V + V floats)
//   backward ii dq = (adjoint up-sampling of t) * s * (1 - s), a gather on the coarse grid    (no atomics: bitwise reproducible)
// VW (4, 2 or 1 floats per access) is chosen on the host from the ADDRESSES of the call: voxels are addressed by their flat index, the fine
// voxel count is a multiple of 4 and so is every channel stride, hence a view at any element offset is served, by the narrower variants.
// All variants evaluate the same expression per voxel and sum the channels in the same order: their results are bit-identical.
#include <initializer_list>
#include "common.h"

namespace {

struct GateGeo {
  int D, H, W;        // coarse grid of q / s
  int Do, Ho, Wo;     // fine grid of x / y: (scale_d ? 2 D : D, 2 H, 2 W)
};

template <int VW> struct VecT;
template <> struct VecT<1> { typedef float T; };
template <> struct VecT<2> { typedef dpi_f32x2 T; };
template <> struct VecT<4> { typedef dpi_f32x4v T; };

// a tensor this large does not survive in the caches until its next reader: stream it past them (the threshold and the measured gain of
// the streaming passes of elementwise.hip, kNtMinFloats there).  `nt` is wave-uniform.
constexpr size_t kGateNtMinFloats = (size_t)32 << 20;          // 128 MB

template <int VW, bool NT>
__device__ __forceinline__ void ldv(const float* __restrict__ p, float (&r)[VW]) {
  const typename VecT<VW>::T* q = reinterpret_cast<const typename VecT<VW>::T*>(p);
  typename VecT<VW>::T v;
  if constexpr (NT) v = __builtin_nontemporal_load(q); else v = *q;
  if constexpr (VW == 1) {
    r[0] = v;
  } else {
#pragma unroll
    for (int k = 0; k < VW; ++k) r[k] = v[k];
  }
}
template <int VW, bool NT>
__device__ __forceinline__ void stv(float* __restrict__ p, const float (&r)[VW]) {
  typename VecT<VW>::T v;
  if constexpr (VW == 1) {
    v = r[0];
  } else {
#pragma unroll
    for (int k = 0; k < VW; ++k) v[k] = r[k];
  }
  typename VecT<VW>::T* q = reinterpret_cast<typename VecT<VW>::T*>(p);
  if constexpr (NT) __builtin_nontemporal_store(v, q); else *q = v;
}

// the tri- / bi-linear blend of upsample_fwd_kernel (elementwise.hip): w innermost, then h, then d
template <bool SD>
__device__ __forceinline__ float gate_blend(float a0, float a1, float b0, float b1, float c0, float c1, float v000, float v001, float v010,
                                            float v011, float v100, float v101, float v110, float v111) {
  float r = a0 * (b0 * (c0 * v000 + c1 * v001) + b1 * (c0 * v010 + c1 * v011));
  if (SD) r += a1 * (b0 * (c0 * v100 + c1 * v101) + b1 * (c0 * v110 + c1 * v111));
  return r;
}

// gate values of the VW fine voxels i .. i + VW - 1 (i % VW == 0)
template <int VW, bool SD>
__device__ __forceinline__ void gate_group(const float* __restrict__ s, const GateGeo& g, unsigned i, float (&a)[VW]) {
  int ow = (int)(i % (unsigned)g.Wo);
  const unsigned r = i / (unsigned)g.Wo;
  int oh = (int)(r % (unsigned)g.Ho), od = (int)(r / (unsigned)g.Ho);
  if (VW > 1 && ow + VW <= g.Wo) {
    // one row, ow even (i and Wo are): the group reads the coarse columns ow/2 - 1 .. ow/2 + VW/2 (edge-clamped) of four coarse rows
    constexpr int NC = VW / 2 + 2;
    int d0, d1, h0, h1;
    float a0, a1, b0, b1;
    if (SD) lin_src(od, g.D, d0, d1, a0, a1); else { d0 = d1 = od; a0 = 1.f; a1 = 0.f; }
    lin_src(oh, g.H, h0, h1, b0, b1);
    const float* __restrict__ r00 = s + ((size_t)d0 * g.H + h0) * g.W;
    const float* __restrict__ r01 = s + ((size_t)d0 * g.H + h1) * g.W;
    const float* __restrict__ r10 = s + ((size_t)d1 * g.H + h0) * g.W;
    const float* __restrict__ r11 = s + ((size_t)d1 * g.H + h1) * g.W;
    float v00[NC], v01[NC], v10[NC], v11[NC];
#pragma unroll
    for (int k = 0; k < NC; ++k) {
      const int col = min(max((ow >> 1) - 1 + k, 0), g.W - 1);
      v00[k] = r00[col];
      v01[k] = r01[col];
      v10[k] = SD ? r10[col] : 0.f;
      v11[k] = SD ? r11[col] : 0.f;
    }
#pragma unroll
    for (int j = 0; j < VW; ++j) {
      // lin_src of output column ow + j on these columns: even -> (k, k + 1) = (j/2, j/2 + 1), odd -> ((j+1)/2, (j+1)/2 + 1)
      const int k = (j + 1) >> 1;
      const bool first = ((ow + j) >> 1) == 0;
      const float c0 = (j & 1) ? .75f : (first ? 0.f : .25f), c1 = (j & 1) ? .25f : (first ? 1.f : .75f);
      a[j] = gate_blend<SD>(a0, a1, b0, b1, c0, c1, v00[k], v00[k + 1], v01[k], v01[k + 1], v10[k], v10[k + 1], v11[k], v11[k + 1]);
    }
  } else {
    // voxel by voxel (VW = 1, or a group that runs over the end of a row when Wo % VW != 0)
#pragma unroll
    for (int j = 0; j < VW; ++j) {
      int d0, d1, h0, h1, w0, w1;
      float a0, a1, b0, b1, c0, c1;
      if (SD) lin_src(od, g.D, d0, d1, a0, a1); else { d0 = d1 = od; a0 = 1.f; a1 = 0.f; }
      lin_src(oh, g.H, h0, h1, b0, b1);
      lin_src(ow, g.W, w0, w1, c0, c1);
      const float* __restrict__ r00 = s + ((size_t)d0 * g.H + h0) * g.W;
      const float* __restrict__ r01 = s + ((size_t)d0 * g.H + h1) * g.W;
      const float* __restrict__ r10 = s + ((size_t)d1 * g.H + h0) * g.W;
      const float* __restrict__ r11 = s + ((size_t)d1 * g.H + h1) * g.W;
      a[j] = gate_blend<SD>(a0, a1, b0, b1, c0, c1, r00[w0], r00[w1], r01[w0], r01[w1], SD ? r10[w0] : 0.f, SD ? r10[w1] : 0.f,
                            SD ? r11[w0] : 0.f, SD ? r11[w1] : 0.f);
      if (++ow == g.Wo) {
        ow = 0;
        if (++oh == g.Ho) { oh = 0; ++od; }
      }
    }
  }
}

__global__ __launch_bounds__(256) void attn_sigmoid_kernel(const float* __restrict__ q, unsigned n, float* __restrict__ s) {
  for (unsigned i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) s[i] = 1.f / (1.f + expf(-q[i]));
}

// the channel walk of one group, with or without the non-temporal hint (a run-time select between the two loads loses the hint)
template <int VW, bool NT>
__device__ __forceinline__ void gate_fwd_channels(const float* __restrict__ x, float* __restrict__ y, int C, unsigned V, const float (&a)[VW]) {
#pragma unroll 4
  for (int c = 0; c < C; ++c) {
    float v[VW];
    ldv<VW, NT>(x + (size_t)c * V, v);
#pragma unroll
    for (int k = 0; k < VW; ++k) v[k] *= a[k];
    stv<VW, NT>(y + (size_t)c * V, v);
  }
}

template <int VW, bool SD>
__global__ __launch_bounds__(256) void attn_gate_fwd_kernel(const float* __restrict__ x, const float* __restrict__ s, int C, GateGeo g,
                                                            unsigned V, float* __restrict__ y) {
  const unsigned ngroups = V / VW;
  const bool nt = (size_t)C * V >= kGateNtMinFloats;
  for (unsigned gi = blockIdx.x * 256 + threadIdx.x; gi < ngroups; gi += gridDim.x * 256) {
    const unsigned i = gi * VW;
    float a[VW];
    gate_group<VW, SD>(s, g, i, a);
    if (nt) gate_fwd_channels<VW, true>(x + i, y + i, C, V, a);
    else gate_fwd_channels<VW, false>(x + i, y + i, C, V, a);
  }
}

// backward, pass i: dx = dy * a and the channel sum t[v] = sum_c dy[c][v] * x[c][v] (c ascending, one fma per channel)
template <int VW, bool NT>
__device__ __forceinline__ void gate_bwd_channels(const float* __restrict__ dy, const float* __restrict__ x, float* __restrict__ dx, int C,
                                                  unsigned V, const float (&a)[VW], float (&acc)[VW]) {
#pragma unroll 4
  for (int c = 0; c < C; ++c) {
    float gv[VW], xv[VW];
    ldv<VW, NT>(dy + (size_t)c * V, gv);
    ldv<VW, NT>(x + (size_t)c * V, xv);
#pragma unroll
    for (int k = 0; k < VW; ++k) {
      acc[k] = fmaf(gv[k], xv[k], acc[k]);
      gv[k] *= a[k];
    }
    stv<VW, NT>(dx + (size_t)c * V, gv);
  }
}

template <int VW, bool SD>
__global__ __launch_bounds__(256) void attn_gate_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                            const float* __restrict__ s, int C, GateGeo g, unsigned V,
                                                            float* __restrict__ dx, float* __restrict__ t) {
  const unsigned ngroups = V / VW;
  const bool nt = (size_t)C * V >= kGateNtMinFloats;
  for (unsigned gi = blockIdx.x * 256 + threadIdx.x; gi < ngroups; gi += gridDim.x * 256) {
    const unsigned i = gi * VW;
    float a[VW], acc[VW];
    gate_group<VW, SD>(s, g, i, a);
#pragma unroll
    for (int k = 0; k < VW; ++k) acc[k] = 0.f;
    if (nt) gate_bwd_channels<VW, true>(dy + i, x + i, dx + i, C, V, a, acc);
    else gate_bwd_channels<VW, false>(dy + i, x + i, dx + i, C, V, a, acc);
    stv<VW, false>(t + i, acc);          // read next by pass ii
  }
}

// backward, pass ii: one thread per coarse voxel gathers the 4 x 4 (x 4) fine neighbourhood of t that read it (the taps and summation
// order of upsample_lin_bwd_gather_kernel), then the sigmoid's derivative
template <bool SD>
__global__ __launch_bounds__(256) void attn_gate_bwd_q_kernel(const float* __restrict__ t, const float* __restrict__ s, GateGeo g,
                                                              unsigned Vc, float* __restrict__ dq) {
  for (unsigned i = blockIdx.x * 256 + threadIdx.x; i < Vc; i += gridDim.x * 256) {
    const int w = (int)(i % (unsigned)g.W);
    const unsigned r = i / (unsigned)g.W;
    const int h = (int)(r % (unsigned)g.H), d = (int)(r / (unsigned)g.H);
    int ow[4], oh[4], od[4];
    float ww[4], wh[4], wd[4];
    lin_bwd_taps(w, g.W, g.Wo, ow, ww);
    lin_bwd_taps(h, g.H, g.Ho, oh, wh);
    if (SD) lin_bwd_taps(d, g.D, g.Do, od, wd);
    float acc = 0.f;
#pragma unroll
    for (int a = 0; a < (SD ? 4 : 1); ++a) {
      const int od_ = SD ? od[a] : d;
      const float wa = SD ? wd[a] : 1.f;
      float accd = 0.f;
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const float* __restrict__ row = t + ((size_t)od_ * g.Ho + oh[b]) * g.Wo;
        const float rsum = ww[0] * row[ow[0]] + ww[1] * row[ow[1]] + ww[2] * row[ow[2]] + ww[3] * row[ow[3]];
        accd = fmaf(wh[b], rsum, accd);
      }
      acc = fmaf(wa, accd, acc);
    }
    const float sv = s[i];
    dq[i] = acc * sv * (1.f - sv);
  }
}

// Guideline 11 of the kernel guide: memory-bound, 256-thread blocks, at most 2048 of them, grid-stride for the rest
inline unsigned gate_blocks(size_t threads) {
  size_t b = cdivz(threads, 256);
  if (b > 2048) b = 2048;
  if (b < 1) b = 1;
  return (unsigned)b;
}

// floats per access that every one of the given addresses allows (the fine voxel count V is a multiple of 4: so is every channel stride)
inline int gate_vec_width(size_t V, std::initializer_list<const void*> ptrs) {
  uintptr_t bits = 0;
  for (const void* p : ptrs) bits |= reinterpret_cast<uintptr_t>(p);
  if (!(bits & 15u) && V % 4 == 0) return 4;
  if (!(bits & 7u) && V % 2 == 0) return 2;
  return 1;
}

inline bool gate_geo(int C, int D, int H, int W, int scale_d, GateGeo* g, size_t* V) {
  if (C <= 0 || D <= 0 || H <= 0 || W <= 0 || (scale_d != 0 && scale_d != 1)) return false;
  const size_t Do = scale_d ? 2 * (size_t)D : (size_t)D, Ho = 2 * (size_t)H, Wo = 2 * (size_t)W;
  if (Do >= (1u << 30) || Ho >= (1u << 30) || Wo >= (1u << 30)) return false;
  const size_t v = Do * Ho * Wo;
  if (Do * Ho >= (1ull << 31) || v >= (1ull << 31)) return false;        // 32-bit voxel indices in the kernels
  *g = GateGeo{D, H, W, (int)Do, (int)Ho, (int)Wo};
  *V = v;
  return true;
}

inline bool aligned4(std::initializer_list<const void*> ptrs) {
  for (const void* p : ptrs)
    if (reinterpret_cast<uintptr_t>(p) & 3u) return false;
  return true;
}

#define DPI_GATE_LAUNCH(KERNEL, vw, sd, GRID, ST, ...)                                      \
  do {                                                                                      \
    if ((vw) == 4) {                                                                        \
      if (sd) KERNEL<4, true><<<GRID, 256, 0, ST>>>(__VA_ARGS__);                           \
      else KERNEL<4, false><<<GRID, 256, 0, ST>>>(__VA_ARGS__);                             \
    } else if ((vw) == 2) {                                                                 \
      if (sd) KERNEL<2, true><<<GRID, 256, 0, ST>>>(__VA_ARGS__);                           \
      else KERNEL<2, false><<<GRID, 256, 0, ST>>>(__VA_ARGS__);                             \
    } else {                                                                                \
      if (sd) KERNEL<1, true><<<GRID, 256, 0, ST>>>(__VA_ARGS__);                           \
      else KERNEL<1, false><<<GRID, 256, 0, ST>>>(__VA_ARGS__);                             \
    }                                                                                       \
  } while (0)

}  // namespace

extern "C" int dpi_attn_gate_fwd(const float* x, const float* q, int C, int D, int H, int W, int scale_d, float* s_out, float* y,
                                 void* stream) {
  GateGeo g;
  size_t V;
  DPI_REQUIRE(x && q && s_out && y, "attn_gate_fwd: NULL tensor");
  DPI_REQUIRE(gate_geo(C, D, H, W, scale_d, &g, &V), "attn_gate_fwd: bad geometry C = %d, coarse %d x %d x %d, scale_d = %d (the fine grid must stay below 2^31 voxels)",
              C, D, H, W, scale_d);
  DPI_REQUIRE(aligned4({x, q, s_out, y}), "attn_gate_fwd: a tensor is not aligned to its fp32 element");
  DPI_REQUIRE(q != s_out && x != y, "attn_gate_fwd: not an in-place operation");
  const hipStream_t st = (hipStream_t)stream;
  const unsigned Vc = (unsigned)((size_t)D * H * W);
  attn_sigmoid_kernel<<<gate_blocks(Vc), 256, 0, st>>>(q, Vc, s_out);
  const int vw = gate_vec_width(V, {x, y});
  DPI_GATE_LAUNCH(attn_gate_fwd_kernel, vw, scale_d != 0, gate_blocks(V / vw), st, x, s_out, C, g, (unsigned)V, y);
  return dpi_check_launch("attn_gate_fwd");
}

extern "C" size_t dpi_attn_gate_bwd_ws_floats(int C, int D, int H, int W, int scale_d) {
  GateGeo g;
  size_t V;
  return gate_geo(C, D, H, W, scale_d, &g, &V) ? V : 0;
}

extern "C" int dpi_attn_gate_bwd(const float* dy, const float* x, const float* s, int C, int D, int H, int W, int scale_d, float* dx,
                                 float* dq, float* ws, void* stream) {
  GateGeo g;
  size_t V;
  DPI_REQUIRE(dy && x && s && dx && dq && ws, "attn_gate_bwd: NULL tensor");
  DPI_REQUIRE(gate_geo(C, D, H, W, scale_d, &g, &V), "attn_gate_bwd: bad geometry C = %d, coarse %d x %d x %d, scale_d = %d (the fine grid must stay below 2^31 voxels)",
              C, D, H, W, scale_d);
  DPI_REQUIRE(aligned4({dy, x, s, dx, dq, ws}), "attn_gate_bwd: a tensor is not aligned to its fp32 element");
  DPI_REQUIRE(dx != x && dq != s && ws != dx && ws != dy && ws != x, "attn_gate_bwd: outputs and workspace must not alias the inputs");
  const hipStream_t st = (hipStream_t)stream;
  const int vw = gate_vec_width(V, {dy, x, dx, ws});
  DPI_GATE_LAUNCH(attn_gate_bwd_kernel, vw, scale_d != 0, gate_blocks(V / vw), st, dy, x, s, C, g, (unsigned)V, dx, ws);
  const unsigned Vc = (unsigned)((size_t)D * H * W);
  if (scale_d) attn_gate_bwd_q_kernel<true><<<gate_blocks(Vc), 256, 0, st>>>(ws, s, g, Vc, dq);
  else attn_gate_bwd_q_kernel<false><<<gate_blocks(Vc), 256, 0, st>>>(ws, s, g, Vc, dq);
  return dpi_check_launch("attn_gate_bwd");
}
