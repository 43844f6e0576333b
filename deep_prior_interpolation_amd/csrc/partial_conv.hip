// Partial convolution of --net part (reference architectures/partial_unet.py:42-80, 119-157): everything around the 3x3(x3) convolution, which
// stays the existing launch on xm.
//   mask fwd  xm[c][v] = x[c][v] * m[c][v],  msum[v] = sum_c m[c][v]                              (3 Cin V + V floats; Cm = 1: 2 Cin V + 2 V)
//   norm fwd  S[v] = 3x3(x3) zero-padded box sum of msum;  y[o][v] = S == 0 ? 0 : c[o][v] / S[v] + b[o];  new_mask[v] = S != 0
//                                                                                                 (2 Cout V + 3 V floats, 27 msum reads by cache)
//   norm bwd  dc[o][v] = S == 0 ? 0 : dy[o][v] / S[v];  db[o] = sum over S != 0 of dy[o][v]         (2 Cout V + V floats)
//   mask bwd  dx[c][v] = dxm[c][v] * m[c][v];  dm[c][v] = dxm[c][v] * x[c][v]  or  dm[v] = sum_c dxm[c][v] * x[c][v]   (Cm = 1)
// The mask m has Cm = Cin channels or one that is broadcast; S is not differentiated (the reference computes it under no_grad).
// A thread owns FOUR consecutive voxels (flat index) and walks the channels with them.  The host chooses the ACCESS width — 16, 8 or 4 bytes —
// from the addresses of the call and from V (a channel stride of V floats keeps 16-byte alignment only for V % 4 == 0), so a view at any element
// offset and any voxel count are served.  Which voxels a thread owns, the expression per voxel and every summation order are the same for the
// three widths: their results are bit-identical, the bias gradient included.  No atomics: wave partials in a fixed order, then a finaliser.
#include <initializer_list>
#include "common.h"

namespace {

struct BoxGeo {
  int D, H, W;
};

// as kGateNtMinFloats of attention_gate.hip: a tensor this large does not survive in the caches until its next reader
constexpr size_t kPcNtMinFloats = (size_t)32 << 20;          // 128 MB

// n of the 4 voxels at p are inside the tensor (n = 4 for AW = 4, even for AW = 2); the others read as 0 and are not stored
template <int AW, bool NT>
__device__ __forceinline__ void ld4(const float* p, int n, float (&r)[4]) {
  if constexpr (AW == 4) {
    const dpi_f32x4v* q = reinterpret_cast<const dpi_f32x4v*>(p);
    dpi_f32x4v v;
    if constexpr (NT) v = __builtin_nontemporal_load(q); else v = *q;
    r[0] = v[0]; r[1] = v[1]; r[2] = v[2]; r[3] = v[3];
  } else if constexpr (AW == 2) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      r[2 * h] = r[2 * h + 1] = 0.f;
      if (2 * h < n) {
        const dpi_f32x2* q = reinterpret_cast<const dpi_f32x2*>(p) + h;
        dpi_f32x2 v;
        if constexpr (NT) v = __builtin_nontemporal_load(q); else v = *q;
        r[2 * h] = v[0]; r[2 * h + 1] = v[1];
      }
    }
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      r[k] = 0.f;
      if (k < n) {
        if constexpr (NT) r[k] = __builtin_nontemporal_load(p + k); else r[k] = p[k];
      }
    }
  }
}
template <int AW, bool NT>
__device__ __forceinline__ void st4(float* p, int n, const float (&r)[4]) {
  if constexpr (AW == 4) {
    const dpi_f32x4v v = {r[0], r[1], r[2], r[3]};
    dpi_f32x4v* q = reinterpret_cast<dpi_f32x4v*>(p);
    if constexpr (NT) __builtin_nontemporal_store(v, q); else *q = v;
  } else if constexpr (AW == 2) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      if (2 * h < n) {
        const dpi_f32x2 v = {r[2 * h], r[2 * h + 1]};
        dpi_f32x2* q = reinterpret_cast<dpi_f32x2*>(p) + h;
        if constexpr (NT) __builtin_nontemporal_store(v, q); else *q = v;
      }
    }
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (k < n) {
        if constexpr (NT) __builtin_nontemporal_store(r[k], p + k); else p[k] = r[k];
      }
    }
  }
}

__device__ __forceinline__ int group_count(unsigned i, unsigned V) { return (int)min(4u, V - i); }

// ---------------------------------------------------------------- mask forward ----------------------------------------------------------
template <int AW, bool NT>
__device__ __forceinline__ void mask_fwd_channels(const float* x, const float* m, float* xm, int Cin, bool per_channel, unsigned V, int n,
                                                  float (&acc)[4]) {
  float mv[4];
  if (!per_channel) ld4<AW, false>(m, n, mv);
#pragma unroll 4
  for (int c = 0; c < Cin; ++c) {
    float xv[4];
    ld4<AW, NT>(x + (size_t)c * V, n, xv);
    if (per_channel) ld4<AW, NT>(m + (size_t)c * V, n, mv);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      xv[k] *= mv[k];
      acc[k] += mv[k];                     // c ascending (Cm = 1: replaced by Cin * m below)
    }
    st4<AW, false>(xm + (size_t)c * V, n, xv);          // read next by the convolution
  }
  if (!per_channel) {
#pragma unroll
    for (int k = 0; k < 4; ++k) acc[k] = (float)Cin * mv[k];
  }
}

template <int AW>
__global__ __launch_bounds__(256) void pconv_mask_fwd_kernel(const float* x, const float* m, int Cin, int Cm, unsigned V, float* xm,
                                                             float* __restrict__ msum) {
  const unsigned ngroups = (V + 3) / 4;
  const bool nt = (size_t)Cin * V >= kPcNtMinFloats;
  for (unsigned gi = blockIdx.x * 256 + threadIdx.x; gi < ngroups; gi += gridDim.x * 256) {
    const unsigned i = gi * 4;
    const int n = group_count(i, V);
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    if (nt) mask_fwd_channels<AW, true>(x + i, m + i, xm + i, Cin, Cm != 1, V, n, acc);
    else mask_fwd_channels<AW, false>(x + i, m + i, xm + i, Cin, Cm != 1, V, n, acc);
    st4<AW, false>(msum + i, n, acc);
  }
}

// ---------------------------------------------------------------- S: the box sum of msum -------------------------------------------------
// 27 additions per voxel in the order d, h, w ascending, a tap outside the volume adding 0 (D = 1: the 3 x 3 window).  The row path (the four
// voxels in one row) reads 6 columns of each of the 9 rows once and adds them in the same order as the voxel-by-voxel path.
__device__ __forceinline__ void box_sums(const float* __restrict__ msum, const BoxGeo& g, unsigned i, int n, float (&S)[4]) {
  int w = (int)(i % (unsigned)g.W);
  const unsigned r = i / (unsigned)g.W;
  int h = (int)(r % (unsigned)g.H), d = (int)(r / (unsigned)g.H);
#pragma unroll
  for (int k = 0; k < 4; ++k) S[k] = 0.f;
  if (n == 4 && w + 4 <= g.W) {
#pragma unroll
    for (int dd = -1; dd <= 1; ++dd) {
#pragma unroll
      for (int dh = -1; dh <= 1; ++dh) {
        const int zd = d + dd, zh = h + dh;
        const bool rowok = zd >= 0 && zd < g.D && zh >= 0 && zh < g.H;
        const float* __restrict__ row = msum + ((size_t)(rowok ? zd : d) * g.H + (rowok ? zh : h)) * g.W;
        float v[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) {
          const int col = w - 1 + k;
          const bool ok = rowok && col >= 0 && col < g.W;
          v[k] = ok ? row[ok ? col : w] : 0.f;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          S[j] += v[j];
          S[j] += v[j + 1];
          S[j] += v[j + 2];
        }
      }
    }
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (j >= n) break;
      float acc = 0.f;
#pragma unroll
      for (int dd = -1; dd <= 1; ++dd) {
#pragma unroll
        for (int dh = -1; dh <= 1; ++dh) {
          const int zd = d + dd, zh = h + dh;
          const bool rowok = zd >= 0 && zd < g.D && zh >= 0 && zh < g.H;
          const float* __restrict__ row = msum + ((size_t)(rowok ? zd : d) * g.H + (rowok ? zh : h)) * g.W;
#pragma unroll
          for (int dw = -1; dw <= 1; ++dw) {
            const int col = w + dw;
            const bool ok = rowok && col >= 0 && col < g.W;
            acc += ok ? row[ok ? col : w] : 0.f;
          }
        }
      }
      S[j] = acc;
      if (++w == g.W) {
        w = 0;
        if (++h == g.H) { h = 0; ++d; }
      }
    }
  }
}

// ---------------------------------------------------------------- normalisation forward --------------------------------------------------
// y may be c itself: a thread reads its four voxels of a channel before it writes them
template <int AW, bool NT>
__device__ __forceinline__ void norm_fwd_channels(const float* c, const float* __restrict__ bias, float* y, int Cout, unsigned V, int n,
                                                  const float (&S)[4]) {
#pragma unroll 4
  for (int o = 0; o < Cout; ++o) {
    float v[4];
    ld4<AW, NT>(c + (size_t)o * V, n, v);
    const float b = bias ? bias[o] : 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = S[k] == 0.f ? 0.f : v[k] / S[k] + b;
    st4<AW, NT>(y + (size_t)o * V, n, v);
  }
}

template <int AW>
__global__ __launch_bounds__(256) void pconv_norm_fwd_kernel(const float* c, const float* __restrict__ msum, const float* __restrict__ bias,
                                                             int Cout, BoxGeo g, unsigned V, float* y, float* __restrict__ new_mask,
                                                             float* __restrict__ S_out) {
  const unsigned ngroups = (V + 3) / 4;
  const bool nt = (size_t)Cout * V >= kPcNtMinFloats;
  for (unsigned gi = blockIdx.x * 256 + threadIdx.x; gi < ngroups; gi += gridDim.x * 256) {
    const unsigned i = gi * 4;
    const int n = group_count(i, V);
    float S[4], nm[4];
    box_sums(msum, g, i, n, S);
#pragma unroll
    for (int k = 0; k < 4; ++k) nm[k] = S[k] == 0.f ? 0.f : 1.f;
    st4<AW, false>(S_out + i, n, S);
    st4<AW, false>(new_mask + i, n, nm);
    if (nt) norm_fwd_channels<AW, true>(c + i, bias, y + i, Cout, V, n, S);
    else norm_fwd_channels<AW, false>(c + i, bias, y + i, Cout, V, n, S);
  }
}

// ---------------------------------------------------------------- normalisation backward -------------------------------------------------
// One group per thread, no grid stride: wave w of the launch owns voxels [256 w, 256 w + 256) whatever the access width, and its partial of the
// bias gradient — the four voxels of a lane added in order, then the butterfly over the lanes — goes to part[o][w].  The channels go four at a
// time by hand: a loop that holds the wave reduction cannot be unrolled with a remainder by the compiler.  A lane past the last group reads
// group 0 (valid addresses), adds nothing and stores nothing, so the reduction always runs with every lane.
template <int AW, bool NT, bool DB>
__device__ __forceinline__ void norm_bwd_channels(const float* dy, float* dc, int Cout, unsigned V, int n, bool active, const float (&S)[4],
                                                  float* __restrict__ part_row, unsigned nrows) {
  const int lane = threadIdx.x & 63;
  for (int o0 = 0; o0 < Cout; o0 += 4) {
    float v[4][4], s[4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (o0 + j < Cout) ld4<AW, NT>(dy + (size_t)(o0 + j) * V, n, v[j]);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      s[j] = 0.f;
      if (o0 + j < Cout) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const bool hole = S[k] == 0.f;
          s[j] += hole ? 0.f : v[j][k];
          v[j][k] = hole ? 0.f : v[j][k] / S[k];
        }
        if (active) st4<AW, false>(dc + (size_t)(o0 + j) * V, n, v[j]);         // read next by the backward convolutions
      }
    }
    if (DB) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float t = wave_sum(active ? s[j] : 0.f);
        if (lane == 0 && o0 + j < Cout) part_row[(size_t)(o0 + j) * nrows] = t;
      }
    }
  }
}

template <int AW, bool DB>
__global__ __launch_bounds__(256) void pconv_norm_bwd_kernel(const float* dy, const float* __restrict__ S_in, int Cout, unsigned V, float* dc,
                                                             float* __restrict__ part) {
  const unsigned ngroups = (V + 3) / 4;
  const unsigned gi = blockIdx.x * 256 + threadIdx.x;
  const bool active = gi < ngroups;
  const unsigned i = active ? gi * 4 : 0;
  const int n = group_count(i, V);
  const bool nt = (size_t)Cout * V >= kPcNtMinFloats;
  float S[4];
  ld4<AW, false>(S_in + i, n, S);
  const unsigned nrows = gridDim.x * 4;
  float* part_row = DB ? part + (gi >> 6) : nullptr;
  if (nt) norm_bwd_channels<AW, true, DB>(dy + i, dc + i, Cout, V, n, active, S, part_row, nrows);
  else norm_bwd_channels<AW, false, DB>(dy + i, dc + i, Cout, V, n, active, S, part_row, nrows);
}

// db[o] = the sum of row o of part[Cout][nrows]: thread t adds the partials t, t + 256, ... in ascending order, then a fixed tree over the threads
__global__ __launch_bounds__(256) void pconv_bias_final_kernel(const float* __restrict__ part, unsigned nrows, float* __restrict__ db) {
  __shared__ float sh[256];
  const float* __restrict__ row = part + (size_t)blockIdx.x * nrows;
  float s = 0.f;
  for (unsigned r = threadIdx.x; r < nrows; r += 256) s += row[r];
  sh[threadIdx.x] = s;
  __syncthreads();
#pragma unroll
  for (int k = 128; k > 0; k >>= 1) {
    if ((int)threadIdx.x < k) sh[threadIdx.x] += sh[threadIdx.x + k];
    __syncthreads();
  }
  if (threadIdx.x == 0) db[blockIdx.x] = sh[0];
}

// ---------------------------------------------------------------- mask backward ----------------------------------------------------------
// dx may be dxm itself.  DM: 0 none, 1 per channel (Cm = Cin), 2 the channel sum (Cm = 1; c ascending, one fma per channel)
template <int AW, bool NT, int DM>
__device__ __forceinline__ void mask_bwd_channels(const float* dxm, const float* x, const float* m, float* dx, float* dm, int Cin,
                                                  bool per_channel, unsigned V, int n, float (&acc)[4]) {
  float mv[4];
  if (!per_channel) ld4<AW, false>(m, n, mv);
#pragma unroll 4
  for (int c = 0; c < Cin; ++c) {
    float gv[4], xv[4];
    ld4<AW, NT>(dxm + (size_t)c * V, n, gv);
    if (per_channel) ld4<AW, NT>(m + (size_t)c * V, n, mv);
    if (DM) {
      ld4<AW, NT>(x + (size_t)c * V, n, xv);
      if (DM == 1) {
#pragma unroll
        for (int k = 0; k < 4; ++k) xv[k] *= gv[k];
        st4<AW, NT>(dm + (size_t)c * V, n, xv);
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[k] = fmaf(gv[k], xv[k], acc[k]);
      }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) gv[k] *= mv[k];
    st4<AW, NT>(dx + (size_t)c * V, n, gv);
  }
}

template <int AW, int DM>
__global__ __launch_bounds__(256) void pconv_mask_bwd_kernel(const float* dxm, const float* x, const float* m, int Cin, int Cm, unsigned V,
                                                             float* dx, float* dm) {
  const unsigned ngroups = (V + 3) / 4;
  const bool nt = (size_t)Cin * V >= kPcNtMinFloats;
  for (unsigned gi = blockIdx.x * 256 + threadIdx.x; gi < ngroups; gi += gridDim.x * 256) {
    const unsigned i = gi * 4;
    const int n = group_count(i, V);
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    const float* xi = DM ? x + i : nullptr;
    float* dmi = DM == 1 ? dm + i : nullptr;
    if (nt) mask_bwd_channels<AW, true, DM>(dxm + i, xi, m + i, dx + i, dmi, Cin, Cm != 1, V, n, acc);
    else mask_bwd_channels<AW, false, DM>(dxm + i, xi, m + i, dx + i, dmi, Cin, Cm != 1, V, n, acc);
    if (DM == 2) st4<AW, false>(dm + i, n, acc);
  }
}

// ---------------------------------------------------------------- host side --------------------------------------------------------------
inline unsigned pc_blocks(size_t groups) {            // Guideline 11 of the kernel guide, as gate_blocks of attention_gate.hip
  size_t b = cdivz(groups, 256);
  if (b > 2048) b = 2048;
  if (b < 1) b = 1;
  return (unsigned)b;
}

// bytes per access / 4 that every address of the call allows; a channel stride of V floats keeps the alignment only if V divides likewise
inline int pc_access_width(size_t V, std::initializer_list<const void*> ptrs) {
  uintptr_t bits = 0;
  for (const void* p : ptrs) bits |= reinterpret_cast<uintptr_t>(p);
  if (!(bits & 15u) && V % 4 == 0) return 4;
  if (!(bits & 7u) && V % 2 == 0) return 2;
  return 1;
}

inline bool pc_aligned4(std::initializer_list<const void*> ptrs) {
  for (const void* p : ptrs)
    if (reinterpret_cast<uintptr_t>(p) & 3u) return false;
  return true;
}

inline bool pc_voxels(size_t V) { return V > 0 && V < (1ull << 31); }          // 32-bit voxel indices in the kernels

inline bool pc_geo(int D, int H, int W, BoxGeo* g, size_t* V) {
  if (D <= 0 || H <= 0 || W <= 0) return false;
  const size_t v = (size_t)D * H * W;
  if ((size_t)D * H >= (1ull << 31) || !pc_voxels(v)) return false;
  *g = BoxGeo{D, H, W};
  *V = v;
  return true;
}

#define DPI_PC_LAUNCH(aw, GRID, ST, KERNEL, ...)                                            \
  do {                                                                                      \
    if ((aw) == 4) KERNEL(4)<<<GRID, 256, 0, ST>>>(__VA_ARGS__);                            \
    else if ((aw) == 2) KERNEL(2)<<<GRID, 256, 0, ST>>>(__VA_ARGS__);                       \
    else KERNEL(1)<<<GRID, 256, 0, ST>>>(__VA_ARGS__);                                      \
  } while (0)

}  // namespace

extern "C" int dpi_pconv_mask_fwd(const float* x, const float* m, int Cin, int Cm, size_t V, float* xm, float* msum, void* stream) {
  DPI_REQUIRE(x && m && xm && msum, "pconv_mask_fwd: NULL tensor");
  DPI_REQUIRE(Cin > 0 && (Cm == Cin || Cm == 1) && pc_voxels(V),
              "pconv_mask_fwd: bad geometry Cin = %d, Cm = %d (Cin or 1), V = %zu (must stay below 2^31 voxels)", Cin, Cm, V);
  DPI_REQUIRE(pc_aligned4({x, m, xm, msum}), "pconv_mask_fwd: a tensor is not aligned to its fp32 element");
  DPI_REQUIRE(xm != x && xm != m && msum != x && msum != m && msum != xm, "pconv_mask_fwd: not an in-place operation");
  const int aw = pc_access_width(V, {x, m, xm, msum});
#define DPI_PC_K(AW) pconv_mask_fwd_kernel<AW>
  DPI_PC_LAUNCH(aw, pc_blocks(cdivz(V, 4)), (hipStream_t)stream, DPI_PC_K, x, m, Cin, Cm, (unsigned)V, xm, msum);
#undef DPI_PC_K
  return dpi_check_launch("pconv_mask_fwd");
}

extern "C" int dpi_pconv_norm_fwd(const float* c, const float* msum, const float* bias, int Cout, int D, int H, int W, float* y,
                                  float* new_mask, float* S, void* stream) {
  BoxGeo g;
  size_t V;
  DPI_REQUIRE(c && msum && y && new_mask && S, "pconv_norm_fwd: NULL tensor");
  DPI_REQUIRE(Cout > 0 && pc_geo(D, H, W, &g, &V), "pconv_norm_fwd: bad geometry Cout = %d, %d x %d x %d (must stay below 2^31 voxels)", Cout, D,
              H, W);
  DPI_REQUIRE(pc_aligned4({c, msum, bias, y, new_mask, S}), "pconv_norm_fwd: a tensor is not aligned to its fp32 element");
  DPI_REQUIRE(msum != y && msum != new_mask && msum != S && new_mask != S && new_mask != y && S != y && new_mask != c && S != c,
              "pconv_norm_fwd: only y may alias c");
  const int aw = pc_access_width(V, {c, y, new_mask, S});
#define DPI_PC_K(AW) pconv_norm_fwd_kernel<AW>
  DPI_PC_LAUNCH(aw, pc_blocks(cdivz(V, 4)), (hipStream_t)stream, DPI_PC_K, c, msum, bias, Cout, g, (unsigned)V, y, new_mask, S);
#undef DPI_PC_K
  return dpi_check_launch("pconv_norm_fwd");
}

// Cout partials per wave of the launch, laid out [Cout][waves]: a wave owns 256 voxels
extern "C" size_t dpi_pconv_norm_bwd_ws_floats(int Cout, size_t V) {
  if (Cout <= 0 || !pc_voxels(V)) return 0;
  return cdivz(cdivz(V, 4), 256) * 4 * (size_t)Cout;
}

extern "C" int dpi_pconv_norm_bwd(const float* dy, const float* S, int Cout, size_t V, float* dc, float* dbias, float* ws, void* stream) {
  DPI_REQUIRE(dy && S && dc, "pconv_norm_bwd: NULL tensor");
  DPI_REQUIRE(Cout > 0 && pc_voxels(V), "pconv_norm_bwd: bad geometry Cout = %d, V = %zu (must stay below 2^31 voxels)", Cout, V);
  DPI_REQUIRE(!dbias || ws, "pconv_norm_bwd: the bias gradient needs a workspace of dpi_pconv_norm_bwd_ws_floats floats");
  DPI_REQUIRE(pc_aligned4({dy, S, dc, dbias, ws}), "pconv_norm_bwd: a tensor is not aligned to its fp32 element");
  DPI_REQUIRE(dc != S && (!dbias || (ws != dy && ws != S && ws != dc && dbias != ws && dbias != dc && dbias != S && dbias != dy)),
              "pconv_norm_bwd: outputs and workspace must not alias the inputs (dc may be dy)");
  const hipStream_t st = (hipStream_t)stream;
  const int aw = pc_access_width(V, {dy, S, dc});
  const unsigned blocks = (unsigned)cdivz(cdivz(V, 4), 256);
  if (dbias) {
#define DPI_PC_K(AW) pconv_norm_bwd_kernel<AW, true>
    DPI_PC_LAUNCH(aw, blocks, st, DPI_PC_K, dy, S, Cout, (unsigned)V, dc, ws);
#undef DPI_PC_K
    pconv_bias_final_kernel<<<(unsigned)Cout, 256, 0, st>>>(ws, blocks * 4, dbias);
  } else {
#define DPI_PC_K(AW) pconv_norm_bwd_kernel<AW, false>
    DPI_PC_LAUNCH(aw, blocks, st, DPI_PC_K, dy, S, Cout, (unsigned)V, dc, nullptr);
#undef DPI_PC_K
  }
  return dpi_check_launch("pconv_norm_bwd");
}

extern "C" int dpi_pconv_mask_bwd(const float* dxm, const float* x, const float* m, int Cin, int Cm, size_t V, float* dx, float* dm,
                                  void* stream) {
  DPI_REQUIRE(dxm && m && dx && (x || !dm), "pconv_mask_bwd: NULL tensor (x is needed for dm)");
  DPI_REQUIRE(Cin > 0 && (Cm == Cin || Cm == 1) && pc_voxels(V),
              "pconv_mask_bwd: bad geometry Cin = %d, Cm = %d (Cin or 1), V = %zu (must stay below 2^31 voxels)", Cin, Cm, V);
  DPI_REQUIRE(pc_aligned4({dxm, x, m, dx, dm}), "pconv_mask_bwd: a tensor is not aligned to its fp32 element");
  DPI_REQUIRE(dx != x && dx != m && (!dm || (dm != dxm && dm != x && dm != m && dm != dx)),
              "pconv_mask_bwd: outputs must not alias the inputs (dx may be dxm)");
  const hipStream_t st = (hipStream_t)stream;
  const unsigned grid = pc_blocks(cdivz(V, 4));
  if (!dm) {
    const int aw = pc_access_width(V, {dxm, m, dx});
#define DPI_PC_K(AW) pconv_mask_bwd_kernel<AW, 0>
    DPI_PC_LAUNCH(aw, grid, st, DPI_PC_K, dxm, x, m, Cin, Cm, (unsigned)V, dx, dm);
#undef DPI_PC_K
  } else if (Cm == Cin) {
    const int aw = pc_access_width(V, {dxm, x, m, dx, dm});
#define DPI_PC_K(AW) pconv_mask_bwd_kernel<AW, 1>
    DPI_PC_LAUNCH(aw, grid, st, DPI_PC_K, dxm, x, m, Cin, Cm, (unsigned)V, dx, dm);
#undef DPI_PC_K
  } else {
    const int aw = pc_access_width(V, {dxm, x, m, dx, dm});
#define DPI_PC_K(AW) pconv_mask_bwd_kernel<AW, 2>
    DPI_PC_LAUNCH(aw, grid, st, DPI_PC_K, dxm, x, m, Cin, Cm, (unsigned)V, dx, dm);
#undef DPI_PC_K
  }
  return dpi_check_launch("pconv_mask_bwd");
}
