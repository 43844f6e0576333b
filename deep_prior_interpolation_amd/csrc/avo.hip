// Linearised amplitude-versus-angle modelling (reference operators/avo.py:67-95 AVOLinearModelling.forward / .adjoint) as gfx950 kernels.
//     forward: y[a][t][s] = sum_k G[a][k][t] * x[k][t][s]        x = [3][T][S] model, y = [A][T][S] angle sections
//     adjoint: x[k][t][s] = sum_a G[a][k][t] * y[a][t][s]        G = [A][3][T] coefficients (a function of angle and time only)
// One pass each, HBM-bound (3 + A planes move once: 4 (3 + A) bytes per (t,s) sample), no atomics: every output sample is written by
// one thread from sums in a fixed order.  A workgroup works on ONE time sample (blockIdx.y, grid-strided past 65535) and a span of 1024
// samples of its row (blockIdx.x), so the 3 A coefficients it needs are the same in every lane: the compiler reads them through the
// constant (SMEM) path.  Along s a thread moves 16 bytes per plane where the rows of this t start on 16 bytes in the input and in the
// output, with a scalar tail of S % 4 samples; other rows (S % 4 != 0 makes most of them so, a view moved off its alignment all of them)
// take the element-wise path, four coalesced samples per thread.  Both paths form the sums in the same order, so they give the same bits.
#include "common.h"

namespace {

constexpr int AVO_SPAN = 1024;      // samples of a row per workgroup: 256 threads x 4

// whether the rows (c, t) of every channel plane c of a [C][T][S] tensor at `p` start on 16 bytes: plane_mult4 = (T * S) % 4 == 0
// (all planes then sit like plane 0).  Wave-uniform.
__device__ __forceinline__ bool avo_row_aligned(const float* p, size_t row, bool plane_mult4) {
  return plane_mult4 && (((reinterpret_cast<uintptr_t>(p) >> 2) + row) & 3u) == 0;
}

__device__ __forceinline__ float avo_fwd1(float g0, float g1, float g2, float x0, float x1, float x2) { return g0 * x0 + g1 * x1 + g2 * x2; }

__global__ __launch_bounds__(256) void avo_fwd_kernel(const float* __restrict__ x, const float* __restrict__ G, int A, int T, size_t S,
                                                      int plane_mult4, float* __restrict__ y) {
  const size_t plane = (size_t)T * S;
  const size_t s0 = (size_t)blockIdx.x * AVO_SPAN;
  for (int t = blockIdx.y; t < T; t += gridDim.y) {
    const size_t row = (size_t)t * S;
    const float* __restrict__ g = G + t;           // g[(a * 3 + k) * T]
    if (avo_row_aligned(x, row, plane_mult4) && avo_row_aligned(y, row, plane_mult4)) {
      const size_t s = s0 + (size_t)threadIdx.x * 4;
      if (s + 4 <= S) {
        const float4 x0 = *reinterpret_cast<const float4*>(x + row + s);
        const float4 x1 = *reinterpret_cast<const float4*>(x + plane + row + s);
        const float4 x2 = *reinterpret_cast<const float4*>(x + 2 * plane + row + s);
        for (int a = 0; a < A; ++a) {
          const float g0 = g[(size_t)(3 * a) * T], g1 = g[(size_t)(3 * a + 1) * T], g2 = g[(size_t)(3 * a + 2) * T];
          *reinterpret_cast<float4*>(y + (size_t)a * plane + row + s) =
              make_float4(avo_fwd1(g0, g1, g2, x0.x, x1.x, x2.x), avo_fwd1(g0, g1, g2, x0.y, x1.y, x2.y),
                          avo_fwd1(g0, g1, g2, x0.z, x1.z, x2.z), avo_fwd1(g0, g1, g2, x0.w, x1.w, x2.w));
        }
      } else {
        for (size_t i = s; i < S; ++i) {           // the tail: at most 3 samples, in one thread of the row's last workgroup
          const float x0 = x[row + i], x1 = x[plane + row + i], x2 = x[2 * plane + row + i];
          for (int a = 0; a < A; ++a)
            y[(size_t)a * plane + row + i] = avo_fwd1(g[(size_t)(3 * a) * T], g[(size_t)(3 * a + 1) * T], g[(size_t)(3 * a + 2) * T], x0, x1, x2);
        }
      }
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const size_t i = s0 + (size_t)j * 256 + threadIdx.x;
        if (i < S) {
          const float x0 = x[row + i], x1 = x[plane + row + i], x2 = x[2 * plane + row + i];
          for (int a = 0; a < A; ++a)
            y[(size_t)a * plane + row + i] = avo_fwd1(g[(size_t)(3 * a) * T], g[(size_t)(3 * a + 1) * T], g[(size_t)(3 * a + 2) * T], x0, x1, x2);
        }
      }
    }
  }
}

__global__ __launch_bounds__(256) void avo_adj_kernel(const float* __restrict__ y, const float* __restrict__ G, int A, int T, size_t S,
                                                      int plane_mult4, float* __restrict__ x) {
  const size_t plane = (size_t)T * S;
  const size_t s0 = (size_t)blockIdx.x * AVO_SPAN;
  for (int t = blockIdx.y; t < T; t += gridDim.y) {
    const size_t row = (size_t)t * S;
    const float* __restrict__ g = G + t;
    if (avo_row_aligned(x, row, plane_mult4) && avo_row_aligned(y, row, plane_mult4)) {
      const size_t s = s0 + (size_t)threadIdx.x * 4;
      if (s + 4 <= S) {
        float4 r0 = make_float4(0.f, 0.f, 0.f, 0.f), r1 = r0, r2 = r0;
        for (int a = 0; a < A; ++a) {
          const float g0 = g[(size_t)(3 * a) * T], g1 = g[(size_t)(3 * a + 1) * T], g2 = g[(size_t)(3 * a + 2) * T];
          const float4 v = *reinterpret_cast<const float4*>(y + (size_t)a * plane + row + s);
          r0.x += g0 * v.x; r0.y += g0 * v.y; r0.z += g0 * v.z; r0.w += g0 * v.w;
          r1.x += g1 * v.x; r1.y += g1 * v.y; r1.z += g1 * v.z; r1.w += g1 * v.w;
          r2.x += g2 * v.x; r2.y += g2 * v.y; r2.z += g2 * v.z; r2.w += g2 * v.w;
        }
        *reinterpret_cast<float4*>(x + row + s) = r0;
        *reinterpret_cast<float4*>(x + plane + row + s) = r1;
        *reinterpret_cast<float4*>(x + 2 * plane + row + s) = r2;
      } else {
        for (size_t i = s; i < S; ++i) {
          float r0 = 0.f, r1 = 0.f, r2 = 0.f;
          for (int a = 0; a < A; ++a) {
            const float v = y[(size_t)a * plane + row + i];
            r0 += g[(size_t)(3 * a) * T] * v;
            r1 += g[(size_t)(3 * a + 1) * T] * v;
            r2 += g[(size_t)(3 * a + 2) * T] * v;
          }
          x[row + i] = r0;
          x[plane + row + i] = r1;
          x[2 * plane + row + i] = r2;
        }
      }
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const size_t i = s0 + (size_t)j * 256 + threadIdx.x;
        if (i < S) {
          float r0 = 0.f, r1 = 0.f, r2 = 0.f;
          for (int a = 0; a < A; ++a) {
            const float v = y[(size_t)a * plane + row + i];
            r0 += g[(size_t)(3 * a) * T] * v;
            r1 += g[(size_t)(3 * a + 1) * T] * v;
            r2 += g[(size_t)(3 * a + 2) * T] * v;
          }
          x[row + i] = r0;
          x[plane + row + i] = r1;
          x[2 * plane + row + i] = r2;
        }
      }
    }
  }
}

// the checks and the grid both entry points share
int avo_check(const char* what, const void* in, const void* G, const void* out, int ntheta, int T, size_t S, dim3* grid) {
  DPI_REQUIRE(in && G && out && in != out && ntheta > 0 && T > 0 && S > 0, "%s: bad argument", what);
  const size_t limit = ((size_t)1 << 60) / (size_t)T / S;      // the largest tensor's element count stays far inside size_t
  DPI_REQUIRE((size_t)ntheta <= limit && 3 <= limit, "%s: a tensor of %d x %d x %zu samples is too large", what, ntheta, T, S);
  const size_t bx = cdivz(S, AVO_SPAN);
  DPI_REQUIRE(bx <= 0x7fffffffu, "%s: a row of %zu samples is too long", what, S);
  *grid = dim3((unsigned)bx, (unsigned)(T < 65535 ? T : 65535), 1);
  return DPI_OK;
}

}  // namespace

extern "C" int dpi_avo_fwd(const float* x, const float* G, int ntheta, int T, size_t S, float* y, void* stream) {
  dim3 grid;
  if (int e = avo_check("avo_fwd", x, G, y, ntheta, T, S, &grid)) return e;
  avo_fwd_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(x, G, ntheta, T, S, ((size_t)T * S) % 4 == 0, y);
  return dpi_check_launch("avo_fwd");
}

extern "C" int dpi_avo_adj(const float* y, const float* G, int ntheta, int T, size_t S, float* x, void* stream) {
  dim3 grid;
  if (int e = avo_check("avo_adj", y, G, x, ntheta, T, S, &grid)) return e;
  avo_adj_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(y, G, ntheta, T, S, ((size_t)T * S) % 4 == 0, x);
  return dpi_check_launch("avo_adj");
}
