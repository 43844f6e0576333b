// Sampling of a regular-grid tensor at the recorded trace positions with a K x K tap table (--trace_interp cubic | sinc8; ours, no
// reference code) as gfx950 kernels.  include/dpi_hip.h has the definition; trace_interp.cpp builds the table w = [2][K][X][Y].
//     forward: y[r][x][y] = sum_kx w[0][kx] * (sum_ky w[1][ky] * in[r][tap_x][tap_y])           r = c * T + t, ky inside, kx outside
//     adjoint: the exact transpose, as a gather: node (x', y') collects from the (K + 1) x (K + 1) traces around it
// Tap k of trace i sits at clamp(i - K/2 + (d >= 0) + k, 0, n - 1): the offsets are read for their sign only.
// Per output sample the forward pass reads K^2 inputs (64 for sinc8) against 8 bytes of HBM traffic, so the reads come from LDS: a
// workgroup owns a tile of TX x TY traces (8 x 32, lanes along y; 256 x 1 for Y = 1) and stages, RS_ROWS rows (c, t) at a time, the
// (TX + K) x (TY + K) halo around it with the clamped indices resolved while staging, so the window walk needs no edge case.  The global
// offsets of a thread's halo elements, its 2K weights (forward) or (K + 1)^2 coefficients (adjoint) are formed once per launch and kept
// in registers; blockIdx.y strides over the row groups.  For Y = 1 (2-D patches) every y tap clamps onto the one node: the kernels take
// the sum sy of the K y weights once (1 exactly for dy = 0) and walk K taps, not K^2.  No atomics: every output sample is written by
// one thread from a sum in a fixed order, so a result does not depend on the launch shape.  Zero offsets give unit taps: both passes are
// then the identity bit for bit.
#include "common.h"

namespace {

constexpr int RS_THREADS = 256;
constexpr int RS_ROWS = 4;          // rows (c, t) staged per step
constexpr int RS_BLOCKS = 2048;     // workgroups aimed at: 256 CUs x 8

template <int K, bool FLAT>
struct rs_geom {
  static constexpr int TX = FLAT ? RS_THREADS : 8, TY = FLAT ? 1 : 32;      // traces of a tile
  static constexpr int KY = FLAT ? 1 : K;                                   // y taps walked
  static constexpr int HX = TX + K, HY = FLAT ? 1 : TY + K, H = HX * HY;    // the halo: traces x0 - K/2 .. x0 + TX - 1 + K/2
  static constexpr int NS = (H + RS_THREADS - 1) / RS_THREADS;              // halo elements a thread stages per row
};

__device__ __forceinline__ int rs_clamp(int i, int n) { return i < 0 ? 0 : (i >= n ? n - 1 : i); }

// the plane offsets of the halo elements this thread stages: clamped to the grid, so every load stays in bounds
template <int K, bool FLAT>
__device__ __forceinline__ void rs_sources(int x0, int y0, int X, int Y, size_t (&src)[rs_geom<K, FLAT>::NS]) {
  using G = rs_geom<K, FLAT>;
#pragma unroll
  for (int e = 0; e < G::NS; ++e) {
    const int idx = (int)threadIdx.x + e * RS_THREADS;
    const int hx = idx / G::HY, hy = idx - hx * G::HY;
    src[e] = (size_t)rs_clamp(x0 - K / 2 + hx, X) * Y + rs_clamp(y0 - K / 2 + hy, Y);      // idx >= H: in bounds and never stored
  }
}

template <int K, bool FLAT>
__device__ __forceinline__ void rs_stage(const float* __restrict__ in, size_t S, size_t r0, size_t R, const size_t (&src)[rs_geom<K, FLAT>::NS],
                                         float (&tile)[RS_ROWS][rs_geom<K, FLAT>::H]) {
  using G = rs_geom<K, FLAT>;
#pragma unroll
  for (int q = 0; q < RS_ROWS; ++q) {
    if (r0 + q < R) {
      const float* __restrict__ p = in + (r0 + q) * S;
#pragma unroll
      for (int e = 0; e < G::NS; ++e) {
        const int idx = (int)threadIdx.x + e * RS_THREADS;
        if (idx < G::H) tile[q][idx] = p[src[e]];
      }
    }
  }
}

// what trace j (offset d, weights wj[k * S]) puts onto node i of an axis of n nodes: the weights of its clamped taps that are i, k ascending
template <int K>
__device__ __forceinline__ float rs_onto(const float* __restrict__ wj, size_t S, float d, int j, int n, int i) {
  const int first = j - K / 2 + (d >= 0.f ? 1 : 0);
  if (i > 0 && i < n - 1) {                                                 // an inner node: nothing clamps onto it, at most one tap is i
    const int k0 = i - first;
    return k0 >= 0 && k0 < K ? wj[(size_t)k0 * S] : 0.f;                    // one load, not K (the adjoint's set-up is K + 1 of these per axis)
  }
  float c = 0.f;
#pragma unroll
  for (int k = 0; k < K; ++k)
    if (rs_clamp(first + k, n) == i) c += wj[(size_t)k * S];
  return c;
}

template <int K, bool FLAT>
__global__ __launch_bounds__(RS_THREADS) void trace_resample_fwd_kernel(const float* __restrict__ in, const float* __restrict__ w,
                                                                        const float* __restrict__ off, size_t R, int X, int Y, int tiles_y,
                                                                        float* __restrict__ out) {
  using G = rs_geom<K, FLAT>;
  __shared__ float tile[RS_ROWS][G::H];
  const size_t S = (size_t)X * Y;
  const int bx = (int)blockIdx.x / tiles_y, by = (int)blockIdx.x - bx * tiles_y;
  const int x0 = bx * G::TX, y0 = by * G::TY;
  size_t src[G::NS];
  rs_sources<K, FLAT>(x0, y0, X, Y, src);
  const int tx = (int)threadIdx.x / G::TY, ty = (int)threadIdx.x - tx * G::TY;
  const int ix = x0 + tx, iy = y0 + ty;
  const bool active = ix < X && iy < Y;
  const size_t s = active ? (size_t)ix * Y + iy : 0;
  float wx[K], wy[K];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    wx[k] = active ? w[(size_t)k * S + s] : 0.f;
    wy[k] = active ? w[(size_t)(K + k) * S + s] : 0.f;
  }
  float sy = wy[0];                                                         // FLAT: all K y taps are node 0
#pragma unroll
  for (int k = 1; k < K; ++k) sy += wy[k];
  // the first tap in the tile: the halo starts K/2 nodes before the tile, the window K/2 - (d >= 0) nodes before the trace
  const int base = (tx + (off[s] >= 0.f ? 1 : 0)) * G::HY + (FLAT ? 0 : ty + (off[S + s] >= 0.f ? 1 : 0));
  const size_t ngroups = (R + RS_ROWS - 1) / RS_ROWS;
  for (size_t g = blockIdx.y; g < ngroups; g += gridDim.y) {
    const size_t r0 = g * RS_ROWS;
    rs_stage<K, FLAT>(in, S, r0, R, src, tile);
    __syncthreads();
    if (active) {
#pragma unroll
      for (int q = 0; q < RS_ROWS; ++q) {
        if (r0 + q < R) {
          const float* t = &tile[q][base];
          float acc = 0.f;
#pragma unroll
          for (int kx = 0; kx < K; ++kx) {
            float inner;
            if (FLAT) {
              inner = sy * t[kx];
            } else {
              inner = wy[0] * t[kx * G::HY];
#pragma unroll
              for (int ky = 1; ky < K; ++ky) inner += wy[ky] * t[kx * G::HY + ky];
            }
            const float term = wx[kx] * inner;
            acc = kx == 0 ? term : acc + term;
          }
          out[(r0 + q) * S + s] = acc;
        }
      }
    }
    __syncthreads();
  }
}

template <int K, bool FLAT>
__global__ __launch_bounds__(RS_THREADS) void trace_resample_adj_kernel(const float* __restrict__ in, const float* __restrict__ w,
                                                                        const float* __restrict__ off, size_t R, int X, int Y, int tiles_y,
                                                                        float* __restrict__ out) {
  using G = rs_geom<K, FLAT>;
  constexpr int NY = FLAT ? 1 : K + 1;                                      // traces around a node along y
  __shared__ float tile[RS_ROWS][G::H];
  const size_t S = (size_t)X * Y;
  const int bx = (int)blockIdx.x / tiles_y, by = (int)blockIdx.x - bx * tiles_y;
  const int x0 = bx * G::TX, y0 = by * G::TY;
  size_t src[G::NS];
  rs_sources<K, FLAT>(x0, y0, X, Y, src);
  const int tx = (int)threadIdx.x / G::TY, ty = (int)threadIdx.x - tx * G::TY;
  const int ix = x0 + tx, iy = y0 + ty;
  const bool active = ix < X && iy < Y;
  const size_t s = active ? (size_t)ix * Y + iy : 0;
  // coefficient of trace (ix - K/2 + a, iy - K/2 + b) on this node; a trace outside the grid: 0 on a halo element that was loaded in bounds
  float c[(K + 1) * NY];
#pragma unroll
  for (int a = 0; a <= K; ++a) {
#pragma unroll
    for (int b = 0; b < NY; ++b) {
      const int jx = ix - K / 2 + a, jy = FLAT ? 0 : iy - K / 2 + b;
      float v = 0.f;
      if (active && jx >= 0 && jx < X && jy >= 0 && jy < Y) {
        const size_t j = (size_t)jx * Y + jy;
        const float cx = rs_onto<K>(w + j, S, off[j], jx, X, ix);
        float cy;
        if (FLAT) {
          cy = w[(size_t)K * S + j];
#pragma unroll
          for (int k = 1; k < K; ++k) cy += w[(size_t)(K + k) * S + j];
        } else {
          cy = rs_onto<K>(w + (size_t)K * S + j, S, off[S + j], jy, Y, iy);
        }
        v = cx * cy;
      }
      c[a * NY + b] = v;
    }
  }
  const int base = tx * G::HY + (FLAT ? 0 : ty);
  const size_t ngroups = (R + RS_ROWS - 1) / RS_ROWS;
  for (size_t g = blockIdx.y; g < ngroups; g += gridDim.y) {
    const size_t r0 = g * RS_ROWS;
    rs_stage<K, FLAT>(in, S, r0, R, src, tile);
    __syncthreads();
    if (active) {
#pragma unroll
      for (int q = 0; q < RS_ROWS; ++q) {
        if (r0 + q < R) {
          const float* t = &tile[q][base];
          float acc = c[0] * t[0];
#pragma unroll
          for (int a = 0; a <= K; ++a) {
#pragma unroll
            for (int b = 0; b < NY; ++b)
              if (a + b > 0) acc += c[a * NY + b] * t[a * G::HY + b];
          }
          out[(r0 + q) * S + s] = acc;
        }
      }
    }
    __syncthreads();
  }
}

// the checks and the grid both entry points share
template <bool FLAT>
int rs_grid(const char* what, size_t R, int X, int Y, int* tiles_y, dim3* grid) {
  using G = rs_geom<2, FLAT>;                                               // the tile does not depend on K
  *tiles_y = cdiv(Y, G::TY);
  const size_t bx = cdivz((size_t)X, G::TX) * (size_t)*tiles_y;
  DPI_REQUIRE(bx <= 0x7fffffffu, "%s: %d x %d traces are too many", what, X, Y);
  size_t by = cdivz(R, RS_ROWS);
  const size_t cap = bx < RS_BLOCKS ? RS_BLOCKS / bx : 1;
  if (by > cap) by = cap;
  if (by > 65535) by = 65535;
  *grid = dim3((unsigned)bx, (unsigned)by, 1);
  return DPI_OK;
}

template <bool ADJ>
int rs_launch(const char* what, const float* in, const float* w, const float* off, int K, int C, int T, int X, int Y, float* out, void* stream) {
  DPI_REQUIRE(in && w && off && out && in != out && C > 0 && T > 0 && X > 0 && Y > 0, "%s: bad argument", what);
  DPI_REQUIRE(K == 2 || K == 4 || K == 8, "%s: K = %d taps per axis, expected 2, 4 or 8", what, K);
  const size_t S = (size_t)X * (size_t)Y, R = (size_t)C * (size_t)T;
  DPI_REQUIRE(R <= ((size_t)1 << 60) / S, "%s: a tensor of %d x %d x %d x %d samples is too large", what, C, T, X, Y);
  const bool flat = Y == 1;
  int tiles_y;
  dim3 grid;
  if (int e = flat ? rs_grid<true>(what, R, X, Y, &tiles_y, &grid) : rs_grid<false>(what, R, X, Y, &tiles_y, &grid)) return e;
  hipStream_t st = (hipStream_t)stream;
#define RS_GO(KK, FF)                                                                                                          \
  do {                                                                                                                         \
    if (ADJ) trace_resample_adj_kernel<KK, FF><<<grid, RS_THREADS, 0, st>>>(in, w, off, R, X, Y, tiles_y, out);                 \
    else trace_resample_fwd_kernel<KK, FF><<<grid, RS_THREADS, 0, st>>>(in, w, off, R, X, Y, tiles_y, out);                     \
  } while (0)
  if (flat) {
    if (K == 2) RS_GO(2, true); else if (K == 4) RS_GO(4, true); else RS_GO(8, true);
  } else {
    if (K == 2) RS_GO(2, false); else if (K == 4) RS_GO(4, false); else RS_GO(8, false);
  }
#undef RS_GO
  return dpi_check_launch(what);
}

}  // namespace

extern "C" int dpi_trace_resample_fwd(const float* x, const float* w, const float* off, int K, int C, int T, int X, int Y, float* y, void* stream) {
  return rs_launch<false>("trace_resample_fwd", x, w, off, K, C, T, X, Y, y, stream);
}

extern "C" int dpi_trace_resample_adj(const float* y, const float* w, const float* off, int K, int C, int T, int X, int Y, float* x, void* stream) {
  return rs_launch<true>("trace_resample_adj", y, w, off, K, C, T, X, Y, x, stream);
}
