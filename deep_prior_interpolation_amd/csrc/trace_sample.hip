// Sampling of a regular-grid tensor at the recorded trace positions (--trace_offsets; ours, no reference code) as gfx950 kernels.
//     forward: y[r][x][y] = sum over the 2 x 2 taps of wx * wy * in[r][tap_x][tap_y]        r = c * T + t: the operator knows neither c nor t
//     adjoint: the exact transpose, as a gather: node (x', y') collects from the 3 x 3 traces around it
// Per axis, from the offset d of the trace alone (|d| <= 0.5, in grid cells): d >= 0 -> taps i, i + 1 with weights 1 - d, d;  d < 0 ->
// taps i - 1, i with weights -d, 1 + d; tap indices clamp to [0, n - 1] and two taps that clamp onto one node both count.
// Both passes move two planes once and are HBM-bound (8 bytes per sample; the 4 / 9 taps of neighbouring lanes overlap and come from
// the caches).  One thread owns one trace column s = x * Y + y, so consecutive lanes run along the innermost axis for Y = 1 (2-D patches)
// and Y > 1 alike; it forms its 4 (forward) or 9 (adjoint) coefficients and clamped tap offsets once and walks spans of TS_SPAN rows with
// them.  blockIdx.y strides over the row spans (at most ~2048 workgroups in flight, never more than 65535 along y).  No atomics: every
// output sample is written by one thread from a sum in a fixed order (x taps outer, y taps inner), so a result does not depend on the
// launch shape.  Zero offsets give the weights 1, 0, 0, 0: forward and adjoint are then the identity bit for bit.
#include "common.h"

namespace {

constexpr int TS_THREADS = 256;     // trace columns per workgroup
constexpr int TS_SPAN = 8;          // rows (c, t) a thread walks per grid-stride step
constexpr int TS_BLOCKS = 2048;     // workgroups aimed at: 256 CUs x 8

struct ts_axis { int i0, i1; float w0, w1; };

// the two clamped taps of trace `i` with offset `d` on an axis of n nodes
__device__ __forceinline__ ts_axis ts_taps(int i, float d, int n) {
  ts_axis a;
  if (d >= 0.f) { a.i0 = i; a.i1 = i + 1 < n ? i + 1 : n - 1; a.w0 = 1.f - d; a.w1 = d; }
  else { a.i0 = i > 0 ? i - 1 : 0; a.i1 = i; a.w0 = -d; a.w1 = 1.f + d; }
  return a;
}

// what trace `j` (offset d) puts onto node `i`: the weights of its taps that are i
__device__ __forceinline__ float ts_onto(int j, float d, int n, int i) {
  const ts_axis a = ts_taps(j, d, n);
  return (a.i0 == i ? a.w0 : 0.f) + (a.i1 == i ? a.w1 : 0.f);
}

__global__ __launch_bounds__(TS_THREADS) void trace_sample_fwd_kernel(const float* __restrict__ in, const float* __restrict__ off, size_t R,
                                                                      int X, int Y, float* __restrict__ out) {
  const size_t S = (size_t)X * Y;
  const size_t s = (size_t)blockIdx.x * TS_THREADS + threadIdx.x;
  if (s >= S) return;
  const int ix = (int)(s / (size_t)Y), iy = (int)(s - (size_t)ix * Y);
  const ts_axis ax = ts_taps(ix, off[s], X), ay = ts_taps(iy, off[S + s], Y);
  const size_t o00 = (size_t)ax.i0 * Y + ay.i0, o01 = (size_t)ax.i0 * Y + ay.i1, o10 = (size_t)ax.i1 * Y + ay.i0, o11 = (size_t)ax.i1 * Y + ay.i1;
  const float w00 = ax.w0 * ay.w0, w01 = ax.w0 * ay.w1, w10 = ax.w1 * ay.w0, w11 = ax.w1 * ay.w1;
  const size_t nspans = (R + TS_SPAN - 1) / TS_SPAN;
  for (size_t span = blockIdx.y; span < nspans; span += gridDim.y) {
    const size_t r0 = span * TS_SPAN, r1 = r0 + TS_SPAN < R ? r0 + TS_SPAN : R;
    const float* __restrict__ p = in + r0 * S;
    float* __restrict__ q = out + r0 * S + s;
#pragma unroll 4
    for (size_t r = r0; r < r1; ++r, p += S, q += S) *q = ((w00 * p[o00] + w01 * p[o01]) + w10 * p[o10]) + w11 * p[o11];
  }
}

__global__ __launch_bounds__(TS_THREADS) void trace_sample_adj_kernel(const float* __restrict__ in, const float* __restrict__ off, size_t R,
                                                                      int X, int Y, float* __restrict__ out) {
  const size_t S = (size_t)X * Y;
  const size_t s = (size_t)blockIdx.x * TS_THREADS + threadIdx.x;
  if (s >= S) return;
  const int ix = (int)(s / (size_t)Y), iy = (int)(s - (size_t)ix * Y);
  size_t o[9];
  float w[9];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
#pragma unroll
    for (int b = 0; b < 3; ++b) {
      const int jx = ix + a - 1, jy = iy + b - 1;
      const bool inside = jx >= 0 && jx < X && jy >= 0 && jy < Y;
      const size_t j = inside ? (size_t)jx * Y + jy : s;          // a trace outside the grid: weight 0 on a load that stays in bounds
      o[a * 3 + b] = j;
      w[a * 3 + b] = inside ? ts_onto(jx, off[j], X, ix) * ts_onto(jy, off[S + j], Y, iy) : 0.f;
    }
  }
  const size_t nspans = (R + TS_SPAN - 1) / TS_SPAN;
  for (size_t span = blockIdx.y; span < nspans; span += gridDim.y) {
    const size_t r0 = span * TS_SPAN, r1 = r0 + TS_SPAN < R ? r0 + TS_SPAN : R;
    const float* __restrict__ p = in + r0 * S;
    float* __restrict__ q = out + r0 * S + s;
#pragma unroll 2
    for (size_t r = r0; r < r1; ++r, p += S, q += S) {
      float acc = w[0] * p[o[0]];
#pragma unroll
      for (int k = 1; k < 9; ++k) acc += w[k] * p[o[k]];
      *q = acc;
    }
  }
}

// the checks and the grid both entry points share
int trace_sample_check(const char* what, const void* in, const void* off, const void* out, int C, int T, int X, int Y, size_t* R, dim3* grid) {
  DPI_REQUIRE(in && off && out && in != out && C > 0 && T > 0 && X > 0 && Y > 0, "%s: bad argument", what);
  const size_t S = (size_t)X * (size_t)Y;
  *R = (size_t)C * (size_t)T;
  DPI_REQUIRE(*R <= ((size_t)1 << 60) / S, "%s: a tensor of %d x %d x %d x %d samples is too large", what, C, T, X, Y);
  const size_t bx = cdivz(S, TS_THREADS);
  DPI_REQUIRE(bx <= 0x7fffffffu, "%s: %zu trace columns are too many", what, S);
  size_t by = cdivz(*R, TS_SPAN);
  const size_t cap = bx < TS_BLOCKS ? TS_BLOCKS / bx : 1;
  if (by > cap) by = cap;
  if (by > 65535) by = 65535;
  *grid = dim3((unsigned)bx, (unsigned)by, 1);
  return DPI_OK;
}

}  // namespace

extern "C" int dpi_trace_sample_fwd(const float* x, const float* off, int C, int T, int X, int Y, float* y, void* stream) {
  size_t R;
  dim3 grid;
  if (int e = trace_sample_check("trace_sample_fwd", x, off, y, C, T, X, Y, &R, &grid)) return e;
  trace_sample_fwd_kernel<<<grid, TS_THREADS, 0, (hipStream_t)stream>>>(x, off, R, X, Y, y);
  return dpi_check_launch("trace_sample_fwd");
}

extern "C" int dpi_trace_sample_adj(const float* y, const float* off, int C, int T, int X, int Y, float* x, void* stream) {
  size_t R;
  dim3 grid;
  if (int e = trace_sample_check("trace_sample_adj", y, off, x, C, T, X, Y, &R, &grid)) return e;
  trace_sample_adj_kernel<<<grid, TS_THREADS, 0, (hipStream_t)stream>>>(y, off, R, X, Y, x);
  return dpi_check_launch("trace_sample_adj");
}
