// The NMO table of sampled laws (--moveout_offset --moveout_table device; ours, no reference code) as a gfx950 kernel: operators.nmo_table for
// a law given at tau = 0 .. T - 1, statement by statement and in its order of operations, for all gathers in one launch.  For the trace in
// column s of gather g, with v = law[g] and off = offset[s], everything in float64:
//     g[j]  = sqrt(j^2 + (off / v[j])^2), j = 0 .. T - 1                           the travel time on the grid
//     jmin  = the LAST index of the minimum of g                                    the branch starts there
//     env[j] = max(g[jmin .. j]), -inf below jmin                                   non-decreasing: searchable
//     j(t)  = (the number of env <= t) - 1, clipped to [0, T - 2]                   the bracket of the recorded sample t = 0 .. T - 1
//     live  iff j >= jmin, env[j] == g[j], env[j + 1] == g[j + 1], g[j + 1] > g[j], g[j] <= t <= g[j + 1]
//               and (stretch == 0 or 1 / (g[j + 1] - g[j]) <= stretch)
//     56 bisection steps of [j, j + 1] on travel(x) = sqrt(x^2 + (off / vel(x))^2) <= t, vel(x) the linear interpolant in numpy's form:
//               v[j] at x == j, v[j + 1] at x == j + 1, else (v[j + 1] - v[j]) * (x - j) + v[j]
//     table[t][s] = hi if travel(hi) == t else lo, clipped to [0, T - 1]; DPI_MOVEOUT_MUTE where not live.         (T = 1: 0 iff off == 0)
// The file is built with -ffp-contract=off: the only operations that can round differently from the host's are the fp64 sqrt and divide.
// One workgroup of four waves per trace.  g and env live in LDS (16 T bytes, T <= 4096).  The last minimum is found by every wave over the
// whole of g (lane-strided, folded by shuffles: no scratch, no second barrier); the running maximum is a workgroup prefix-maximum: every wave
// scans its quarter of T in tiles of 64 by shuffles with a carry, then raises it by the totals of the quarters before it.  A lane then takes
// the rows t = lane, lane + 256, ...: an upper-bound search over env in LDS and the bisection in registers (v[j] and v[j + 1] are read once
// per sample; all traces of a gather read the same T doubles of the law, from L2).  A lane stores its own sample with one plain 8-byte
// store; the traces of neighbouring workgroups are neighbouring columns of the same rows (trace_stride 1) and fill the same lines in L2.
// No atomics, one thread per output, a fixed order everywhere: the same bits every launch.  Every LDS index is t < T, j or j + 1 with
// 0 <= j <= T - 2, or a search position below T; every store goes to row t < T of a column the entry point checked against S: no law or offset
// (NaN included: every comparison fails, the sample is muted) reads or writes out of bounds.
#include "common.h"

namespace {

constexpr int NT_THREADS = 256;
constexpr int NT_WAVES = NT_THREADS / 64;
constexpr int NT_MAX_T = 4096;              // 16 T bytes of LDS: 64 KiB
constexpr unsigned NT_MAX_BLOCKS = 1u << 20;
constexpr double NT_MUTE = -1.0;            // operators.MOVEOUT_MUTE

__device__ __forceinline__ double nt_travel(double x, double j, double a, double b, double off) {
  const double v = x == j ? a : (x == j + 1.0 ? b : (b - a) * (x - j) + a);
  const double q = off / v;
  return sqrt(x * x + q * q);
}

__global__ __launch_bounds__(NT_THREADS) void nmo_table_kernel(const double* __restrict__ law, const double* __restrict__ offset, double stretch,
                                                               int T, size_t S, size_t group_stride, int n_traces, size_t trace_stride, size_t items,
                                                               double* __restrict__ table) {
  extern __shared__ double nt_lds[];
  double* __restrict__ g = nt_lds;
  double* __restrict__ env = nt_lds + T;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int seg = (T + NT_WAVES - 1) / NT_WAVES;               // rows per wave of the prefix-maximum
  const int s0 = wave * seg, s1 = s0 + seg < T ? s0 + seg : T;
  const double ninf = -__builtin_huge_val();
  for (size_t item = blockIdx.x; item < items; item += gridDim.x) {
    const size_t grp = item / (size_t)n_traces, k = item % (size_t)n_traces;
    const size_t s = grp * group_stride + k * trace_stride;
    const double off = offset[s];
    const double* __restrict__ v = law + grp * (size_t)T;
    if (T == 1) {
      if (threadIdx.x == 0) table[s] = off == 0.0 ? 0.0 : NT_MUTE;
      continue;
    }
    for (int t = threadIdx.x; t < T; t += NT_THREADS) {
      const double tau = (double)t;
      const double q = off / v[t];
      g[t] = sqrt(tau * tau + q * q);
    }
    __syncthreads();
    // the last minimum: smaller value first, the larger index among equal values; every wave computes it for itself
    double mv = __builtin_huge_val();
    int mi = -1;
    for (int i = lane; i < T; i += 64) {
      const double x = g[i];
      if (x <= mv) { mv = x; mi = i; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const double ov = __shfl_xor(mv, o, 64);
      const int oi = __shfl_xor(mi, o, 64);
      if (ov < mv || (ov == mv && oi > mi)) { mv = ov; mi = oi; }
    }
    const int jmin = mi < 0 ? 0 : mi;
    // the running maximum from jmin: within the wave's rows first
    double carry = ninf;
    for (int base = s0; base < s1; base += 64) {
      const int i = base + lane;
      double b = (i < s1 && i >= jmin) ? g[i] : ninf;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const double up = __shfl_up(b, o, 64);
        if (lane >= o && up > b) b = up;
      }
      if (carry > b) b = carry;
      if (i < s1) env[i] = b;
      carry = __shfl(b, 63, 64);
    }
    __syncthreads();
    double before = ninf;                                      // the largest value of the waves' rows before this one's
    for (int w = 0; w < wave; ++w) {
      const int e = (w + 1) * seg - 1;
      if (e < T && env[e] > before) before = env[e];
    }
    __syncthreads();
    for (int i = s0 + lane; i < s1; i += 64)
      if (before > env[i]) env[i] = before;
    __syncthreads();
    for (int t = threadIdx.x; t < T; t += NT_THREADS) {
      const double want = (double)t;
      int lo = 0, hi = T;                                      // the number of env <= want
      while (lo < hi) {
        const int m = (lo + hi) >> 1;
        if (env[m] <= want) lo = m + 1; else hi = m;
      }
      int j = lo - 1;
      j = j < 0 ? 0 : j;
      j = j > T - 2 ? T - 2 : j;
      const double g0 = g[j], g1 = g[j + 1];
      bool live = j >= jmin && env[j] == g0 && env[j + 1] == g1 && g1 > g0 && want >= g0 && want <= g1;
      if (live && stretch > 0.0) live = 1.0 / (g1 - g0) <= stretch;
      double out = NT_MUTE;
      if (live) {
        const double fj = (double)j, a = v[j], b = v[j + 1];
        double l = fj, h = fj + 1.0;
        for (int it = 0; it < 56; ++it) {
          const double mid = 0.5 * (l + h);
          if (nt_travel(mid, fj, a, b, off) <= want) l = mid; else h = mid;
        }
        out = nt_travel(h, fj, a, b, off) == want ? h : l;
        out = out < 0.0 ? 0.0 : out;
        out = out > (double)(T - 1) ? (double)(T - 1) : out;
      }
      table[(size_t)t * S + s] = out;
    }
    __syncthreads();                                           // g and env belong to the next trace from here
  }
}

}  // namespace

extern "C" int dpi_nmo_table(const double* law, const double* offset, double stretch, int T, int S, int n_groups, int group_stride, int n_traces,
                             int trace_stride, double* table, void* stream) {
  DPI_REQUIRE(law != nullptr && offset != nullptr && table != nullptr && (const double*)table != law && (const double*)table != offset,
              "nmo_table: null or aliased pointer");
  DPI_REQUIRE(T >= 1 && S >= 1 && n_groups >= 1 && n_traces >= 1, "nmo_table: T, S, n_groups and n_traces must be >= 1, got %d, %d, %d, %d", T, S,
              n_groups, n_traces);
  DPI_REQUIRE(stretch >= 0.0 && stretch < __builtin_huge_val(), "nmo_table: stretch must be finite and >= 0 (0 = no stretch mute), got %g", stretch);
  // every (gather, trace) must be a column of its own below S: strides >= 1 where there is more than one, the last column inside
  DPI_REQUIRE(group_stride >= 0 && trace_stride >= 0 && (n_groups == 1 || group_stride >= 1) && (n_traces == 1 || trace_stride >= 1),
              "nmo_table: %d gathers %d apart of %d traces %d apart: strides must be >= 1", n_groups, group_stride, n_traces, trace_stride);
  const long long last = (long long)(n_groups - 1) * group_stride + (long long)(n_traces - 1) * trace_stride;
  DPI_REQUIRE(last <= (long long)S - 1, "nmo_table: %d gathers %d apart of %d traces %d apart reach past the %d columns", n_groups, group_stride,
              n_traces, trace_stride, S);
  // g and env of a trace live in LDS, 16 T bytes
  DPI_REQUIRE(T <= NT_MAX_T, "nmo_table: T = %d rows: at most %d on the device (build the table on the host)", T, NT_MAX_T);
  const size_t items = (size_t)n_groups * (size_t)n_traces;
  const unsigned nb = items < NT_MAX_BLOCKS ? (unsigned)items : NT_MAX_BLOCKS;
  const size_t lds = 2 * sizeof(double) * (size_t)(T < 2 ? 2 : T);
  nmo_table_kernel<<<nb, NT_THREADS, lds, (hipStream_t)stream>>>(law, offset, stretch, T, (size_t)S, (size_t)group_stride, n_traces,
                                                                 (size_t)trace_stride, items, table);
  return dpi_check_launch("nmo_table");
}
