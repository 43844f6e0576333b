// Semblance velocity scan (--moveout_offset; ours, no reference code) as a gfx950 kernel: the three sums behind a semblance panel, for every
// gather g, trial velocity v and zero-offset row tau, over the traces s of the gather along the hyperbola t = sqrt(tau^2 + (offset[s] / v)^2):
//     live  iff t <= T - 1, (stretch <= 0 or t <= stretch * tau) and both tap rows i, i + 1 of column s are known (mask != 0)
//     i = min(floor(t), T - 2), f = t - i, a = (1 - f) d[i][s] + f d[i + 1][s]       (T = 1: i = 0, row 0 only, a = d[0][s])
//     num = sum a, den = sum a^2, cnt = the number of live traces
// everything past the two fp32 reads in float64.  d and mask are [T][S] fp32; trace k of gather g is column g * group_stride + k * trace_stride.
// A workgroup of four waves owns ONE (g, v) and a contiguous run of rows tau, so its taps walk down the same few rows of d and mask and
// neighbouring workgroups hit the same lines in L2.  Lanes run along the traces of the gather: where trace_stride = 1 (the layouts
// `volume`, the whole cube as one gather, and `x`, the Y traces of every x index) the two tap rows of a wave are read coalesced; the
// layout `y` (the X traces of every y index) reads with stride Y and is merely correct.  A lane forms (offset / v)^2 once per trace and walks its SS_RUN rows with that value, SS_RUN x (num, den, cnt) in registers.
// `wpr` waves share a row (1 for gathers of up to 64 traces, 2 up to 128, 4 beyond), the other 4 / wpr groups of waves take the next
// SS_RUN rows each, so a small gather still fills the workgroup.  Reduction: a lane adds its traces in ascending order, the wave is
// folded by shuffles, the wave sums go through LDS and one thread per row adds them in ascending order: no atomics, the same bits
// every launch.  A sample that is not live reads nothing, and a live one has 0 <= i <= T - 2: no offset, velocity or mask can send a
// load out of bounds (a NaN fails every comparison: not live).
#include "common.h"

namespace {

constexpr int SS_THREADS = 256;
constexpr int SS_WAVES = SS_THREADS / 64;
constexpr int SS_RUN = 8;                   // rows of tau per wave
constexpr unsigned SS_MAX_BLOCKS = 1u << 20;

__global__ __launch_bounds__(SS_THREADS) void semblance_sums_kernel(const float* __restrict__ d, const float* __restrict__ mask,
                                                                    const double* __restrict__ offset, const double* __restrict__ vel, int NV,
                                                                    double stretch, int T, size_t S, size_t group_stride, int n_traces,
                                                                    size_t trace_stride, int wpr, int chunks, size_t items,
                                                                    double* __restrict__ num, double* __restrict__ den, int* __restrict__ cnt) {
  __shared__ double sh_num[SS_WAVES][SS_RUN], sh_den[SS_WAVES][SS_RUN];
  __shared__ int sh_cnt[SS_WAVES][SS_RUN];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int slice = wave % wpr, rgroup = wave / wpr;          // which traces, which rows of the workgroup's run
  const int rows_per_block = SS_RUN * (SS_WAVES / wpr);
  const double tmax = (double)(T - 1);
  for (size_t item = blockIdx.x; item < items; item += gridDim.x) {
    const int chunk = (int)(item % (size_t)chunks);
    const size_t gv = item / (size_t)chunks;
    const int iv = (int)(gv % (size_t)NV);
    const size_t g = gv / (size_t)NV;
    const double v = vel[iv];
    const int tau0 = chunk * rows_per_block + rgroup * SS_RUN;
    double an[SS_RUN], ad[SS_RUN];
    int ac[SS_RUN];
#pragma unroll
    for (int r = 0; r < SS_RUN; ++r) { an[r] = 0.0; ad[r] = 0.0; ac[r] = 0; }
    if (tau0 < T) {
      for (int k = slice * 64 + lane; k < n_traces; k += 64 * wpr) {
        const size_t s = g * group_stride + (size_t)k * trace_stride;
        const double x = offset[s] / v;
        const double q = x * x;
        const float* __restrict__ dc = d + s;
        const float* __restrict__ mc = mask + s;
#pragma unroll
        for (int r = 0; r < SS_RUN; ++r) {
          const int row = tau0 + r;
          if (row >= T) break;
          const double tau = (double)row;
          const double t = sqrt(tau * tau + q);
          bool live = t <= tmax && (stretch <= 0.0 || t <= stretch * tau);
          if (!live) continue;
          double a;
          if (T == 1) {
            if (mc[0] == 0.f) continue;
            a = (double)dc[0];
          } else {
            int i = (int)floor(t);                             // 0 <= t <= T - 1 <= 2^24
            i = i < T - 2 ? i : T - 2;
            const size_t at = (size_t)i * S;
            if (mc[at] == 0.f || mc[at + S] == 0.f) continue;
            const double f = t - (double)i;
            a = (1.0 - f) * (double)dc[at] + f * (double)dc[at + S];
          }
          an[r] += a;
          ad[r] += a * a;
          ac[r] += 1;
        }
      }
    }
#pragma unroll
    for (int r = 0; r < SS_RUN; ++r) {
      const double sn = wave_sum(an[r]), sd = wave_sum(ad[r]);
      int sc = ac[r];
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) sc += __shfl_xor(sc, o, 64);
      if (lane == 0) { sh_num[wave][r] = sn; sh_den[wave][r] = sd; sh_cnt[wave][r] = sc; }
    }
    __syncthreads();
    if ((int)threadIdx.x < rows_per_block) {
      const int rg = threadIdx.x / SS_RUN, r = threadIdx.x % SS_RUN;
      const int row = chunk * rows_per_block + threadIdx.x;
      if (row < T) {
        double sn = 0.0, sd = 0.0;
        int sc = 0;
        for (int w = 0; w < wpr; ++w) { sn += sh_num[rg * wpr + w][r]; sd += sh_den[rg * wpr + w][r]; sc += sh_cnt[rg * wpr + w][r]; }
        const size_t o = gv * (size_t)T + (size_t)row;
        num[o] = sn;
        den[o] = sd;
        cnt[o] = sc;
      }
    }
    __syncthreads();                                           // the LDS rows belong to the next item from here
  }
}

}  // namespace

extern "C" int dpi_semblance_sums(const float* d, const float* mask, const double* offset, const double* vel, int NV, double stretch, int T,
                                  size_t S, int n_groups, size_t group_stride, int n_traces, size_t trace_stride, double* num, double* den,
                                  int* cnt, void* stream) {
  const void* in[4] = {d, mask, offset, vel};
  const void* out[3] = {num, den, cnt};
  bool ok = true;
  for (int i = 0; i < 4; ++i) ok = ok && in[i] != nullptr;
  for (int i = 0; i < 3; ++i) {
    ok = ok && out[i] != nullptr;
    for (int j = 0; j < 4; ++j) ok = ok && out[i] != in[j];
    for (int j = 0; j < i; ++j) ok = ok && out[i] != out[j];
  }
  DPI_REQUIRE(ok, "semblance_sums: null or aliased pointer");      // inputs are read only and may share memory; no output may share any
  DPI_REQUIRE(T >= 1 && S >= 1 && NV >= 1 && n_groups >= 1 && n_traces >= 1,
              "semblance_sums: T, S, NV, n_groups and n_traces must be >= 1, got %d, %zu, %d, %d, %d", T, S, NV, n_groups, n_traces);
  // the last column the geometry names is (n_groups - 1) group_stride + (n_traces - 1) trace_stride: it must lie below S (no product wraps)
  const size_t gm = (size_t)(n_groups - 1), km = (size_t)(n_traces - 1);
  bool inside = (gm == 0 || group_stride <= (S - 1) / gm) && (km == 0 || trace_stride <= (S - 1) / km);
  inside = inside && gm * group_stride <= (S - 1) - km * trace_stride;
  DPI_REQUIRE(inside, "semblance_sums: %d gathers %zu apart of %d traces %zu apart reach past the %zu columns", n_groups, group_stride, n_traces,
              trace_stride, S);
  // T <= 2^24: the bound of the other kernels along t (every row index an exact float)
  DPI_REQUIRE(T <= (1 << 24), "semblance_sums: T = %d rows: at most 2^24", T);
  DPI_REQUIRE(S <= ((size_t)1 << 60) / (size_t)T && (size_t)n_groups <= (((size_t)1 << 60) / (size_t)T) / (size_t)NV,
              "semblance_sums: %d x %zu samples, %d x %d x %d sums: too large", T, S, n_groups, NV, T);
  const int wpr = n_traces <= 64 ? 1 : (n_traces <= 128 ? 2 : SS_WAVES);
  const int rows_per_block = SS_RUN * (SS_WAVES / wpr);
  const int chunks = cdiv(T, rows_per_block);
  const size_t items = (size_t)n_groups * (size_t)NV * (size_t)chunks;
  const unsigned nb = items < SS_MAX_BLOCKS ? (unsigned)items : SS_MAX_BLOCKS;
  semblance_sums_kernel<<<nb, SS_THREADS, 0, (hipStream_t)stream>>>(d, mask, offset, vel, NV, stretch, T, S, group_stride, n_traces, trace_stride,
                                                                   wpr, chunks, items, num, den, cnt);
  return dpi_check_launch("semblance_sums");
}
