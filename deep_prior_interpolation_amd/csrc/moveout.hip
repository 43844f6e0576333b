// Moveout along the time axis (--moveout; ours, no reference code) as gfx950 kernels: d = L m, the model m is the flattened gather the
// network writes, d what the loss sees.  A table tau[t][s] (fp32, shared by the channels) names, for every recorded sample, the fractional
// row of its own trace column it is read from; a sample is live when 0 <= tau <= T - 1 and muted (d = 0) otherwise.
//     linear (K = 2): i0 = floor(tau), f = tau - i0, rows i0, i0 + 1, weights 1 - f, f
//     cubic  (K = 4): Keys, a = -1/2, rows i0 - 1 .. i0 + 2, weights ((-.5f+1)f-.5)f, (1.5f-2.5)f^2+1, ((-1.5f+2)f+.5)f, (.5f-.5)f^2
// Row indices clamp to [0, T - 1] and every clamped tap counts (the convention of trace_sample.hip).  f = 0 gives the weights 1, 0 and
// 0, 1, 0, 0 exactly: the identity table is the identity bit for bit, both ways.
//     forward: one thread per (t, s), s fastest: the table read and the store are coalesced, the K row reads differ per lane and land in
//              a few neighbouring rows of the same columns (lines the wave's other lanes use as well).  The weights are formed once and
//              serve every channel.  d = ((w0 m0 + w1 m1) + w2 m2) + w3 m3.
//     adjoint: the exact transpose as a gather, no atomics: model sample (i, s) walks the samples t0 <= t < t1 of its own column in
//              ascending t, forms the weights of each live one with the same expressions as the forward pass and adds w_k d[t] for every
//              tap k (ascending) whose clamped row is i.  [t0, t1) comes from the caller: range[0][i][s] = t0, range[1][i][s] = t1, any
//              range that holds every live sample touching row i (operators/moveout.py builds the tightest one from the monotone table,
//              once per patch).  The bounds are clamped to [0, T] here and every tap is checked against i, so a range that is too wide
//              costs time only and no table can send a load or a store out of bounds.  One thread writes one output from a sum in a
//              fixed order: the same bits every run, whatever the launch shape.  A constant table makes one thread walk all T samples.
// Both passes move the tensor twice plus the table (forward) or the table and two range planes (adjoint) and are bound by those bytes.
#include "common.h"

namespace {

constexpr int MO_THREADS = 256;     // trace columns per workgroup

// rows and weights of one sample; false for a muted one (NaN included: every comparison fails)
template <int K>
__device__ __forceinline__ bool mo_taps(float tau, int T, int (&r)[K], float (&w)[K]) {
  if (!(tau >= 0.f && tau <= (float)(T - 1))) return false;
  const float fl = floorf(tau);
  const int i0 = (int)fl;           // 0 <= i0 <= T - 1
  const float f = tau - fl;         // exact
  if constexpr (K == 2) {
    r[0] = i0;
    r[1] = i0 + 1 < T ? i0 + 1 : T - 1;
    w[0] = 1.f - f;
    w[1] = f;
  } else {
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int i = i0 - 1 + k;
      r[k] = i < 0 ? 0 : (i < T ? i : T - 1);
    }
    const float f2 = f * f;
    w[0] = ((-.5f * f + 1.f) * f - .5f) * f;
    w[1] = (1.5f * f - 2.5f) * f2 + 1.f;
    w[2] = ((-1.5f * f + 2.f) * f + .5f) * f;
    w[3] = (.5f * f - .5f) * f2;
  }
  return true;
}

template <int K>
__global__ __launch_bounds__(MO_THREADS) void moveout_fwd_kernel(const float* __restrict__ m, const float* __restrict__ tau, int C, int T,
                                                                 size_t S, float* __restrict__ d) {
  const size_t s = (size_t)blockIdx.x * MO_THREADS + threadIdx.x;
  if (s >= S) return;
  const size_t plane = (size_t)T * S;
  for (int t = blockIdx.y; t < T; t += gridDim.y) {
    int r[K];
    float w[K];
    const bool live = mo_taps<K>(tau[(size_t)t * S + s], T, r, w);
    const float* __restrict__ p = m + s;
    float* __restrict__ q = d + (size_t)t * S + s;
    for (int c = 0; c < C; ++c, p += plane, q += plane) {
      float acc = 0.f;
      if (live) {
        acc = w[0] * p[(size_t)r[0] * S];
#pragma unroll
        for (int k = 1; k < K; ++k) acc += w[k] * p[(size_t)r[k] * S];
      }
      *q = acc;
    }
  }
}

template <int K>
__global__ __launch_bounds__(MO_THREADS) void moveout_adj_kernel(const float* __restrict__ d, const float* __restrict__ tau,
                                                                 const int* __restrict__ range, int T, size_t S, float* __restrict__ m) {
  const size_t s = (size_t)blockIdx.x * MO_THREADS + threadIdx.x;
  if (s >= S) return;
  const size_t plane = (size_t)T * S;
  const float* __restrict__ dc = d + (size_t)blockIdx.z * plane + s;
  const float* __restrict__ tc = tau + s;
  float* __restrict__ mc = m + (size_t)blockIdx.z * plane + s;
  for (int i = blockIdx.y; i < T; i += gridDim.y) {
    int t0 = range[(size_t)i * S + s], t1 = range[plane + (size_t)i * S + s];
    t0 = t0 < 0 ? 0 : t0;
    t1 = t1 > T ? T : t1;
    float acc = 0.f;
    for (int t = t0; t < t1; ++t) {
      int r[K];
      float w[K];
      if (!mo_taps<K>(tc[(size_t)t * S], T, r, w)) continue;      // a mute gap inside the range
      const float v = dc[(size_t)t * S];
#pragma unroll
      for (int k = 0; k < K; ++k)
        if (r[k] == i) acc += w[k] * v;
    }
    mc[(size_t)i * S] = acc;
  }
}

// the checks and the grid both entry points share; per_channel: one grid plane per channel (the forward pass walks the channels
// inside the thread, with the weights of its sample)
int moveout_check(const char* what, const void* in, const void* tau, const void* range, const void* out, int interp, int C, int T, size_t S,
                  bool per_channel, dim3* grid) {
  DPI_REQUIRE(in && tau && range && out && in != out, "%s: null or aliased pointer", what);
  DPI_REQUIRE(interp == 0 || interp == 1, "%s: interp must be 0 (linear) or 1 (cubic), got %d", what, interp);
  DPI_REQUIRE(C >= 1 && T >= 1 && S >= 1, "%s: C, T and S must be >= 1, got %d, %d, %zu", what, C, T, S);
  const size_t bx = cdivz(S, MO_THREADS);
  // T <= 2^24: every row index is an exact float
  DPI_REQUIRE(C <= 65535 && T <= (1 << 24) && bx <= 0x7fffffffu && S <= (((size_t)1 << 60) / (size_t)T) / (size_t)C,
              "%s: a tensor of %d x %d x %zu samples is too large", what, C, T, S);
  *grid = dim3((unsigned)bx, (unsigned)(T < 65535 ? T : 65535), per_channel ? (unsigned)C : 1u);
  return DPI_OK;
}

}  // namespace

extern "C" int dpi_moveout_fwd(const float* m, const float* tau, int interp, int C, int T, size_t S, float* d, void* stream) {
  dim3 grid;
  if (int e = moveout_check("moveout_fwd", m, tau, tau, d, interp, C, T, S, false, &grid)) return e;
  if (interp) moveout_fwd_kernel<4><<<grid, MO_THREADS, 0, (hipStream_t)stream>>>(m, tau, C, T, S, d);
  else moveout_fwd_kernel<2><<<grid, MO_THREADS, 0, (hipStream_t)stream>>>(m, tau, C, T, S, d);
  return dpi_check_launch("moveout_fwd");
}

extern "C" int dpi_moveout_adj(const float* d, const float* tau, const int* range, int interp, int C, int T, size_t S, float* m,
                               void* stream) {
  dim3 grid;
  if (int e = moveout_check("moveout_adj", d, tau, range, m, interp, C, T, S, true, &grid)) return e;
  if (interp) moveout_adj_kernel<4><<<grid, MO_THREADS, 0, (hipStream_t)stream>>>(d, tau, range, T, S, m);
  else moveout_adj_kernel<2><<<grid, MO_THREADS, 0, (hipStream_t)stream>>>(d, tau, range, T, S, m);
  return dpi_check_launch("moveout_adj");
}
