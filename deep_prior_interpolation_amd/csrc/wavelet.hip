// The convolutional model of seismic data along the time axis (--wavelet): reference operators/signal.py:8-45 (VerticalConv) behind
// operators/derivative.py:8-21 (VerticalGrad), fused into one launch each way, on [C][T][S] fp32 tensors (S = X or X * Y).
//     forward: d[c][t][s] = sum_k taps[k] * u[c][t + K/2 - k][s]   (zero outside [0, T); the arithmetic of dpi_fir_axis0)
//              diff = 0: u = m;   diff = 1: u[t] = m[t + 1] - m[t] for t < T - 1, u[T - 1] = 0
//     adjoint: g[t] = sum_k taps[k] * d[t - K/2 + k];   diff = 0: m = g;   diff = 1: m[t] = -g[t] [t < T - 1] + g[t - 1] [t >= 1]
// fir_axis0_kernel reads K global values per output.  Here a workgroup of 256 threads owns WV_ROWS = 128 rows x WV_COLS = 64 columns of
// the output and stages the rows it needs once in LDS: 128 + (taps of the chunk - 1) rows of 64 floats, at most 193 rows = 48.25 KiB, so
// three workgroups share the 160 KiB of a CU.  A row of the tile is 256 bytes, all 64 banks once: a wave that reads one row with its 64
// lanes on consecutive columns has no bank conflict, and neither has the 16-byte staging write (16 lanes per row).
// The difference of the forward pass is taken while staging.  Staging uses 16-byte loads when S % 4 == 0 and the input starts on 16
// bytes, one element per lane otherwise; both put the same values into LDS, so both paths give the same bits.
// A thread owns one column and four groups of WV_R = 8 consecutive rows.  For a group it keeps the 8 inputs of the current tap in a
// register window: a step k is 8 FMAs and ONE new LDS value (the window slides by one row per tap; the slot an input sits in is a
// compile-time function of the unrolled step, so nothing moves): (K + 7) / 8 LDS reads per output instead of K.  Taps are read with a
// wave-uniform index from a read-only pointer, i.e. through the scalar cache into scalar registers.  Per output the taps are summed in
// ascending k into one fmaf chain starting from 0: the order of fir_axis0_kernel, whatever the tile.
// The adjoint is the same convolution with the taps read backwards.  Its difference comes AFTER the filter and needs g[t - 1] beside
// g[t]: those threads carry 9 sums for their 8 outputs (one more staged row, 1/8 more FMAs) instead of a second pass.
// Wavelets longer than WV_KC = 65 taps (K <= 255: up to 254 halo rows) are taken in chunks of 65 taps: the tile is staged again for every
// chunk and the sums stay in registers, so the LDS need does not grow with K and the order of the sum does not change.
#include "common.h"

namespace {

constexpr int WV_COLS = 64, WV_ROWS = 128, WV_R = 8, WV_KC = 65;
constexpr int WV_GROUPS = WV_ROWS / WV_R / 4;                 // row groups per thread: 4 waves share the 16 groups of a tile
constexpr int WV_LROWS = WV_ROWS + 1 + WV_KC - 1;             // staged rows at most: tile + the adjoint's extra row + halo of a chunk

// u[q][s .. s + N) of one channel plane x = [T][S]: the input itself, or (DIFF) its forward difference with the last row zero
template <bool DIFF>
__device__ __forceinline__ float wv_load1(const float* __restrict__ x, int q, int T, size_t S, size_t s) {
  if (DIFF) return (q >= 0 && q < T - 1) ? x[(size_t)(q + 1) * S + s] - x[(size_t)q * S + s] : 0.f;
  return (q >= 0 && q < T) ? x[(size_t)q * S + s] : 0.f;
}
template <bool DIFF>
__device__ __forceinline__ float4 wv_load4(const float* __restrict__ x, int q, int T, size_t S, size_t s) {
  if (DIFF) {
    if (q < 0 || q >= T - 1) return make_float4(0.f, 0.f, 0.f, 0.f);
    const float4 a = *reinterpret_cast<const float4*>(x + (size_t)(q + 1) * S + s), b = *reinterpret_cast<const float4*>(x + (size_t)q * S + s);
    return make_float4(a.x - b.x, a.y - b.y, a.z - b.z, a.w - b.w);
  }
  if (q < 0 || q >= T) return make_float4(0.f, 0.f, 0.f, 0.f);
  return *reinterpret_cast<const float4*>(x + (size_t)q * S + s);
}

// The kcn taps [kc0, kc0 + kcn) of one chunk for the NOUT sums of one row group.  lcol = the thread's column of the staged tile, whose
// row (gi + kcn - 1 - kl) holds the input of sum gi at the chunk's tap kl.  REV: the taps are read backwards (the adjoint).
template <int NOUT, bool REV>
__device__ __forceinline__ void wv_group(const float* lcol, const float* __restrict__ taps, int K, int kc0, int kcn, int gi0, float (&acc)[NOUT]) {
  const float* top = lcol + (gi0 + kcn - 1) * WV_COLS;
  float win[NOUT];                                            // slot (q mod NOUT) holds the row top + q, q = r - kl
#pragma unroll
  for (int q = 0; q < NOUT; ++q) win[q] = top[q * WV_COLS];
  int kl = 0;
  for (; kl + NOUT <= kcn; kl += NOUT) {
#pragma unroll
    for (int i = 0; i < NOUT; ++i) {
      const int k = kc0 + kl + i;
      const float w = taps[REV ? K - 1 - k : k];
#pragma unroll
      for (int r = 0; r < NOUT; ++r) acc[r] = fmaf(w, win[(r - i + NOUT) % NOUT], acc[r]);
      if (kl + i + 1 < kcn) win[NOUT - 1 - i] = top[-(kl + i + 1) * WV_COLS];          // the row the next tap adds below the window
    }
  }
#pragma unroll
  for (int i = 0; i < NOUT - 1; ++i) {                        // the last kcn % NOUT taps
    if (kl + i < kcn) {
      const int k = kc0 + kl + i;
      const float w = taps[REV ? K - 1 - k : k];
#pragma unroll
      for (int r = 0; r < NOUT; ++r) acc[r] = fmaf(w, win[(r - i + NOUT) % NOUT], acc[r]);
      if (kl + i + 1 < kcn) win[NOUT - 1 - i] = top[-(kl + i + 1) * WV_COLS];
    }
  }
}

// grid (columns / 64, rows / 128, C).  ADJ = 0: out = W (D) in;  ADJ = 1: out = (D^T) W^T in.
template <bool ADJ, bool DIFF>
__global__ __launch_bounds__(256) void wavelet_kernel(const float* __restrict__ in, const float* __restrict__ taps, int K, int T, size_t S,
                                                      int vec, float* __restrict__ out) {
  constexpr int E = (ADJ && DIFF) ? 1 : 0;                    // sums in front of the tile's first row: g[t0 - 1]
  constexpr int NOUT = WV_R + E;
  __shared__ __attribute__((aligned(16))) float lds[WV_LROWS * WV_COLS];
  const size_t plane = (size_t)T * S;
  const float* __restrict__ x = in + (size_t)blockIdx.z * plane;
  float* __restrict__ y = out + (size_t)blockIdx.z * plane;
  const int t0 = (int)blockIdx.y * WV_ROWS;
  const size_t s0 = (size_t)blockIdx.x * WV_COLS;
  const int col = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int p = K / 2;
  float acc[WV_GROUPS][NOUT];
#pragma unroll
  for (int g = 0; g < WV_GROUPS; ++g)
#pragma unroll
    for (int r = 0; r < NOUT; ++r) acc[g][r] = 0.f;

  for (int kc0 = 0; kc0 < K; kc0 += WV_KC) {
    const int kcn = K - kc0 < WV_KC ? K - kc0 : WV_KC;
    const int lrows = WV_ROWS + E + kcn - 1;                  // <= WV_LROWS
    const int base = t0 - E + p - (kc0 + kcn - 1);            // the input row staged as row 0: sum gi (row t0 - E + gi) reads row gi + kcn - 1 - kl
    if (kc0) __syncthreads();                                 // every wave is done with the previous chunk's tile
    if (vec) {
      const int cv = (threadIdx.x & 15) * 4;
      const size_t s = s0 + cv;
      for (int lr = threadIdx.x >> 4; lr < lrows; lr += 16) {
        // S % 4 == 0: four columns are inside together or not at all
        const float4 v = s < S ? wv_load4<DIFF && !ADJ>(x, base + lr, T, S, s) : make_float4(0.f, 0.f, 0.f, 0.f);
        *reinterpret_cast<float4*>(&lds[lr * WV_COLS + cv]) = v;
      }
    } else {
      const size_t s = s0 + col;
      for (int lr = wv; lr < lrows; lr += 4) lds[lr * WV_COLS + col] = s < S ? wv_load1<DIFF && !ADJ>(x, base + lr, T, S, s) : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int g = 0; g < WV_GROUPS; ++g) {
      const int gi0 = (g * 4 + wv) * WV_R;
      if (t0 + gi0 < T) wv_group<NOUT, ADJ>(lds + col, taps, K, kc0, kcn, gi0, acc[g]);          // wave-uniform
    }
  }

  const size_t s = s0 + col;
  if (s >= S) return;
#pragma unroll
  for (int g = 0; g < WV_GROUPS; ++g) {
    const int tg = t0 + (g * 4 + wv) * WV_R;
#pragma unroll
    for (int r = 0; r < WV_R; ++r) {
      const int t = tg + r;
      if (t < T) {
        float v;
        if (E) v = (t < T - 1 ? -acc[g][r + E] : 0.f) + (t >= 1 ? acc[g][r] : 0.f);          // acc[r] = g[t - 1], acc[r + 1] = g[t]
        else v = acc[g][r];
        y[(size_t)t * S + s] = v;
      }
    }
  }
}

int wavelet_launch(const char* what, bool adj, const float* in, const float* taps, int K, int diff, int C, int T, size_t S, float* out,
                   void* stream) {
  DPI_REQUIRE(in && taps && out && in != out, "%s: null or aliased pointer", what);
  DPI_REQUIRE(K >= 1 && K <= 255 && (K & 1), "%s: K must be odd and lie in [1, 255], got %d", what, K);
  DPI_REQUIRE(diff == 0 || diff == 1, "%s: diff must be 0 or 1, got %d", what, diff);
  DPI_REQUIRE(C >= 1 && T >= 1 && S >= 1, "%s: C, T and S must be >= 1, got %d, %d, %zu", what, C, T, S);
  const size_t bx = cdivz(S, WV_COLS), by = cdivz((size_t)T, WV_ROWS);
  DPI_REQUIRE(C <= 65535 && by <= 65535 && bx <= 0x7fffffffu && S <= (((size_t)1 << 60) / (size_t)T) / (size_t)C,
              "%s: a tensor of %d x %d x %zu samples is too large", what, C, T, S);
  const dim3 grid((unsigned)bx, (unsigned)by, (unsigned)C);
  const int vec = S % 4 == 0 && reinterpret_cast<uintptr_t>(in) % 16 == 0;
  hipStream_t st = (hipStream_t)stream;
  if (!adj) {
    if (diff) wavelet_kernel<false, true><<<grid, 256, 0, st>>>(in, taps, K, T, S, vec, out);
    else wavelet_kernel<false, false><<<grid, 256, 0, st>>>(in, taps, K, T, S, vec, out);
  } else {
    if (diff) wavelet_kernel<true, true><<<grid, 256, 0, st>>>(in, taps, K, T, S, vec, out);
    else wavelet_kernel<true, false><<<grid, 256, 0, st>>>(in, taps, K, T, S, vec, out);
  }
  return dpi_check_launch(what);
}

}  // namespace

extern "C" int dpi_wavelet_fwd(const float* m, const float* taps, int K, int diff, int C, int T, size_t S, float* d, void* stream) {
  return wavelet_launch("wavelet_fwd", false, m, taps, K, diff, C, T, S, d, stream);
}

extern "C" int dpi_wavelet_adj(const float* d, const float* taps, int K, int diff, int C, int T, size_t S, float* m, void* stream) {
  return wavelet_launch("wavelet_adj", true, d, taps, K, diff, C, T, S, m, stream);
}
