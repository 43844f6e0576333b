// Ops used only by the plain 3-D UNet (architectures/unet.py, UNet3D): MaxPool3d(2, 2) and ConvTranspose3d(Cin, Cout, kernel 4, stride 2,
// padding 1) with their backward passes.  In 3-D the transposed convolutions are on the hot path, so where Cin and Cout are
// multiples of 16 they run on v_mfma_f32_16x16x4_f32; every other channel count takes one-thread-per-output VALU kernels.
//
// A k = 4, s = 2, p = 1 transposed convolution is eight independent 2x2x2 convolutions on the COARSE (input) grid, one per output-parity
// class p = (pd, ph, pw): output voxel o = 2 q + p of an axis reads, for its two taps a = 0, 1,
//     p = 0:  k = 1 + 2a, input q - a          p = 1:  k = 2 - 2a, input q + a
// so Y_p[co][q] = sum_{ci, a, b, c} W[ci][co][kd][kh][kw] X[ci][q + off]: a GEMM with M = Cout, K = 8 Cin, N = coarse voxels.
//   forward          one workgroup = 16 output channels x (1 x 8 x 16) coarse voxels x all 8 classes, which share one haloed input tile
//                    (3 x 10 x 18 per channel); K runs over chunks of 4 input channels staged in LDS with their 4 x 16 x 64 weights.
//   backward-data    dx[ci][q] = sum over the 8 classes and their 8 taps = all 64 taps of the 4 x 4 x 4 window of dy around 2 q: M = Cin,
//                    K = 64 Cout; the dy tile is stored de-interleaved in w (even / odd columns apart) so that 16 lanes read 16 banks.
//   backward-weight  dw[ci][co][tap] = sum_q x[ci][q] dy[co][2 q - 1 + k]: M = 16 ci, N = 16 co, K = voxels, one accumulator per tap
//                    (wave kd holds the 16 taps (kh, kw)); a workgroup sums a fixed range of (d, h-pair, w-block) units into its slice of
//                    the workspace and dpi_reduce_chunks adds the slices in order: no atomics, the same bits on every launch.
// MFMA operand maps (16x16x4 f32): A[i = lane & 15][k = lane >> 4], B[k = lane >> 4][j = lane & 15], D[row = 4 (lane >> 4) + r][col = lane & 15].
// LDS strides are chosen so that the four k-groups of a wave land in different banks (stride = 16 or 4 modulo 64).
#include "common.h"

namespace {

// ---- MaxPool 2x2x2, stride 2, floor mode; ties resolve to the first element in (kd, kh, kw) scan order like aten --------------------
__global__ __launch_bounds__(256) void maxpool3_fwd_kernel(const float* __restrict__ x, int D, int H, int W, int Do, int Ho, int Wo,
                                                           float* __restrict__ y) {
  const int c = blockIdx.y;
  const size_t Vo = (size_t)Do * Ho * Wo, HW = (size_t)H * W;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < Vo; i += (size_t)gridDim.x * 256) {
    const int ow = i % Wo, oh = (i / Wo) % Ho, od = i / ((size_t)Wo * Ho);
    const float* p = x + (size_t)c * D * HW + (size_t)(2 * od) * HW + (size_t)(2 * oh) * W + 2 * ow;
    float m = p[0];
#pragma unroll
    for (int t = 1; t < 8; ++t) {
      const float v = p[(size_t)(t >> 2) * HW + (size_t)((t >> 1) & 1) * W + (t & 1)];
      m = v > m ? v : m;
    }
    y[(size_t)c * Vo + i] = m;
  }
}

__global__ __launch_bounds__(256) void maxpool3_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ x, int D, int H, int W,
                                                           int Do, int Ho, int Wo, float* __restrict__ dx) {
  const int c = blockIdx.y;
  const size_t HW = (size_t)H * W, V = (size_t)D * HW;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < V; i += (size_t)gridDim.x * 256) {
    const int w = i % W, h = (i / W) % H, d = i / HW;
    const int od = d >> 1, oh = h >> 1, ow = w >> 1;
    float g = 0.f;
    if (od < Do && oh < Ho && ow < Wo) {
      const float* p = x + (size_t)c * V + (size_t)(2 * od) * HW + (size_t)(2 * oh) * W + 2 * ow;
      int arg = 0;
      float m = p[0];
#pragma unroll
      for (int t = 1; t < 8; ++t) {
        const float v = p[(size_t)(t >> 2) * HW + (size_t)((t >> 1) & 1) * W + (t & 1)];
        if (v > m) { m = v; arg = t; }
      }
      if (arg == ((d & 1) * 4 + (h & 1) * 2 + (w & 1))) g = dy[(size_t)c * Do * Ho * Wo + ((size_t)od * Ho + oh) * Wo + ow];
    }
    dx[(size_t)c * V + i] = g;
  }
}

// ---- ConvTranspose3d k=4 s=2 p=1, VALU path (any channel count): one thread per output ----------------------------------------------
__global__ __launch_bounds__(256) void deconv3_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                          const float* __restrict__ bias, int Cin, int Cout, int D, int H, int W,
                                                          float* __restrict__ y) {
  const int co = blockIdx.y, Ho = 2 * H, Wo = 2 * W;
  const size_t V = (size_t)D * H * W, Vo = 8 * V;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < Vo; i += (size_t)gridDim.x * 256) {
    const int ow = i % Wo, oh = (i / Wo) % Ho, od = i / ((size_t)Wo * Ho);
    float acc = bias ? bias[co] : 0.f;
    for (int a = 0; a < 2; ++a) {
      const int kd = ((od + 1) & 1) + 2 * a, id = (od + 1 - kd) >> 1;
      if (od + 1 - kd < 0 || id >= D) continue;
      for (int b = 0; b < 2; ++b) {
        const int kh = ((oh + 1) & 1) + 2 * b, ih = (oh + 1 - kh) >> 1;
        if (oh + 1 - kh < 0 || ih >= H) continue;
        for (int c = 0; c < 2; ++c) {
          const int kw = ((ow + 1) & 1) + 2 * c, iw = (ow + 1 - kw) >> 1;
          if (ow + 1 - kw < 0 || iw >= W) continue;
          const float* xp = x + ((size_t)id * H + ih) * W + iw;
          const float* wp = w + (size_t)co * 64 + (kd * 4 + kh) * 4 + kw;
          for (int ci = 0; ci < Cin; ++ci) acc = fmaf(xp[(size_t)ci * V], wp[(size_t)ci * Cout * 64], acc);
        }
      }
    }
    y[(size_t)co * Vo + i] = acc;
  }
}

__global__ __launch_bounds__(256) void deconv3_bwd_data_kernel(const float* __restrict__ dy, const float* __restrict__ w, int Cin, int Cout,
                                                               int D, int H, int W, float* __restrict__ dx) {
  const int ci = blockIdx.y, Do = 2 * D, Ho = 2 * H, Wo = 2 * W;
  const size_t V = (size_t)D * H * W, Vo = 8 * V;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < V; i += (size_t)gridDim.x * 256) {
    const int iw = i % W, ih = (i / W) % H, id = i / ((size_t)W * H);
    float acc = 0.f;
    for (int kd = 0; kd < 4; ++kd) {
      const int od = 2 * id - 1 + kd;
      if (od < 0 || od >= Do) continue;
      for (int kh = 0; kh < 4; ++kh) {
        const int oh = 2 * ih - 1 + kh;
        if (oh < 0 || oh >= Ho) continue;
        for (int kw = 0; kw < 4; ++kw) {
          const int ow = 2 * iw - 1 + kw;
          if (ow < 0 || ow >= Wo) continue;
          const float* gp = dy + ((size_t)od * Ho + oh) * Wo + ow;
          const float* wp = w + (size_t)ci * Cout * 64 + (kd * 4 + kh) * 4 + kw;
          for (int co = 0; co < Cout; ++co) acc = fmaf(gp[(size_t)co * Vo], wp[(size_t)co * 64], acc);
        }
      }
    }
    dx[(size_t)ci * V + i] = acc;
  }
}

// one block per (ci, co, kd): 16 tap accumulators per thread, then a fixed-order block reduction
__global__ __launch_bounds__(256) void deconv3_bwd_weight_kernel(const float* __restrict__ x, const float* __restrict__ dy, int Cin, int Cout,
                                                                 int D, int H, int W, float* __restrict__ dw) {
  const int kd = blockIdx.x & 3, pair = blockIdx.x >> 2, ci = pair / Cout, co = pair % Cout;
  const int Do = 2 * D, Ho = 2 * H, Wo = 2 * W;
  const size_t V = (size_t)D * H * W, Vo = 8 * V;
  float acc[16];
#pragma unroll
  for (int t = 0; t < 16; ++t) acc[t] = 0.f;
  for (size_t i = threadIdx.x; i < V; i += 256) {
    const int iw = i % W, ih = (i / W) % H, id = i / ((size_t)W * H);
    const int od = 2 * id - 1 + kd;
    if (od < 0 || od >= Do) continue;
    const float xv = x[(size_t)ci * V + i];
#pragma unroll
    for (int kh = 0; kh < 4; ++kh) {
      const int oh = 2 * ih - 1 + kh;
#pragma unroll
      for (int kw = 0; kw < 4; ++kw) {
        const int ow = 2 * iw - 1 + kw;
        if (oh >= 0 && oh < Ho && ow >= 0 && ow < Wo)
          acc[kh * 4 + kw] = fmaf(xv, dy[(size_t)co * Vo + ((size_t)od * Ho + oh) * Wo + ow], acc[kh * 4 + kw]);
      }
    }
  }
  __shared__ float red[4][16];
#pragma unroll
  for (int t = 0; t < 16; ++t) {
    const float r = wave_sum(acc[t]);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][t] = r;
  }
  __syncthreads();
  if (threadIdx.x < 16)
    dw[((size_t)ci * Cout + co) * 64 + kd * 16 + threadIdx.x] = red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
}

// ---- MFMA path (Cin % 16 == 0 and Cout % 16 == 0) ------------------------------------------------------------------------------------
typedef float f32x4 __attribute__((ext_vector_type(4)));
constexpr int TH = 8, TW = 16;            // coarse voxels of one workgroup: 1 x TH x TW, two rows per wave
constexpr int WTS = 20;                   // LDS weight tile [k 4][tap 64][WTS]: 16 rows used; 4 taps apart = 80 floats = 16 banks apart
constexpr int WKS = 64 * WTS + 16;        // 1296 = 16 (mod 64)
constexpr int XHW = (TH + 2) * (TW + 2);  // forward: haloed input tile [3][TH + 2][TW + 2] per channel
constexpr int XCS = 592;                  // >= 3 * XHW = 540, = 16 (mod 64)
constexpr int GRW = 2 * TW + 2;           // backward: a fine row of 34 = 2 x 17 (even columns, then odd columns)
constexpr int GCS = 4 * (2 * TH + 2) * GRW;   // backward-data: dy tile [4][2 TH + 2][2][17] per channel = 2448 = 16 (mod 64)
static_assert(XCS >= 3 * XHW && XCS % 64 == 16 && WKS % 64 == 16 && GCS % 64 == 16, "LDS strides");

// Global -> LDS staging of N elements by 256 threads, U loads of a thread in flight at once.  f(idx, off, dst) gives element idx its LDS index
// and, when it lies inside the tensor (return value), its global offset; elements outside are staged as 0.  The loads are unconditional
// (an outside element reads g[0], which every tensor has) so that U of them are issued back to back: a loop with one guarded load per
// trip waits for every load before it issues the next, and the staging phase then costs U round trips instead of one.
template <int N, int U, class F>
__device__ __forceinline__ void stage_tile(const float* __restrict__ g, float* __restrict__ lds, F f) {
  for (int base = threadIdx.x; base < N; base += 256 * U) {
    float v[U];
    int dst[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int idx = base + u * 256;
      size_t off = 0;
      dst[u] = -1;
      bool ok = false;
      if (idx < N) ok = f(idx, off, dst[u]);
      const float t = g[ok ? off : 0];
      v[u] = ok ? t : 0.f;
    }
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (dst[u] >= 0) lds[dst[u]] = v[u];
  }
}

// 4 x 16 x 64 weights w[(r0 + k or i) ...] -> ws[k][tap][i]; ROWS_CI: the 16 rows i are input channels (backward-data), else output channels.
// Thread f: row i = f % 16, tap group (f / 16) % 16, k = f / 256: a wave reads 16 rows x 64 B and writes 16 consecutive floats per tap.
template <bool ROWS_CI>
__device__ __forceinline__ void stage_w(const float* __restrict__ w, int Cout, int ci0, int co0, float* __restrict__ ws, bool vec) {
  const int i = threadIdx.x & 15, tg = threadIdx.x >> 4;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const size_t g = ROWS_CI ? ((size_t)(ci0 + i) * Cout + co0 + k) * 64 + tg * 4 : ((size_t)(ci0 + k) * Cout + co0 + i) * 64 + tg * 4;
    float4 v;
    if (vec) v = *reinterpret_cast<const float4*>(w + g);
    else v = make_float4(w[g], w[g + 1], w[g + 2], w[g + 3]);
    float* o = ws + k * WKS + tg * 4 * WTS + i;
    o[0] = v.x; o[WTS] = v.y; o[2 * WTS] = v.z; o[3 * WTS] = v.w;
  }
}

__global__ __launch_bounds__(256) void deconv3_fwd_mfma_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                               const float* __restrict__ bias, int Cin, int Cout, int D, int H, int W,
                                                               int nH, int nW, float* __restrict__ y) {
  __shared__ float xs[4 * XCS];
  __shared__ float ws[4 * WKS];
  const int wb = blockIdx.x % nW, hb = (blockIdx.x / nW) % nH, d = blockIdx.x / (nW * nH);
  const int h0 = hb * TH, w0 = wb * TW, co0 = blockIdx.y * 16;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, lj = lane & 15, lk = lane >> 4;
  const size_t V = (size_t)D * H * W;
  const bool vec = (reinterpret_cast<uintptr_t>(w) & 15) == 0;
  f32x4 acc[8][2];
#pragma unroll
  for (int p = 0; p < 8; ++p)
#pragma unroll
    for (int n = 0; n < 2; ++n) acc[p][n] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int c0 = 0; c0 < Cin; c0 += 4) {
    __syncthreads();
    stage_tile<4 * 3 * XHW, 9>(x, xs, [&](int idx, size_t& off, int& dst) {
      const int k = idx / (3 * XHW), r = idx % (3 * XHW);
      const int gd = d - 1 + r / XHW, gh = h0 - 1 + (r % XHW) / (TW + 2), gw = w0 - 1 + r % (TW + 2);
      dst = k * XCS + r;
      off = (size_t)(c0 + k) * V + ((size_t)gd * H + gh) * W + gw;
      return gd >= 0 && gd < D && gh >= 0 && gh < H && gw >= 0 && gw < W;
    });
    stage_w<false>(w, Cout, c0, co0, ws, vec);
    __syncthreads();
    // this wave's rows 2 wv, 2 wv + 1 read halo rows 2 wv .. 2 wv + 3; three depth planes; three column shifts
    float b[3][4][3];
#pragma unroll
    for (int dd = 0; dd < 3; ++dd)
#pragma unroll
      for (int hh = 0; hh < 4; ++hh)
#pragma unroll
        for (int s = 0; s < 3; ++s) b[dd][hh][s] = xs[lk * XCS + dd * XHW + (2 * wv + hh) * (TW + 2) + lj + s];
#pragma unroll
    for (int p = 0; p < 8; ++p) {
      const int pd = p >> 2, ph = (p >> 1) & 1, pw = p & 1;
#pragma unroll
      for (int t = 0; t < 8; ++t) {
        const int a = t >> 2, bb = (t >> 1) & 1, c = t & 1;
        const int kd = pd ? 2 - 2 * a : 1 + 2 * a, kh = ph ? 2 - 2 * bb : 1 + 2 * bb, kw = pw ? 2 - 2 * c : 1 + 2 * c;
        const int od = 1 + (pd ? a : -a), oh = 1 + (ph ? bb : -bb), ow = 1 + (pw ? c : -c);      // halo offsets of the tap's input
        const float av = ws[lk * WKS + ((kd * 4 + kh) * 4 + kw) * WTS + lj];
#pragma unroll
        for (int n = 0; n < 2; ++n) acc[p][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, b[od][n + oh][ow], acc[p][n], 0, 0, 0);
      }
    }
  }
  // epilogue: D row = co0 + 4 lk + r, D column = coarse voxel w0 + lj of row h0 + 2 wv + n
  const int Ho = 2 * H, Wo = 2 * W;
  const size_t Vo = 8 * V;
  const bool pairs = (reinterpret_cast<uintptr_t>(y) & 7) == 0;
  if (w0 + lj < W) {
#pragma unroll
    for (int n = 0; n < 2; ++n) {
      const int h = h0 + 2 * wv + n;
      if (h >= H) continue;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int co = co0 + 4 * lk + r;
        const float bv = bias ? bias[co] : 0.f;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int pd = q >> 1, ph = q & 1;
          float* o = y + (size_t)co * Vo + ((size_t)(2 * d + pd) * Ho + 2 * h + ph) * Wo + 2 * (w0 + lj);
          const float v0 = acc[2 * q][n][r] + bv, v1 = acc[2 * q + 1][n][r] + bv;
          if (pairs) *reinterpret_cast<float2*>(o) = make_float2(v0, v1);
          else { o[0] = v0; o[1] = v1; }
        }
      }
    }
  }
}

__global__ __launch_bounds__(256) void deconv3_bwd_data_mfma_kernel(const float* __restrict__ dy, const float* __restrict__ w, int Cin, int Cout,
                                                                    int D, int H, int W, int nH, int nW, float* __restrict__ dx) {
  __shared__ float gs[4 * GCS];
  __shared__ float ws[4 * WKS];
  const int wb = blockIdx.x % nW, hb = (blockIdx.x / nW) % nH, d = blockIdx.x / (nW * nH);
  const int h0 = hb * TH, w0 = wb * TW, ci0 = blockIdx.y * 16;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, lj = lane & 15, lk = lane >> 4;
  const int Do = 2 * D, Ho = 2 * H, Wo = 2 * W;
  const size_t V = (size_t)D * H * W, Vo = 8 * V;
  const bool vec = (reinterpret_cast<uintptr_t>(w) & 15) == 0;
  constexpr int PL = (2 * TH + 2) * GRW;      // one fine depth plane of the tile
  f32x4 acc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};

  for (int c0 = 0; c0 < Cout; c0 += 4) {
    __syncthreads();
    stage_tile<4 * GCS, 10>(dy, gs, [&](int idx, size_t& off, int& dst) {
      const int k = idx / GCS, r = idx % GCS;
      const int e = r / PL, f = (r % PL) / GRW, g = r % GRW;
      const int od = 2 * d - 1 + e, oh = 2 * h0 - 1 + f, ow = 2 * w0 - 1 + g;
      dst = k * GCS + e * PL + f * GRW + (g & 1) * 17 + (g >> 1);
      off = (size_t)(c0 + k) * Vo + ((size_t)od * Ho + oh) * Wo + ow;
      return od >= 0 && od < Do && oh >= 0 && oh < Ho && ow >= 0 && ow < Wo;
    });
    stage_w<true>(w, Cout, ci0, c0, ws, vec);
    __syncthreads();
#pragma unroll
    for (int kd = 0; kd < 4; ++kd)
#pragma unroll
      for (int kh = 0; kh < 4; ++kh)
#pragma unroll
        for (int kw = 0; kw < 4; ++kw) {
          const float av = ws[lk * WKS + ((kd * 4 + kh) * 4 + kw) * WTS + lj];
#pragma unroll
          for (int n = 0; n < 2; ++n) {
            const float bv = gs[lk * GCS + kd * PL + (2 * (2 * wv + n) + kh) * GRW + (kw & 1) * 17 + (kw >> 1) + lj];
            acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc[n], 0, 0, 0);
          }
        }
  }
  if (w0 + lj < W) {
#pragma unroll
    for (int n = 0; n < 2; ++n) {
      const int h = h0 + 2 * wv + n;
      if (h >= H) continue;
#pragma unroll
      for (int r = 0; r < 4; ++r) dx[(size_t)(ci0 + 4 * lk + r) * V + ((size_t)d * H + h) * W + w0 + lj] = acc[n][r];
    }
  }
}

// backward-weight: one unit = 2 coarse rows x 16 columns of one depth plane
constexpr int BXS = 36;                       // x tile [16 ci][2 x 16], = 4 (mod 8): 16 rows x 4 voxels in 64 banks
constexpr int BPL = 6 * GRW;                  // dy tile [16 co][4 od][6 oh][2][17]
constexpr int BGS = 836;                      // >= 4 * BPL = 816, = 4 (mod 64)
static_assert(BGS >= 4 * BPL && BGS % 64 == 4, "LDS strides");

__global__ __launch_bounds__(256) void deconv3_bwd_weight_mfma_kernel(const float* __restrict__ x, const float* __restrict__ dy, int Cin, int Cout,
                                                                      int D, int H, int W, int nH2, int nW, int units, int upc,
                                                                      float* __restrict__ part) {
  __shared__ float xs[16 * BXS];
  __shared__ float gs[16 * BGS];
  const int ci0 = blockIdx.x * 16, co0 = blockIdx.y * 16, chunk = blockIdx.z;
  const int lane = threadIdx.x & 63, kd = threadIdx.x >> 6, lj = lane & 15, lk = lane >> 4;
  const int Do = 2 * D, Ho = 2 * H, Wo = 2 * W;
  const size_t V = (size_t)D * H * W, Vo = 8 * V;
  f32x4 acc[16];
#pragma unroll
  for (int t = 0; t < 16; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int u1 = min(units, (chunk + 1) * upc);
  for (int u = chunk * upc; u < u1; ++u) {
    const int wb = u % nW, hb = (u / nW) % nH2, d = u / (nW * nH2);
    const int h0 = 2 * hb, w0 = wb * TW;
    __syncthreads();
    stage_tile<16 * 32, 2>(x, xs, [&](int idx, size_t& off, int& dst) {
      const int c = idx >> 5, n = (idx >> 4) & 1, j = idx & 15;
      dst = c * BXS + n * 16 + j;
      off = (size_t)(ci0 + c) * V + ((size_t)d * H + h0 + n) * W + w0 + j;
      return h0 + n < H && w0 + j < W;
    });
    stage_tile<16 * 4 * BPL, 13>(dy, gs, [&](int idx, size_t& off, int& dst) {
      const int c = idx / (4 * BPL), r = idx % (4 * BPL);
      const int e = r / BPL, f = (r % BPL) / GRW, g = r % GRW;
      const int od = 2 * d - 1 + e, oh = 2 * h0 - 1 + f, ow = 2 * w0 - 1 + g;
      dst = c * BGS + e * BPL + f * GRW + (g & 1) * 17 + (g >> 1);
      off = (size_t)(co0 + c) * Vo + ((size_t)od * Ho + oh) * Wo + ow;
      return od >= 0 && od < Do && oh >= 0 && oh < Ho && ow >= 0 && ow < Wo;
    });
    __syncthreads();
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const float av = xs[lj * BXS + n * 16 + 4 * s + lk];          // A[i = ci][k = voxel 4 s + lk of row n]
#pragma unroll
        for (int kh = 0; kh < 4; ++kh)
#pragma unroll
          for (int kw = 0; kw < 4; ++kw) {
            const float bv = gs[lj * BGS + kd * BPL + (2 * n + kh) * GRW + (kw & 1) * 17 + (kw >> 1) + 4 * s + lk];   // B[k = voxel][j = co]
            acc[kh * 4 + kw] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc[kh * 4 + kw], 0, 0, 0);
          }
      }
  }
  float* o = part + (size_t)chunk * Cin * Cout * 64;
#pragma unroll
  for (int t = 0; t < 16; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) o[((size_t)(ci0 + 4 * lk + r) * Cout + co0 + lj) * 64 + kd * 16 + t] = acc[t][r];
}

inline unsigned nb(size_t n) { size_t b = cdivz(n, 256); if (b > 2048) b = 2048; if (b < 1) b = 1; return (unsigned)b; }

constexpr long long IDX_MAX = 0x7fffffffll;
// every tensor of a call within the 32-bit index range (the VALU kernels split flat indices with 32-bit results, the grids are 32-bit)
inline bool deconv_geom_ok(int Cin, int Cout, int D, int H, int W) {
  if (Cin <= 0 || Cout <= 0 || D <= 0 || H <= 0 || W <= 0) return false;
  const long long V = (long long)D * H * W;
  if (V > IDX_MAX / 8) return false;
  return (long long)Cin * V <= IDX_MAX && (long long)Cout * 8 * V <= IDX_MAX && (long long)Cin * Cout * 64 <= IDX_MAX;
}
inline bool use_mfma(int Cin, int Cout) { return Cin % 16 == 0 && Cout % 16 == 0; }

struct BwwPlan { int nH2, nW, units, upc, nchunks; };
inline BwwPlan bww_plan(int Cin, int Cout, int D, int H, int W) {
  BwwPlan p;
  p.nH2 = cdiv(H, 2); p.nW = cdiv(W, TW);
  const long long units = (long long)D * p.nH2 * p.nW;          // <= V <= 2^28
  const long long tiles = (long long)(Cin / 16) * (Cout / 16);
  long long want = 1024 / tiles; if (want < 1) want = 1; if (want > units) want = units;
  p.units = (int)units;
  p.upc = (int)((units + want - 1) / want);
  p.nchunks = (int)((units + p.upc - 1) / p.upc);
  return p;
}

}  // namespace

extern "C" int dpi_maxpool2x2x2_fwd(const float* x, int C, int D, int H, int W, float* y, void* stream) {
  DPI_REQUIRE(x && y && x != y, "maxpool3d_fwd: null or aliased pointer");
  DPI_REQUIRE(C > 0 && D >= 2 && H >= 2 && W >= 2 && C <= 65535, "maxpool3d_fwd: bad size (C=%d D=%d H=%d W=%d)", C, D, H, W);
  DPI_REQUIRE((long long)C * D * H * W <= IDX_MAX, "maxpool3d_fwd: %lld elements are past the index range", (long long)C * D * H * W);
  maxpool3_fwd_kernel<<<dim3(nb((size_t)(D / 2) * (H / 2) * (W / 2)), C), 256, 0, (hipStream_t)stream>>>(x, D, H, W, D / 2, H / 2, W / 2, y);
  return dpi_check_launch("maxpool3d_fwd");
}
extern "C" int dpi_maxpool2x2x2_bwd(const float* dy, const float* x, int C, int D, int H, int W, float* dx, void* stream) {
  DPI_REQUIRE(dy && x && dx && dx != dy && dx != x, "maxpool3d_bwd: null or aliased pointer");
  DPI_REQUIRE(C > 0 && D >= 2 && H >= 2 && W >= 2 && C <= 65535, "maxpool3d_bwd: bad size (C=%d D=%d H=%d W=%d)", C, D, H, W);
  DPI_REQUIRE((long long)C * D * H * W <= IDX_MAX, "maxpool3d_bwd: %lld elements are past the index range", (long long)C * D * H * W);
  maxpool3_bwd_kernel<<<dim3(nb((size_t)D * H * W), C), 256, 0, (hipStream_t)stream>>>(dy, x, D, H, W, D / 2, H / 2, W / 2, dx);
  return dpi_check_launch("maxpool3d_bwd");
}

extern "C" int dpi_deconv4x4x4s2_fwd(const float* x, const float* w, const float* bias, int Cin, int Cout, int D, int H, int W, float* y,
                                     void* stream) {
  DPI_REQUIRE(x && w && y && y != x && y != w && y != bias, "deconv3d_fwd: null or aliased pointer");
  DPI_REQUIRE(deconv_geom_ok(Cin, Cout, D, H, W) && Cin <= 65535 && Cout <= 65535,
              "deconv3d_fwd: bad size or past the index range (Cin=%d Cout=%d D=%d H=%d W=%d)", Cin, Cout, D, H, W);
  if (use_mfma(Cin, Cout)) {
    const int nH = cdiv(H, TH), nW = cdiv(W, TW);
    deconv3_fwd_mfma_kernel<<<dim3((unsigned)((size_t)D * nH * nW), Cout / 16), 256, 0, (hipStream_t)stream>>>(x, w, bias, Cin, Cout, D, H, W, nH, nW, y);
  } else {
    deconv3_fwd_kernel<<<dim3(nb((size_t)8 * D * H * W), Cout), 256, 0, (hipStream_t)stream>>>(x, w, bias, Cin, Cout, D, H, W, y);
  }
  return dpi_check_launch("deconv3d_fwd");
}
extern "C" int dpi_deconv4x4x4s2_bwd_data(const float* dy, const float* w, int Cin, int Cout, int D, int H, int W, float* dx, void* stream) {
  DPI_REQUIRE(dy && w && dx && dx != dy && dx != w, "deconv3d_bwd_data: null or aliased pointer");
  DPI_REQUIRE(deconv_geom_ok(Cin, Cout, D, H, W) && Cin <= 65535 && Cout <= 65535,
              "deconv3d_bwd_data: bad size or past the index range (Cin=%d Cout=%d D=%d H=%d W=%d)", Cin, Cout, D, H, W);
  if (use_mfma(Cin, Cout)) {
    const int nH = cdiv(H, TH), nW = cdiv(W, TW);
    deconv3_bwd_data_mfma_kernel<<<dim3((unsigned)((size_t)D * nH * nW), Cin / 16), 256, 0, (hipStream_t)stream>>>(dy, w, Cin, Cout, D, H, W, nH, nW, dx);
  } else {
    deconv3_bwd_data_kernel<<<dim3(nb((size_t)D * H * W), Cin), 256, 0, (hipStream_t)stream>>>(dy, w, Cin, Cout, D, H, W, dx);
  }
  return dpi_check_launch("deconv3d_bwd_data");
}
extern "C" size_t dpi_deconv4x4x4s2_bwd_weight_ws_floats(int Cin, int Cout, int D, int H, int W) {
  if (!deconv_geom_ok(Cin, Cout, D, H, W)) return 0;
  if (!use_mfma(Cin, Cout)) return 16;      // the VALU path reduces inside its blocks; a token buffer keeps 0 for bad geometry alone
  return (size_t)bww_plan(Cin, Cout, D, H, W).nchunks * Cin * Cout * 64;
}
extern "C" int dpi_deconv4x4x4s2_bwd_weight(const float* x, const float* dy, int Cin, int Cout, int D, int H, int W, float* dw, float* ws,
                                            void* stream) {
  DPI_REQUIRE(x && dy && dw && ws && dw != x && dw != dy && ws != x && ws != dy && ws != dw, "deconv3d_bwd_weight: null or aliased pointer");
  DPI_REQUIRE(deconv_geom_ok(Cin, Cout, D, H, W) && (long long)Cin * Cout * 4 <= IDX_MAX,
              "deconv3d_bwd_weight: bad size or past the index range (Cin=%d Cout=%d D=%d H=%d W=%d)", Cin, Cout, D, H, W);
  if (use_mfma(Cin, Cout)) {
    DPI_REQUIRE(Cout / 16 <= 65535, "deconv3d_bwd_weight: Cout=%d is past the grid range", Cout);
    const BwwPlan p = bww_plan(Cin, Cout, D, H, W);
    deconv3_bwd_weight_mfma_kernel<<<dim3(Cin / 16, Cout / 16, p.nchunks), 256, 0, (hipStream_t)stream>>>(x, dy, Cin, Cout, D, H, W, p.nH2, p.nW,
                                                                                                          p.units, p.upc, ws);
    int rc = dpi_check_launch("deconv3d_bwd_weight");
    if (rc) return rc;
    dpi_reduce_chunks(ws, dw, (size_t)Cin * Cout * 64, p.nchunks, (hipStream_t)stream);
  } else {
    deconv3_bwd_weight_kernel<<<(unsigned)(Cin * Cout * 4), 256, 0, (hipStream_t)stream>>>(x, dy, Cin, Cout, D, H, W, dw);
  }
  return dpi_check_launch("deconv3d_bwd_weight");
}
