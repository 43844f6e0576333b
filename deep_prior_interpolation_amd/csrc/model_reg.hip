// L1 / anisotropic total-variation penalty on the tensor the network writes (--model_reg; ours, no reference code) as gfx950 kernels:
// the value and its gradient in one pass over m = [C][n0][n1][n2] fp32, N = C n0 n1 n2 elements, A = the axes named by the bits of `axes`.
//     R = (1/N) sum_{a in A} sum_i |m[i + e_a] - m[i]|      (A empty: (1/N) sum_i |m[i]|)
//     grad[i] = k[i] / N,  k[i] = sum_{a in A} ( sgn(m[i] - m[i - e_a]) [i_a >= 1] - sgn(m[i + e_a] - m[i]) [i_a < n_a - 1] )   (A empty: sgn(m[i]))
// Channels are never differenced; an axis of extent 1 has no neighbour and contributes nothing.
// A thread owns a QUAD: four consecutive elements of one row along n2 (the last quad of a row is cut where n2 % 4 != 0).  It reads its
// quad, the quads one row (n1) and one plane (n0) before and behind it and the two elements left and right of it, forms k as an INTEGER
// from comparisons (sgn(a - b) = (a > b) - (a < b), so sgn(0) = 0 and no rounding decides a sign), and writes grad = (float)k / (float)N:
// one rounding, one thread per output, no atomics.  Element i owns the forward differences |m[i + e_a] - m[i]|: each is formed in fp32
// and added to the thread's double in the order axis n0, n1, n2, then element 0..3 of the quad.
// Quads are read and written 16 bytes at a time when n2 % 4 == 0 and both tensors start on 16 bytes (then every quad of every row does),
// else as four guarded 4-byte accesses per lane.  The owner of every element and term and the order of every sum are the same on both
// paths, so both give the same bits of grad and of R.
// The neighbour quads are the centre quads of other threads: cache hits (a plane of 128 x 128 floats is 64 KiB), so the launch moves the
// tensor about once in and once out.  Quads are dealt to a fixed grid (one per thread, grid-stride past MR_BLOCKS workgroups); a
// workgroup's threads are summed in a fixed order into one double of the workspace, and a second launch of one wave adds the workgroup
// sums in a fixed order and divides by N: the reduction scheme of dpi_masked_loss.  Same bits every run.
#include "common.h"

namespace {

constexpr int MR_THREADS = 256;
constexpr int MR_BLOCKS = 2048;      // workgroups at most = doubles of the workspace

__device__ __forceinline__ int mr_sgn(float a, float b) { return (int)(a > b) - (int)(a < b); }      // sgn(a - b); 0 for a tie or a NaN

struct MrQuad {
  float v[4];
};

// the quad at element offset `at` (nv = its elements inside the row)
template <bool VEC>
__device__ __forceinline__ MrQuad mr_load(const float* __restrict__ m, size_t at, int nv) {
  MrQuad q;
  if (VEC) {
    const float4 f = *reinterpret_cast<const float4*>(m + at);
    q.v[0] = f.x; q.v[1] = f.y; q.v[2] = f.z; q.v[3] = f.w;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) q.v[j] = j < nv ? m[at + j] : 0.f;
  }
  return q;
}

// one axis whose neighbours are whole quads (n0: stride n1 n2, n1: stride n2)
template <bool VEC>
__device__ __forceinline__ void mr_axis(const float* __restrict__ m, size_t at, size_t stride, bool prev, bool next, int nv, const MrQuad& c,
                                        int (&k)[4], double& acc) {
  if (prev) {
    const MrQuad p = mr_load<VEC>(m, at - stride, nv);
#pragma unroll
    for (int j = 0; j < 4; ++j) k[j] += mr_sgn(c.v[j], p.v[j]);
  }
  if (next) {
    const MrQuad x = mr_load<VEC>(m, at + stride, nv);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      k[j] -= mr_sgn(x.v[j], c.v[j]);
      if (j < nv) acc += (double)fabsf(x.v[j] - c.v[j]);
    }
  }
}

template <bool VEC>
__global__ __launch_bounds__(MR_THREADS) void model_reg_kernel(const float* __restrict__ m, unsigned n0, unsigned n1, size_t n2, unsigned qpr,
                                                               size_t nquads, int axes, float den, float* __restrict__ grad,
                                                               double* __restrict__ ws) {
  double acc = 0.0;
  const size_t s1 = n2, s0 = (size_t)n1 * n2;
  for (size_t q = (size_t)blockIdx.x * MR_THREADS + threadIdx.x; q < nquads; q += (size_t)gridDim.x * MR_THREADS) {
    const unsigned row = (unsigned)q / qpr, qx = (unsigned)q - row * qpr;        // nquads < 2^32 (checked by the caller)
    const size_t x0 = (size_t)qx * 4;
    const size_t at = (size_t)row * n2 + x0;
    const int nv = n2 - x0 < 4 ? (int)(n2 - x0) : 4;
    const MrQuad c = mr_load<VEC>(m, at, nv);
    int k[4] = {0, 0, 0, 0};
    if (axes == 0) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        k[j] = mr_sgn(c.v[j], 0.f);
        if (j < nv) acc += (double)fabsf(c.v[j]);
      }
    }
    if (axes & 3) {
      const unsigned r0 = row / n1, i1 = row - r0 * n1;
      if (axes & 1) {
        const unsigned i0 = r0 % n0;
        mr_axis<VEC>(m, at, s0, i0 >= 1, i0 + 1 < n0, nv, c, k, acc);
      }
      if (axes & 2) mr_axis<VEC>(m, at, s1, i1 >= 1, i1 + 1 < n1, nv, c, k, acc);
    }
    if (axes & 4) {
      // inside the quad the neighbours are registers; its two ends read one element each
      float left = 0.f, right = 0.f;
      const bool hl = x0 >= 1, hr = x0 + 4 < n2;
      if (hl) left = m[at - 1];
      if (hr) right = m[at + 4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (j < nv) {
          if (j > 0) k[j] += mr_sgn(c.v[j], c.v[j - 1]);
          else if (hl) k[j] += mr_sgn(c.v[j], left);
          const bool hn = j < 3 ? j + 1 < nv : hr;
          if (hn) {
            const float nx = j < 3 ? c.v[j + 1] : right;
            k[j] -= mr_sgn(nx, c.v[j]);
            acc += (double)fabsf(nx - c.v[j]);
          }
        }
      }
    }
    if (VEC) {
      *reinterpret_cast<float4*>(grad + at) = make_float4((float)k[0] / den, (float)k[1] / den, (float)k[2] / den, (float)k[3] / den);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (j < nv) grad[at + j] = (float)k[j] / den;
    }
  }
  __shared__ double sh[MR_THREADS / 64];
  const double r = block_sum(acc, sh);
  if (threadIdx.x == 0) ws[blockIdx.x] = r;
}

__global__ __launch_bounds__(64) void model_reg_final_kernel(const double* __restrict__ ws, int nblk, double n, double* __restrict__ res) {
  double s = 0.0;
  for (int b = threadIdx.x; b < nblk; b += 64) s += ws[b];
  s = wave_sum(s);
  if (threadIdx.x == 0) res[0] = s / n;
}

}  // namespace

extern "C" size_t dpi_model_reg_ws_doubles(size_t n) { (void)n; return (size_t)MR_BLOCKS; }

extern "C" int dpi_model_reg(const float* m, int C, size_t n0, size_t n1, size_t n2, int axes, float* grad, double* ws, double* res,
                             void* stream) {
  DPI_REQUIRE(m && grad && ws && res && m != grad && (const void*)ws != (const void*)res, "model_reg: null or aliased pointer");
  DPI_REQUIRE(C >= 1 && n0 >= 1 && n1 >= 1 && n2 >= 1, "model_reg: C, n0, n1 and n2 must be >= 1, got %d, %zu, %zu, %zu", C, n0, n1, n2);
  DPI_REQUIRE(axes >= 0 && axes <= 7, "model_reg: axes must lie in [0, 7] (bit k: differences along n_k), got %d", axes);
  // quads are numbered in 32 bits (rows too: a row holds at least one), element offsets in 64
  const size_t lim = 0xffffffffu;
  DPI_REQUIRE(n0 <= lim && n1 <= lim / n0 && (size_t)C <= lim / (n0 * n1) && n2 <= lim * 4 && cdivz(n2, 4) <= lim / ((size_t)C * n0 * n1),
              "model_reg: a tensor of %d x %zu x %zu x %zu samples is too large", C, n0, n1, n2);
  const size_t qpr = cdivz(n2, 4), nquads = (size_t)C * n0 * n1 * qpr, n = (size_t)C * n0 * n1 * n2;
  size_t nb = cdivz(nquads, MR_THREADS);
  if (nb > MR_BLOCKS) nb = MR_BLOCKS;
  const bool vec = n2 % 4 == 0 && reinterpret_cast<uintptr_t>(m) % 16 == 0 && reinterpret_cast<uintptr_t>(grad) % 16 == 0;
  const float den = (float)n;
  hipStream_t st = (hipStream_t)stream;
  if (vec) model_reg_kernel<true><<<(unsigned)nb, MR_THREADS, 0, st>>>(m, (unsigned)n0, (unsigned)n1, n2, (unsigned)qpr, nquads, axes, den, grad, ws);
  else model_reg_kernel<false><<<(unsigned)nb, MR_THREADS, 0, st>>>(m, (unsigned)n0, (unsigned)n1, n2, (unsigned)qpr, nquads, axes, den, grad, ws);
  if (int e = dpi_check_launch("model_reg")) return e;
  model_reg_final_kernel<<<1, 64, 0, st>>>(ws, (int)nb, (double)n, res);
  return dpi_check_launch("model_reg_final");
}
