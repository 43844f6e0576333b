// 1x1x1 convolutions (channel GEMMs) on fp32 MFMA: forward / backward-data and backward-weight.
//
// These are the only true channel x channel GEMMs of the network (Block3d.shortcut, ResPath3d.conv1x1;
// reference mulresunet.py:72,103) and they are HBM-bound (AI ~ 10 FLOP/B): every activation is read once as
// float4 and each MFMA tile is fed straight from those registers, no LDS staging.
//
//   forward:   D[co 16][vox 16] += A[co][ci 4] * B[ci 4][vox 16]
//              lane (lk = l>>4, lj = l&15) loads float4 x[c0+lk][v0 + 4*lj .. +3]; element e of the float4 is column lj of
//              voxel tile e, so 4 MFMAs consume one load and the epilogue stores float4 y[co][v0 + 4*lj .. +3].
//   bwd-weight: D[co 16][ci 16] += A[co][vox 4] * B[vox 4][ci]
//              lane loads float4 dy[co = lj][v0 + 4*lk .. +3] and x[ci = lj][v0 + 4*lk .. +3]; element e pairs the voxels
//              {v0 + 4*lk + e} of both operands.
#include "conv_kernels.h"
#include <stdlib.h>
#include <type_traits>

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

struct PwMArgs {
  const float* __restrict__ x;
  const float* __restrict__ chain;
  const float* __restrict__ w;
  const float* __restrict__ bias;
  float* __restrict__ y;
  double* __restrict__ partials;
  int Cin, Cout;
  size_t V;
  long w_out_stride, w_in_stride;
  int accumulate;
  int gpb;                  // 64-voxel groups per workgroup: 16 (1024 voxels) or 4 (256 voxels, coarse levels)
  int xb, yb;               // storage type of x / y in HBM: 1 = bf16 (dpi_conv_desc.io), 0 = fp32
  int nt;                   // the tensors are far larger than the Infinity Cache and streamed once: non-temporal loads / stores (as elementwise.hip)
};

// block = 4 waves = 1024 voxels (wave w takes 64-voxel groups w, w+4, w+8, w+12); MT cout tiles per block.
// WLDS: the block's weight tile [Cin/4 chunks][MT][64 lanes] is gathered ONCE into LDS in MFMA-operand order (lane-linear,
// conflict-free ds_read_b32), so the streaming loop's only global loads are the activations.
constexpr int kPwLdsFloats = 12288;     // 48 KiB

// IOB: the launch touches a bf16 tensor (PwMArgs::xb / yb).  A template parameter, as in conv_mfma.hip: the run-time flags alone cost the
// fp32 instantiations 10 % (forward) to 3.8 x (backward-weight: every row's loads landed in a branch of their own and serialised).
template <int MT, bool WLDS, bool IOB = false>
__global__ __launch_bounds__(256) void conv_pw_mfma_kernel(PwMArgs a) {
  if constexpr (!IOB) { a.xb = 0; a.yb = 0; }
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int lk = lane >> 4, lj = lane & 15;
  const int n0 = blockIdx.y * 16 * MT;
  const bool vec = (a.V & 3) == 0;
  const int nchunk = (a.Cin + 3) >> 2;
  extern __shared__ float wl[];                        // WLDS: nchunk * MT * 64 floats (launch argument)
  if constexpr (WLDS) {
    for (int e = tid; e < nchunk * MT * 64; e += 256) {
      const int l = e & 63, m = (e >> 6) % MT, ch = (e >> 6) / MT;
      const int co = n0 + m * 16 + (l & 15), ci = ch * 4 + (l >> 4);
      wl[e] = (co < a.Cout && ci < a.Cin) ? a.w[co * a.w_out_stride + ci * a.w_in_stride] : 0.f;
    }
    __syncthreads();
  }
  double ssum[MT][4], qsum[MT][4];
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int r = 0; r < 4; ++r) { ssum[m][r] = 0.0; qsum[m][r] = 0.0; }

  const int mt_valid = min(MT, (a.Cout - n0 + 15) / 16);
  for (int grp = wid; grp < a.gpb; grp += 4) {
    const size_t g0 = ((size_t)blockIdx.x * a.gpb + grp) * 64;
    const size_t v0 = g0 + 4 * lj;
    if (g0 >= a.V) break;
    f32x4 acc[MT][4];
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[m][e] = (f32x4){0.f, 0.f, 0.f, 0.f};
    // channel chunks in batches of PF: all loads of a batch are in flight before its first MFMA (branch-free: clamped
    // channel / address + select), so a wave keeps PF KB outstanding instead of one
    constexpr int PF = 8;
    const bool full4 = vec && v0 + 3 < a.V;
    for (int cb = 0; cb < nchunk; cb += PF) {
      float b[PF][4];
      if (a.xb && full4) {      // bf16 tensor: the batch's 8-byte pieces are all requested (raw) before any is widened — one uniform branch (common.h)
        float4 h[PF];
#pragma unroll
        for (int p = 0; p < PF; ++p) {
          const int ci = min((cb + p) * 4 + lk, a.Cin - 1);
          h[p] = dpi_ld4_raw_bf16(dpi_at(a.x, (size_t)ci * a.V, true), v0);
        }
#pragma unroll
        for (int p = 0; p < PF; ++p) {
          const float4 f = dpi_widen_raw4(h[p]);
          b[p][0] = f.x; b[p][1] = f.y; b[p][2] = f.z; b[p][3] = f.w;
        }
      } else {
#pragma unroll
        for (int p = 0; p < PF; ++p) {
          const int ci = min((cb + p) * 4 + lk, a.Cin - 1);       // past Cin: re-read the last channel, weights are zero
          const float* __restrict__ xp = dpi_at(a.x, (size_t)ci * a.V, a.xb);
          if (full4) {
            const float4 f = dpi_ld4(xp, v0, false, a.nt != 0);
            b[p][0] = f.x; b[p][1] = f.y; b[p][2] = f.z; b[p][3] = f.w;
          } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) { const float v = dpi_ld(xp, v0 + e < a.V ? v0 + e : 0, a.xb); b[p][e] = v0 + e < a.V ? v : 0.f; }
          }
        }
      }
#pragma unroll
      for (int p = 0; p < PF; ++p) {
        const int ch = cb + p;
        if (ch < nchunk) {
          const int ci = ch * 4 + lk;
          const bool cok = ci < a.Cin;
          if (a.chain) {
            const Chain t = load_chain(a.chain, min(ci, a.Cin - 1));
#pragma unroll
            for (int e = 0; e < 4; ++e) b[p][e] = apply_chain(t, b[p][e]);
          }
#pragma unroll
          for (int m = 0; m < MT; ++m) {
            if (m >= mt_valid) continue;               // 16-channel tile entirely past Cout (block-uniform)
            float wv;
            if constexpr (WLDS) wv = wl[(ch * MT + m) * 64 + lane];
            else {
              const int co = n0 + m * 16 + lj;
              const float wraw = a.w[(co < a.Cout ? co : 0) * a.w_out_stride + (cok ? ci : 0) * a.w_in_stride];
              wv = (cok && co < a.Cout) ? wraw : 0.f;
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[m][e] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv, b[p][e], acc[m][e], 0, 0, 0);
          }
        }
      }
    }
    // D row = co (4*lk + r), D col lj of tile e = voxel v0 + e
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int co = n0 + m * 16 + 4 * lk + r;
        if (co < a.Cout) {
          const float bv = a.bias ? a.bias[co] : 0.f;
          float* yp = dpi_at(a.y, (size_t)co * a.V, a.yb);
          float v[4];
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = acc[m][e][r] + bv;
          if (vec && v0 + 3 < a.V) {
            if (a.accumulate) {
              const float4 o = dpi_ld4(yp, v0, a.yb, false);
              v[0] += o.x; v[1] += o.y; v[2] += o.z; v[3] += o.w;
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = dpi_stored(v[e], a.yb);          // statistics describe what is stored
            dpi_st4(yp, v0, make_float4(v[0], v[1], v[2], v[3]), a.yb, a.nt != 0);
#pragma unroll
            for (int e = 0; e < 4; ++e) { ssum[m][r] += v[e]; qsum[m][r] += (double)v[e] * v[e]; }
          } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
              if (v0 + e < a.V) {
                if (a.accumulate) v[e] += dpi_ld(yp, v0 + e, a.yb);
                v[e] = dpi_stored(v[e], a.yb);
                dpi_st(yp, v0 + e, v[e], a.yb);
                ssum[m][r] += v[e]; qsum[m][r] += (double)v[e] * v[e];
              }
          }
        }
      }
  }
  if (a.partials) {
    __shared__ double red[4][16 * MT][2];
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        double s = ssum[m][r], q = qsum[m][r];
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) { s += __shfl_xor(s, o, 64); q += __shfl_xor(q, o, 64); }
        if (lj == 0) { red[wid][m * 16 + 4 * lk + r][0] = s; red[wid][m * 16 + 4 * lk + r][1] = q; }
      }
    __syncthreads();
    if (tid < 32 * MT) {
      const int c = tid >> 1, which = tid & 1;
      const double rs = red[0][c][which] + red[1][c][which] + red[2][c][which] + red[3][c][which];
      if (n0 + c < a.Cout) a.partials[((size_t)blockIdx.x * a.Cout + n0 + c) * 2 + which] = rs;
    }
  }
}

// ---- backward-weight ---------------------------------------------------------------------------------------------
struct PwBwArgs {
  const float* __restrict__ x;
  const float* __restrict__ chain;
  const float* __restrict__ dy;
  float* __restrict__ ws;   // [nchunks][Cout][Cin]
  int Cin, Cout;
  size_t V;
  size_t vox_per_chunk;     // multiple of 64
  int xb, dyb;              // storage type of x / dy: 1 = bf16
  int nt;                   // streaming operands (>= 128 MB): non-temporal loads
};

// XB / DYB: storage type of x / dy (bf16 = true) as TEMPLATE parameters.  As run-time flags every row's loads sat in a branch of their own
// whose results had to be copied into the common registers at the branch's end — i.e. waited for — and the six rows of a round loaded one
// after the other (67->25 @256x128x128: 0.41 -> 1.99 ms with HALF the bytes).
template <int MT, int NT, bool XB = false, bool DYB = false>   // MT cout tiles x NT cin tiles per block
__global__ __launch_bounds__(256) void conv_pw_bwd_weight_mfma_kernel(PwBwArgs a) {
  a.xb = XB; a.dyb = DYB;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int lk = lane >> 4, lj = lane & 15;
  const int ci0 = blockIdx.y * 16 * NT, co0 = blockIdx.z * 16 * MT;
  const bool vec = (a.V & 3) == 0 && dpi_vec4_base(a.x, XB) && dpi_vec4_base(a.dy, DYB);   // the fall-back for unaligned views, too
  f32x4 acc[MT][NT];
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int n = 0; n < NT; ++n) acc[m][n] = (f32x4){0.f, 0.f, 0.f, 0.f};
  Chain ch[NT];
#pragma unroll
  for (int n = 0; n < NT; ++n) ch[n] = load_chain(a.chain, min(ci0 + n * 16 + lj, a.Cin - 1));

  const size_t vbeg = (size_t)blockIdx.x * a.vox_per_chunk;
  const size_t vend = vbeg + a.vox_per_chunk < a.V ? vbeg + a.vox_per_chunk : a.V;
  // A wave takes 64 voxels per round: lane (row lj, k = lk) owns four float4 per operand row (256 B contiguous per channel
  // and round), all requested before the first MFMA of the round.
  // Rows past Cout / Cin re-read the last real channel (their products land in rows that are never written).
  const float* __restrict__ dyr[MT];
  const float* __restrict__ xr[NT];
#pragma unroll
  for (int m = 0; m < MT; ++m) dyr[m] = dpi_at(a.dy, (size_t)min(co0 + m * 16 + lj, a.Cout - 1) * a.V, a.dyb);
#pragma unroll
  for (int n = 0; n < NT; ++n) xr[n] = dpi_at(a.x, (size_t)min(ci0 + n * 16 + lj, a.Cin - 1) * a.V, a.xb);
  const int mt_valid = min(MT, (a.Cout - co0 + 15) / 16), nt_valid = min(NT, (a.Cin - ci0 + 15) / 16);
  for (size_t g0 = vbeg + (size_t)wid * 64; g0 < vend; g0 += 256) {
    // element e = 4j + i of a lane is voxel g0 + 16j + 4lk + i: float4 j of the four lk lanes of a row is ONE 64-byte piece
    // (16 rows x 1 line per load instruction; with voxel = 16lk + e the same instruction touched 4 pieces 64 B apart per row)
    const size_t v0 = g0 + 4 * lk;
    auto vox = [&](int e) { return v0 + 16 * (e >> 2) + (e & 3); };
    const bool whole = vec && g0 + 63 < vend;
    float ga[DYB ? 1 : MT][16], xb[XB ? 1 : NT][16];       // fp32 rows: the 16 values; bf16 rows live in gr / xq (raw) only
    // bf16 rows: the raw 8-byte pieces wait in their own registers (gr / xq) and are widened into ga / xb once every row of the round has
    // been requested.  (Widening in place — raw dwords in o[4j], o[4j + 1], values written over them — sent the arrays to scratch: 400 bytes
    // per lane, 67->25 1.94 ms.)
    float gr[DYB ? MT : 1][8], xq[XB ? NT : 1][8];
    auto load16 = [&](const float* __restrict__ p, float (&o)[16], float (&rw)[8], bool bf) {
      if (whole && bf) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float4 f = dpi_ld4_raw_bf16(p, v0 + 16 * j);
          rw[2 * j] = f.x; rw[2 * j + 1] = f.y;
        }
      } else if (bf) {         // ragged round of a bf16 row: the same raw layout (two elements per dword), element by element
        const unsigned short* __restrict__ ph = reinterpret_cast<const unsigned short*>(p);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const unsigned lo = vox(2 * k) < vend ? ph[vox(2 * k)] : 0u, hi = vox(2 * k + 1) < vend ? ph[vox(2 * k + 1)] : 0u;
          rw[k] = __builtin_bit_cast(float, lo | (hi << 16));
        }
      } else if (whole) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float4 f = dpi_ld4(p, v0 + 16 * j, false, a.nt != 0);
          o[4 * j] = f.x; o[4 * j + 1] = f.y; o[4 * j + 2] = f.z; o[4 * j + 3] = f.w;
        }
      } else {
#pragma unroll
        for (int e = 0; e < 16; ++e) { const float v = dpi_ld(p, vox(e) < vend ? vox(e) : vbeg, bf); o[e] = vox(e) < vend ? v : 0.f; }
      }
    };
    // 16-channel tiles that lie entirely past Cout / Cin (e.g. Cin = 67: the second 64-channel block holds 3 channels)
    // are skipped — block-uniform tests; without them those tiles re-read the clamped last channel 16 times over
#pragma unroll
    for (int m = 0; m < MT; ++m)
      if (m < mt_valid) load16(dyr[m], ga[DYB ? 0 : m], gr[DYB ? m : 0], DYB);
#pragma unroll
    for (int n = 0; n < NT; ++n)
      if (n < nt_valid) load16(xr[n], xb[XB ? 0 : n], xq[XB ? n : 0], XB);
    if constexpr (XB || DYB) {
      // bf16 rows are widened piece by piece right before their MFMAs (raw 8 registers per row + 4 live values instead of 16 per row);
      // the MFMA order per accumulator is the fp32 kernel's (e ascending), so both instantiations give bit-identical sums
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float gv[MT][4], xv[NT][4];
#pragma unroll
        for (int m = 0; m < MT; ++m)
          if (m < mt_valid) {
            if (DYB) {
              const float4 f = dpi_widen_raw4(make_float4(gr[DYB ? m : 0][2 * j], gr[DYB ? m : 0][2 * j + 1], 0.f, 0.f));
              gv[m][0] = f.x; gv[m][1] = f.y; gv[m][2] = f.z; gv[m][3] = f.w;
            } else {
#pragma unroll
              for (int i = 0; i < 4; ++i) gv[m][i] = ga[DYB ? 0 : m][4 * j + i];
            }
          }
#pragma unroll
        for (int n = 0; n < NT; ++n)
          if (n < nt_valid) {
            if (XB) {
              const float4 f = dpi_widen_raw4(make_float4(xq[XB ? n : 0][2 * j], xq[XB ? n : 0][2 * j + 1], 0.f, 0.f));
              xv[n][0] = f.x; xv[n][1] = f.y; xv[n][2] = f.z; xv[n][3] = f.w;
            } else {
#pragma unroll
              for (int i = 0; i < 4; ++i) xv[n][i] = xb[XB ? 0 : n][4 * j + i];
            }
            if (a.chain) {
#pragma unroll
              for (int i = 0; i < 4; ++i) xv[n][i] = (vox(4 * j + i) < vend) ? apply_chain(ch[n], xv[n][i]) : 0.f;
            }
          }
#pragma unroll
        for (int m = 0; m < MT; ++m)
          if (m < mt_valid) {
#pragma unroll
            for (int n = 0; n < NT; ++n)
              if (n < nt_valid) {
#pragma unroll
                for (int i = 0; i < 4; ++i) acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(gv[m][i], xv[n][i], acc[m][n], 0, 0, 0);
              }
          }
      }
    } else {
    if (a.chain) {
#pragma unroll
      for (int n = 0; n < NT; ++n)
        if (n < nt_valid) {
#pragma unroll
          for (int e = 0; e < 16; ++e) xb[n][e] = (vox(e) < vend) ? apply_chain(ch[n], xb[n][e]) : 0.f;
        }
    }
#pragma unroll
    for (int m = 0; m < MT; ++m)
      if (m < mt_valid) {
#pragma unroll
        for (int n = 0; n < NT; ++n)
          if (n < nt_valid) {
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(ga[m][e], xb[n][e], acc[m][n], 0, 0, 0);
          }
      }
    }
  }
  // cross-wave reduction; D row = co (4*lk + r), col = ci lj
  __shared__ float red[4][MT * NT * 4 * 64];
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int n = 0; n < NT; ++n)
#pragma unroll
      for (int r = 0; r < 4; ++r) red[wid][((m * NT + n) * 4 + r) * 64 + lane] = acc[m][n][r];
  __syncthreads();
  for (int e = tid; e < MT * NT * 4 * 64; e += 256) {
    const int l = e & 63, r = (e >> 6) & 3, n = (e >> 8) % NT, m = (e >> 8) / NT;
    const int co = co0 + m * 16 + 4 * (l >> 4) + r, ci = ci0 + n * 16 + (l & 15);
    if (co < a.Cout && ci < a.Cin)
      a.ws[((size_t)blockIdx.x * a.Cout + co) * a.Cin + ci] = red[0][e] + red[1][e] + red[2][e] + red[3][e];
  }
}

// bf16-MFMA variant for bf16 tensors in the bf16 arithmetic mode (dpi_conv_desc.precision = 1, io: x and dy bf16, V a multiple of 8):
//     dW[co][ci] = sum_v dY[co][v] * T(X)[ci][v]      as      D[co 16][ci 16] += A[co 16][K 32 voxels] * B[K 32 voxels][ci 16]
// K runs over VOXELS, and 8 consecutive voxels of a channel row are 16 contiguous bytes of a bf16 tensor — exactly one lane's share of a
// v_mfma_f32_16x16x32_bf16 operand (lane = (row lj, octet lk)).  Both operands therefore go from global memory straight into MFMA
// registers: no LDS, no transposition, no conversion when X has no chain (with one: widen, apply, round to bf16 — the operand rounding of
// the mode, as in conv_bf16_bwd_weight_kernel).  The fp32-MFMA kernel above spends 16 cycles per 4 voxels of a 16 x 16 tile, this one 16
// per 32: 67->25 at 256x128x128 is matrix-bound there (0.35 ms for 0.77 GB) and HBM-bound here.
typedef __bf16 pw_bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned int pw_u32x4 __attribute__((ext_vector_type(4)));
template <int MT, int NT>
__global__ __launch_bounds__(256) void conv_pw_bwd_weight_bf16_kernel(PwBwArgs a) {
  constexpr int U = 2;                                   // 32-voxel steps in flight per wave (4: no faster, 208-248 registers)
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int lk = lane >> 4, lj = lane & 15;
  const int ci0 = blockIdx.y * 16 * NT, co0 = blockIdx.z * 16 * MT;
  f32x4 acc[MT][NT];
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int n = 0; n < NT; ++n) acc[m][n] = (f32x4){0.f, 0.f, 0.f, 0.f};
  Chain ch[NT];
#pragma unroll
  for (int n = 0; n < NT; ++n) ch[n] = load_chain(a.chain, min(ci0 + n * 16 + lj, a.Cin - 1));
  const size_t vbeg = (size_t)blockIdx.x * a.vox_per_chunk;
  const size_t vend = vbeg + a.vox_per_chunk < a.V ? vbeg + a.vox_per_chunk : a.V;
  // rows past Cout / Cin re-read the last real channel (their products land in rows / columns that are never written)
  const unsigned short* __restrict__ dyr[MT];
  const unsigned short* __restrict__ xr[NT];
#pragma unroll
  for (int m = 0; m < MT; ++m) dyr[m] = reinterpret_cast<const unsigned short*>(a.dy) + (size_t)min(co0 + m * 16 + lj, a.Cout - 1) * a.V;
#pragma unroll
  for (int n = 0; n < NT; ++n) xr[n] = reinterpret_cast<const unsigned short*>(a.x) + (size_t)min(ci0 + n * 16 + lj, a.Cin - 1) * a.V;
  const int mt_valid = min(MT, (a.Cout - co0 + 15) / 16), nt_valid = min(NT, (a.Cin - ci0 + 15) / 16);
  for (size_t g0 = vbeg + (size_t)wid * (32 * U); g0 < vend; g0 += 4 * 32 * U) {
    pw_u32x4 ga[U][MT], xb[U][NT];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const size_t v = g0 + 32 * u + 8 * lk;             // this lane's octet: whole or absent (V, the chunk length and g0 are multiples of 8)
      const bool in = v < vend;
#pragma unroll
      for (int m = 0; m < MT; ++m)
        if (m < mt_valid) ga[u][m] = in ? *reinterpret_cast<const pw_u32x4*>(dyr[m] + v) : (pw_u32x4){0u, 0u, 0u, 0u};
#pragma unroll
      for (int n = 0; n < NT; ++n)
        if (n < nt_valid) xb[u][n] = in ? *reinterpret_cast<const pw_u32x4*>(xr[n] + v) : (pw_u32x4){0u, 0u, 0u, 0u};
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (a.chain) {
#pragma unroll
        for (int n = 0; n < NT; ++n)
          if (n < nt_valid) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
              const unsigned w2 = xb[u][n][k];
              const float lo = apply_chain(ch[n], __builtin_bit_cast(float, w2 << 16)), hi = apply_chain(ch[n], __builtin_bit_cast(float, w2 & 0xffff0000u));
              xb[u][n][k] = dpi_pack_bf16(lo, hi);        // (an absent octet meets dY = 0)
            }
          }
      }
#pragma unroll
      for (int m = 0; m < MT; ++m)
        if (m < mt_valid) {
#pragma unroll
          for (int n = 0; n < NT; ++n)
            if (n < nt_valid)
              acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(pw_bf16x8, ga[u][m]), __builtin_bit_cast(pw_bf16x8, xb[u][n]), acc[m][n], 0, 0, 0);
        }
    }
  }
  // cross-wave reduction; D row = co (4*lk + r), col = ci lj
  __shared__ float red[4][MT * NT * 4 * 64];
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int n = 0; n < NT; ++n)
#pragma unroll
      for (int r = 0; r < 4; ++r) red[wid][((m * NT + n) * 4 + r) * 64 + lane] = acc[m][n][r];
  __syncthreads();
  for (int e = tid; e < MT * NT * 4 * 64; e += 256) {
    const int l = e & 63, r = (e >> 6) & 3, n = (e >> 8) % NT, m = (e >> 8) / NT;
    const int co = co0 + m * 16 + 4 * (l >> 4) + r, ci = ci0 + n * 16 + (l & 15);
    if (co < a.Cout && ci < a.Cin)
      a.ws[((size_t)blockIdx.x * a.Cout + co) * a.Cin + ci] = red[0][e] + red[1][e] + red[2][e] + red[3][e];
  }
}

__global__ void reduce_chunks_pw_kernel(const float* __restrict__ ws, float* __restrict__ out, size_t n, int nchunks) {
  const size_t gid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t i = gid >> 3;
  const int part = gid & 7;
  float s = 0.f;
  if (i < n)
    for (int c = part; c < nchunks; c += 8) s += ws[(size_t)c * n + i];
  s += __shfl_xor(s, 1, 64); s += __shfl_xor(s, 2, 64); s += __shfl_xor(s, 4, 64);
  if (i < n && part == 0) out[i] = s;
}

static int pw_nt_knob() {         // A/B knob: DPI_PW_NT=0 in the environment switches the non-temporal accesses of the 1x1x1 kernels off
  static int v = -1;
  if (v < 0) { const char* e = getenv("DPI_PW_NT"); v = (e && e[0] == '0') ? 0 : 1; }
  return v;
}
#define g_pw_nt pw_nt_knob()
struct PwBwPlan { int nchunks; size_t vox_per_chunk; int mt, nt; };
// whether conv_pw_bwd_weight_bf16_kernel serves the layer (x and dy bf16, bf16 arithmetic, 16-byte octets); alignment is checked at launch
static bool pw_bw_bf16(const dpi_conv_desc* d) {
  return d->precision == 1 && (d->io & DPI_IO_X_BF16) && (d->io & DPI_IO_DY_BF16) && (((size_t)d->D * d->H * d->W) & 7) == 0;
}
PwBwPlan pw_bw_plan(const dpi_conv_desc* d) {
  PwBwPlan p{};
  const size_t V = (size_t)d->D * d->H * d->W;
  p.mt = d->Cout > 16 ? 2 : 1;
  p.nt = d->Cin > 32 ? 4 : (d->Cin > 16 ? 2 : 1);
  const size_t blocks_other = (size_t)cdiv(d->Cin, 16 * p.nt) * cdiv(d->Cout, 16 * p.mt);
  const size_t units = cdivz(V, 64);
  const size_t per = (size_t)d->Cout * d->Cin;
  const size_t max_chunks_mem = per ? ((size_t)32 << 20) / per : 1;
  size_t want = cdivz(1024, blocks_other);
  if (want > units) want = units;
  if (want > max_chunks_mem) want = max_chunks_mem;
  if (want < 1) want = 1;
  const size_t upc = cdivz(units, want);
  p.vox_per_chunk = upc * 64;
  p.nchunks = (int)cdivz(units, upc);
  return p;
}

}  // namespace

// Work split of the pointwise MFMA kernel: (voxels per workgroup, 16-channel tiles per workgroup).  The fine levels use
// 1024 voxels x up to 64 output channels (the input tile is read once for all of them); the coarse levels of the U-Net
// (a few thousand voxels, hundreds of channels) would leave most CUs idle that way, so they get 256-voxel workgroups
// and, if that is still not ~4 waves per CU, one channel tile per workgroup.
static void pw_mfma_plan(size_t V, int cout, int* vox_per_block, int* mt) {
  int m = cout <= 16 ? 1 : (cout <= 32 ? 2 : 4);
  int vpb = 1024;
  auto waves = [&]() { return (long)cdivz(V, vpb) * (vpb / 256) * cdiv(cout, 16 * m); };
  if (waves() < 1024) vpb = 256;
  if (waves() < 1024 && m == 4) m = 2;
  if (waves() < 1024 && m == 2) m = 1;
  *vox_per_block = vpb;
  *mt = m;
}
// one BatchNorm partial row per workgroup column of the forward launch
int dpi_conv_pw_mfma_stat_blocks(const dpi_conv_desc* d) {
  const size_t V = (size_t)d->D * d->H * d->W;
  int vpb, mt;
  pw_mfma_plan(V, d->Cout, &vpb, &mt);
  return (int)cdivz(V, vpb);
}

int dpi_conv_pw_mfma_run(const dpi_conv_desc* d, const float* x, const float* chain, const float* w, const float* bias, float* y,
                         double* partials, bool flip, int accumulate, hipStream_t st) {
  const int cin = flip ? d->Cout : d->Cin, cout = flip ? d->Cin : d->Cout;
  const long w_out = flip ? 1 : (long)d->Cin, w_in = flip ? (long)d->Cin : 1;
  int vpb, mt;
  PwMArgs a{x, chain, w, bias, y, partials, cin, cout, (size_t)d->D * d->H * d->W, w_out, w_in, accumulate, 0, dpi_io_in(d, flip), dpi_io_out(d, flip), 0};
  a.nt = (g_pw_nt && !accumulate && (size_t)cin * a.V >= ((size_t)32 << 20)) ? 1 : 0;
  pw_mfma_plan(a.V, cout, &vpb, &mt);
  a.gpb = vpb / 64;
  const unsigned gx = (unsigned)cdivz(a.V, vpb);
  const bool wlds = (long)cdiv(cin, 4) * mt * 64 <= kPwLdsFloats;
  const dim3 grid(gx, cdiv(cout, 16 * mt));
  // the weight tile is the kernel's only sizeable LDS: allocated to size (8-9 KB for the full-resolution layers), so that registers
  // and not a fixed 48 KB bound the number of resident workgroups (= loads in flight per CU of an HBM-bound kernel)
  const size_t wbytes = wlds ? (size_t)cdiv(cin, 4) * mt * 64 * sizeof(float) : 0;
  if (a.xb || a.yb) {
    if (mt == 1) { if (wlds) conv_pw_mfma_kernel<1, true, true><<<grid, 256, wbytes, st>>>(a); else conv_pw_mfma_kernel<1, false, true><<<grid, 256, 0, st>>>(a); }
    else if (mt == 2) { if (wlds) conv_pw_mfma_kernel<2, true, true><<<grid, 256, wbytes, st>>>(a); else conv_pw_mfma_kernel<2, false, true><<<grid, 256, 0, st>>>(a); }
    else { if (wlds) conv_pw_mfma_kernel<4, true, true><<<grid, 256, wbytes, st>>>(a); else conv_pw_mfma_kernel<4, false, true><<<grid, 256, 0, st>>>(a); }
    return dpi_check_launch("conv_pw_mfma");
  }
  if (mt == 1) { if (wlds) conv_pw_mfma_kernel<1, true><<<grid, 256, wbytes, st>>>(a); else conv_pw_mfma_kernel<1, false><<<grid, 256, 0, st>>>(a); }
  else if (mt == 2) { if (wlds) conv_pw_mfma_kernel<2, true><<<grid, 256, wbytes, st>>>(a); else conv_pw_mfma_kernel<2, false><<<grid, 256, 0, st>>>(a); }
  else { if (wlds) conv_pw_mfma_kernel<4, true><<<grid, 256, wbytes, st>>>(a); else conv_pw_mfma_kernel<4, false><<<grid, 256, 0, st>>>(a); }
  return dpi_check_launch("conv_pw_mfma");
}

size_t dpi_conv_pw_bwd_weight_mfma_ws_floats(const dpi_conv_desc* d) {
  const PwBwPlan p = pw_bw_plan(d);
  return (size_t)p.nchunks * d->Cout * d->Cin;
}

int dpi_conv_pw_bwd_weight_mfma_run(const dpi_conv_desc* d, const float* x, const float* chain, const float* dy, float* dw, float* ws,
                                    hipStream_t st) {
  const PwBwPlan p = pw_bw_plan(d);
  PwBwArgs a{x, chain, dy, ws, d->Cin, d->Cout, (size_t)d->D * d->H * d->W, p.vox_per_chunk, (d->io & DPI_IO_X_BF16) != 0, (d->io & DPI_IO_DY_BF16) != 0, 0};
  a.nt = (g_pw_nt && (size_t)d->Cin * a.V >= ((size_t)32 << 20)) ? 1 : 0;
  dim3 grid(p.nchunks, cdiv(d->Cin, 16 * p.nt), cdiv(d->Cout, 16 * p.mt));
  auto launch = [&](auto xb_, auto dyb_) {
    constexpr bool XB = decltype(xb_)::value, DYB = decltype(dyb_)::value;
    if (p.mt == 1) {
      if (p.nt == 1) conv_pw_bwd_weight_mfma_kernel<1, 1, XB, DYB><<<grid, 256, 0, st>>>(a);
      else if (p.nt == 2) conv_pw_bwd_weight_mfma_kernel<1, 2, XB, DYB><<<grid, 256, 0, st>>>(a);
      else conv_pw_bwd_weight_mfma_kernel<1, 4, XB, DYB><<<grid, 256, 0, st>>>(a);
    } else {
      if (p.nt == 1) conv_pw_bwd_weight_mfma_kernel<2, 1, XB, DYB><<<grid, 256, 0, st>>>(a);
      else if (p.nt == 2) conv_pw_bwd_weight_mfma_kernel<2, 2, XB, DYB><<<grid, 256, 0, st>>>(a);
      else conv_pw_bwd_weight_mfma_kernel<2, 4, XB, DYB><<<grid, 256, 0, st>>>(a);
    }
  };
  // both tensors bf16 in the bf16 arithmetic mode: operands straight from memory into the bf16 MFMA (16-byte octets: V % 8, aligned bases)
  if (pw_bw_bf16(d) && (((uintptr_t)x | (uintptr_t)dy) & 15) == 0) {
    if (p.mt == 1) {
      if (p.nt == 1) conv_pw_bwd_weight_bf16_kernel<1, 1><<<grid, 256, 0, st>>>(a);
      else if (p.nt == 2) conv_pw_bwd_weight_bf16_kernel<1, 2><<<grid, 256, 0, st>>>(a);
      else conv_pw_bwd_weight_bf16_kernel<1, 4><<<grid, 256, 0, st>>>(a);
    } else {
      if (p.nt == 1) conv_pw_bwd_weight_bf16_kernel<2, 1><<<grid, 256, 0, st>>>(a);
      else if (p.nt == 2) conv_pw_bwd_weight_bf16_kernel<2, 2><<<grid, 256, 0, st>>>(a);
      else conv_pw_bwd_weight_bf16_kernel<2, 4><<<grid, 256, 0, st>>>(a);
    }
  }
  else if (a.xb && a.dyb) launch(std::true_type{}, std::true_type{});
  else if (a.xb) launch(std::true_type{}, std::false_type{});
  else if (a.dyb) launch(std::false_type{}, std::true_type{});
  else launch(std::false_type{}, std::false_type{});
  if (int e = dpi_check_launch("conv_pw_bwd_weight_mfma")) return e;
  const size_t per = (size_t)d->Cout * d->Cin;
  dpi_reduce_chunks(ws, dw, per, p.nchunks, st);
  return dpi_check_launch("reduce_chunks_pw");
}
