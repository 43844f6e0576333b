// Linear operators of the anti-aliasing add-on and the POCS regulariser (reference operators/derivative.py, utils/slopes.py,
// utils/processing.py:139-181, utils/pocs.py) as gfx950 kernels.  All of them are HBM-bound one-pass stencils / maps over
// small 2-D sections (datasets/lines is 170 x 100): one thread per output sample, W contiguous, no LDS needed — the
// neighbours of a sample sit in the same or the adjacent cache line.
#include "common.h"

namespace {

inline unsigned op_blocks(size_t n) {
  size_t b = cdivz(n, 256);
  if (b > 8192) b = 8192;
  if (b < 1) b = 1;
  return (unsigned)b;
}

// ---- first / second derivative along the middle axis of [outer][n][inner] ----------------------------------------
// stencil 0 forward : y[i] = (x[i+1] - x[i]) / h   for i <= n-2, 0 at i = n-1        (utils/processing.py:154-155)
// stencil 1 backward: y[i] = (x[i] - x[i-1]) / h   for i >= 1,   0 at i = 0          (156-157)
// stencil 2 centred : y[i] = (x[i+1] - x[i-1]) / 2h for 1 <= i <= n-2, 0 at the ends (152-153)
// stencil 3 second  : y[i] = (x[i+1] - 2 x[i] + x[i-1]) / h^2 for 1 <= i <= n-2      (177)
// adjoint = 1 applies the transpose of that matrix (what autograd needs for a loss term built on the operator).
__global__ __launch_bounds__(256) void diff_axis_kernel(const float* __restrict__ x, size_t total, int n, size_t inner, int stencil,
                                                        float scale, int adjoint, float* __restrict__ y) {
  for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (size_t)gridDim.x * 256) {
    const int i = (int)((idx / inner) % (size_t)n);
    const float c = x[idx];
    const float up = i + 1 < n ? x[idx + inner] : 0.f;     // x[i+1]
    const float dn = i >= 1 ? x[idx - inner] : 0.f;        // x[i-1]
    float r;
    if (!adjoint) {
      if (stencil == 0) r = i <= n - 2 ? (up - c) : 0.f;
      else if (stencil == 1) r = i >= 1 ? (c - dn) : 0.f;
      else if (stencil == 2) r = (i >= 1 && i <= n - 2) ? 0.5f * up - 0.5f * dn : 0.f;
      else r = (i >= 1 && i <= n - 2) ? (up - 2.f * c + dn) : 0.f;
    } else {
      // row j of the forward matrix is active for j in [lo, hi]; column i collects the active rows that touch it
      if (stencil == 0) r = (i >= 1 ? dn : 0.f) - (i <= n - 2 ? c : 0.f);                        // rows j = i-1 (+1) and j = i (-1)
      else if (stencil == 1) r = (i >= 1 ? c : 0.f) - (i + 1 <= n - 1 ? up : 0.f);               // rows j = i (+1) and j = i+1 (-1)
      else if (stencil == 2) r = 0.5f * ((i - 1 >= 1 && i - 1 <= n - 2) ? dn : 0.f) - 0.5f * ((i + 1 >= 1 && i + 1 <= n - 2) ? up : 0.f);
      else r = ((i - 1 >= 1 && i - 1 <= n - 2) ? dn : 0.f) - 2.f * ((i >= 1 && i <= n - 2) ? c : 0.f) + ((i + 1 >= 1 && i + 1 <= n - 2) ? up : 0.f);
    }
    y[idx] = r / scale;        // a division, like the reference (bit parity of stencils 0-2 for spacings that are not powers of two)
  }
}

// ---- Hale2D / directional_laplacian (utils/slopes.py:51-105) on [N][H][W] planes ---------------------------------
// With Dv, Dh the forward differences (last row / column zero) the reference computes
//     p1 = a*Dv x + b*Dh x,  p2 = b*Dv x + c*Dh x,   y = -( Dh p1 + Dv p2 )
// (it re-applies the FORWARD difference instead of the divergence, and crosses the axes; reproduced as is).  One thread per
// sample evaluates p1 at (i,j),(i,j+1) and p2 at (i,j),(i+1,j) from the 3x3 neighbourhood: 4 reads of x and 3 coefficient
// planes per sample, all served by L1/L2 after the first touch.
// The per-sample arithmetic (hale_pv / hale_qv, on values) is shared with the vertical sections of a 3-D patch below, so both
// paths give the same bits for the same section.
struct HaleP {
  float p1, p2;
};
// p1, p2 at one sample from x there (x0), at its v / h neighbours (xv, xh; used only where hv / hh: inside the section)
__device__ __forceinline__ HaleP hale_pv(float x0, float xv, float xh, bool hv, bool hh, float a, float b, float c) {
  const float gv = hv ? xv - x0 : 0.f;
  const float gh = hh ? xh - x0 : 0.f;
  HaleP r;
  r.p1 = a * gv + b * gh;
  r.p2 = b * gv + c * gh;
  return r;
}
__device__ __forceinline__ HaleP hale_p(const float* __restrict__ x, const float* __restrict__ a, const float* __restrict__ b,
                                        const float* __restrict__ c, size_t base, int i, int j, int H, int W) {
  const size_t o = base + (size_t)i * W + j;
  const bool hv = i <= H - 2, hh = j <= W - 2;
  return hale_pv(x[o], hv ? x[o + W] : 0.f, hh ? x[o + 1] : 0.f, hv, hh, a[o], b[o], c[o]);
}
__global__ __launch_bounds__(256) void hale2d_fwd_kernel(const float* __restrict__ x, const float* __restrict__ a, const float* __restrict__ b,
                                                         const float* __restrict__ c, size_t total, int H, int W, float* __restrict__ y) {
  const size_t plane = (size_t)H * W;
  for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (size_t)gridDim.x * 256) {
    const size_t base = idx / plane * plane;
    const int i = (int)((idx - base) / W), j = (int)((idx - base) % W);
    const HaleP p = hale_p(x, a, b, c, base, i, j, H, W);
    float ata1 = 0.f, ata2 = 0.f;
    if (j <= W - 2) ata1 = hale_p(x, a, b, c, base, i, j + 1, H, W).p1 - p.p1;      // Dh p1
    if (i <= H - 2) ata2 = hale_p(x, a, b, c, base, i + 1, j, H, W).p2 - p.p2;      // Dv p2
    y[idx] = -(ata1 + ata2);
  }
}
// transpose: with r1 = Dh^T g, r2 = Dv^T g (D^T u)(k) = u(k-1)[k >= 1] - u(k)[k <= n-2]:
//     q1 = a*r1 + b*r2,  q2 = b*r1 + c*r2,   x = -( Dv^T q1 + Dh^T q2 )
__device__ __forceinline__ float dT(float prev, float cur, int k, int n) { return (k >= 1 ? prev : 0.f) - (k <= n - 2 ? cur : 0.f); }
// q1, q2 at sample (i,j) of an H x W section from g there (g0) and at its h / v predecessors (gh, gv)
__device__ __forceinline__ HaleP hale_qv(float g0, float gh, float gv, int i, int j, int H, int W, float a, float b, float c) {
  const float r1 = dT(gh, g0, j, W);
  const float r2 = dT(gv, g0, i, H);
  HaleP r;
  r.p1 = a * r1 + b * r2;
  r.p2 = b * r1 + c * r2;
  return r;
}
__device__ __forceinline__ HaleP hale_q(const float* __restrict__ g, const float* __restrict__ a, const float* __restrict__ b,
                                        const float* __restrict__ c, size_t base, int i, int j, int H, int W) {
  const size_t o = base + (size_t)i * W + j;
  return hale_qv(g[o], j >= 1 ? g[o - 1] : 0.f, i >= 1 ? g[o - W] : 0.f, i, j, H, W, a[o], b[o], c[o]);
}
__global__ __launch_bounds__(256) void hale2d_adj_kernel(const float* __restrict__ g, const float* __restrict__ a, const float* __restrict__ b,
                                                         const float* __restrict__ c, size_t total, int H, int W, float* __restrict__ xo) {
  const size_t plane = (size_t)H * W;
  for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (size_t)gridDim.x * 256) {
    const size_t base = idx / plane * plane;
    const int i = (int)((idx - base) / W), j = (int)((idx - base) % W);
    const HaleP q = hale_q(g, a, b, c, base, i, j, H, W);
    const float q1_up = i >= 1 ? hale_q(g, a, b, c, base, i - 1, j, H, W).p1 : 0.f;
    const float q2_left = j >= 1 ? hale_q(g, a, b, c, base, i, j - 1, H, W).p2 : 0.f;
    xo[idx] = -(dT(q1_up, q.p1, i, H) + dT(q2_left, q.p2, j, W));
  }
}

// ---- Hale2D on both families of vertical sections of a [C][T][X][Y] patch ----------------------------------------------
// (t,x) sections: v = t (stride X*Y), h = x (stride Y); (t,y) sections: v = t, h = y (stride 1).  Coefficients: six [C][T][X][Y]
// fields a, b, c of the (t,x) family, then of the (t,y) family.  One thread owns V consecutive samples of a y-row (float4 when
// Y % 4 == 0) and reads the rows its 3x3 neighbourhoods touch; the rows of the neighbouring x / t come back through L2 / MALL,
// so HBM sees x, the six coefficient fields and the two outputs once: 36 bytes per sample either way.
template <int V>
__device__ __forceinline__ void ld_row(const float* __restrict__ p, size_t o, bool ok, float* r) {
  if (V == 4) {
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (ok) v = *reinterpret_cast<const float4*>(p + o);
    r[0] = v.x; r[1] = v.y; r[2] = v.z; r[3] = v.w;
  } else {
    r[0] = ok ? p[o] : 0.f;
  }
}
template <int V>
__device__ __forceinline__ void st_row(float* __restrict__ p, size_t o, const float* r) {
  if (V == 4) *reinterpret_cast<float4*>(p + o) = make_float4(r[0], r[1], r[2], r[3]);
  else p[o] = r[0];
}

template <int V>
__global__ __launch_bounds__(256) void hale_sections_fwd_kernel(const float* __restrict__ x, const float* __restrict__ coef, unsigned rows, int T,
                                                                int X, int Y, size_t n, float* __restrict__ y) {
  const unsigned nq = (unsigned)Y / V, total = rows * nq;
  const size_t sv = (size_t)X * Y;
  const float *a0 = coef, *b0 = coef + n, *c0 = coef + 2 * n, *a1 = coef + 3 * n, *b1 = coef + 4 * n, *c1 = coef + 5 * n;
  for (unsigned idx = blockIdx.x * 256 + threadIdx.x; idx < total; idx += gridDim.x * 256) {
    const unsigned r = idx / nq, q = idx - r * nq;
    const int xi = (int)(r % (unsigned)X), t = (int)(r / (unsigned)X % (unsigned)T), y0 = (int)q * V;
    const size_t o = (size_t)r * Y + y0;
    const bool t1 = t <= T - 2, t2 = t <= T - 3, x1 = xi <= X - 2, x2 = xi <= X - 3;
    const bool e1 = y0 + V < Y, e2 = y0 + V + 1 < Y;           // the samples past the row segment along y exist
    // x at (t,x) [+2 along y], (t+1,x) [+1], (t+2,x), (t,x+1), (t+1,x+1), (t,x+2)
    float xa[V + 2], xb[V + 1], xc[V], xd[V], xe[V], xf[V];
    ld_row<V>(x, o, true, xa);
    xa[V] = e1 ? x[o + V] : 0.f;
    xa[V + 1] = e2 ? x[o + V + 1] : 0.f;
    ld_row<V>(x, o + sv, t1, xb);
    xb[V] = t1 && e1 ? x[o + sv + V] : 0.f;
    ld_row<V>(x, o + 2 * sv, t2, xc);
    ld_row<V>(x, o + Y, x1, xd);
    ld_row<V>(x, o + sv + Y, t1 && x1, xe);
    ld_row<V>(x, o + 2 * (size_t)Y, x2, xf);
    // (t,x) coefficients at (t,x), (t,x+1), (t+1,x); (t,y) coefficients at (t,x) [+1 along y], (t+1,x)
    float A[V], B[V], Cc[V], Ah[V], Bh[V], Ch[V], Av[V], Bv[V], Cv[V];
    ld_row<V>(a0, o, true, A); ld_row<V>(b0, o, true, B); ld_row<V>(c0, o, true, Cc);
    ld_row<V>(a0, o + Y, x1, Ah); ld_row<V>(b0, o + Y, x1, Bh); ld_row<V>(c0, o + Y, x1, Ch);
    ld_row<V>(a0, o + sv, t1, Av); ld_row<V>(b0, o + sv, t1, Bv); ld_row<V>(c0, o + sv, t1, Cv);
    float P[V + 1], Q[V + 1], R[V + 1], Pv[V], Qv[V], Rv[V];
    ld_row<V>(a1, o, true, P); ld_row<V>(b1, o, true, Q); ld_row<V>(c1, o, true, R);
    P[V] = e1 ? a1[o + V] : 0.f;
    Q[V] = e1 ? b1[o + V] : 0.f;
    R[V] = e1 ? c1[o + V] : 0.f;
    ld_row<V>(a1, o + sv, t1, Pv); ld_row<V>(b1, o + sv, t1, Qv); ld_row<V>(c1, o + sv, t1, Rv);
    float out0[V], out1[V];
#pragma unroll
    for (int l = 0; l < V; ++l) {
      // (t,x) section: p at (t,x), p1 at (t,x+1), p2 at (t+1,x)
      HaleP p = hale_pv(xa[l], xb[l], xd[l], t1, x1, A[l], B[l], Cc[l]);
      float ata1 = 0.f, ata2 = 0.f;
      if (x1) ata1 = hale_pv(xd[l], xe[l], xf[l], t1, x2, Ah[l], Bh[l], Ch[l]).p1 - p.p1;
      if (t1) ata2 = hale_pv(xb[l], xc[l], xe[l], t2, x1, Av[l], Bv[l], Cv[l]).p2 - p.p2;
      out0[l] = -(ata1 + ata2);
      // (t,y) section: p at (t,y), p1 at (t,y+1), p2 at (t+1,y)
      const int j = y0 + l;
      const bool y1 = j <= Y - 2, y2 = j <= Y - 3;
      p = hale_pv(xa[l], xb[l], xa[l + 1], t1, y1, P[l], Q[l], R[l]);
      ata1 = 0.f;
      ata2 = 0.f;
      if (y1) ata1 = hale_pv(xa[l + 1], xb[l + 1], xa[l + 2], t1, y2, P[l + 1], Q[l + 1], R[l + 1]).p1 - p.p1;
      if (t1) ata2 = hale_pv(xb[l], xc[l], xb[l + 1], t2, y1, Pv[l], Qv[l], Rv[l]).p2 - p.p2;
      out1[l] = -(ata1 + ata2);
    }
    st_row<V>(y, o, out0);
    st_row<V>(y, n + o, out1);
  }
}

// adjoint: x = L_tx^T g[0] + L_ty^T g[1], each term as hale2d_adj_kernel evaluates it on its section
template <int V>
__global__ __launch_bounds__(256) void hale_sections_adj_kernel(const float* __restrict__ g, const float* __restrict__ coef, unsigned rows, int T,
                                                                int X, int Y, size_t n, float* __restrict__ xo) {
  const unsigned nq = (unsigned)Y / V, total = rows * nq;
  const size_t sv = (size_t)X * Y;
  const float *a0 = coef, *b0 = coef + n, *c0 = coef + 2 * n, *a1 = coef + 3 * n, *b1 = coef + 4 * n, *c1 = coef + 5 * n;
  const float *g0 = g, *g1 = g + n;
  for (unsigned idx = blockIdx.x * 256 + threadIdx.x; idx < total; idx += gridDim.x * 256) {
    const unsigned r = idx / nq, q = idx - r * nq;
    const int xi = (int)(r % (unsigned)X), t = (int)(r / (unsigned)X % (unsigned)T), y0 = (int)q * V;
    const size_t o = (size_t)r * Y + y0;
    const bool t1 = t >= 1, t2 = t >= 2, x1 = xi >= 1, x2 = xi >= 2;
    // g[0] at (t,x), (t,x-1), (t-1,x), (t-1,x-1), (t-2,x), (t,x-2)
    float ga[V], gb[V], gc[V], gd[V], ge[V], gf[V];
    ld_row<V>(g0, o, true, ga);
    ld_row<V>(g0, o - (x1 ? Y : 0), x1, gb);
    ld_row<V>(g0, o - (t1 ? sv : 0), t1, gc);
    ld_row<V>(g0, o - (t1 && x1 ? sv + Y : 0), t1 && x1, gd);
    ld_row<V>(g0, o - (t2 ? 2 * sv : 0), t2, ge);
    ld_row<V>(g0, o - (x2 ? 2 * (size_t)Y : 0), x2, gf);
    // g[1] at (t,x) [-2 along y: ha[k] = y0 - 2 + k], (t-1,x) [-1: hb[k] = y0 - 1 + k], (t-2,x)
    float ha[V + 2], hb[V + 1], hc[V];
    ha[0] = y0 >= 2 ? g1[o - 2] : 0.f;
    ha[1] = y0 >= 1 ? g1[o - 1] : 0.f;
    ld_row<V>(g1, o, true, ha + 2);
    hb[0] = t1 && y0 >= 1 ? g1[o - sv - 1] : 0.f;
    ld_row<V>(g1, o - (t1 ? sv : 0), t1, hb + 1);
    ld_row<V>(g1, o - (t2 ? 2 * sv : 0), t2, hc);
    // (t,x) coefficients at (t,x), (t-1,x), (t,x-1); (t,y) coefficients at (t,x) [-1 along y], (t-1,x)
    float A[V], B[V], Cc[V], Au[V], Bu[V], Cu[V], Al[V], Bl[V], Cl[V];
    ld_row<V>(a0, o, true, A); ld_row<V>(b0, o, true, B); ld_row<V>(c0, o, true, Cc);
    ld_row<V>(a0, o - (t1 ? sv : 0), t1, Au); ld_row<V>(b0, o - (t1 ? sv : 0), t1, Bu); ld_row<V>(c0, o - (t1 ? sv : 0), t1, Cu);
    ld_row<V>(a0, o - (x1 ? Y : 0), x1, Al); ld_row<V>(b0, o - (x1 ? Y : 0), x1, Bl); ld_row<V>(c0, o - (x1 ? Y : 0), x1, Cl);
    float P[V + 1], Q[V + 1], R[V + 1], Pu[V], Qu[V], Ru[V];
    P[0] = y0 >= 1 ? a1[o - 1] : 0.f;
    Q[0] = y0 >= 1 ? b1[o - 1] : 0.f;
    R[0] = y0 >= 1 ? c1[o - 1] : 0.f;
    ld_row<V>(a1, o, true, P + 1); ld_row<V>(b1, o, true, Q + 1); ld_row<V>(c1, o, true, R + 1);
    ld_row<V>(a1, o - (t1 ? sv : 0), t1, Pu); ld_row<V>(b1, o - (t1 ? sv : 0), t1, Qu); ld_row<V>(c1, o - (t1 ? sv : 0), t1, Ru);
    float out[V];
#pragma unroll
    for (int l = 0; l < V; ++l) {
      // (t,x) section: q at (t,x), q1 at (t-1,x), q2 at (t,x-1)
      HaleP qq = hale_qv(ga[l], gb[l], gc[l], t, xi, T, X, A[l], B[l], Cc[l]);
      float q1_up = t1 ? hale_qv(gc[l], gd[l], ge[l], t - 1, xi, T, X, Au[l], Bu[l], Cu[l]).p1 : 0.f;
      float q2_left = x1 ? hale_qv(gb[l], gf[l], gd[l], t, xi - 1, T, X, Al[l], Bl[l], Cl[l]).p2 : 0.f;
      const float s0 = -(dT(q1_up, qq.p1, t, T) + dT(q2_left, qq.p2, xi, X));
      // (t,y) section: q at (t,y), q1 at (t-1,y), q2 at (t,y-1)
      const int j = y0 + l;
      qq = hale_qv(ha[l + 2], ha[l + 1], hb[l + 1], t, j, T, Y, P[l + 1], Q[l + 1], R[l + 1]);
      q1_up = t1 ? hale_qv(hb[l + 1], hb[l], hc[l], t - 1, j, T, Y, Pu[l], Qu[l], Ru[l]).p1 : 0.f;
      q2_left = j >= 1 ? hale_qv(ha[l + 1], ha[l], hb[l], t, j - 1, T, Y, P[l], Q[l], R[l]).p2 : 0.f;
      const float s1 = -(dT(q1_up, qq.p1, t, T) + dT(q2_left, qq.p2, j, Y));
      out[l] = s0 + s1;
    }
    st_row<V>(xo, o, out);
  }
}

// ---- structure tensor (utils/slopes.py:6-48) ----------------------------------------------------------------------
__global__ __launch_bounds__(256) void structure_tensor_kernel(const float* __restrict__ x, size_t total, int H, int W, float dv, float dh,
                                                               float* __restrict__ gvv, float* __restrict__ gvh, float* __restrict__ ghh) {
  const size_t plane = (size_t)H * W;
  for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (size_t)gridDim.x * 256) {
    const size_t base = idx / plane * plane;
    const int i = (int)((idx - base) / W), j = (int)((idx - base) % W);
    const float x0 = x[idx];
    const float gv = i <= H - 2 ? (x[idx + W] - x0) / dv : 0.f;
    const float gh = j <= W - 2 ? (x[idx + 1] - x0) / dh : 0.f;
    gvv[idx] = gv * gv;
    gvh[idx] = gv * gh;
    ghh[idx] = gh * gh;
  }
}
// the same forward-difference gradients along t, x and y of a [C][T][X][Y] patch, and the five products of the (t,x) and (t,y)
// section tensors in one pass (gtt is shared by both families)
__global__ __launch_bounds__(256) void structure_tensor_sections_kernel(const float* __restrict__ x, size_t total, int T, int X, int Y, float dt,
                                                                        float dx, float dy, float* __restrict__ gtt, float* __restrict__ gtx,
                                                                        float* __restrict__ gxx, float* __restrict__ gty, float* __restrict__ gyy) {
  const size_t sv = (size_t)X * Y;
  for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (size_t)gridDim.x * 256) {
    const int yi = (int)(idx % (size_t)Y);
    const size_t r = idx / (size_t)Y;
    const int xi = (int)(r % (size_t)X), t = (int)(r / (size_t)X % (size_t)T);
    const float x0 = x[idx];
    const float gt = t <= T - 2 ? (x[idx + sv] - x0) / dt : 0.f;
    const float gx = xi <= X - 2 ? (x[idx + Y] - x0) / dx : 0.f;
    const float gy = yi <= Y - 2 ? (x[idx + 1] - x0) / dy : 0.f;
    gtt[idx] = gt * gt;
    gtx[idx] = gt * gx;
    gxx[idx] = gx * gx;
    gty[idx] = gt * gy;
    gyy[idx] = gy * gy;
  }
}
// eigen-decomposition of the 2x2 tensor per sample: phi = atan((l1 - gvv) / gvh) with NaN -> 0 (0/0 where the tensor is
// diagonal), anisotropy = 1 - l2 / l1 (left as IEEE gives it, like the reference)
__global__ __launch_bounds__(256) void dips_kernel(const float* __restrict__ gvv, const float* __restrict__ gvh, const float* __restrict__ ghh,
                                                   size_t n, float* __restrict__ phi, float* __restrict__ aniso) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    const float vv = gvv[i], vh = gvh[i], hh = ghh[i];
    const float t1 = 0.5f * (vv + hh);
    const float d = vv - hh;
    const float t2 = 0.5f * sqrtf(d * d + 4.f * (vh * vh));
    const float l1 = t1 + t2, l2 = t1 - t2;
    float p = atanf((l1 - vv) / vh);
    if (p != p) p = 0.f;
    phi[i] = p;
    aniso[i] = 1.f - l2 / l1;
  }
}

// ---- POCS (utils/pocs.py:5-19, 80-84) -----------------------------------------------------------------------------
// max over a real tensor (the reference thresholds real and imaginary parts of the spectrum as independent reals), two
// stages, deterministic; the threshold th = max * perc / 100 stays on the device.
__global__ __launch_bounds__(256) void max_partial_kernel(const float* __restrict__ x, size_t n, float* __restrict__ part) {
  __shared__ float sh[4];
  float m = -INFINITY;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) m = fmaxf(m, x[i]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = fmaxf(fmaxf(sh[0], sh[1]), fmaxf(sh[2], sh[3]));
}
__global__ __launch_bounds__(256) void max_final_kernel(const float* __restrict__ part, int nb, float scale, float* __restrict__ out) {
  __shared__ float sh[4];
  float m = -INFINITY;
  for (int i = threadIdx.x; i < nb; i += 256) m = fmaxf(m, part[i]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) out[0] = fmaxf(fmaxf(sh[0], sh[1]), fmaxf(sh[2], sh[3])) * scale;
}
// y = x * ((x > th) + (x < -th))
__global__ __launch_bounds__(256) void threshold_kernel(const float* __restrict__ x, size_t n, const float* __restrict__ th_ptr, float* __restrict__ y) {
  const float th = *th_ptr;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    const float v = x[i];
    y[i] = v * ((v > th ? 1.f : 0.f) + (v < -th ? 1.f : 0.f));
  }
}
// y = wdata + wmask * x      (weighted_data + weighted_mask * adjoint(threshold(forward(x))))
__global__ __launch_bounds__(256) void pocs_project_kernel(const float* __restrict__ x, const float* __restrict__ wdata, const float* __restrict__ wmask,
                                                           size_t n, float* __restrict__ y) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) y[i] = wdata[i] + wmask[i] * x[i];
}

}  // namespace

extern "C" int dpi_diff_axis(const float* x, size_t outer, int n, size_t inner, int stencil, float spacing, int adjoint, float* y, void* stream) {
  DPI_REQUIRE(x && y && x != y && outer > 0 && n > 0 && inner > 0, "diff_axis: bad argument");
  DPI_REQUIRE(stencil >= 0 && stencil <= 3, "diff_axis: stencil must be 0 (forward), 1 (backward), 2 (centered) or 3 (second)");
  DPI_REQUIRE(spacing != 0.f, "diff_axis: zero spacing");
  const size_t total = outer * (size_t)n * inner;
  const float scale = stencil == 3 ? spacing * spacing : spacing;
  diff_axis_kernel<<<op_blocks(total), 256, 0, (hipStream_t)stream>>>(x, total, n, inner, stencil, scale, adjoint, y);
  return dpi_check_launch("diff_axis");
}

extern "C" int dpi_hale2d(const float* x, const float* a, const float* b, const float* c, size_t N, int H, int W, int adjoint, float* y, void* stream) {
  DPI_REQUIRE(x && a && b && c && y && x != y && N > 0 && H > 0 && W > 0, "hale2d: bad argument");
  const size_t total = N * (size_t)H * W;
  if (adjoint) hale2d_adj_kernel<<<op_blocks(total), 256, 0, (hipStream_t)stream>>>(x, a, b, c, total, H, W, y);
  else hale2d_fwd_kernel<<<op_blocks(total), 256, 0, (hipStream_t)stream>>>(x, a, b, c, total, H, W, y);
  return dpi_check_launch("hale2d");
}

extern "C" int dpi_hale_sections(const float* x, const float* coef, int C, int T, int X, int Y, int adjoint, float* y, void* stream) {
  DPI_REQUIRE(x && coef && y && x != y && C > 0 && T > 0 && X > 0 && Y > 0, "hale_sections: bad argument");
  const size_t rows = (size_t)C * T * X, n = rows * Y;
  DPI_REQUIRE(n < ((size_t)1 << 31), "hale_sections: patch of %zu samples exceeds 2^31", n);
  const bool v4 = Y % 4 == 0 && ((uintptr_t)x | (uintptr_t)coef | (uintptr_t)y) % 16 == 0;
  const unsigned nb = op_blocks(v4 ? n / 4 : n);
  hipStream_t st = (hipStream_t)stream;
  if (adjoint) {
    if (v4) hale_sections_adj_kernel<4><<<nb, 256, 0, st>>>(x, coef, (unsigned)rows, T, X, Y, n, y);
    else hale_sections_adj_kernel<1><<<nb, 256, 0, st>>>(x, coef, (unsigned)rows, T, X, Y, n, y);
  } else {
    if (v4) hale_sections_fwd_kernel<4><<<nb, 256, 0, st>>>(x, coef, (unsigned)rows, T, X, Y, n, y);
    else hale_sections_fwd_kernel<1><<<nb, 256, 0, st>>>(x, coef, (unsigned)rows, T, X, Y, n, y);
  }
  return dpi_check_launch("hale_sections");
}

extern "C" int dpi_structure_tensor_sections(const float* x, int C, int T, int X, int Y, float dt, float dx, float dy, float* gtt, float* gtx,
                                             float* gxx, float* gty, float* gyy, void* stream) {
  DPI_REQUIRE(x && gtt && gtx && gxx && gty && gyy && C > 0 && T > 0 && X > 0 && Y > 0 && dt != 0.f && dx != 0.f && dy != 0.f,
              "structure_tensor_sections: bad argument");
  const size_t total = (size_t)C * T * X * Y;
  structure_tensor_sections_kernel<<<op_blocks(total), 256, 0, (hipStream_t)stream>>>(x, total, T, X, Y, dt, dx, dy, gtt, gtx, gxx, gty, gyy);
  return dpi_check_launch("structure_tensor_sections");
}

extern "C" int dpi_structure_tensor(const float* x, size_t N, int H, int W, float dv, float dh, float* gvv, float* gvh, float* ghh, void* stream) {
  DPI_REQUIRE(x && gvv && gvh && ghh && N > 0 && H > 0 && W > 0 && dv != 0.f && dh != 0.f, "structure_tensor: bad argument");
  const size_t total = N * (size_t)H * W;
  structure_tensor_kernel<<<op_blocks(total), 256, 0, (hipStream_t)stream>>>(x, total, H, W, dv, dh, gvv, gvh, ghh);
  return dpi_check_launch("structure_tensor");
}

extern "C" int dpi_dips(const float* gvv, const float* gvh, const float* ghh, size_t n, float* phi, float* anisotropy, void* stream) {
  DPI_REQUIRE(gvv && gvh && ghh && phi && anisotropy && n > 0, "dips: bad argument");
  dips_kernel<<<op_blocks(n), 256, 0, (hipStream_t)stream>>>(gvv, gvh, ghh, n, phi, anisotropy);
  return dpi_check_launch("dips");
}

extern "C" size_t dpi_max_ws_floats(size_t n) { return (size_t)op_blocks(n); }

extern "C" int dpi_scaled_max(const float* x, size_t n, float scale, float* ws, float* out, void* stream) {
  DPI_REQUIRE(x && ws && out && n > 0, "scaled_max: bad argument");
  const unsigned nb = op_blocks(n);
  max_partial_kernel<<<nb, 256, 0, (hipStream_t)stream>>>(x, n, ws);
  max_final_kernel<<<1, 256, 0, (hipStream_t)stream>>>(ws, (int)nb, scale, out);
  return dpi_check_launch("scaled_max");
}

extern "C" int dpi_threshold(const float* x, size_t n, const float* thresh, float* y, void* stream) {
  DPI_REQUIRE(x && y && thresh && n > 0, "threshold: bad argument");
  threshold_kernel<<<op_blocks(n), 256, 0, (hipStream_t)stream>>>(x, n, thresh, y);
  return dpi_check_launch("threshold");
}

extern "C" int dpi_pocs_project(const float* x, const float* wdata, const float* wmask, size_t n, float* y, void* stream) {
  DPI_REQUIRE(x && wdata && wmask && y && n > 0, "pocs_project: bad argument");
  pocs_project_kernel<<<op_blocks(n), 256, 0, (hipStream_t)stream>>>(x, wdata, wmask, n, y);
  return dpi_check_launch("pocs_project");
}
