// The per-trace interpolation weights of --trace_interp (ours, no reference code): plain C++ on host pointers, no device code, so that the
// Python operator, C-ABI users and a stand-alone sanitizer build (tests/host_weights) share this one definition.  include/dpi_hip.h has
// the definition: kinds 0 / 1 / 2 = linear / cubic (Keys, a = -1/2) / sinc8 (8-tap Kaiser-windowed sinc) with K = 2 / 4 / 8 taps per
// axis; tap k of a trace with offset d sits at u = (k - K/2 + (d >= 0)) - d from the trace; float64 arithmetic from the fp32 offset, one
// rounding to fp32 at the end; d == 0 is the unit tap with exact zeros around it.
#include <math.h>
#include <stddef.h>
#include "../../include/dpi_hip.h"

void dpi_set_error(const char* fmt, ...);

namespace {

constexpr double TI_SINC8_BETA = 6.0;      // Kaiser window of sinc8; not tuned: 3 .. 8 move the stand-in's modelling floor by < 1.2 dB
constexpr double TI_PI = 3.14159265358979323846;

// modified Bessel function of the first kind, order 0: sum ((x/2)^2 / j^2 ...), x in [0, beta]
double ti_i0(double x) {
  const double q = 0.25 * x * x;
  double term = 1.0, sum = 1.0;
  for (int j = 1; j < 200; ++j) {
    term *= q / ((double)j * (double)j);
    sum += term;
    if (term < 1e-17 * sum) break;
  }
  return sum;
}

// Keys, a = -1/2, in the factored spelling of its two cubics: 1.5 s^3 - 2.5 s^2 + 1 = 1 - s^2 (2.5 - 1.5 s) and
// -0.5 s^3 + 2.5 s^2 - 4 s + 2 = -0.5 (s - 1) (s - 2)^2.  No cancellation between large terms: the four weights sum to 1 within 4e-16.
double ti_keys(double u) {
  const double s = fabs(u);
  if (s <= 1.0) return 1.0 - s * s * (2.5 - 1.5 * s);
  if (s < 2.0) return -0.5 * (s - 1.0) * (s - 2.0) * (s - 2.0);
  return 0.0;
}

double ti_kaiser_sinc(double u) {
  const double a = 1.0 - (u / 4.0) * (u / 4.0);
  const double win = ti_i0(TI_SINC8_BETA * sqrt(a > 0.0 ? a : 0.0)) / ti_i0(TI_SINC8_BETA);
  return (u == 0.0 ? 1.0 : sin(TI_PI * u) / (TI_PI * u)) * win;
}

// the K weights of one axis of one trace for an offset d >= 0 (or not a number), taps k - K/2 + 1 .. ; d < 0 is its mirror image
void ti_axis(int kind, int K, double d, double* w) {
  for (int k = 0; k < K; ++k) {
    const double u = (double)(k - K / 2 + 1) - d;
    w[k] = kind == 0 ? 1.0 - fabs(u) : kind == 1 ? ti_keys(u) : ti_kaiser_sinc(u);
  }
  if (kind == 2) {
    double sum = 0.0;
    for (int k = 0; k < K; ++k) sum += w[k];
    for (int k = 0; k < K; ++k) w[k] /= sum;
  }
}

}  // namespace

extern "C" int dpi_trace_interp_taps(int kind) { return kind == 0 ? 2 : kind == 1 ? 4 : kind == 2 ? 8 : -1; }

extern "C" int dpi_trace_interp_weights(const float* off, int kind, int X, int Y, float* w) {
  const int K = dpi_trace_interp_taps(kind);
  if (!off || !w || K < 0 || X <= 0 || Y <= 0) {
    dpi_set_error("trace_interp_weights: bad argument (kind %d, %d x %d traces)", kind, X, Y);
    return DPI_E_ARG;
  }
  const size_t S = (size_t)X * (size_t)Y;
  double ws[8];
  for (int axis = 0; axis < 2; ++axis) {
    for (size_t s = 0; s < S; ++s) {
      const float d = off[(size_t)axis * S + s];
      float* out = w + (size_t)axis * K * S + s;
      if (d == 0.f) {                                                       // on its node: the identity bit for bit
        for (int k = 0; k < K; ++k) out[(size_t)k * S] = k == K / 2 - 1 ? 1.f : 0.f;
      } else if (d < 0.f) {                                                 // taps i - K/2 .. : w(d)[k] = w(-d)[K - 1 - k] exactly
        ti_axis(kind, K, -(double)d, ws);
        for (int k = 0; k < K; ++k) out[(size_t)k * S] = (float)ws[K - 1 - k];
      } else {
        ti_axis(kind, K, (double)d, ws);
        for (int k = 0; k < K; ++k) out[(size_t)k * S] = (float)ws[k];
      }
    }
  }
  return DPI_OK;
}
