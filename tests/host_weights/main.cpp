// Stand-alone driver of the --trace_interp weight builder (csrc/trace_interp.cpp: plain C++, no device code), built with
// the address and undefined-behaviour sanitizers (host only) by tests/test_trace_interp_host.py and run as a program on the CPU.  Every buffer is a heap block of
// exactly the size the entry point is entitled to, so a read or write past [2][X][Y] / [2][K][X][Y] is reported by AddressSanitizer.
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "../../include/dpi_hip.h"

static char last_error[256];
void dpi_set_error(const char* fmt, ...) {          // the library's own lives in api.cpp, which is not part of this build
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(last_error, sizeof last_error, fmt, ap);
  va_end(ap);
}

static int failures = 0;
#define EXPECT(cond, ...)                 \
  do {                                    \
    if (!(cond)) {                        \
      ++failures;                         \
      printf("FAIL %s:%d: ", __FILE__, __LINE__); \
      printf(__VA_ARGS__);                \
      printf("\n");                       \
    }                                     \
  } while (0)

static unsigned lcg_state = 12345u;
static float lcg_uniform() {                        // [-0.5, 0.5], a quarter of the draws exactly 0
  lcg_state = lcg_state * 1664525u + 1013904223u;
  const unsigned r = lcg_state >> 8;
  if ((r & 3u) == 0u) return 0.f;
  return (float)((double)(r >> 2) / (double)(1u << 22)) - 0.5f;
}

int main() {
  const int shapes[][2] = {{1, 1}, {2, 1}, {67, 1}, {5, 7}, {33, 67}, {2, 3}, {16, 64}, {9, 12}};      // (X, Y) of the host cases
  const char* kinds[] = {"zero", "plus_half", "minus_half", "random"};
  int tables = 0;
  for (const auto& sh : shapes) {
    const int X = sh[0], Y = sh[1];
    const size_t S = (size_t)X * Y;
    for (int ok = 0; ok < 4; ++ok) {
      float* off = (float*)malloc(2 * S * sizeof(float));
      for (size_t i = 0; i < 2 * S; ++i) off[i] = ok == 0 ? 0.f : ok == 1 ? 0.5f : ok == 2 ? -0.5f : lcg_uniform();
      for (int kind = 0; kind < 3; ++kind) {
        const int K = dpi_trace_interp_taps(kind);
        EXPECT(K == (kind == 0 ? 2 : kind == 1 ? 4 : 8), "taps of kind %d: %d", kind, K);
        float* w = (float*)malloc(2 * (size_t)K * S * sizeof(float));
        for (size_t i = 0; i < 2 * (size_t)K * S; ++i) w[i] = NAN;
        EXPECT(dpi_trace_interp_weights(off, kind, X, Y, w) == DPI_OK, "%s kind %d %d x %d: %s", kinds[ok], kind, X, Y, last_error);
        for (int axis = 0; axis < 2; ++axis) {
          for (size_t s = 0; s < S; ++s) {
            double sum = 0.0;
            for (int k = 0; k < K; ++k) sum += (double)w[((size_t)axis * K + k) * S + s];
            EXPECT(fabs(sum - 1.0) <= K * ldexp(1.0, -24), "%s kind %d %d x %d axis %d trace %zu: weights sum to %.9g", kinds[ok], kind, X, Y,
                   axis, s, sum);
            if (off[(size_t)axis * S + s] == 0.f)
              for (int k = 0; k < K; ++k)
                EXPECT(w[((size_t)axis * K + k) * S + s] == (k == K / 2 - 1 ? 1.f : 0.f), "unit tap: kind %d tap %d", kind, k);
          }
        }
        free(w);
        ++tables;
      }
      free(off);
    }
  }
  // refusals: nothing is read or written
  float one = 0.25f, eight[16];
  EXPECT(dpi_trace_interp_taps(3) == -1 && dpi_trace_interp_taps(-1) == -1, "unknown kinds");
  EXPECT(dpi_trace_interp_weights(nullptr, 1, 1, 1, eight) == DPI_E_ARG, "null offsets");
  EXPECT(dpi_trace_interp_weights(&one, 1, 1, 1, nullptr) == DPI_E_ARG, "null table");
  EXPECT(dpi_trace_interp_weights(&one, 3, 1, 1, eight) == DPI_E_ARG, "kind 3");
  EXPECT(dpi_trace_interp_weights(&one, -1, 1, 1, eight) == DPI_E_ARG, "kind -1");
  EXPECT(dpi_trace_interp_weights(&one, 1, 0, 1, eight) == DPI_E_ARG, "X = 0");
  EXPECT(dpi_trace_interp_weights(&one, 1, 1, -2, eight) == DPI_E_ARG, "Y = -2");
  // offsets the Python operator refuses still address nothing out of bounds: the taps do not depend on the size of d
  std::vector<float> bad = {NAN, 7.5f}, wb(16);
  EXPECT(dpi_trace_interp_weights(bad.data(), 2, 1, 1, wb.data()) == DPI_OK, "out-of-range offsets");
  printf("%d tables, %d failures\n", tables, failures);
  return failures ? 1 : 0;
}
