// csrc/loop_rule.h as plain C++ on the CPU (tests/test_iteration_refs_host.py builds and runs this, under the address and
// undefined-behaviour sanitizers).  Reads runs from stdin, every floating-point number as the hex bit pattern of its type:
//   run <holdout> <ema> <max_iters> <calls> <doubles per input> <lr0> <use_plateau> <factor> <threshold> <patience> <min_lr> <lr_eps>
//       <es_patience> <es_min_delta>
//   then per call the doubles of metrics and, with ema, those of the average.
// state, hist and the inputs are heap buffers of exactly the documented sizes, hist NaN-filled.  Calls stop once *active is 0, as a
// driver does.  Prints per call `C improved active lr state...`, per run `H hist...`, again as bit patterns.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "loop_rule.h"

static double read_double() {
  uint64_t b = 0;
  if (std::scanf("%" SCNx64, &b) != 1) { std::fprintf(stderr, "bad input\n"); std::exit(2); }
  double d;
  std::memcpy(&d, &b, 8);
  return d;
}
static int read_int() {
  int v = 0;
  if (std::scanf("%d", &v) != 1) { std::fprintf(stderr, "bad input\n"); std::exit(2); }
  return v;
}
static void print_double(double d) {
  uint64_t b;
  std::memcpy(&b, &d, 8);
  std::printf(" %016" PRIx64, b);
}

int main() {
  char word[8];
  int runs = 0;
  while (std::scanf("%7s", word) == 1) {
    if (std::strcmp(word, "run") != 0) { std::fprintf(stderr, "expected `run`\n"); return 2; }
    const int holdout = read_int(), has_ema = read_int(), max_iters = read_int(), calls = read_int(), n_in = read_int();
    uint32_t lr_bits = 0;
    if (std::scanf("%" SCNx32, &lr_bits) != 1) return 2;
    dpi_loop_rules r;
    r.use_plateau = read_int(); r.factor = read_double(); r.threshold = read_double(); r.patience = read_int();
    r.min_lr = read_double(); r.lr_eps = read_double(); r.es_patience = read_int(); r.es_min_delta = read_double();
    std::vector<double> state(has_ema ? 12 : (holdout ? 10 : 8), 0.0);
    state[LOOP_PLATEAU_BEST] = INFINITY;
    std::vector<double> hist((size_t)dpi_loop_row_doubles(holdout, has_ema) * max_iters, NAN);
    std::vector<double> metrics(n_in), ema(has_ema ? n_in : 0);
    std::vector<float> step_lr(2, 1.0f);
    std::memcpy(&step_lr[1], &lr_bits, 4);
    std::vector<int> active(1, 1), improved(1, 7);
    for (int c = 0; c < calls; ++c) {
      for (double& x : metrics) x = read_double();
      for (double& x : ema) x = read_double();
      if (!active[0]) continue;
      improved[0] = 7;
      dpi_loop_rule(metrics.data(), has_ema ? ema.data() : nullptr, holdout != 0, state.data(), hist.data(), max_iters, step_lr.data(),
                    active.data(), improved.data(), r);
      uint32_t lb;
      std::memcpy(&lb, &step_lr[1], 4);
      std::printf("C %d %d %08" PRIx32, improved[0], active[0], lb);
      for (double s : state) print_double(s);
      std::printf("\n");
    }
    std::printf("H");
    for (double h : hist) print_double(h);
    std::printf("\n");
    ++runs;
  }
  std::printf("%d runs\n", runs);
  return 0;
}
