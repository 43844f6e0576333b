// The loop-control rule, once: history row, minima and best-output selection, ReduceLROnPlateau, EarlyStopping, the NaN stop.  One thread
// runs it once per iteration (the dpi_loop_control* kernels of loss_optim.hip); plain C++, so a host program can include it as well.
// The host's description of the same layouts is deep_prior_interpolation_amd/loop.py (LoopRule).
#pragma once
#include <math.h>
#include <stddef.h>

#if defined(__HIP__) || defined(__CUDACC__)
#define DPI_LOOP_FN __host__ __device__ inline
#else
#define DPI_LOOP_FN inline
#endif

// state: 8 doubles (plain), 10 (held-out part), 12 (running average, with or without a held-out part); slots 7 and 11 are reserved
enum dpi_loop_slot {
  LOOP_ITERATION = 0,     // calls made while *active: the next history row
  LOOP_LOSS_MIN = 1,      // minimum of the raw training loss (the selection minimum of the plain variant)
  LOOP_PLATEAU_BEST = 2,  // ReduceLROnPlateau: best raw training loss (starts at +inf) ...
  LOOP_PLATEAU_BAD = 3,   // ... and the calls since it improved
  LOOP_ES_BEST = 4,       // EarlyStopping on q: best ...
  LOOP_ES_BAD = 5,        // ... calls since it improved ...
  LOOP_ES_HAS_BEST = 6,   // ... and whether a first value was seen
  LOOP_VAL_MIN = 8,       // held-out part: minimum of the raw held-out loss (its selection minimum without a running average)
  LOOP_BEST_ITER = 9,     // held-out part or running average: the iteration last selected
  LOOP_Q_MIN = 10         // running average: minimum of its selection misfit
};

struct dpi_loop_rules {
  int use_plateau; double factor, threshold; int patience; double min_lr, lr_eps;       // torch ReduceLROnPlateau, mode min / rel
  int es_patience; double es_min_delta;                                                 // utils/torch.py:216-275, percentage mode
};

// history row: {loss, snr, pcorr, lr[, val_loss, val_snr][, ema_loss, ema_snr[, ema_val_loss, ema_val_snr]]}
DPI_LOOP_FN int dpi_loop_row_doubles(bool holdout, bool ema) { return 4 + (holdout ? 2 : 0) + (ema ? (holdout ? 4 : 2) : 0); }

// metrics: the raw iterate's doubles (dpi_masked_loss, with `holdout` dpi_masked_loss_holdout); ema: those of the running average
// (dpi_ema_loss) or null.  *improved, best_iter, early stopping and the NaN stop follow the selection misfit q — loss, val_loss with a
// held-out part, the AVERAGE's ema_loss / ema_val_loss with one — the later iterate winning a tie (main.py:173-180); ReduceLROnPlateau
// follows the raw training loss.  A call with *active == 0 only clears *improved.
DPI_LOOP_FN void dpi_loop_rule(const double* metrics, const double* ema, bool holdout, double* state, double* hist, int max_iters,
                               float* step_lr, int* active, int* improved, const dpi_loop_rules& r) {
  *improved = 0;
  if (!*active) return;
  const int it = (int)state[LOOP_ITERATION];
  const double loss = metrics[0];
  const double q = ema ? (holdout ? ema[8] : ema[0]) : (holdout ? metrics[8] : loss);
  const int q_slot = ema ? LOOP_Q_MIN : (holdout ? LOOP_VAL_MIN : LOOP_LOSS_MIN);
  const double lr = (double)step_lr[1];
  if (it < max_iters) {
    double* row = hist + (size_t)dpi_loop_row_doubles(holdout, ema != nullptr) * it;
    *row++ = loss; *row++ = metrics[1]; *row++ = metrics[2]; *row++ = lr;
    if (holdout) { *row++ = metrics[8]; *row++ = metrics[9]; }
    if (ema) { *row++ = ema[0]; *row++ = ema[1]; if (holdout) { *row++ = ema[8]; *row++ = ema[9]; } }
  }
  const bool select = it == 0 || q <= state[q_slot];      // before any minimum is written: q_slot may be loss_min / val_min itself
  if (it == 0 || loss <= state[LOOP_LOSS_MIN]) state[LOOP_LOSS_MIN] = loss;
  if (holdout && (it == 0 || metrics[8] <= state[LOOP_VAL_MIN])) state[LOOP_VAL_MIN] = metrics[8];
  if (select) {
    state[q_slot] = q;
    if (q_slot != LOOP_LOSS_MIN) state[LOOP_BEST_ITER] = (double)it;      // the plain variant owns 8 doubles
    *improved = 1;
  }
  if (r.use_plateau) {
    if (loss < state[LOOP_PLATEAU_BEST] * (1.0 - r.threshold)) { state[LOOP_PLATEAU_BEST] = loss; state[LOOP_PLATEAU_BAD] = 0.0; }
    else state[LOOP_PLATEAU_BAD] += 1.0;
    if (state[LOOP_PLATEAU_BAD] > (double)r.patience) {
      const double nl = fmax(lr * r.factor, r.min_lr);
      if (lr - nl > r.lr_eps) step_lr[1] = (float)nl;
      state[LOOP_PLATEAU_BAD] = 0.0;
    }
  }
  if (r.es_patience != 0) {
    if (state[LOOP_ES_HAS_BEST] == 0.0) { state[LOOP_ES_BEST] = q; state[LOOP_ES_HAS_BEST] = 1.0; }
    else if (q != q) *active = 0;                                                       // a NaN misfit stops immediately
    else {
      if (q < state[LOOP_ES_BEST] - state[LOOP_ES_BEST] * r.es_min_delta / 100.0) { state[LOOP_ES_BAD] = 0.0; state[LOOP_ES_BEST] = q; }
      else state[LOOP_ES_BAD] += 1.0;
      if (state[LOOP_ES_BAD] >= (double)r.es_patience) *active = 0;
    }
  }
  state[LOOP_ITERATION] = (double)(it + 1);
}
