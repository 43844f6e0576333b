"""The loop-control rule as the host sees it: one LoopRule per (held-out part, running average) says what the device rule of
csrc/loop_rule.h (dpi_loop_rule) reads and writes — history columns, state slots, entry point — and what the eager loop selects on.
The rule itself (selection with the later iterate winning a tie, ReduceLROnPlateau on the raw training loss, EarlyStopping and the NaN
stop on the selection misfit q) is stated in that header; the eager loop applies it with utils.select_latest_min, optim.DevicePlateau
and utils.EarlyStopping."""
import torch

from . import _lib

# state slots, by the names of enum dpi_loop_slot
SLOTS = dict(iteration=0, loss_min=1, plateau_best=2, plateau_bad=3, es_best=4, es_bad=5, es_has_best=6, val_min=8, best_iter=9, q_min=10)


class LoopRule:
    def __init__(self, holdout, ema):
        self.holdout, self.ema = bool(holdout), bool(ema)
        ema_cols = ("ema_loss", "ema_snr") + (("ema_val_loss", "ema_val_snr") if holdout else ())
        self.columns = ("loss", "snr", "pcorr", "lr") + (("val_loss", "val_snr") if holdout else ()) + (ema_cols if ema else ())
        self.metrics_doubles = 10 if holdout else 3              # what the eager loop reads back of a loss pass's result
        self.state_doubles = 12 if ema else (10 if holdout else 8)
        self.entry = "dpi_loop_control_ema" if ema else ("dpi_loop_control_holdout" if holdout else "dpi_loop_control")
        # the selection misfit q: its history column and the Interpolator attribute of its minimum (state slot q_min / val_min / loss_min)
        self.q_column = ("ema_" if ema else "") + ("val_loss" if holdout else "loss")
        self.q_min_attr = "ema_min" if ema else ("val_min" if holdout else "loss_min")
        self.tracks_best_iter = self.holdout or self.ema

    def q(self, history):
        """The selection misfit of the newest row of `history`: what out_best, best_iter, early stopping and the NaN stop follow."""
        return getattr(history, self.q_column)[-1]

    def new_state(self, epochs, device):
        """(state, hist, improved) of a fresh loop on the device."""
        state = torch.zeros(self.state_doubles, dtype=torch.float64, device=device)
        state[SLOTS["plateau_best"]] = float("inf")
        return (state, torch.zeros(epochs * len(self.columns), dtype=torch.float64, device=device),
                torch.zeros(1, dtype=torch.int32, device=device))

    def launch(self, metrics, ema, state, hist, max_iters, step_lr, active, improved, rules):
        p = _lib.ptr
        head = (p(metrics), p(ema), int(self.holdout)) if self.ema else (p(metrics),)
        _lib.check(getattr(_lib.load(), self.entry)(*head, p(state), p(hist), max_iters, p(step_lr), p(active), p(improved), *rules,
                                                    _lib.stream()), self.entry)

    def rows(self, state, hist):
        """(n, [n][columns] numpy rows, state as a list) of the loop so far: one read-back each of state and history."""
        st = state.tolist()
        n, cols = int(st[SLOTS["iteration"]]), len(self.columns)
        return n, hist[:cols * n].view(n, cols).cpu().numpy(), st

    def fill(self, T, history, h, st):
        """The device's rows `h` and state `st` into `history` and the minima / best_iter of the Interpolator T."""
        for k, name in enumerate(self.columns):
            setattr(history, name, h[:, k].tolist())
        T.loss_min = st[SLOTS["loss_min"]]
        if self.holdout:
            T.val_min = st[SLOTS["val_min"]]
        if self.ema:
            T.ema_min = st[SLOTS["q_min"]]
        if self.tracks_best_iter:
            T.best_iter = int(st[SLOTS["best_iter"]])

    def progress(self, n, row):
        r = dict(zip(self.columns, row))
        msg = "Iter %d, Loss = %+.2e, SNR = %+2.2f dB, PCORR = %+.2f %%" % (n, r["loss"], r["snr"], r["pcorr"] * 100)
        if self.holdout:
            msg += ", VAL = %.2e, VSNR = %+.2f dB" % (r["val_loss"], r["val_snr"])
        if self.ema:
            msg += ", ESNR = %+.2f dB" % r["ema_snr"]
        return msg
