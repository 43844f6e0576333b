"""SNR / Pearson correlation and the per-iteration History container (drop-in for reference utils/metrics.py).

Inside the optimisation loop the same quantities come out of the fused loss kernel (dpi_masked_loss);
these host/torch versions serve offline evaluation of reconstructed volumes."""
import numpy as np
import torch

from .generic import ten_digit

__all__ = ["snr", "pcorr", "History", "HistoryReg", "HistoryHoldout", "HistoryRegHoldout", "HistoryEma", "HistoryRegEma",
           "HistoryHoldoutEma", "HistoryRegHoldoutEma", "HistoryModelReg", "HistoryModelRegHoldout", "HistoryModelRegEma",
           "HistoryModelRegHoldoutEma", "history_class", "select_latest_min"]


def _lib(output, target):
    if target.shape != output.shape:
        raise ValueError("There is something wrong with the dimensions!")
    return torch if isinstance(output, torch.Tensor) and isinstance(target, torch.Tensor) else np


def snr(output, target):
    """10 log10( sum t^2 / sum (t-o)^2 ) in dB, on the full (unmasked) target."""
    xp = _lib(output, target)
    return 10 * xp.log10(xp.sum(target ** 2) / xp.sum((target - output) ** 2))


def pcorr(output, target):
    xp = _lib(output, target)
    td, od = target - xp.mean(target), output - xp.mean(output)
    return xp.sum(td * od) / (xp.sqrt(xp.sum(td ** 2)) * xp.sqrt(xp.sum(od ** 2)))


class History:
    """loss / snr / pcorr / lr lists, pickled into <patch>_run.npy (reference main.py:226-235)."""

    def __init__(self, epochs):
        self.loss, self.snr, self.pcorr, self.lr = [], [], [], []
        self.msg = "Iter %s, Loss = %+.2e, SNR = %+2.2f dB, PCORR = %+.2f %%"
        self.zfill = ten_digit(epochs)

    def __getitem__(self, i):
        return self.loss[i], self.snr[i], self.pcorr[i]

    def __setitem__(self, i, values):
        self.loss[i], self.snr[i], self.pcorr[i] = values

    def append(self, values):
        l, s, p = values
        self.loss.append(l)
        self.snr.append(s)
        self.pcorr.append(p)

    def __len__(self):
        assert len(self.loss) == len(self.snr) == len(self.pcorr) == len(self.lr)
        return len(self.loss)

    def log_message(self, idx):
        return self.msg % (str(idx + 1).zfill(self.zfill), self.loss[idx], self.snr[idx], self.pcorr[idx] * 100)

    def __str__(self):
        return "Loss : %s\nSNR  : %s\nPCORR: %s" % (self.loss, self.snr, self.pcorr)

    __repr__ = __str__


class HistoryReg:
    """History with the data-fidelity and regularisation terms split (reference utils/metrics.py:88-137; main_pocs.py:35)."""

    def __init__(self, epochs):
        self.loss, self.snr, self.pcorr, self.lr, self.df, self.reg = [], [], [], [], [], []
        self.msg = "Iter %s, Loss = %+.2e, DF = %.2e, REG = %.2e, SNR = %+.2f dB, PCORR = %+.2f %%"
        self.zfill = ten_digit(epochs)

    def __getitem__(self, i):
        return self.loss[i], self.reg[i], self.snr[i], self.pcorr[i]

    def __setitem__(self, i, values):
        self.loss[i], self.df[i], self.reg[i], self.snr[i], self.pcorr[i] = values

    def append(self, values):
        l, d, r, s, p = values
        self.loss.append(l)
        self.df.append(d)
        self.reg.append(r)
        self.snr.append(s)
        self.pcorr.append(p)

    def __len__(self):
        assert len(self.loss) == len(self.snr) == len(self.pcorr) == len(self.lr) == len(self.df) == len(self.reg)
        return len(self.loss)

    def log_message(self, idx):
        return self.msg % (str(idx + 1).zfill(self.zfill), self.loss[idx], self.df[idx], self.reg[idx], self.snr[idx], self.pcorr[idx] * 100)

    def __str__(self):
        return "Loss : %s\nReg  : %s\nSNR  : %s\nPCORR: %s" % (self.loss, self.reg, self.snr, self.pcorr)

    __repr__ = __str__


class _HoldoutColumns:
    """val_loss / val_snr columns of a run with held-out traces (--holdout): the misfit and the SNR on the held-out samples."""
    _vmsg = ", VAL = %.2e, VSNR = %+.2f dB"

    def append_val(self, val_loss, val_snr):
        self.val_loss.append(val_loss)
        self.val_snr.append(val_snr)

    def log_message(self, idx):
        return super().log_message(idx) + self._vmsg % (self.val_loss[idx], self.val_snr[idx])

    def __len__(self):
        n = super().__len__()
        assert len(self.val_loss) == len(self.val_snr) == n
        return n

    def __str__(self):
        return super().__str__() + "\nVAL  : %s\nVSNR : %s" % (self.val_loss, self.val_snr)

    __repr__ = __str__


class HistoryHoldout(_HoldoutColumns, History):
    """History of a run with --holdout."""

    def __init__(self, epochs):
        History.__init__(self, epochs)
        self.val_loss, self.val_snr = [], []


class HistoryRegHoldout(_HoldoutColumns, HistoryReg):
    """HistoryReg of a run with --holdout and a regulariser (--aa_weight): val_loss stays the pure data misfit."""

    def __init__(self, epochs):
        HistoryReg.__init__(self, epochs)
        self.val_loss, self.val_snr = [], []


class _EmaColumns:
    """ema_loss / ema_snr columns of a run with --out_ema: the misfit and the SNR of the running average of the network output (the
    out_avg of the deep-image-prior method), which is what such a run selects its output from.  With --holdout the classes below also
    carry ema_val_loss / ema_val_snr, the average's numbers on the held-out samples."""
    _emsg = ", ESNR = %+.2f dB"

    def _init_ema(self, holdout):
        self.ema_loss, self.ema_snr = [], []
        if holdout:
            self.ema_val_loss, self.ema_val_snr = [], []

    def append_ema(self, ema_loss, ema_snr, ema_val_loss=None, ema_val_snr=None):
        self.ema_loss.append(ema_loss)
        self.ema_snr.append(ema_snr)
        if hasattr(self, "ema_val_loss"):
            self.ema_val_loss.append(ema_val_loss)
            self.ema_val_snr.append(ema_val_snr)

    def log_message(self, idx):
        msg = super().log_message(idx) + self._emsg % self.ema_snr[idx]
        if hasattr(self, "ema_val_snr"):
            msg += ", EVSNR = %+.2f dB" % self.ema_val_snr[idx]
        return msg

    def __len__(self):
        n = super().__len__()
        assert len(self.ema_loss) == len(self.ema_snr) == n
        if hasattr(self, "ema_val_loss"):
            assert len(self.ema_val_loss) == len(self.ema_val_snr) == n
        return n

    def __str__(self):
        s = super().__str__() + "\nELOSS: %s\nESNR : %s" % (self.ema_loss, self.ema_snr)
        if hasattr(self, "ema_val_loss"):
            s += "\nEVAL : %s\nEVSNR: %s" % (self.ema_val_loss, self.ema_val_snr)
        return s

    __repr__ = __str__


class HistoryEma(_EmaColumns, History):
    """History of a run with --out_ema."""

    def __init__(self, epochs):
        History.__init__(self, epochs)
        self._init_ema(False)


class HistoryRegEma(_EmaColumns, HistoryReg):
    """HistoryReg of a run with --out_ema and a regulariser (--aa_weight): ema_loss is the pure data misfit of the average."""

    def __init__(self, epochs):
        HistoryReg.__init__(self, epochs)
        self._init_ema(False)


class HistoryHoldoutEma(_EmaColumns, HistoryHoldout):
    """History of a run with --holdout and --out_ema."""

    def __init__(self, epochs):
        HistoryHoldout.__init__(self, epochs)
        self._init_ema(True)


class HistoryRegHoldoutEma(_EmaColumns, HistoryRegHoldout):
    """HistoryReg of a run with --holdout, --out_ema and a regulariser."""

    def __init__(self, epochs):
        HistoryRegHoldout.__init__(self, epochs)
        self._init_ema(True)


class _ModelRegColumns:
    """model_reg column of a run with --model_reg: the unweighted penalty R(m) on the tensor the network wrote.  Such a history is of
    the HistoryReg family: loss is the total, df the misfit, reg the unweighted anti-aliasing term (0.0 without --aa_weight)."""
    _mmsg = ", MREG = %.2e"

    def _init_model_reg(self):
        self.model_reg = []

    def append_model_reg(self, value):
        self.model_reg.append(value)

    def log_message(self, idx):
        return super().log_message(idx) + self._mmsg % self.model_reg[idx]

    def __len__(self):
        n = super().__len__()
        assert len(self.model_reg) == n
        return n

    def __str__(self):
        return super().__str__() + "\nMREG : %s" % (self.model_reg,)

    __repr__ = __str__


class HistoryModelReg(_ModelRegColumns, HistoryReg):
    """HistoryReg of a run with --model_reg."""

    def __init__(self, epochs):
        HistoryReg.__init__(self, epochs)
        self._init_model_reg()


class HistoryModelRegHoldout(_ModelRegColumns, HistoryRegHoldout):
    """HistoryReg of a run with --model_reg and --holdout: val_loss stays the pure data misfit."""

    def __init__(self, epochs):
        HistoryRegHoldout.__init__(self, epochs)
        self._init_model_reg()


class HistoryModelRegEma(_ModelRegColumns, HistoryRegEma):
    """HistoryReg of a run with --model_reg and --out_ema."""

    def __init__(self, epochs):
        HistoryRegEma.__init__(self, epochs)
        self._init_model_reg()


class HistoryModelRegHoldoutEma(_ModelRegColumns, HistoryRegHoldoutEma):
    """HistoryReg of a run with --model_reg, --holdout and --out_ema."""

    def __init__(self, epochs):
        HistoryRegHoldoutEma.__init__(self, epochs)
        self._init_model_reg()


def history_class(reg=False, holdout=False, ema=False, model_reg=False):
    """The History class of a run: reg = a regulariser splits the loss, holdout = --holdout > 0, ema = --out_ema > 0, model_reg =
    --model_reg (always of the HistoryReg family, with the model_reg column)."""
    if model_reg:
        return {(False, False): HistoryModelReg, (True, False): HistoryModelRegHoldout,
                (False, True): HistoryModelRegEma, (True, True): HistoryModelRegHoldoutEma}[(bool(holdout), bool(ema))]
    return {(False, False, False): History, (True, False, False): HistoryReg,
            (False, True, False): HistoryHoldout, (True, True, False): HistoryRegHoldout,
            (False, False, True): HistoryEma, (True, False, True): HistoryRegEma,
            (False, True, True): HistoryHoldoutEma, (True, True, True): HistoryRegHoldoutEma}[(bool(reg), bool(holdout), bool(ema))]


def select_latest_min(it, misfit, best, best_iter):
    """The selection rule of the loop, one iteration of it: (improved, best, best_iter) after iteration `it` (0-based) showed `misfit`.
    Iteration 0 always selects; later ones when misfit <= best, so the later iterate wins a tie and a NaN never selects (after a NaN at
    iteration 0 nothing does).  The selection of the one device rule (dpi_loop_rule, csrc/loop_rule.h), on the same doubles."""
    if it == 0 or misfit <= best:
        return True, misfit, it
    return False, best, best_iter
