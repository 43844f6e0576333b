"""Deep prior with the POCS regulariser — drop-in for reference main_pocs.py (Interpolator + main()).

total = main_loss(out * mask, data) + eps * MSE(out, POCS(out).detach())          (main_pocs.py:178-193)
POCS(out) = alpha * data + (1 - alpha * mask) * IFFT(threshold(FFT(out)))           (utils/pocs.py:80-84)

The reference script cannot run on torch >= 1.8 (torch.rfft / irfft removed, main_pocs.py:156-157) and reads an undefined
`args.reg_weight` (main_pocs.py:192) — SURVEY §2 row 5g.  Here the transform is torch.fft (rocFFT), thresholding and the
projection are HIP kernels (dpi_scaled_max / dpi_threshold / dpi_pocs_project), and the weight is
  * --pocs_weight W given: eps = W  (what `args.reg_weight` evidently meant);
  * not given: eps = main_loss / reg_loss, DETACHED — the reference writes `eps.detach()` without using the result
    (main_pocs.py:189-190), which would make eps * reg_loss == main_loss identically and switch the regulariser off; the
    detached ratio balances the two terms as the surrounding code intends.
"""
import os

import numpy as np
import torch

from . import ops
from . import utils as u
from .main import Interpolator as _Base, run_cli


class Interpolator(_Base):
    def __init__(self, args, outpath, device=None, seed=0):
        if getattr(args, "holdout", 0.0) > 0.0:
            raise ValueError("main_pocs does not support --holdout (got %g): the POCS projection re-inserts every known trace into its "
                             "target, held-out ones included; run main.py for self-validation" % args.holdout)
        if getattr(args, "optimizer", "adam") != "adam":
            raise ValueError("main_pocs does not support --optimizer %s: the POCS target follows the current output, there is no fixed "
                             "posterior to sample; run main.py for Langevin sampling" % args.optimizer)
        if (getattr(args, "out_ema", 0.0) or 0.0) != 0.0:
            raise ValueError("main_pocs does not support --out_ema (got %g): the POCS target follows the current output, an average of "
                             "outputs has no target of its own to be measured against; run main.py" % args.out_ema)
        if getattr(args, "avo_theta", None) is not None:
            raise ValueError("main_pocs does not support --avo_theta: the POCS projection thresholds the spectrum of a section, which knows "
                             "nothing of the three-parameter subspace the AVO operator confines the output to; run main.py")
        if getattr(args, "trace_offsets", None) is not None:
            raise ValueError("main_pocs does not support --trace_offsets: the POCS projection re-inserts the traces at their grid nodes, "
                             "which is the assumption the flag removes; run main.py")
        if getattr(args, "wavelet_domain", None) is not None:
            raise ValueError("main_pocs does not support --wavelet_domain: it orders --wavelet and --moveout, neither of which the POCS "
                             "projection can sit behind; run main.py")
        if getattr(args, "wavelet", None) is not None:
            raise ValueError("main_pocs does not support --wavelet: the POCS projection re-inserts the known traces into the output, which "
                             "takes it out of the range of the wavelet operator; run main.py")
        if getattr(args, "moveout", None) is not None:
            raise ValueError("main_pocs does not support --moveout: the POCS projection thresholds and re-inserts traces in the data "
                             "domain, the network writes the flattened one; run main.py")
        if getattr(args, "moveout_offset", None) is not None:
            raise ValueError("main_pocs does not support --moveout_offset: the scanned table feeds the operator of --moveout, which the "
                             "POCS projection cannot sit behind; run main.py")
        if getattr(args, "model_reg", None) is not None:
            raise ValueError("main_pocs does not support --model_reg: its regularisation hook and its history hold the POCS term; run "
                             "main.py")
        super().__init__(args, outpath, device=device, seed=seed)
        self.history = u.HistoryReg(args.epochs)
        self.pocs = None
        self.reg_data = None
        self._ones = None

    def has_regularizer(self):
        return True

    def build_regularizer(self):
        coarse = self.img_ * self.mask_
        self.pocs = u.POCS(data=coarse, mask=self.mask_, weight=self.args.pocs_alpha, thresh_perc=self.args.pocs_thresh)
        self._ones = torch.ones_like(self.img_)
        self.history = u.HistoryReg(self.args.epochs)

    def regularization(self, out_, main_loss):
        reg_data = self.pocs(out_.detach())
        self._reg_data_dev = reg_data
        reg_loss, _ = ops.masked_loss(out_, reg_data, self._ones, "mse")          # loss_reg_fn = MSELoss (main_pocs.py:28)
        if self.args.pocs_weight is None:
            eps = (main_loss / reg_loss).detach()
        else:
            eps = float(self.args.pocs_weight)
        return eps, reg_loss

    def optimize(self, net_inputs=None, verbose=True, mode="eager", check_every=64):
        super().optimize(net_inputs=net_inputs, verbose=verbose, mode="eager")
        rd = self._reg_data_dev
        self.reg_data = u.torch_to_np(rd.squeeze(0), False)

    def save_result(self):
        np.save(os.path.join(self.outpath, self.image_name + "_run.npy"), {
            "device": u.get_gpu_name(), "elapsed": u.sec2time(self.elapsed), "outpath": self.outpath,
            "history": self.history, "mask": self.mask, "image": self.img, "output": self.out_best,
            "noise": self.input_list, "pocs": self.reg_data,
        })
        if self.args.savemodel:
            torch.save(self.net.state_dict(), os.path.join(self.outpath, self.image_name + "_model.pth"))


def main(argv=None):
    run_cli(Interpolator, argv)


if __name__ == "__main__":
    main()
