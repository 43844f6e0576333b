"""Per-patch deep-prior optimiser — drop-in for reference main.py (Interpolator life-cycle
load_data -> build_model -> build_input -> optimize -> save_result -> clean, and the `main()` CLI).  The life-cycle of one patch is
written once, in Interpolator.take_patch / prepare_patch / run_patch: every driver (run_cli here, parallel.py) goes through them.

Everything inside the iteration runs on the GPU through libdpi_hip.so: input perturbation (Philox),
network forward/backward (HIP convs / BN / up-sampling), fused masked loss + SNR/PCORR, fused Adam.
"""
import os
import warnings
from time import time

import numpy as np
import torch

from . import _lib, ops
from . import utils as u
from .architectures import build_net
from .data import extract_patches
from .forward_model import ForwardModel, to_numpy_out
from .loop import LoopRule
from .optim import DevicePlateau, FusedAdam, FusedLangevin, posterior_sample_count
from .parameter import check_model_reg, check_out_ema, net_args_are_same, parse_arguments

warnings.filterwarnings("ignore")


class Interpolator:
    def __init__(self, args, outpath, device=None, seed=0):
        self.args = args
        if device is None:
            if not torch.cuda.is_available():
                raise _lib.DpiError("no HIP device: deep_prior_interpolation_amd has no CPU path")
            device = torch.device("cuda", torch.cuda.current_device())
        self.device = torch.device(device)
        self.outpath = outpath
        self.loss_kind = "mse" if args.loss == "mse" else "mae"
        self.elapsed = None
        self.iiter = 0
        self.iter_to_be_saved = list(range(0, args.epochs, int(args.save_every))) if args.save_every is not None else [0]
        self.loss_min = None
        self.outchannel = args.imgchannel
        self.holdout = float(getattr(args, "holdout", 0.0))      # --holdout (ours); Namespaces of reference args.txt files lack the key
        if not 0.0 <= self.holdout <= 0.5:
            raise ValueError("--holdout must lie in [0, 0.5], got %r" % self.holdout)
        self.holdout_sel = self._holdout_dev = None              # per-trace selection: numpy (patch order without t) / device (C, S...)
        self.best_iter = self.val_min = None
        # --out_ema (ours): the output is selected from an exponential running average of the iterates (deep image prior's out_avg)
        self.out_ema = check_out_ema(args)
        self._ema_avg = self._ema_best = self._ema_one = None    # per patch: the average, its selected snapshot, a constant 1 flag
        self.ema_min = None
        # --avo_theta, --wavelet, --moveout, --trace_offsets (ours): the operators between the network and the loss (net_forward,
        # data_forward) and what is kept of them for the selected output
        self.forward_model = ForwardModel(args)
        # --model_reg (ours): None, or (kind, weight, dims) of the penalty on the tensor the network itself writes, and that tensor of
        # the current iteration with its graph (net_forward)
        self.model_reg = check_model_reg(args)
        self._net_out = None
        # --optimizer sgld | psgld (ours): Langevin sampling; Namespaces of reference args.txt files lack the keys
        self.optimizer_kind = getattr(args, "optimizer", "adam")
        if self.optimizer_kind not in ("adam", "sgld", "psgld"):
            raise ValueError("--optimizer must be adam, sgld or psgld, got %r" % (self.optimizer_kind,))
        burn = getattr(args, "posterior_burnin", None)
        self.posterior_burnin = int(args.epochs) // 2 if burn is None else int(burn)
        self.posterior_thin = int(getattr(args, "posterior_thin", None) or 1)
        self._post_mean = self._post_m2 = None                   # Welford buffers of the patch (dpi_moments_update)
        self._reset_posterior()
        self.history = self._new_history()
        self.image_name = None
        self.img = self.img_ = self.mask = self.mask_ = None
        self.out_best = None
        self._out_best_dev = None
        self.zfill = u.ten_digit(args.epochs)
        self.input_ = None
        self.add_data_ = None
        self.add_data_weight = None
        self.input_list = []
        self.net = None
        self.num_params = None
        self.optimizer = None
        self.noise_seed = int(seed)
        self._noise_step = torch.zeros(1, dtype=torch.int64, device=self.device)
        self._patches_seen = 0          # mixed into the Philox stream id of z: every patch gets its own z (main.py:62-64 draws a fresh one)
        self.patch_index = self.patch_std = None                 # of the patch taken last (take_patch)

    # ---- the life-cycle of one patch (reference main.py:274-295): the drivers call these, none spells the steps out ------------------
    def take_patch(self, index, patch):
        """Load patch `index` and decide whether there is anything to optimise.  A flat patch (std of the masked data 0: nothing
        recorded in it) is its own result, out_best = img * mask at no cost.  Returns whether the patch is live."""
        self.patch_index = int(index)
        self.patch_std = self.load_data(patch)
        live = not np.isclose(self.patch_std, 0.0, atol=1e-12)
        if not live:
            self.out_best, self.elapsed, self._out_best_dev = self.img * self.mask, 0.0, None
        return live

    def prepare_patch(self):
        """Everything between take_patch() and the loop of a live patch: the seeds, the network (kept from the patch before with
        --start_from_prev, read from --netdir when given), z and the regulariser.  Separate from take_patch() because the concurrent
        drivers prepare one patch while the captured iterations of others replay."""
        i, a = self.patch_index, self.args
        self.begin_patch(i)
        if self.net is None or not a.start_from_prev:
            self.build_model(netpath=a.netdir[i]) if len(a.netdir) != 0 else self.build_model()
        self.build_input()
        self.build_regularizer()

    def run_patch(self, index, patch, verbose=True):
        """One patch from its data to out_best, sequentially.  verbose prints what the reference's loop prints.  Returns take_patch()'s
        answer; save_result() and clean() are the driver's."""
        live = self.take_patch(index, patch)
        if verbose:
            print("\nThe data shape is %s, the std of coarse data is %.2e" % (str(patch["image"].shape), self.patch_std))
            if not live:
                print("skipping...")
        if live:
            self.prepare_patch()
            self.optimize(verbose=verbose)
        return live

    def output_for_reassembly(self):
        """The selected output as overlap-add takes it, without batch and channel axes: the device tensor of an optimised patch, the
        host fp32 tensor of out_best for a flat one."""
        if self._out_best_dev is None:
            return torch.from_numpy(np.ascontiguousarray(self.out_best[..., 0], dtype=np.float32))
        return self._out_best_dev.reshape(self._out_best_dev.shape[2:])

    def begin_patch(self, index, base_seed=0):
        """Seed everything patch `index` draws — initial weights (torch's CPU generator, consumed by init_weights), z and the
        per-iteration perturbation (Philox key) — from the patch index alone, so its result does not depend on which process,
        rank or concurrency slot optimises it.  Patch 0 with base_seed 0 reproduces `u.set_seed(0)` + a fresh Interpolator
        (bit-identical initial weights to the reference's first patch, tests/test_host.py)."""
        seed = int(base_seed) + int(index)
        torch.manual_seed(seed)
        self.noise_seed = seed
        self._patches_seen = 0
        self._noise_step.zero_()
        self.holdout_sel = self._holdout_dev = None              # drawn again from the new seed (build_holdout)
        self._zero_moments()

    def load_data(self, data):
        """(T,X,Y,C) numpy patch -> (1,C,T,X,Y) fp32 device tensors; returns std of the masked data (main.py:118-139)."""
        self.image_name = data["name"]
        self.img = data["image"]
        self.mask = data["mask"]
        if self.mask.shape != self.img.shape:
            raise ValueError("The loaded mask shape has to be", self.img.shape)
        perm = (self.img.ndim - 1,) + tuple(range(self.img.ndim - 1))
        to_dev = lambda a: torch.from_numpy(np.ascontiguousarray(np.transpose(a, perm))).unsqueeze(0).float().to(self.device)
        self.img_ = to_dev(self.img)
        self.mask_ = to_dev(self.mask)
        self.holdout_sel = self._holdout_dev = None
        live = self.forward_model.load_patch(data, self.img.shape, self.mask, self.device, self.image_name)
        if live is not None:                                     # --moveout: muted samples count nowhere; the host mask that is saved stays the file's
            self.mask_ = self.mask_ * torch.from_numpy(live.astype(np.float32)).to(self.device)[None, None]
        return torch.std(self.img_ * self.mask_).item()

    def known_mask(self):
        """The host mask of the samples that count: the file's, with --moveout without the muted samples."""
        live = self.forward_model.live
        return self.mask if live is None else self.mask * live[..., None].astype(self.mask.dtype)

    def moveout_model(self):
        """--moveout: the flattened section behind the selected output (ForwardModel.model)."""
        return self.forward_model.model("moveout")

    def wavelet_model(self):
        """--wavelet: the reflectivity or log-impedance section behind the selected output — behind --avo_theta: the angle sections
        before the wavelet (ForwardModel.model)."""
        return self.forward_model.model("wavelet")

    def avo_model(self):
        """--avo_theta: the three parameter sections (T, X, 3) behind the selected output (ForwardModel.model).  Every selected output —
        the best iterate, the running average, the posterior mean — is a linear combination of iterates G m_i, so the pseudo-inverse
        returns the same combination of the m_i: no second tracking path on the device.  None for a patch that was not optimised."""
        return self.forward_model.model("avo", self._optimised_output())

    def _optimised_output(self):
        return None if self._out_best_dev is None else self.out_best

    trace_offsets = property(lambda self: self.forward_model.trace_offsets, doc="per patch: (X, Y, 2) as used, i.e. zero at unknown traces")
    trace_interp = property(lambda self: self.forward_model.trace_interp, doc="--trace_interp: the kernel R samples with")

    def data_forward(self, out_):
        """What the loss compares with the recorded traces: the grid output itself, or with --trace_offsets the grid output sampled at the
        recorded trace positions.  Everything that keeps an output (out_best, --save_every, the --aa_weight term) keeps the grid tensor."""
        return self.forward_model.apply_data(out_)

    def build_holdout(self):
        """--holdout: draw the per-trace split of the loaded patch from the patch seed (begin_patch) and upload it once.  optimize() and
        graph_prepare() call it when the patch has none yet.  The selection lives in self.holdout_sel (numpy order (X[, Y], C)) and, as
        the (C, S...) float 0/1 tensor the loss pass reads, in self._holdout_dev."""
        if self.holdout <= 0.0:
            return
        self.holdout_sel = u.holdout_traces(self.known_mask(), self.holdout, self.noise_seed, name=self.image_name)
        dev = np.moveaxis(self.holdout_sel, -1, 0)                # (C, X[, Y]): the trace index (c, s) of the device layout (1, C, T, S...)
        self._holdout_dev = torch.from_numpy(np.ascontiguousarray(dev)).to(self.device)

    def _ensure_holdout(self):
        if self.holdout > 0.0 and self._holdout_dev is None:
            self.build_holdout()

    # ---- Langevin sampling (--optimizer sgld | psgld) ---------------------------------------------------------
    def is_sampler(self):
        return self.optimizer_kind != "adam"

    def _reset_posterior(self):
        self.posterior_std = self.output_selected = self.posterior_samples = self.posterior_snr = self.posterior_val_snr = None
        self._post_std_dev = None                                # posterior_std on the device, for the re-assembled std volume

    def _zero_moments(self):
        if self._post_mean is not None:
            self._post_mean.zero_()
            self._post_m2.zero_()

    def langevin_temperature(self):
        """--langevin_temperature, or 1/N with N the number of samples the loss averages over (the non-zeros of the patch's training
        mask): the reference's noise rule belongs to a SUMMED misfit, our loss is its mean, so temperature 1 over-heats the chain N-fold."""
        t = getattr(self.args, "langevin_temperature", None)
        if t is not None:
            return float(t)
        n = int(torch.count_nonzero(self.training_mask()).item())
        return 1.0 / n if n > 0 else 1.0

    def make_optimizer(self):
        """The optimiser of one patch: FusedAdam, or the Langevin sampler --optimizer names, keyed by the patch seed (its noise does not
        depend on rank or slot).  A new optimiser starts a new chain: the posterior moments of the patch start from zero."""
        a = self.args
        self._reset_posterior()
        self._zero_moments()
        if not self.is_sampler():
            return FusedAdam(self.net.parameters(), lr=a.lr)
        return FusedLangevin(self.net.parameters(), self.optimizer_kind, lr=a.lr, weight_decay=float(getattr(a, "weight_decay", 0.0)),
                             beta=float(getattr(a, "psgld_beta", 0.99)), Lambda=float(getattr(a, "psgld_lambda", 1e-8)),
                             noise_scale=float(getattr(a, "sgld_noise_scale", 0.1)), temperature=self.langevin_temperature(),
                             seed=self.noise_seed, noise="torch_cpu" if self.noise_source() == "torch_cpu" else "philox")

    def _moments_update(self, out_):
        """Fold the output of this iteration into the running mean / m2 when the iteration is a sampled one (decided on the device from the
        optimiser's step counter: call before optimizer.step())."""
        o = out_.detach()
        if o.dtype != torch.float32 or not o.is_contiguous():
            o = o.float().contiguous()
        if self._post_mean is None or self._post_mean.shape != o.shape:
            self._post_mean, self._post_m2 = torch.zeros_like(o), torch.zeros_like(o)
        opt = self.optimizer
        _lib.check(_lib.load().dpi_moments_update(_lib.ptr(o), _lib.ptr(self._post_mean), _lib.ptr(self._post_m2), o.numel(),
                                                  _lib.ptr(opt.step_lr), self.posterior_burnin, self.posterior_thin, _lib.ptr(opt.active),
                                                  _lib.stream()), "dpi_moments_update")

    # ---- running average of the output (--out_ema) -------------------------------------------------------------
    def _ema_pass(self, out_):
        """Fold the output of this iteration into the running average (reset on the device at iteration 0 of the optimiser's step counter:
        call before optimizer.step()) and return the device metrics of the stored average.  The buffers live as long as the patch (clean())."""
        o = out_.detach()
        if self._ema_avg is None or self._ema_avg.shape != o.shape:
            self._ema_avg = torch.empty(o.shape, dtype=torch.float32, device=o.device)
            self._ema_best = torch.empty_like(self._ema_avg)
            self._ema_one = torch.ones(1, dtype=torch.int32, device=o.device)
        opt = self.optimizer
        return ops.ema_loss(o, self._ema_avg, self.img_, self.mask_, self._holdout_dev, self.out_ema, opt.step_lr, opt.active, self.loss_kind)

    def loop_rule(self):
        """The loop-control layout of the loaded patch (loop.LoopRule): with or without a held-out part and a running average."""
        return LoopRule(self._holdout_dev is not None, self.out_ema > 0.0)

    def _read_back(self, metrics, ema):
        """The one read-back of an iteration: the raw iterate's doubles and, with --out_ema, the average's."""
        if ema is None:
            return metrics[:self.loop_rule().metrics_doubles].tolist(), None
        both = torch.cat([metrics, ema]).tolist()
        return both[:metrics.numel()], both[metrics.numel():]

    def ema_snr(self):
        """ema_snr of the selected average (iteration best_iter) of the last optimised patch; None without --out_ema."""
        if self.best_iter is None or not hasattr(self.history, "ema_snr"):
            return None
        return float(self.history.ema_snr[self.best_iter])

    def _finish_posterior(self):
        """After the loop of a sampler run (eager and graph): out_best becomes the posterior mean over the K sampled iterations, the
        loss- / holdout-selected iterate stays available as output_selected, posterior_std = sqrt(m2 / (K - 1)); one more loss pass on the
        mean gives its SNR (and, with --holdout, its held-out SNR)."""
        if not self.is_sampler():
            return
        self._reset_posterior()
        K = posterior_sample_count(self.iiter, self.posterior_burnin, self.posterior_thin)
        self.output_selected = self.out_best
        if K < 1:
            return
        self.posterior_samples = K
        mean = self._post_mean.clone()
        self._out_best_dev = mean
        self.out_best = self._to_numpy_out(mean)
        if K >= 2:
            self._post_std_dev = torch.sqrt(self._post_m2 / float(K - 1))
            self.posterior_std = self._to_numpy_out(self._post_std_dev)
        with torch.no_grad():
            if self._holdout_dev is None:
                _, metrics = ops.masked_loss(mean, self.img_, self.mask_, self.loss_kind)
                self.posterior_snr = float(metrics[1].item())
            else:
                _, metrics = ops.masked_loss_holdout(mean, self.img_, self.mask_, self._holdout_dev, self.loss_kind)
                m = metrics[:10].tolist()
                self.posterior_snr, self.posterior_val_snr = float(m[1]), float(m[9])

    def _print_posterior(self):
        if self.posterior_samples is None:
            print("posterior: no iteration was sampled (%d run, burn-in %d): the output is the selected iterate"
                  % (self.iiter, self.posterior_burnin))
            return
        msg = "posterior mean over %d samples: SNR %+.2f dB" % (self.posterior_samples, self.posterior_snr)
        if self.posterior_val_snr is not None:
            msg += ", held-out SNR %+.2f dB (selected iterate: %+.2f dB)" % (self.posterior_val_snr, self.holdout_snr())
        print(msg)

    def training_mask(self):
        """The mask of the samples the network may see: mask_ itself without --holdout, else m_tr = mask_ * (1 - h) (drawn here if the patch
        has no split yet).  Everything built from the data once per patch — the data-forgetting term of the input, the dips of the
        anti-aliasing add-on — takes it, so no held-out sample reaches the network other than through the misfit it is measured by."""
        self._ensure_holdout()
        if self._holdout_dev is None:
            return self.mask_
        h = self._holdout_dev.reshape((1, self.mask_.shape[1], 1) + tuple(self.mask_.shape[3:]))
        return self.mask_ * (1 - h)

    def net_forward(self, z):
        """The one place the network is called.  --net part takes the mask of known samples beside its input (the reference calls net(input_),
        main.py:159, which its PartialUNet.forward(x, mask) cannot serve): training_mask(), so held-out traces are holes for the net too, as one
        channel (amax over dim 1: the 2.5-D slab's channels; in 3-D the mask itself).  Constant per patch: built once, so a captured
        iteration replays it unchanged.  With --avo_theta the network writes three parameter sections and the AVO operator behind it maps
        them to the patch's angle sections; with --wavelet the wavelet operator comes last (d = W G m); with --moveout the network writes
        the flattened gather and the moveout operator comes last (d = L m); with both, --wavelet_domain orders them (d = W L r or
        d = L W r): what this returns is a data-domain tensor either way."""
        m = self._net_forward(z)
        if self.model_reg is not None:
            # --model_reg: what the network wrote is kept with its graph until model_regularization() takes it.  Without the flag nothing
            # is kept: a tensor that outlives the iteration would change what is alive while an iteration is captured
            self._net_out = m
        return self.forward_model.apply_model(m)

    def _net_forward(self, z):
        if getattr(self.args, "net", "multiunet") != "part":
            return self.net(z)
        src = getattr(self, "_net_mask_src", None)
        if src is None or src[0] is not self.mask_ or src[1] is not self._holdout_dev:
            self._net_mask = self.training_mask().amax(dim=1, keepdim=True).contiguous()          # (draws the hold-out split if the patch has none yet)
            self._net_mask_src = (self.mask_, self._holdout_dev)
        return self.net(z, self._net_mask)

    def release_packed_weights(self):
        """Hand the packed-weight scratch slots of this Interpolator's network back to the library (dpi_pack_forget, ABI 402): the bf16
        arithmetic modes keep one slot per (weight tensor, shape) and every patch builds a new network (reference main.py:286), so a
        343-patch job would otherwise hold 343 networks' worth of slots.  Called when the network is replaced; the patch that used it has
        been synchronised by then (optimize() / graph_finish() read the best output back)."""
        if self.net is None or getattr(self.args, "precision", "fp32") == "fp32":
            return 0
        L = _lib.load()
        n = 0
        for p in self.net.parameters():
            if p.ndim >= 4 and p.is_cuda:
                n += L.dpi_pack_forget(p.data_ptr())
        self._graph = None            # a captured iteration of the old network holds the slot addresses: it must not be replayed again
        return n

    def net_outchannel(self):
        """Channels the network itself writes: the patch's, or with --avo_theta the three parameter sections."""
        return self.forward_model.net_outchannel(self.outchannel)

    def build_model(self, netpath=None):
        self.release_packed_weights()
        if self.outchannel is None:
            self.outchannel = self.img_.shape[1]
        if len(self.args.netdir) != 0:
            saved = u.read_args(os.path.join("./results", *netpath.split("/")[:-1], "args.txt"))
            assert net_args_are_same(self.args, saved)
            self.net = build_net(saved, self.net_outchannel())
            self.net.load_state_dict(torch.load(os.path.join("./results", netpath), map_location="cpu"))
        else:
            self.net = build_net(self.args, self.net_outchannel())
            u.init_weights(self.net, self.args.inittype, self.args.initgain)
        self.net = self.net.float().to(self.device)
        self._storage_ok = None
        self.num_params = sum(int(np.prod(list(p.size()))) for p in self.net.parameters())

    def build_input(self):
        """z = noise_std * N(0,1) of shape (1, inputdepth, *patch), optionally FIR-filtered along t (wavelet / Butterworth)
        and prepared for the data-forgetting term (main.py:59-97)."""
        a = self.args
        philox_z = (None,)
        self._z_cpu = None
        if self.noise_source() == "torch_cpu":
            # parity mode: the reference's own draw (main.py:61-64: get_noise(...).type(dtype); input_ *= noise_std) from torch's CPU generator
            z = u.get_noise((1, a.inputdepth) + self.img.shape[:-1], a.noise_dist).float()
            z *= a.noise_std
            self._z_cpu = z
            z = z.to(self.device)
        elif a.noise_dist != "n":
            z = u.get_noise((1, a.inputdepth) + self.img.shape[:-1], a.noise_dist).to(self.device) * a.noise_std
        else:
            z = torch.empty((1, a.inputdepth) + self.img.shape[:-1], dtype=torch.float32, device=self.device)
            # stream id: high word marks "z" (the per-iteration perturbation uses the iteration counter as stream id), low word =
            # running patch count of this Interpolator, so consecutive patches do not share z
            zstream = (0xFFFFFFFF << 32) | (self._patches_seen & 0xFFFFFFFF)
            _lib.check(_lib.load().dpi_fill_normal(_lib.ptr(z), z.numel(), 0.0, float(a.noise_std), self.noise_seed, zstream, _lib.stream()),
                       "dpi_fill_normal")
            philox_z = (z, float(a.noise_std), int(self.noise_seed), int(zstream))      # dropped below if anything rewrites z
        self._patches_seen += 1
        self._z_philox = None
        if a.filter_noise_with_wavelet:                         # main.py:66-72
            z = u.ConvolveKernel_1d(kernel=np.load(os.path.join(a.imgdir, "wavelet.npy")), ndim=z.ndim - 2)(z)
        if a.lowpass_fs and a.lowpass_fc:                       # main.py:74-84: 4th-order Butterworth as an FIR along t
            z = u.LowPassButterworth(fc=a.lowpass_fc, ndim=z.ndim - 2, fs=a.lowpass_fs, ntaps=a.lowpass_ntaps, order=4,
                                     nfft=2 ** u.nextpow2(z.shape[2]))(z)
        if a.data_forgetting_factor != 0:                       # main.py:86-97
            data_ = self.img_ * self.training_mask()
            rep = int(np.ceil(z.shape[1] / data_.shape[1]))
            data_ = data_.repeat([1, rep] + [1] * (z.ndim - 2))[:, :a.inputdepth].contiguous()
            data_ = data_ * (torch.std(z) / torch.std(data_))
            self.add_data_ = data_
            self.add_data_weight = np.logspace(0, -4, a.data_forgetting_factor)
        self.input_ = z
        if self._z_cpu is not None and (a.filter_noise_with_wavelet or (a.lowpass_fs and a.lowpass_fc)):
            self._z_cpu = z.float().cpu()                       # the perturbation below is added to the FILTERED z (main.py:148-150)
        # z is still the plain Philox fill: the per-iteration perturbation COULD re-draw it instead of reading it (dpi_noise_add_regen_io,
        # DPI_Z_REGEN=1).  Off by default — measured slower: a second Philox4x32-10 + Box-Muller per four elements makes the pass ALU-bound
        # (0.45 ms at 256x128x128 x 64 channels against 0.36-0.41 ms for reading z: 134 M normal deviates per iteration either way)
        if a.noise_dist == "n" and z is philox_z[0] and os.environ.get("DPI_Z_REGEN") == "1":
            self._z_philox = philox_z

    # ------------------------------------------------------------------------------------------
    def perturbed_input(self):
        """input = z + reg_noise_std * N(0,1), fresh every iteration (main.py:148-150)."""
        if self.noise_source() == "torch_cpu":
            return self._perturbed_input_torch_cpu()
        if self.args.reg_noise_std <= 0:
            return self.input_
        # (bf16 storage: the perturbed input is the first activation the net reads — 64 channels at full resolution — and is written as
        #  bf16 straight away; z itself stays fp32)
        bf = ops.storage_bf16() and self.input_.ndim == 5
        out = torch.empty_like(self.input_, dtype=torch.bfloat16) if bf else torch.empty_like(self.input_)
        self._noise_step += 1
        zp = getattr(self, "_z_philox", None)
        if zp is not None and zp[0] is self.input_:
            _lib.check(_lib.load().dpi_noise_add_regen_io(out.numel(), zp[1], zp[2], zp[3], float(self.args.reg_noise_std), self.noise_seed,
                                                          _lib.ptr(self._noise_step), _lib.ptr(out), _lib.STORE_FWD_BF16 if bf else 0,
                                                          _lib.stream()), "dpi_noise_add_regen")
            return out
        _lib.check(_lib.load().dpi_noise_add_io(_lib.ptr(self.input_), out.numel(), float(self.args.reg_noise_std),
                                                self.noise_seed, _lib.ptr(self._noise_step), _lib.ptr(out),
                                                _lib.STORE_FWD_BF16 if bf else 0, _lib.stream()), "dpi_noise_add")
        return out

    def noise_source(self):
        return getattr(self.args, "noise_source", "philox")

    def _perturbed_input_torch_cpu(self):
        """--noise_source torch_cpu (parity mode): the reference's draws of one iteration in the reference's order, from torch's CPU generator —
        main.py:143-145: with --param_noise (ON by default in the CLI) one normal_() per 4-D / 5-D parameter, whose result the
        reference discards (it rebinds a local) but which moves the generator; main.py:148-150: input = z + reg_noise_std * z.clone().normal_()
        in fp32 on the host — then uploaded.  ~3 s of host time per iteration at 256x128x128 x 64 channels: a parity tool, not the fast path."""
        a = self.args
        if a.param_noise:
            for p in self.net.parameters():
                if p.ndim in (4, 5):
                    torch.empty(p.shape, dtype=torch.float32).normal_()
        inp = self._z_cpu.clone()
        if a.reg_noise_std > 0:
            inp += a.reg_noise_std * inp.clone().normal_()
        inp = inp.to(self.device)
        return inp.to(torch.bfloat16) if (ops.storage_bf16() and inp.ndim == 5) else inp

    _to_numpy_out = staticmethod(to_numpy_out)

    def precision_scope(self):
        """--precision of THIS Interpolator as an ops.mode_scope: the arithmetic mode of the convolutions and the storage type of the activations of
        everything built inside it, on this host thread only (round 6; rounds 2-5 flipped module globals of `ops` at the top of every iteration).
        Every iteration, eager or captured, runs inside one — so the mode never depends on which Interpolator ran before in the process, and two
        Interpolators of different --precision cannot disturb each other whichever way they are interleaved.  DPI_PRECISION / DPI_STORAGE in the
        environment are tools-only overrides of the fp32 default: an fp32 Interpolator leaves that half to the process default.
        bf16 STORAGE of the activations (BASELINE configs[4]) where every node of the net is a fused 3-D node that takes it (storage_bf16_ok)."""
        prec = getattr(self.args, "precision", "fp32")
        p = prec if (prec != "fp32" or "DPI_PRECISION" not in os.environ) else None
        st = ("bf16" if (prec == "bf16" and self.storage_bf16_ok()) else "fp32") if (prec != "fp32" or "DPI_STORAGE" not in os.environ) else None
        return ops.mode_scope(p, st)

    def wants_weight_grad_overlap(self):
        """Weight gradients on side streams next to the backward-data chain (and with them the once-per-step join and the ResPath branch
        stream, ops.py): patches of >= 2^20 voxels, eager.  fp32: 32.3 -> 29.6 ms at 256x128x128 (round 5).  bf16 storage: round 4 measured
        20.2 ms with the side stream against 18.9 without (per-node joins) and kept it off; with the round-5 schedule the order is
        reversed — 15.8-16.1 ms eager with it, 16.2 ms replayed from a graph without, 17.1-17.3 eager without; configs[4] (512x256x256
        patches) 8.4-8.8 against 8.2 it/s — so it is on for every storage type."""
        if getattr(self.args, "net", "multiunet") == "part":
            # every `down` convolution of the partial-convolution net is used twice (on the tensor and on the hole map): autograd ACCUMULATES its
            # weight gradient on the main stream, which a side stream that has not run yet cannot feed (ops.sched.deferred)
            return False
        big = int(np.prod(self.img.shape[:-1])) >= (1 << 20)
        if os.environ.get("DPI_FORCE_OVERLAP") in ("0", "1"):       # A/B knob
            return big and os.environ["DPI_FORCE_OVERLAP"] == "1"
        return big

    def storage_bf16_ok(self):
        """Whether this net runs with bf16 activations: the 3-D MultiRes-UNet whose blocks all execute as the fused nodes
        (LeakyReLU, no dropout) — Block3dFn / SkipJoinFn / ConvBnActFn allocate the tensors and every kernel under them takes the
        storage type.  Other nets keep fp32 storage under --precision bf16 (operand rounding only, as --precision bf16mm)."""
        ok = getattr(self, "_storage_ok", None)
        if ok is None:
            from .architectures import mulresunet as M
            a = self.args
            # (the data-forgetting term adds the fp32 data to the network input on the host side of the node boundary: fp32 storage)
            ok = bool(self.net is not None and a.datadim == "3d" and getattr(a, "net", "multiunet") in ("multiunet", "load") and M.FUSE_BLOCKS
                      and a.data_forgetting_factor == 0)
            if ok:
                blocks = [m for m in self.net.modules() if isinstance(m, (M.MultiResBlock, M.ResPath))]
                ok = bool(blocks) and all(m.nd == 3 and m._fusable() for m in blocks)
            if self.net is not None:
                self._storage_ok = ok
        return ok

    def optimization_loop(self, net_input=None):
        try:
            with self.precision_scope():
                return self._optimization_loop(net_input)
        except BaseException:
            ops.abort_iteration()          # streams joined, per-iteration state of ops forgotten: a later bare backward() joins per node again
            raise

    def _optimization_loop(self, net_input=None):
        ops.begin_iteration()
        input_ = self.perturbed_input() if net_input is None else net_input
        if self.iiter < self.args.data_forgetting_factor:       # main.py:153-155
            if input_ is self.input_ or net_input is not None:
                input_ = input_.clone()
            _lib.check(_lib.load().dpi_axpy(float(self.add_data_weight[self.iiter]), _lib.ptr(self.add_data_), input_.numel(),
                                            _lib.ptr(input_), _lib.stream()), "dpi_axpy")
            self.input_list.append(u.torch_to_np(input_, True))
        out_, ema, total_loss, metrics = self._forward_and_loss(input_)
        reg = self.regularization(out_, total_loss)          # None, or (weight tensor / float, reg loss) of a subclass / add-on
        mreg = self.model_regularization()                   # None, or (weight, R(m)) of --model_reg
        total = total_loss if reg is None else total_loss + reg[0] * reg[1]
        if mreg is not None:
            total = total + mreg[0] * mreg[1]
        total.backward()
        ops.finish_backward(self._grad_params())
        m, em = self._read_back(metrics, ema)                  # one read-back
        l, s, p = m[:3]
        if reg is None and mreg is None:
            self.history.append((l, s, p))
        else:
            main_l, l = l, float(total.item())                 # the loop follows the total
            self.history.append((l, main_l, 0.0 if reg is None else float(reg[1].item()), s, p))          # HistoryReg layout (main_pocs.py:198-202)
            if mreg is not None:
                self.history.append_model_reg(float(mreg[1].item()))
        self.history.lr.append(self.optimizer.param_groups[0]["lr"])
        # the rule of csrc/loop_rule.h on the doubles of the same read-back: the raw columns and minima as ever, the selection on q —
        # decided before a minimum is written, as q's minimum may be loss_min / val_min itself
        rule, it = self.loop_rule(), self.iiter
        if rule.holdout:
            self.history.append_val(m[8], m[9])
        if rule.ema:
            self.history.append_ema(em[0], em[1], *((em[8], em[9]) if rule.holdout else ()))
        improved, q_min, best_iter = u.select_latest_min(it, rule.q(self.history), getattr(self, rule.q_min_attr), self.best_iter)
        self.loss_min = u.select_latest_min(it, l, self.loss_min, None)[1]
        if rule.holdout:
            self.val_min = u.select_latest_min(it, m[8], self.val_min, None)[1]
        setattr(self, rule.q_min_attr, q_min)
        if rule.tracks_best_iter:
            self.best_iter = best_iter
        if improved and rule.ema:
            # the selected average is snapshot on the device (dpi_copy_if with a constant 1 flag: the next iteration overwrites the average)
            _lib.check(_lib.load().dpi_copy_if(_lib.ptr(self._ema_one), _lib.ptr(self._ema_avg), _lib.ptr(self._ema_best),
                                               self._ema_avg.numel(), _lib.stream()), "dpi_copy_if")
            self._out_best_dev = self._ema_best
        elif improved:
            self._out_best_dev = out_.detach()       # stays on the GPU; copied to the host once, after the loop
            self.forward_model.select()              # W and L are not invertible: the section behind the output is kept beside it
        if self.iiter in self.iter_to_be_saved and self.iiter != 0:
            np.save(os.path.join(self.outpath, self.image_name.split(".")[0]
                                 + "_output%s.npy" % str(self.iiter).zfill(self.zfill)), self._to_numpy_out(out_))
        self.iiter += 1
        return l

    def _forward_and_loss(self, input_):
        """The middle of an iteration, eager or captured: forward, posterior moments, running average, misfit.  Returns (out, ema metrics or
        None, loss, metrics)."""
        out_ = self.net_forward(input_)
        if self.is_sampler():
            self._moments_update(out_)
        ema = self._ema_pass(out_) if self.out_ema > 0.0 else None
        data_ = self.data_forward(out_)                          # --trace_offsets: the misfit is measured where the traces were recorded
        if self._holdout_dev is None:
            loss, metrics = ops.masked_loss(data_, self.img_, self.mask_, self.loss_kind)
        else:
            loss, metrics = ops.masked_loss_holdout(data_, self.img_, self.mask_, self._holdout_dev, self.loss_kind)
        return out_, ema, loss, metrics

    def _grad_params(self):
        """The parameters ops.finish_backward() checks the deferred gradients against (only when a side / branch stream ran: big patches)."""
        return self.optimizer._params if (ops.sched.deferred and self.optimizer is not None) else None

    def regularization(self, out_, main_loss):
        """Extra loss term hook.  The base path has none.  With --aa_weight > 0 the anti-aliasing add-on is active:
        aa_weight * loss_fn(Hale2D(dips)(out), 0) on 2-D / 2.5-D sections — the directional Laplacian of utils/slopes.py along dips
        estimated once per patch from the Gaussian-smoothed structure tensor of the decimated data (build_regularizer) — and
        aa_weight * (loss_fn(L_tx out, 0) + loss_fn(L_ty out, 0)) on 3-D patches, the same operator on the (t,x) and the (t,y)
        sections (Hale2DSections)."""
        if getattr(self, "_aa_op", None) is None:
            return None
        lap = self._aa_op(out_)
        reg_loss, _ = ops.masked_loss(lap, self._aa_zero, self._aa_one, self.loss_kind)
        if lap.ndim == out_.ndim + 1:
            # one loss pass over [L_tx out, L_ty out]: both halves have C*T*X*Y samples, so the sum of their two means is twice the mean
            reg_loss = 2.0 * reg_loss
        return float(self.args.aa_weight), reg_loss

    def model_regularization(self):
        """--model_reg: None, or (W, R) with R = ops.model_reg of the tensor the network wrote in this iteration (net_forward), before
        any operator of the forward model: plain L1 or total variation along the flag's axes, divided by the element count."""
        if self.model_reg is None:
            return None
        _, weight, dims = self.model_reg
        m, self._net_out = self._net_out, None
        return weight, ops.model_reg(m, dims)

    def build_regularizer(self):
        """Anti-aliasing add-on (BASELINE configs[3]; the reference ships the operators — utils/slopes.py, operators/ — but no
        caller): dips from the structure tensor of the available traces, smoothed with --aa_smooth.  On a 3-D patch
        (1,C,T,X,Y) the 2-D add-on runs on both families of vertical sections, (t,x) and (t,y), each with its own dip field;
        --aa_dips then holds 2*C*T*X*Y values, the (t,x) dips first."""
        self._aa_op = None
        a = self.args
        if not getattr(a, "aa_weight", 0.0):
            return
        if self.img_.ndim == 5:
            self._build_regularizer_sections()
            return
        if a.aa_dips is not None:
            dips = torch.from_numpy(np.load(a.aa_dips).astype(np.float32)).to(self.device).reshape(self.img_.shape)
        else:
            dips, _ = u.structure_tensor_dips(self.img_ * self.training_mask(), smooth=float(a.aa_smooth))
        self._aa_op = u.Hale2D(dips)
        self._aa_zero = torch.zeros_like(self.img_)
        self._aa_one = torch.ones_like(self.img_)
        self.history = self._new_history()

    def _build_regularizer_sections(self):
        a = self.args
        if a.aa_dips is not None:
            d = np.load(a.aa_dips)
            if d.size != 2 * self.img_.numel():
                raise ValueError("--aa_dips %s holds %d values; a 3-D patch of shape %s needs 2*C*T*X*Y = %d (the (t,x) dips, then the "
                                 "(t,y) dips)" % (a.aa_dips, d.size, tuple(self.img_.shape[1:]), 2 * self.img_.numel()))
            dips = torch.from_numpy(d.astype(np.float32)).to(self.device).reshape((2,) + tuple(self.img_.shape))
            phi_tx, phi_ty = dips[0], dips[1]
        else:
            phi_tx, phi_ty = u.structure_tensor_dips_sections(self.img_ * self.training_mask(), smooth=float(a.aa_smooth))
        self._aa_op = u.Hale2DSections(phi_tx, phi_ty)
        self._aa_zero = torch.zeros((2,) + tuple(self.img_.shape), dtype=torch.float32, device=self.device)
        self._aa_one = torch.ones((2,) + tuple(self.img_.shape), dtype=torch.float32, device=self.device)
        self.history = self._new_history()

    def optimize(self, net_inputs=None, verbose=True, mode="auto", check_every=64):
        """Adam loop with optional ReduceLROnPlateau and EarlyStopping (main.py:195-220).

        mode "eager": the reference's control flow, one host read-back of {loss, snr, pcorr} per iteration.
        mode "graph": iteration 0 runs eagerly, iteration 1 is captured into a hipGraph and replayed; history, best-output
        tracking, plateau LR and early stopping live on the device (dpi_loop_control / dpi_copy_if), the host only polls
        the `active` flag every `check_every` replays.  Same arithmetic, same stopping iteration.
        "auto" picks "graph" unless per-iteration host work was requested (net_inputs, --save_every) or the patch has >= 2^20 voxels
        (eager with the weight-gradient and branch streams).  A patch of that size that does not take those streams (--net part) is
        eager only when the run is short: from 1000 iterations on it is captured.
        --holdout: out_best and early stopping follow the misfit on the held-out traces, ReduceLROnPlateau the training loss.
        --out_ema: out_best is the running average of the outputs at the iteration where ITS misfit (training, or held-out with --holdout)
        was lowest, and early stopping follows that misfit; the gradient and ReduceLROnPlateau see the raw iterate as ever."""
        a = self.args
        self._ensure_holdout()
        big = self.wants_weight_grad_overlap()
        if mode == "auto":
            # small patches are launch-bound without a graph; big ones run eager with the weight-gradient / branch streams (`big`)
            reasons = self._eager_reasons(net_inputs)
            # the one difference from graph_capable(): a big patch WITHOUT those streams (DPI_FORCE_OVERLAP=0, --net part) is captured when the
            # run is long: the capture allocates a memory pool of its own — as much again as one iteration's activations, 20 GB at
            # 512x256x256 — and costs 0.1-3 s of hipMalloc / instantiation depending on the box (measured on configs[4], 30 iterations per
            # patch: 160-210 ms per iteration with the capture, 113 ms eager)
            mode = "graph" if (not reasons or (reasons == ["size"] and not big and a.epochs >= 1000)) else "eager"
        self.optimizer = self.make_optimizer()
        ops.set_weight_grad_overlap(big, in_graph=(mode == "graph" and big))
        start = time()
        if mode == "graph":
            self._check_capturable()
            self._optimize_graph(verbose, check_every)
        else:
            sched = DevicePlateau(self.optimizer, a.lr_factor, a.lr_thresh, a.lr_patience) if a.reduce_lr else None
            stopper = u.EarlyStopping(patience=a.earlystop_patience, min_delta=a.earlystop_min_delta, percentage=True)
            for j in range(a.epochs):
                self.optimizer.zero_grad()
                loss = self.optimization_loop(None if net_inputs is None else net_inputs[j])
                self.optimizer.step()
                if sched is not None:
                    sched.step(loss)
                if verbose:
                    print(self.history.log_message(self.iiter - 1), "\r", end="")
                if stopper.step(self.loop_rule().q(self.history)):          # the selection misfit the loop itself followed
                    break
            torch.cuda.synchronize(self.device)
            self.out_best = self._to_numpy_out(self._out_best_dev)
            self._finish_posterior()
        self.elapsed = time() - start
        if verbose:
            print("\n" + u.sec2time(self.elapsed))
            if self._holdout_dev is not None:
                print("held-out SNR %+.2f dB at iteration %d (the selected output)" % (self.holdout_snr(), self.best_iter + 1))
            if self.out_ema > 0.0:
                print("running average (beta %g) selected at iteration %d: SNR %+.2f dB" % (self.out_ema, self.best_iter + 1, self.ema_snr()))
            if self.is_sampler():
                self._print_posterior()

    def holdout_snr(self):
        """val_snr of the selected output (iteration best_iter) of the last optimised patch — with --out_ema the selected average's,
        ema_val_snr; None without --holdout."""
        if self.best_iter is None or not hasattr(self.history, "val_snr"):
            return None
        col = self.history.ema_val_snr if hasattr(self.history, "ema_val_snr") else self.history.val_snr
        return float(col[self.best_iter])

    # ---- hipGraph path -------------------------------------------------------------------------------------
    def graph_prepare(self, quiet_device=True):
        """Allocate the device-resident loop state, run iteration 0 eagerly and capture iteration 1.
        Returns the captured graph; `graph_finish()` reads history / best output back.
        quiet_device=False (optimize_concurrently, round 5): other streams keep replaying the graphs of other patches meanwhile — only THIS
        stream is synchronised before the capture and the capture is opened with CUDAGraph.capture_begin() directly (torch.cuda.graph()
        would synchronise the whole device, collect garbage and empty the allocator's cache first)."""
        a = self.args
        self._check_capturable()
        L = _lib.load()
        dev = self.device
        if self.optimizer is None:
            self.optimizer = self.make_optimizer()
            # prepared directly (optimize_concurrently, bench.py): the weight-gradient side streams follow THIS patch's size, not
            # whatever an earlier optimize() in the process left behind; optimize() / bench.py set it before they
            # call graph_prepare with an optimiser of their own
            big = self.wants_weight_grad_overlap()
            ops.set_weight_grad_overlap(big, in_graph=big)
        opt = self.optimizer
        self._ensure_holdout()
        rule = self._g_rule = self.loop_rule()
        self._g_state, self._g_hist, self._g_improved = rule.new_state(a.epochs, dev)
        self._g_best = None
        self.forward_model.new_buffer()

        def one_iteration():
            with self.precision_scope():
                _one_iteration()

        def _one_iteration():
            ops.begin_iteration()
            opt.zero_grad()
            out_, ema, loss, metrics = self._forward_and_loss(self.perturbed_input())
            loss.backward()
            ops.finish_backward(self._grad_params())
            opt.step()                                   # skipped on the device once `active` is 0
            if self._g_best is None:
                self._g_best = torch.empty_like(out_)
            rules = (int(bool(a.reduce_lr)), float(a.lr_factor), float(a.lr_thresh), int(a.lr_patience), 0.0, 1e-8,
                     int(a.earlystop_patience), float(a.earlystop_min_delta))
            rule.launch(metrics, ema, self._g_state, self._g_hist, a.epochs, opt.step_lr, opt.active, self._g_improved, rules)
            best_src = self._ema_avg if rule.ema else out_       # --out_ema: the selected AVERAGE is kept
            _lib.check(L.dpi_copy_if(_lib.ptr(self._g_improved), _lib.ptr(best_src), _lib.ptr(self._g_best), out_.numel(),
                                     _lib.stream()), "dpi_copy_if")
            if not rule.ema:
                self.forward_model.select_if(self._g_improved)       # the section behind the selected iterate, on the same flag

        one_iteration()                                  # iteration 0, eager (also warms every lazy cache)
        if quiet_device:
            torch.cuda.synchronize(dev)
        else:
            torch.cuda.current_stream(dev).synchronize()
        opt.prepare_capture()
        graph = torch.cuda.CUDAGraph()
        if quiet_device:
            with torch.cuda.graph(graph):
                one_iteration()                          # recorded, not executed
        else:
            graph.capture_begin(capture_error_mode="thread_local")     # on the current (non-default) stream, a private memory pool of its own;
                                                                       # thread_local: another host thread may keep launching its patches' replays
            try:
                one_iteration()
            finally:
                graph.capture_end()
        self._graph = graph
        return graph

    def graph_finish(self, quiet_device=True):
        """quiet_device=False: wait for the CURRENT stream only (other patches keep running on theirs)."""
        if quiet_device:
            torch.cuda.synchronize(self.device)
        else:
            torch.cuda.current_stream(self.device).synchronize()
        n, h, st = self._g_rule.rows(self._g_state, self._g_hist)
        self.history = self._new_history()
        self._g_rule.fill(self, self.history, h, st)
        self.iiter = n
        self._out_best_dev = self._g_best
        self.forward_model.take_buffer()
        self.out_best = self._to_numpy_out(self._g_best)
        self._finish_posterior()

    def _optimize_graph(self, verbose, check_every):
        graph = self.graph_prepare()
        for j in range(1, self.args.epochs):
            graph.replay()
            if j % check_every == 0:
                if int(self.optimizer.active.item()) == 0:     # early stop / NaN decided on the device
                    break
                if verbose:
                    n, h, _ = self._g_rule.rows(self._g_state, self._g_hist)
                    print(self._g_rule.progress(n, h[-1]), "\r", end="")
        self.graph_finish()

    def _check_capturable(self):
        """The runs no captured iteration can serve, refused by optimize(mode='graph') and graph_prepare() alike (_eager_reasons() is
        why mode='auto' never gets here with them)."""
        if self.noise_source() != "philox":
            raise ValueError("--noise_source torch_cpu draws on the host every iteration: it cannot be captured into a graph (mode='eager')")
        if self.model_reg is not None:
            raise ValueError("--model_reg %s cannot be captured into a graph (mode='eager'): the captured iteration evaluates no "
                             "regulariser, and the term must not be dropped silently" % self.model_reg[0])

    def has_regularizer(self):
        return getattr(self, "_aa_op", None) is not None or self.model_reg is not None

    def _eager_reasons(self, net_inputs=None):
        """Why the loaded patch is optimised eagerly instead of from a captured iteration: each reason once, for optimize(mode='auto')
        and graph_capable()."""
        a = self.args
        return [name for name, holds in (
            ("per-iteration host work", net_inputs is not None or a.save_every is not None or a.epochs < 3),
            ("regulariser", self.has_regularizer()),
            ("data forgetting", a.data_forgetting_factor != 0),
            ("noise source", self.noise_source() != "philox"),
            ("size", int(np.prod(self.img.shape[:-1])) >= (1 << 20))) if holds]       # >= 2^20 voxels: GPU-bound either way

    def graph_capable(self):
        """True when the loaded patch can share the GPU as one of several captured iterations (parallel.py asks)."""
        return not self._eager_reasons()

    # ------------------------------------------------------------------------------------------
    def save_result(self):
        run = {
            "device": u.get_gpu_name(), "elapsed": u.sec2time(self.elapsed), "outpath": self.outpath,
            "history": self.history, "mask": self.mask, "image": self.img, "output": self.out_best,
            "noise": self.input_list,
        }
        if self.holdout > 0.0:
            # the selection with a unit t axis, in the patch's numpy order (broadcasts against mask: m_ho = mask * holdout); None for a
            # flat patch that was not optimised
            run["holdout"] = None if self.holdout_sel is None else self.holdout_sel[None]
            run["best_iter"] = self.best_iter
        if self.out_ema > 0.0:
            run["out_ema"] = self.out_ema                        # `output` is the selected running average, best_iter its iteration
            run["best_iter"] = self.best_iter
        run.update(self.forward_model.run_fields(self._optimised_output()))
        if self.model_reg is not None:
            run.update(model_reg=self.model_reg[0], model_reg_weight=self.model_reg[1])
        if self.is_sampler():
            run.update(posterior_std=self.posterior_std, posterior_samples=self.posterior_samples, output_selected=self.output_selected,
                       posterior_snr=self.posterior_snr, posterior_val_snr=self.posterior_val_snr)
        np.save(os.path.join(self.outpath, self.image_name + "_run.npy"), run)
        if self.args.savemodel:
            torch.save(self.net.state_dict(), os.path.join(self.outpath, self.image_name + "_model.pth"))

    def clean(self):
        self.iiter = 0
        self.loss_min = None
        self.best_iter = self.val_min = self.ema_min = None
        self._out_best_dev = None
        self.forward_model.clean()
        self._net_out = None
        self._ema_avg = self._ema_best = None                    # the running average belongs to the patch
        self._reset_posterior()
        self._zero_moments()
        self.history = self._new_history()

    def _new_history(self):
        return u.history_class(self.has_regularizer(), self.holdout > 0.0, self.out_ema > 0.0,
                               model_reg=self.model_reg is not None)(self.args.epochs)


def optimize_concurrently(Ts, check_every=64, prepare=None, timings=None):
    """Optimise several Interpolators at the same time on ONE GPU: each iteration is a captured hipGraph, the graphs are replayed
    round-robin on one stream per patch.  A 64^3 patch keeps only a fraction of an MI355X busy (its coarse levels are a few workgroups
    wide), six of them side by side give ~1.8x the patch-iterations per second of one (tools/c3_probe.py).  Same arithmetic per patch as
    optimize().

    prepare(T) (round 5): the host-side set-up of a patch — weights, z (Interpolator.build_model / build_input; ~30 ms of host time) — is
    done HERE, patch by patch, and between two patches the graphs that are already captured get a burst of replays: the device works on
    the first patches while the host prepares the next ones, instead of idling through the set-up of the whole group (6 x ~55 ms per
    group of 100-iteration patches).  Without `prepare` the Interpolators come prepared (data, model and input built).
    timings (dict): `prepare_s` = host seconds spent in prepare + capture (they overlap device work, so they are not additive to the loop)."""
    if not Ts:
        return
    start = time()
    epochs = Ts[0].args.epochs
    streams = [torch.cuda.Stream(device=T.device) for T in Ts]
    graphs, left = [], []
    t_prep = 0.0

    def burst(n):
        """n rounds of replays over the patches captured so far (asynchronous: ~0.2 ms of host time per replay)."""
        for _ in range(n):
            for k, g in enumerate(graphs):
                if left[k] > 0:
                    with torch.cuda.stream(streams[k]):
                        g.replay()
                    left[k] -= 1
    for T, st in zip(Ts, streams):
        t0 = time()
        if prepare is not None:
            prepare(T)
        st.wait_stream(torch.cuda.current_stream(T.device))      # z / data / weights were produced on the caller's stream
        with torch.cuda.stream(st):
            T.optimizer = None
            graphs.append(T.graph_prepare(quiet_device=prepare is None))
        left.append(epochs - 1)
        t_prep += time() - t0
        if prepare is not None and len(graphs) < len(Ts):
            burst(min(check_every, 24))       # what the device chews on while the next patch is being prepared (bounded: the early-stop poll below)
    alive = [True] * len(Ts)
    j = 0
    while any(a and n > 0 for a, n in zip(alive, left)):
        for k, (g, st) in enumerate(zip(graphs, streams)):
            if alive[k] and left[k] > 0:
                with torch.cuda.stream(st):
                    g.replay()
                left[k] -= 1
        j += 1
        if j % check_every == 0:
            # poll every patch on ITS stream: the read-back waits for the replays queued so far, so the host never runs more than
            # check_every replays ahead of the device and stops replaying a patch whose loop ended on the device (early stop / NaN)
            for k, (T, st) in enumerate(zip(Ts, streams)):
                if alive[k]:
                    with torch.cuda.stream(st):
                        alive[k] = int(T.optimizer.active.item()) != 0
    for T, st in zip(Ts, streams):
        with torch.cuda.stream(st):
            T.graph_finish()
        torch.cuda.current_stream(T.device).wait_stream(st)      # consumers (overlap-add, save_result) run on the caller's stream
        T.elapsed = time() - start
    if timings is not None:
        timings["prepare_s"] = timings.get("prepare_s", 0.0) + t_prep


def run_cli(interpolator_cls, argv=None):
    """The sequential command-line driver of main.py and main_pocs.py: every patch of the data set, one after the other, through
    `interpolator_cls`."""
    args = parse_arguments(argv)
    u.set_gpu(args.gpu if args.gpu is not None else -1)
    u.set_seed(0)
    outpath = os.path.join("./results/", args.outdir if args.outdir is not None else u.random_code())
    os.makedirs(outpath, exist_ok=True)
    print("Saving to %s" % outpath)
    u.write_args(os.path.join(outpath, "args.txt"), args)
    patches = extract_patches(args)
    print("Processing %d patches" % len(patches))
    T = interpolator_cls(args, outpath)
    for i, patch in enumerate(patches):
        T.run_patch(i, patch)
        T.save_result()
        T.clean()
    print("Interpolation done! Saved to %s" % outpath)


def main(argv=None):
    run_cli(Interpolator, argv)


if __name__ == "__main__":
    main()
