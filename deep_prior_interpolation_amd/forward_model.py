"""What lies between the network and the loss (ours): the linear operators of --avo_theta (G), --wavelet (W), --moveout (L) and
--trace_offsets (R) as stages of one ForwardModel.  The "model" stages follow the network in the order avo, wavelet, moveout
(d = W G m, d = L m), so everything that keeps an output sees a data-domain tensor; the "data" stage R follows only on the way to the
misfit, so everything that keeps an output keeps the grid tensor.  W and L cannot be inverted: their stage is `tracked`, i.e. its input
is kept beside the output when an iterate is selected (`pre` / `best`).  G is not tracked: every selected output, an average of iterates
included, is a linear combination of iterates G m_i, and the pseudo-inverse returns the same combination of the m_i.
The order rule: W and L together need --wavelet_domain, which orders them: "model" keeps the order above (d = L W r, the wavelet
stretches with the events), "data" is avo, moveout, wavelet (d = W L r, the wavelet acts in recorded time).  There is still one
pre / best pair: it holds the input of the FIRST of the two, the tensor the network writes, and the section in front of the second
one is the first operator applied to it when the result is asked for."""
import os
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib
from . import utils as u
from .parameter import check_avo, check_moveout, check_trace_offsets_flag, check_wavelet, check_wavelet_domain

ORDER = ("avo", "wavelet", "moveout", "sampling")              # the default, and --wavelet_domain model
ORDER_DATA = ("avo", "moveout", "wavelet", "sampling")         # --wavelet_domain data


@dataclass
class Stage:
    name: str                       # one of ORDER
    op: object = None               # forward / adjoint / upload(device); the per-patch ones are set by load_patch
    domain: str = "model"           # "model": applied by apply_model; "data": by apply_data
    tracked: bool = False           # the input of the selected iterate is kept


def to_numpy_out(out_):
    """(1,1,T,X,Y) -> (T,X,Y) ; (1,C,H,W) -> (H,W,C)  (main.py:175-176)."""
    return u.torch_to_np(out_, True) if out_.ndim > 4 else u.torch_to_np(out_, False)[0].transpose((1, 2, 0))


class ForwardModel:
    """Built once per Interpolator from `args` (the four check_* of parameter.py decide which stages there are; the wavelet is read from
    --imgdir here), loaded once per patch (load_patch), applied every iteration (apply_model, apply_data).  `stages` adds or replaces
    stages with ready-made ones.  A fifth operator is a check_* result in `flags`, a Stage in __init__, its per-patch part in
    load_patch and its keys in run_fields; if it is tracked and may meet W or L, it also needs its place in both orders (ORDER,
    ORDER_DATA): two tracked stages are accepted only when the args carry a --wavelet_domain, the first of them owns pre / best, and
    model() of the second is the first one's operator applied to `best`.  W and L themselves stay two stages, so each keeps its name,
    its keys and its model; with both, load_patch joins their operators in one operators.PrestackModelling (`pair`), which runs the
    iteration in their place (one autograd node: the tensor between them is not kept for the backward pass) and whose `live` is the map."""

    def __init__(self, args, stages=()):
        self.args = args
        # None when the flag is off, else: (theta, vsvp, linearization) / (file name, kind) / (file name, interp) / file name
        self.flags = {"avo": check_avo(args), "wavelet": check_wavelet(args), "moveout": check_moveout(args),
                      "sampling": check_trace_offsets_flag(args)}
        self.domain = check_wavelet_domain(args)                 # --wavelet_domain: "data" | "model", None = undecided
        self.trace_interp = getattr(args, "trace_interp", None) or "linear"     # --trace_interp: the kernel R samples with (linear = bilinear)
        # --out_ema and the samplers select an average of iterates, whose model is not tracked
        self.averaged = (getattr(args, "out_ema", 0.0) or 0.0) > 0.0 or getattr(args, "optimizer", "adam") != "adam"
        by_name = {n: Stage(n, None, "data" if n == "sampling" else "model", n in ("wavelet", "moveout"))
                   for n in ORDER if self.flags[n] is not None}
        if "wavelet" in by_name:
            by_name["wavelet"].op = self._read_wavelet()
        by_name.update((s.name, s) for s in stages)
        order = ORDER_DATA if self.domain == "data" else ORDER
        self.stages = sorted(by_name.values(), key=lambda s: order.index(s.name))
        tracked = [s.name for s in self.stages if s.tracked]
        if len(tracked) > 1 and self.domain is None:
            raise ValueError("the stages %s both keep their input for the selected iterate: there is one pre / best pair, and which of "
                             "the two operators comes first is not decided yet" % " and ".join(tracked))
        self._tracked = [s for s in self.stages if s.tracked]
        self._model = [s for s in self.stages if s.domain == "model"]
        self._data = [s for s in self.stages if s.domain == "data"]
        self.pre = self.best = self._buffer = None               # the first tracked stage's input: this iteration / selected / captured copy
        self.trace_offsets = self.live = None                    # per patch: (X, Y, 2) as used, i.e. zero at unknown traces / the live map
        self.pair = None                                         # per patch, W and L together: their PrestackModelling
        self.velocity = None                                     # per patch, --moveout_offset: (T,) or (T, G_window), the picked law(s)
        self.pick = None                                         # per patch, --moveout_smooth: the staircase(s) behind the smoothed law(s)

    def stage(self, name):
        """The stage `name`, or None when there is none (its flag is off)."""
        return next((s for s in self.stages if s.name == name), None)

    def _read_wavelet(self):
        from .operators import ConvolutionalModelling
        name, kind = self.flags["wavelet"]
        path = os.path.join(self.args.imgdir, name)
        try:
            return ConvolutionalModelling(np.load(path, allow_pickle=False), kind=kind)
        except (OSError, ValueError) as e:
            raise ValueError("--wavelet %s: %s" % (path, e)) from e

    # ---- per patch ---------------------------------------------------------------------------------------------
    def load_patch(self, data, shape, mask, device, name):
        """The per-patch stages of the patch dict `data` with image shape `shape` (numpy order, channels last) and host mask `mask`;
        every stage goes to `device` here, before iteration 0, so a captured iteration replays the stages unchanged.  Returns the
        boolean map (T, X[, Y]) of the samples L leaves live, or None: the caller multiplies it into the DEVICE mask, so a muted sample
        counts in no loss, SNR or hold-out draw (and a patch without a live known sample has std 0: skipped).  Under --wavelet_domain
        data the map is L's eroded along t by the reach of the wavelet (operators.erode_live): W reads the zeros L writes at muted
        samples, and a data sample next to a mute would be compared with a truncated convolution."""
        self._load_sampling(data.get("offsets"), shape, mask, name)
        self._load_moveout(data.get("moveout"), shape, name)
        self.velocity = data.get("moveout_velocity")             # --moveout_offset: the law(s) behind the patch's table
        self.pick = data.get("moveout_pick")                     # --moveout_smooth: the picked staircase(s) behind the law(s)
        avo = self.stage("avo")
        if self.flags["avo"] is not None and (avo.op is None or avo.op.nt0 != int(shape[0])):       # kept while T stays the same
            from .operators import AVOLinearModelling
            theta, vsvp, lin = self.flags["avo"]
            avo.op = AVOLinearModelling(theta, vsvp=vsvp, nt0=int(shape[0]), spatdims=(1,), linearization=lin)
        for s in self.stages:
            s.op.upload(device)
        self._join_pair(device)
        return self.live

    def _join_pair(self, device):
        """W and L of this patch as one operator in the order of --wavelet_domain: it takes their place in the iteration and its live
        map is the patch's.  Stand-in stages (the `stages` of __init__) stay two."""
        from .operators import ConvolutionalModelling, Moveout, PrestackModelling
        self.pair = None
        self._model = [s for s in self.stages if s.domain == "model"]
        wav, mov = self.stage("wavelet"), self.stage("moveout")
        if self.domain is None or wav is None or mov is None:
            return
        if not (isinstance(wav.op, ConvolutionalModelling) and isinstance(mov.op, Moveout)):
            return
        self.pair = PrestackModelling(wav.op, mov.op, domain=self.domain)
        self.pair.upload(device)
        self.live = self.pair.live
        i = min(self._model.index(wav), self._model.index(mov))
        assert abs(self._model.index(wav) - self._model.index(mov)) == 1, "W and L must be neighbours in ORDER and ORDER_DATA"
        self._model[i:i + 2] = [Stage("prestack", self.pair, "model", True)]

    def _load_sampling(self, offsets, shape, mask, name):
        """--trace_offsets: the patch's (X, Y, 2) offsets -> R.  Offsets of traces the mask marks unknown are zeroed: the operator is
        the identity there, so nothing off-grid leaks into a trace no data belongs to."""
        self.trace_offsets = None
        file = self.flags["sampling"]
        if file is None:
            if offsets is not None:
                raise ValueError("patch %s carries trace offsets but --trace_offsets is off" % (name,))
            return
        st = self.stage("sampling")
        st.op = None
        if offsets is None:
            raise ValueError("--trace_offsets %s: patch %s carries no offsets (data.extract_patches cuts them)" % (file, name))
        off = np.asarray(offsets, dtype=np.float32)
        if len(shape) not in (3, 4) or off.shape != (shape[1], shape[2] if len(shape) == 4 else 1, 2):
            raise ValueError("--trace_offsets: offsets %s do not belong to a patch of shape %s: expected (X, Y, 2)"
                             % (tuple(off.shape), tuple(shape)))
        known = (np.asarray(mask) != 0).any(axis=(0, -1)).reshape(off.shape[:2])
        self.trace_offsets = off * known[..., None].astype(np.float32)
        from .operators import TraceSampling
        try:
            st.op = TraceSampling(np.moveaxis(self.trace_offsets, -1, 0), interp=self.trace_interp)       # [2][X][Y]
        except ValueError as e:
            raise ValueError("--trace_offsets: %s" % e) from e

    def _load_moveout(self, table, shape, name):
        """--moveout: the patch's table window -> L and its live map."""
        self.live = None
        if self.flags["moveout"] is None:
            if table is not None:
                raise ValueError("patch %s carries a moveout table but --moveout is off" % (name,))
            return
        st = self.stage("moveout")
        st.op = None
        if table is None:
            raise ValueError("--moveout %s: patch %s carries no table (data.extract_patches cuts it)" % (self.flags["moveout"][0], name))
        table = np.asarray(table)
        if table.shape != tuple(shape[:-1]):
            raise ValueError("--moveout: a table of shape %s does not belong to a patch of shape %s: expected %s (all of t, the patch's "
                             "traces)" % (tuple(table.shape), tuple(shape), tuple(shape[:-1])))
        from .operators import Moveout
        try:
            st.op = Moveout(table, interp=self.flags["moveout"][1])
        except ValueError as e:
            raise ValueError("--moveout: %s" % e) from e
        self.live = st.op.live

    # ---- per iteration -----------------------------------------------------------------------------------------
    def apply_model(self, out):
        """The network's output -> the data-domain tensor that everything downstream keeps and compares."""
        kept = False
        for s in self._model:
            if s.tracked and not kept:                           # the first tracked stage: what the network writes (behind G)
                self.pre = out.detach()                          # kept when this iterate is selected
                kept = True
            out = s.op(out)
        return out

    def apply_data(self, out):
        """The data-domain tensor -> what the misfit compares with the recorded traces (fp32 in every --precision mode: the output layer
        writes fp32)."""
        for s in self._data:
            out = s.op(out)
        return out

    def select(self):
        """This iterate is the selected one (eager): its tracked input is kept, as a reference."""
        self.best = self.pre

    def select_if(self, flag):
        """The captured form of select(): dpi_copy_if on the device flag into a buffer of the forward model's own."""
        if self.pre is None:
            return
        if self._buffer is None:
            self._buffer = torch.empty_like(self.pre)
        _lib.check(_lib.load().dpi_copy_if(_lib.ptr(flag), _lib.ptr(self.pre), _lib.ptr(self._buffer), self.pre.numel(), _lib.stream()),
                   "dpi_copy_if")

    def new_buffer(self):
        """Ahead of a capture: the next select_if allocates."""
        self._buffer = None

    def take_buffer(self):
        """After the last replay: what select_if kept is the selected iterate's."""
        self.best = self._buffer

    def clean(self):
        self.pre = self.best = None                              # the section behind the output belongs to the patch

    # ---- results -----------------------------------------------------------------------------------------------
    def model(self, name, out_best=None):
        """The section behind the selected output for stage `name`, in the numpy order and shape of `output`, in the patch's gained
        units.  A tracked stage: its input at the selected iteration; None for a patch that was not optimised, and with --out_ema or a
        sampler.  The second of two tracked stages (--wavelet_domain): the first one's operator applied to the kept tensor, now, with
        the operator object and the kernel of the iteration, so it has the bits the iteration saw.  "avo": m_t = pinv(G_t) out_best_t
        per time sample in float64 with the fp32 G of the device, stored as fp32, from the selected output `out_best` (numpy; None for a
        patch that was not optimised)."""
        st = self.stage(name)
        if st is None or st.op is None:
            return None
        if name == "avo":
            if out_best is None:
                return None
            from .operators import avo_model_from_data
            return avo_model_from_data(out_best, st.op.G.numpy().reshape(st.op.ntheta, 3, st.op.nt0)).astype(np.float32)
        if not st.tracked or self.best is None or self.averaged:
            return None
        if st is self._tracked[0]:
            return to_numpy_out(self.best)
        with torch.no_grad():
            return to_numpy_out(self._tracked[0].op(self.best))

    def run_fields(self, out_best=None):
        """What the result file says about the stages (merged into `run` by save_result)."""
        f = self.flags
        run = {}
        if f["avo"] is not None:
            run.update(avo_theta=list(f["avo"][0]), avo_vsvp=f["avo"][1], avo_linearization=f["avo"][2],
                       avo_model=self.model("avo", out_best))
        if f["wavelet"] is not None:
            # the taps as used (w, or w / 2 for impedance) and the section behind `output`
            op = self.stage("wavelet").op
            run.update(wavelet=op.taps.copy(), wavelet_model_kind=op.kind, wavelet_model=self.model("wavelet"))
        if f["moveout"] is not None:
            # the fp32 table window as used and the flattened section behind `output`
            op = self.stage("moveout").op
            run.update(moveout=None if op is None else op.table.copy(), moveout_interp=f["moveout"][1], moveout_model=self.model("moveout"))
            if f["moveout"][0].startswith("scan:"):
                # --moveout_offset: the picked law(s) the table was built from and the trial velocities [VMIN, VMAX, NV] of the scan
                run.update(moveout_velocity=None if self.velocity is None else np.array(self.velocity, dtype=np.float64),
                           moveout_vscan=[float(v) for v in self.args.moveout_vscan])
                smooth = float(getattr(self.args, "moveout_smooth", None) or 0.0)
                if smooth > 0.0:                                 # the law above is the smoothed one: the length and the staircase behind it
                    run.update(moveout_smooth=smooth, moveout_pick=None if self.pick is None else np.array(self.pick, dtype=np.float64))
                if (getattr(self.args, "moveout_table", None) or "host") == "device":
                    run["moveout_table"] = "device"
        if self.domain is not None:
            run["wavelet_domain"] = self.domain                  # d = W L r (data) or d = L W r (model): which model is which
        if f["sampling"] is not None:
            run["trace_offsets"] = self.trace_offsets            # (X, Y, 2) as used: zero at unknown traces; `output` is the grid tensor
            run["trace_interp"] = self.trace_interp
        return run

    def net_outchannel(self, outchannel):
        """Channels the network itself writes: the patch's, or with --avo_theta the three parameter sections."""
        return 3 if self.flags["avo"] is not None else outchannel

    def volumes(self):
        """(result field, file name) of the model volumes a multi-patch run re-assembles beside reconstructed.npy (--out_ema and the
        samplers track no model: nothing to re-assemble for W and L)."""
        kept = not self.averaged
        files = (("avo", True, "reconstructed_avo.npy"), ("wavelet", kept, "reconstructed_model.npy"), ("moveout", kept, "reconstructed_flat.npy"))
        return [(n + "_model", file) for n, ok, file in files if ok and self.flags[n] is not None]
