"""Command-line flags — drop-in for reference parameter.py (same flag names, defaults and post-processing,
parameter.py:4-130), table-driven.  Differences, both fixing upstream crashes:
  * --netdir defaults to [] (upstream: None -> len(None) TypeError at main.py:105,287);
  * 'skip' is an accepted --net choice (upstream builds Skip3D for it but the parser rejects it).
"""
from argparse import ArgumentParser, Namespace

_ACT = ["LeakyReLU", "ReLU", "ELU", "Tanh", "Sigmoid"]
MODEL_REG_KINDS = ("l1", "tv_t", "tv_x", "tv")

# (flags, kwargs)
_FLAGS = [
    # dataset
    (("--imgdir",), dict(type=str, required=True, default="./datasets/", help="Directory containing the processed data")),
    (("--outdir",), dict(type=str, required=False, help="Subfolder in ./results/ for saving.")),
    (("--imgname",), dict(type=str, help="The name of original images")),
    (("--maskname",), dict(type=str, help="The name of corrupted images")),
    (("--gain",), dict(type=float, required=False, default=2e3, help="gain for the input")),
    (("--datadim",), dict(type=str, required=False, default="2d", choices=["2d", "2.5d", "3d"],
                          help="The dimensionality of the data")),
    (("--slice",), dict(type=str, required=False, default="xy", choices=["tx", "ty", "xy"],
                        help="The type of slice of 3D data when datadim=2.5d")),
    (("--imgchannel",), dict(type=int, required=False, help="Number of 2.5d patches to be stacked in the channel dimension.")),
    (("--adirandel",), dict(type=float, required=False, default=0.0, help="The percent of addictive random deleting samples")),
    (("--padwidth",), dict(type=int, required=False, default=0, help="The padding width to the process data using edge mode")),
    (("--patch_shape",), dict(nargs="+", type=int, required=False, help="Patch shape to be processed (2D, 2.5D, 3D)")),
    (("--patch_stride",), dict(nargs="+", type=int, required=False, help="Patch stride for the extraction (2D, 2.5D, 3D)")),
    # network design
    (("--net",), dict(type=str, required=False, default="multiunet",
                      choices=["multiunet", "attmultiunet", "part", "unet", "load", "skip"], help="The network architecture")),
    (("--gpu",), dict(type=int, required=False, help="GPU to use (default lowest memory usage)")),
    (("--activation",), dict(type=str, default="LeakyReLU", required=False, choices=_ACT,
                             help="Activation function to be used in the convolution block")),
    (("--last_activation",), dict(type=str, required=False, choices=_ACT, help="Activation function to the network output")),
    (("--dropout",), dict(type=float, default=0.0, required=False, help="Dropout rate to be applied in each convolution")),
    (("--filters",), dict(nargs="+", type=int, required=False, default=[16, 32, 64, 128, 256],
                          help="Numbers of channels in every layer of encoder and decoder")),
    (("--skip",), dict(nargs="+", type=int, required=False, default=[16, 32, 64, 128],
                       help="Number of channels for skip-connection")),
    (("--inputdepth",), dict(type=int, required=False, default=64, help="Depth of the input noise tensor")),
    (("--upsample",), dict(type=str, required=False, default="nearest", choices=["nearest", "linear", "deconv"],
                           help="Network's upgoing deconvolution strategy; deconv (ours on the command line) = transposed convolution "
                                "(k=4, s=2, p=1), --net unet only")),
    (("--inittype",), dict(type=str, required=False, default="xavier",
                           choices=["xavier", "normal", "default", "kaiming", "orthogonal"],
                           help="Initialization strategy for the network weights")),
    (("--initgain",), dict(type=float, required=False, default=0.02,
                           help="Initialization scaling factor for normal, xavier and orthogonal.")),
    (("--savemodel",), dict(action="store_true", default=False, help="Save the optimized model to disk")),
    (("--netdir",), dict(type=str, nargs="+", required=False, default=[], help="Path for loading the optimized network")),
    # input noise
    (("--param_noise",), dict(action="store_false", help="Add normal noise to the parameters every epoch")),
    (("--reg_noise_std",), dict(type=float, required=False, default=0.03,
                                help="Standard deviation of the normal noise to be added to the input every epoch")),
    (("--noise_dist",), dict(type=str, default="n", required=False, choices=["n", "u", "c"],
                             help="Type of noise for the input tensor [(n)ormal, (u)niform, (c)auchy]")),
    (("--noise_std",), dict(type=float, default=0.1, required=False, help="Standard deviation of the noise for the input tensor")),
    (("--noise_source",), dict(type=str, default="philox", required=False, choices=["philox", "torch_cpu"],
                             help="ours: philox = z and the per-iteration perturbation drawn on the GPU (counter-based, the default); torch_cpu = parity "
                                  "mode: both drawn by torch's CPU generator in the reference's order (main.py:59-64,143-150, including the "
                                  "--param_noise draws that only shift the stream) and uploaded: same seed, same input stream as the reference")),
    (("--data_forgetting_factor",), dict(type=int, default=0, required=False,
                                         help="Duration of additional decimated data to the input noise tensor")),
    (("--filter_noise_with_wavelet",), dict(action="store_true", default=False,
                                            help="Filter input noise tensor with the wavelet bandwidth")),
    (("--lowpass_fs",), dict(type=float, required=False, help="Butterworth LPF on the input noise: sampling frequency")),
    (("--lowpass_fc",), dict(type=float, required=False, help="Butterworth LPF on the input noise: cutoff frequency")),
    (("--lowpass_ntaps",), dict(type=int, required=False, default=7, help="Low pass filter lenght")),
    # training
    (("--loss",), dict(type=str, required=False, choices=["mae", "mse"], default="mae", help="Loss function to be used.")),
    (("--epochs", "-e", "--iter"), dict(type=int, required=False, default=2001, help="Number of optimization iterations")),
    (("--lr",), dict(type=float, default=1e-3, required=False, help="Learning Rate for Adam optimizer")),
    (("--lr_factor",), dict(type=float, default=0.9, required=False, help="LR reduction for Plateau scheduler.")),
    (("--lr_thresh",), dict(type=float, default=1e-5, required=False, help="LR threshold for Plateau scheduler.")),
    (("--lr_patience",), dict(type=int, default=100, required=False, help="LR patience for Plateau scheduler.")),
    (("--save_every",), dict(type=int, required=False, help="Number of epochs every which to save the results")),
    (("--start_from_prev",), dict(action="store_true", default=False, help="Start training from previous patch")),
    (("--reduce_lr",), dict(action="store_true", default=False, help="Use ReduceLROnPlateau scheduler")),
    (("--earlystop_patience",), dict(type=int, required=False, help="Early stopping patience")),
    (("--earlystop_min_delta",), dict(type=float, required=False, default=1.0, help="Early stopping min percentage delta")),
    # mixed precision (ours; BASELINE configs[4]): bf16 operands / fp32 accumulate in the 3x3(x3) convolutions, everything else fp32
    (("--precision",), dict(type=str, required=False, default="fp32", choices=["fp32", "bf16", "bf16mm", "split"],
                          help="fp32 (reference); bf16 = BASELINE configs[4]: activations and their gradients STORED as bf16 (3-D MultiRes-UNet), "
                               "bf16 operands in the 3x3x3 convolutions, fp32 accumulation / master weights / BatchNorm statistics / Adam; "
                               "bf16mm = bf16 operands only, fp32 storage; split = fp32-accurate three-term bf16 split.  bf16 STORAGE applies to the 3-D MultiRes-UNet "
                               "with LeakyReLU and no dropout (the fused nodes); 2-D / 2.5-D nets, Skip3D, UNet, ELU / dropout nets and runs with "
                               "--data_forgetting_factor keep fp32 tensors under --precision bf16 (operand rounding only, as bf16mm)")),
    # anti-aliasing add-on (ours: the reference ships operators/ + utils/slopes.py without a caller)
    (("--aa_weight",), dict(type=float, required=False, default=0.0, help="Weight of the directional-Laplacian regulariser (0 = off); "
                                                                          "on 3-D patches it acts on the (t,x) and the (t,y) sections")),
    (("--aa_smooth",), dict(type=float, required=False, default=2.0, help="Gaussian smoothing (std, samples) of the structure tensor")),
    (("--aa_dips",), dict(type=str, required=False, help="Optional .npy with a precomputed dip field (same shape as a section; "
                                                         "3-D: 2*C*T*X*Y values, the (t,x) dips then the (t,y) dips)")),
    # self-validation (ours): held-out traces select the output and drive early stopping
    (("--holdout",), dict(type=float, required=False, default=0.0,
                          help="Fraction in [0, 0.5] of the known traces withheld from the loss (0 = off).  The output with the lowest misfit on "
                               "them is kept and early stopping follows that misfit; each trace is drawn independently from the patch seed")),
    # running average of the output (ours: the out_avg of the deep-image-prior method, which the reference dropped)
    (("--out_ema",), dict(type=float, required=False, default=0.0,
                          help="ours: decay BETA in [0, 1) of an exponential running average of the network output (0 = off; deep image prior "
                               "uses 0.99).  The output is selected from the average (lowest training misfit, or held-out misfit with "
                               "--holdout) and early stopping follows that misfit; the weights' trajectory does not change.  Not with "
                               "--optimizer sgld | psgld, whose posterior mean is that path's average")),
    # Langevin sampling (ours: the reference ships architectures/optimizers.py — SGLD, pSGLD — without a caller, main.py:200 builds Adam)
    (("--optimizer",), dict(type=str, required=False, default="adam", choices=["adam", "sgld", "psgld"],
                           help="ours: adam (reference), or a Langevin sampler of the reference's optimizers.py: the output becomes the mean of "
                                "the iterates after --posterior_burnin and their spread is saved as posterior_std")),
    (("--weight_decay",), dict(type=float, required=False, default=0.0, help="ours: L2 penalty of the Langevin samplers (sgld, psgld)")),
    (("--sgld_noise_scale",), dict(type=float, required=False, default=0.1, help="ours: variance of the isotropic noise of sgld (SGLD noise_scale)")),
    (("--psgld_beta",), dict(type=float, required=False, default=0.99, help="ours: decay of the squared-gradient average of psgld (pSGLD beta)")),
    (("--psgld_lambda",), dict(type=float, required=False, default=1e-8, help="ours: added to the preconditioner of psgld (pSGLD Lambda)")),
    (("--langevin_temperature",), dict(type=float, required=False,
                                      help="ours: factor on the VARIANCE of the injected noise.  Unset = 1/N with N the number of samples the "
                                           "loss averages over (non-zeros of the patch's training mask): our loss is a mean, not a sum, so the "
                                           "reference's noise rule over-heats it N-fold; 1 = the reference's rule verbatim; 0 = no noise")),
    (("--posterior_burnin",), dict(type=int, required=False, help="ours: iterations before the first sampled one (default: half of --epochs)")),
    (("--posterior_thin",), dict(type=int, required=False, help="ours: sample every K-th iteration after the burn-in (default 1)")),
    # re-assembly of the volume (ours: the reference crops to the regular window grid and averages overlaps with a box window)
    (("--reassembly",), dict(type=str, required=False, default="crop", choices=["crop", "cover"],
                            help="ours: crop = the regular window grid, which drops the tail of an axis where (n - d) %% s != 0 (reference); "
                                 "cover = one more window flush with the end of such an axis: the result has the input's shape")),
    (("--blend",), dict(type=str, required=False, default="flat", choices=["flat", "taper"],
                       help="ours: flat = overlapping patches are averaged (reference); taper = weighted by sin^2 ramps over the overlap, "
                            "which removes the step at every window edge")),
    # AVO-constrained interpolation of angle gathers (ours: the reference ships operators/avo.py without a caller)
    (("--avo_theta",), dict(nargs="+", type=float, required=False,
                           help="ours: incidence angles in degrees of a (T, X, ntheta) volume of angle gathers (absent = off).  The network "
                                "then outputs three elastic-parameter sections and the linearised AVO operator maps them to the ntheta angle "
                                "sections the loss sees; needs --datadim 2.5d --slice tx --imgchannel ntheta.  The parameter sections are "
                                "saved as avo_model")),
    (("--avo_vsvp",), dict(type=float, required=False, default=0.5, help="ours: vs/vp ratio of the AVO coefficients (--avo_theta)")),
    (("--avo_linearization",), dict(type=str, required=False, default="akirich", choices=["akirich", "fatti"],
                                   help="ours: Aki-Richards or Fatti form of the AVO coefficients (--avo_theta)")),
    # off-grid traces (ours: the reference takes every known trace to sit on a grid node)
    (("--trace_offsets",), dict(type=str, required=False,
                               help="ours: a .npy in --imgdir with the recorded position of every trace minus its bin centre, in grid cells "
                                    "(|d| <= 0.5; absent = off): (X, Y, 2) = dx, dy for --datadim 3d on a (T, X, Y) volume, (X,) or (X, 1) = dx "
                                    "for --datadim 2d on a (T, X) section.  The loss then compares the traces with the network's grid output "
                                    "sampled bilinearly at those positions; what is selected and saved stays the regular-grid output")),
    (("--trace_interp",), dict(type=str, required=False, default="linear", choices=["linear", "cubic", "sinc8"],
                              help="ours: how --trace_offsets samples the grid output at the recorded positions: linear = 2 taps per axis "
                                   "(bilinear), cubic = 4 taps (Keys, a = -1/2), sinc8 = 8 taps (Kaiser-windowed sinc).  The wider kernels "
                                   "keep more of the spatial wavenumbers close to aliasing; needs --trace_offsets")),
    # convolutional modelling (ours: the reference ships operators/signal.py VerticalConv and operators/derivative.py VerticalGrad without a caller)
    (("--wavelet",), dict(type=str, required=False,
                         help="ours: a .npy in --imgdir with a known wavelet, 1-D, odd length <= 255, centre sample = time zero (absent = off).  "
                              "The network then writes the section behind the traces and the wavelet maps it to what the loss sees, so every "
                              "output is confined to the wavelet's band along t; the section is saved as wavelet_model.  Time must be dim 2 of "
                              "the device tensor: --datadim 2d, 3d, or 2.5d with --slice tx | ty")),
    (("--wavelet_model",), dict(type=str, required=False, default="reflectivity", choices=["reflectivity", "impedance"],
                               help="ours: what the network writes under --wavelet: reflectivity = r, traces d = w * r; impedance = m = ln(AI), "
                                    "traces d = 0.5 w * D m with D the forward difference along t; needs --wavelet")),
    (("--wavelet_domain",), dict(type=str, required=False, choices=["data", "model"],
                                help="ours: where the wavelet acts when --wavelet meets --moveout or --moveout_offset (absent = undecided: the "
                                     "pair is refused): data = d = W L r, the wavelet is applied in recorded time behind the moveout and is not "
                                     "stretched (the pre-stack convolutional model of a recorded gather); model = d = L W r, the wavelet is "
                                     "applied in zero-offset time and stretches with the events; needs --wavelet and a moveout flag")),
    # moveout along t (ours: the reference warps no axis)
    (("--moveout",), dict(type=str, required=False,
                         help="ours: a .npy in --imgdir with a moveout table tau (absent = off): (T, X, Y) for --datadim 3d on a (T, X, Y) "
                              "volume, (T, X) for --datadim 2d on a (T, X) section.  The network then writes the flattened gather m and "
                              "the loss sees d[t] = m[tau[t]] of the same trace (NMO, LMO, flattening on a horizon: operators.nmo_table, "
                              "shift_table); a sample is live where 0 <= tau <= T - 1, any other finite value (-1) mutes it: d = 0 there "
                              "and it counts in no loss.  The live values of a trace must not decrease along t and a patch must span the "
                              "whole time axis; the section is saved as moveout_model")),
    (("--moveout_interp",), dict(type=str, required=False, default="linear", choices=["linear", "cubic"],
                                help="ours: how --moveout reads the model along t: linear = 2 taps, cubic = 4 taps (Keys, a = -1/2); needs "
                                     "--moveout or --moveout_offset")),
    # the moveout table from a semblance velocity scan (ours: the reference estimates no velocity)
    (("--moveout_offset",), dict(type=str, required=False,
                                help="ours: a .npy in --imgdir with the source-receiver offset of every trace in cells (absent = off): "
                                     "(X, Y) for --datadim 3d, (X,) or (X, 1) for --datadim 2d.  The table of --moveout is then built from "
                                     "the data: a semblance scan over the known traces (--moveout_vscan), a picked law v(tau) per gather "
                                     "and operators.nmo_table on it; everything else is the path of --moveout, which it replaces")),
    (("--moveout_vscan",), dict(type=float, nargs=3, required=False, metavar=("VMIN", "VMAX", "NV"),
                               help="ours: the trial velocities of --moveout_offset, np.linspace(VMIN, VMAX, NV) in cells per sample, "
                                    "0 < VMIN <= VMAX, NV >= 1; required with --moveout_offset")),
    (("--moveout_gather",), dict(type=str, required=False, choices=["volume", "x", "y"],
                                help="ours: what shares one law v(tau) under --moveout_offset: volume = all traces (the default), x = the "
                                     "Y traces of every x index, y = the X traces of every y index; --datadim 2d takes volume only")),
    (("--moveout_stretch",), dict(type=float, required=False,
                                 help="ours: the stretch mute S > 0 of --moveout_offset (absent = none): the scan skips samples with "
                                      "t > S * tau and the table mutes samples stretched by more than S")),
    (("--moveout_window",), dict(type=int, required=False,
                                help="ours: half width in rows of the semblance window of --moveout_offset (default 2)")),
    (("--moveout_min_fold",), dict(type=int, required=False,
                                  help="ours: fewest live traces a row of the scan of --moveout_offset counts with (default 4)")),
    (("--moveout_max_step",), dict(type=int, required=False,
                                  help="ours: most velocity steps the picked law of --moveout_offset changes by from one row to the "
                                       "next (default 1)")),
    (("--moveout_smooth",), dict(type=float, required=False, metavar="L",
                                help="ours: smooth the picked law of --moveout_offset along tau with a Gaussian of L rows, weighted by the "
                                     "semblance on the picked path, before the table is built (absent = 0 = the staircase pick itself)")),
    (("--moveout_table",), dict(type=str, required=False, choices=["host", "device"],
                               help="ours: where the table of --moveout_offset is built from the law: host = operators.nmo_table (the "
                                    "default), device = the same statements as one kernel launch for all gathers, at most 4096 rows")),
    # penalty on the tensor the network writes (ours: the reference has no prior on the model but the architecture)
    (("--model_reg",), dict(type=str, required=False, choices=list(MODEL_REG_KINDS),
                           help="ours: penalty on the tensor the network itself writes, before --avo_theta / --wavelet / --moveout map it to "
                                "the data (absent = off): l1 = mean |m| (sparse reflectivity), tv_t = mean |difference along t| (blocky "
                                "impedance), tv_x = the same along every other non-channel axis (flat gathers), tv = along all of them "
                                "(anisotropic total variation).  Every kind divides by the element count; needs --model_reg_weight")),
    (("--model_reg_weight",), dict(type=float, required=False, default=0.0,
                                  help="ours: weight W > 0 of --model_reg: total = misfit (+ aa_weight * R_aa) + W * R(m)")),
    # POCS regulariser (main_pocs.py)
    (("--pocs_alpha",), dict(type=float, required=False, default=0.1, help="POCS data weighting.")),
    (("--pocs_thresh",), dict(type=float, required=False, default=5.0, help="POCS thresholding percentage")),
    (("--pocs_weight",), dict(type=float, required=False, help="POCS regularization weight")),
]

_MUST_MATCH = ["datadim", "slice", "imgchannel", "patch_shape", "inputdepth", "loss", "lr", "lr_factor", "lr_thresh",
               "lr_patience", "reduce_lr"]
_OVERRIDDEN = ["net", "activation", "last_activation", "dropout", "filters", "skip", "upsample", "inittype", "initgain"]


def build_parser() -> ArgumentParser:
    parser = ArgumentParser()
    for flags, kw in _FLAGS:
        parser.add_argument(*flags, **kw)
    return parser


def postprocess(args: Namespace) -> Namespace:
    """Derived defaults of parameter.py:113-125."""
    if args.upsample == "linear":
        args.upsample = "trilinear" if args.datadim == "3d" else "bilinear"
    if args.upsample == "deconv" and getattr(args, "net", "multiunet") not in ("unet", "load"):     # load: the saved args.txt decides
        raise ValueError("--upsample deconv needs --net unet (2d, 2.5d or 3d), got --net %s: the other nets up-sample by interpolation "
                         "and have no transposed convolution" % getattr(args, "net", "multiunet"))
    if args.patch_shape is None:
        args.patch_shape = [-1, -1] if args.datadim == "2d" else [-1, -1, -1]
    if args.patch_stride is None:
        args.patch_stride = args.patch_shape
    if args.earlystop_patience is None:
        args.earlystop_patience = args.epochs
    if args.netdir is None:
        args.netdir = []
    if not 0.0 <= getattr(args, "holdout", 0.0) <= 0.5:
        raise ValueError("--holdout must lie in [0, 0.5], got %r" % args.holdout)
    _postprocess_sampler(args)
    check_out_ema(args)
    check_trace_offsets_flag(args)
    check_avo(args)
    check_wavelet(args)
    check_moveout(args)
    check_wavelet_domain(args)
    check_model_reg(args)
    return args


def check_trace_offsets_flag(args: Namespace):
    """--trace_offsets and what it cannot be combined with; returns the file name, or None when it is off (also for a Namespace without the
    key, as those of older args.txt files).  The file itself is read and checked by data.extract_patches."""
    name = getattr(args, "trace_offsets", None)
    interp = getattr(args, "trace_interp", None) or "linear"
    if interp not in ("linear", "cubic", "sinc8"):
        raise ValueError("--trace_interp must be linear, cubic or sinc8, got %r" % (interp,))
    if name is None:
        if interp != "linear":
            raise ValueError("--trace_interp %s needs --trace_offsets: without offsets nothing is sampled and the flag would silently do "
                             "nothing" % interp)
        return None
    if getattr(args, "avo_theta", None) is not None:
        raise ValueError("--trace_offsets does not combine with --avo_theta, which needs --datadim 2.5d")
    if args.datadim not in ("2d", "3d"):
        raise ValueError("--trace_offsets needs --datadim 2d or 3d, got --datadim %s: a 2.5-D slab stacks one spatial axis into channels, "
                         "across which nothing can be sampled" % args.datadim)
    if (getattr(args, "out_ema", 0.0) or 0.0) != 0.0:
        raise ValueError("--trace_offsets does not combine with --out_ema (got %g): the misfit of the running average is evaluated inside "
                         "a fused kernel that compares grid node with trace sample by sample" % args.out_ema)
    if getattr(args, "optimizer", "adam") != "adam":
        raise ValueError("--trace_offsets does not combine with --optimizer %s: the misfit of the posterior mean is evaluated on the grid, "
                         "not at the recorded positions" % args.optimizer)
    return name


def check_wavelet(args: Namespace):
    """--wavelet and what it needs; returns None when it is off (also for a Namespace without the keys, as those of older args.txt files),
    else (file name, kind).  The file itself is read and checked where the operator is built (main.Interpolator)."""
    name = getattr(args, "wavelet", None)
    kind = getattr(args, "wavelet_model", None) or "reflectivity"
    if kind not in ("reflectivity", "impedance"):
        raise ValueError("--wavelet_model must be reflectivity or impedance, got %r" % (kind,))
    if name is None:
        if kind != "reflectivity":
            raise ValueError("--wavelet_model %s needs --wavelet: without a wavelet nothing is modelled and the flag would silently do "
                             "nothing" % kind)
        return None
    # the operator filters along dim 2 of the device tensor (1, C, T, ...): data.transpose_patches_25d leaves t there for the tx slabs
    # (T, X, Y-as-channels) and the ty slabs (T, Y, X-as-channels); the xy slabs are (X, Y, T-as-channels)
    if args.datadim == "2.5d" and args.slice not in ("tx", "ty"):
        raise ValueError("--wavelet needs the time axis as dim 2 of the patch: --datadim 2d, 3d, or 2.5d with --slice tx or ty; "
                         "--slice %s stacks t into the channels" % args.slice)
    return name, kind


_VSCAN_ONLY = ("moveout_vscan", "moveout_gather", "moveout_stretch", "moveout_window", "moveout_min_fold", "moveout_max_step", "moveout_smooth",
               "moveout_table")


def check_moveout_scan(args: Namespace):
    """--moveout_offset and its own flags; returns None when it is off (also for a Namespace without the keys), else the dict of what
    operators.scan_table takes: file, vmin, vmax, nv, gather, stretch_mute, window, min_fold, max_step, and, only where they differ from
    the default, smooth (--moveout_smooth L > 0) and table (--moveout_table device).  The flags of the scan are refused without
    --moveout_offset, where they would silently do nothing."""
    name = getattr(args, "moveout_offset", None)
    if name is None:
        given = [k for k in _VSCAN_ONLY if getattr(args, k, None) is not None]
        if given:
            raise ValueError("--%s needs --moveout_offset: without offsets nothing is scanned and the flag would silently do nothing"
                             % ", --".join(given))
        return None
    if getattr(args, "moveout", None) is not None:
        raise ValueError("--moveout_offset does not combine with --moveout %s: the table is either read or scanned" % (args.moveout,))
    vscan = getattr(args, "moveout_vscan", None)
    if vscan is None:
        raise ValueError("--moveout_offset needs --moveout_vscan VMIN VMAX NV: the trial velocities of the scan, in cells per sample")
    if len(vscan) != 3:
        raise ValueError("--moveout_vscan takes VMIN VMAX NV, got %r" % (vscan,))
    vmin, vmax, nv = (float(v) for v in vscan)
    if not (vmin > 0.0 and vmax >= vmin and vmax < float("inf")):
        raise ValueError("--moveout_vscan needs 0 < VMIN <= VMAX (cells per sample), got %g, %g" % (vmin, vmax))
    if not (nv >= 1.0 and nv == int(nv)):
        raise ValueError("--moveout_vscan needs a whole number NV >= 1 of velocities, got %r" % (vscan[2],))
    gather = getattr(args, "moveout_gather", None) or "volume"
    if gather not in ("volume", "x", "y"):
        raise ValueError("--moveout_gather must be volume, x or y, got %r" % (gather,))
    if args.datadim == "2d" and gather != "volume":
        raise ValueError("--moveout_gather %s needs --datadim 3d: a (T, X) section is one gather (volume)" % gather)
    stretch = getattr(args, "moveout_stretch", None)
    if stretch is not None and not (float(stretch) > 0.0 and float(stretch) < float("inf")):
        raise ValueError("--moveout_stretch must be a finite value > 0, got %r" % (stretch,))
    out = {"file": name, "vmin": vmin, "vmax": vmax, "nv": int(nv), "gather": gather,
           "stretch_mute": None if stretch is None else float(stretch)}
    for key, default, least in (("window", 2, 0), ("min_fold", 4, 0), ("max_step", 1, 0)):
        v = getattr(args, "moveout_" + key, None)
        v = default if v is None else v
        if int(v) != v or v < least:
            raise ValueError("--moveout_%s must be a whole number >= %d, got %r" % (key, least, v))
        out[key] = int(v)
    smooth = getattr(args, "moveout_smooth", None)
    if smooth is not None:
        if not (float(smooth) >= 0.0 and float(smooth) < float("inf")):
            raise ValueError("--moveout_smooth must be a finite length >= 0 (rows of tau), got %r" % (smooth,))
        if float(smooth) > 0.0:
            out["smooth"] = float(smooth)
    builder = getattr(args, "moveout_table", None) or "host"
    if builder not in ("host", "device"):
        raise ValueError("--moveout_table must be host or device, got %r" % (builder,))
    if builder == "device":
        out["table"] = builder
    return out


def check_moveout(args: Namespace):
    """--moveout / --moveout_offset and what they cannot be combined with; returns None when both are off (also for a Namespace without
    the keys, as those of older args.txt files), else (file name, interp) for --moveout and ("scan:" + file name, interp) for
    --moveout_offset (check_moveout_scan has its flags).  The file itself is read and checked by data.extract_patches, which also refuses
    a patch that does not span the time axis."""
    scan = check_moveout_scan(args)
    name = getattr(args, "moveout", None)
    flag = "--moveout"
    if scan is not None:
        name, flag = "scan:" + scan["file"], "--moveout_offset"
    interp = getattr(args, "moveout_interp", None) or "linear"
    if interp not in ("linear", "cubic"):
        raise ValueError("--moveout_interp must be linear or cubic, got %r" % (interp,))
    if name is None:
        if interp != "linear":
            raise ValueError("--moveout_interp %s needs --moveout: without a table nothing is moved and the flag would silently do "
                             "nothing" % interp)
        return None
    if args.datadim not in ("2d", "3d"):
        raise ValueError("%s needs --datadim 2d or 3d, got --datadim %s: a 2.5-D slab is not served" % (flag, args.datadim))
    if getattr(args, "avo_theta", None) is not None:
        raise ValueError("%s does not combine with --avo_theta, which needs --datadim 2.5d" % flag)
    if getattr(args, "wavelet", None) is not None and getattr(args, "wavelet_domain", None) is None:
        raise ValueError("%s does not combine with --wavelet: which of the two operators comes first is not decided yet.  "
                         "--wavelet_domain data | model decides it" % flag)
    if getattr(args, "net", "multiunet") == "part":
        raise ValueError("%s does not combine with --net part: its hole map would live on the model's time axis, the mask on the "
                         "data's" % flag)
    if (getattr(args, "data_forgetting_factor", 0) or 0) > 0:
        raise ValueError("%s does not combine with --data_forgetting_factor %d: it adds data-domain traces to the input of a "
                         "network that writes the model domain" % (flag, args.data_forgetting_factor))
    return name, interp


def check_wavelet_domain(args: Namespace):
    """--wavelet_domain and what it needs; returns None when it is absent (also for a Namespace without the key, as those of older
    args.txt files), else "data" (d = W L r) or "model" (d = L W r).  The flag is refused without both of its partners, where it would
    silently do nothing; the pair without the flag is refused by check_moveout."""
    domain = getattr(args, "wavelet_domain", None)
    if domain is None:
        return None
    if domain not in ("data", "model"):
        raise ValueError("--wavelet_domain must be data or model, got %r" % (domain,))
    missing = [flag for flag, on in (("--wavelet", getattr(args, "wavelet", None) is not None),
                                     ("--moveout or --moveout_offset", getattr(args, "moveout", None) is not None
                                      or getattr(args, "moveout_offset", None) is not None)) if not on]
    if missing:
        raise ValueError("--wavelet_domain %s needs %s: it orders the two operators, and with one of them nothing is ordered and the "
                         "flag would silently do nothing" % (domain, " and ".join(missing)))
    return domain


def model_reg_axes(kind, datadim, slice):
    """The dims of the device tensor (1, C, n0, n1[, n2]) that --model_reg `kind` differences: () for l1.  Time is dim 2 for --datadim 2d,
    3d and 2.5d with --slice tx | ty (the rule of check_wavelet); the xy slabs are (X, Y, T-as-channels): both dims lateral, no time axis."""
    if kind not in MODEL_REG_KINDS:
        raise ValueError("--model_reg must be one of %s, got %r" % (", ".join(MODEL_REG_KINDS), kind))
    dims = (2, 3, 4) if datadim == "3d" else (2, 3)
    time = () if (datadim == "2.5d" and slice == "xy") else (2,)
    if kind == "l1":
        return ()
    if kind == "tv_t":
        if not time:
            raise ValueError("--model_reg tv_t needs the time axis as dim 2 of the patch: --datadim 2d, 3d, or 2.5d with --slice tx or ty; "
                             "--slice %s stacks t into the channels" % slice)
        return time
    return dims if kind == "tv" else tuple(d for d in dims if d not in time)


def check_model_reg(args: Namespace):
    """--model_reg and what it needs; returns None when it is off (also for a Namespace without the keys, as those of older args.txt
    files), else (kind, weight, dims of the device tensor that are differenced)."""
    kind = getattr(args, "model_reg", None)
    weight = getattr(args, "model_reg_weight", None)
    weight = 0.0 if weight is None else float(weight)
    if kind is None:
        if weight != 0.0:
            raise ValueError("--model_reg_weight %g needs --model_reg: without a kind nothing is penalised and the flag would silently do "
                             "nothing" % weight)
        return None
    axes = model_reg_axes(kind, args.datadim, args.slice)
    if not (weight > 0.0 and weight < float("inf")):
        raise ValueError("--model_reg %s needs --model_reg_weight W with a finite W > 0, got %r" % (kind, weight))
    return kind, weight, axes


def check_avo(args: Namespace):
    """--avo_theta and what it needs; returns None when it is off (also for a Namespace without the key, as those of older args.txt files),
    else (theta list, vsvp, linearization)."""
    theta = getattr(args, "avo_theta", None)
    if theta is None:
        return None
    theta = [float(t) for t in theta]
    vsvp = float(getattr(args, "avo_vsvp", 0.5))
    lin = getattr(args, "avo_linearization", "akirich")
    if args.datadim != "2.5d" or args.slice != "tx":
        raise ValueError("--avo_theta needs --datadim 2.5d --slice tx (a (T, X, ntheta) volume whose stacked channel axis is the angle "
                         "axis), got --datadim %s --slice %s" % (args.datadim, args.slice))
    if args.imgchannel != len(theta):
        raise ValueError("--avo_theta names %d angles: --imgchannel must be %d, got %r" % (len(theta), len(theta), args.imgchannel))
    if len(set(theta)) < 3:
        raise ValueError("--avo_theta needs at least 3 distinct angles for the three parameter sections, got %r" % (theta,))
    if not vsvp > 0.0:
        raise ValueError("--avo_vsvp must be > 0, got %r" % (vsvp,))
    if lin not in ("akirich", "fatti"):
        raise ValueError("--avo_linearization must be akirich or fatti, got %r" % (lin,))
    import numpy as np
    from .operators.avo import avo_coefficients
    try:
        G = avo_coefficients(theta, vsvp, 1, lin)[:, :, 0]
    except ValueError as e:
        raise ValueError("--avo_theta: %s" % e) from e
    if np.linalg.matrix_rank(G) < 3:
        raise ValueError("--avo_theta %r with --avo_vsvp %g gives coefficients of rank %d: the three parameter sections cannot be told "
                         "apart (angles of equal sin^2 count once)" % (theta, vsvp, int(np.linalg.matrix_rank(G))))
    args.avo_theta = theta
    return theta, vsvp, lin


def check_out_ema(args: Namespace) -> float:
    """Range of --out_ema and what it cannot be combined with; returns the value (0.0 for a Namespace without the key, as those of
    reference args.txt files)."""
    beta = getattr(args, "out_ema", 0.0)
    beta = 0.0 if beta is None else float(beta)
    if not 0.0 <= beta < 1.0:
        raise ValueError("--out_ema must lie in [0, 1), got %r" % (beta,))
    if beta > 0.0 and getattr(args, "optimizer", "adam") != "adam":
        raise ValueError("--out_ema does not combine with --optimizer %s: the posterior mean is that path's average" % args.optimizer)
    return beta


def _postprocess_sampler(args: Namespace) -> None:
    """Ranges and derived defaults of the Langevin flags (ours).  The sampler-only flags are refused with --optimizer adam, where they
    would silently do nothing."""
    opt = getattr(args, "optimizer", "adam")
    if opt not in ("adam", "sgld", "psgld"):
        raise ValueError("--optimizer must be adam, sgld or psgld, got %r" % (opt,))
    sampler_only = ("langevin_temperature", "posterior_burnin", "posterior_thin")
    if opt == "adam":
        given = [k for k in sampler_only if getattr(args, k, None) is not None]
        if given:
            raise ValueError("--%s needs a sampler (--optimizer sgld or psgld), not --optimizer adam" % ", --".join(given))
        args.posterior_burnin, args.posterior_thin = args.epochs // 2, 1        # the listed defaults; inert without a sampler
        return
    for k in ("weight_decay", "sgld_noise_scale", "psgld_beta", "psgld_lambda"):
        if not getattr(args, k) >= 0.0:
            raise ValueError("--%s must be >= 0, got %r" % (k, getattr(args, k)))
    if args.psgld_beta > 1.0:
        raise ValueError("--psgld_beta must lie in [0, 1], got %r" % args.psgld_beta)
    if args.langevin_temperature is not None and not args.langevin_temperature >= 0.0:
        raise ValueError("--langevin_temperature must be >= 0, got %r" % args.langevin_temperature)
    if args.posterior_burnin is None:
        args.posterior_burnin = args.epochs // 2
    if args.posterior_burnin < 0:
        raise ValueError("--posterior_burnin must be >= 0, got %r" % args.posterior_burnin)
    if args.posterior_thin is None:
        args.posterior_thin = 1
    if args.posterior_thin < 1:
        raise ValueError("--posterior_thin must be >= 1, got %r" % args.posterior_thin)


def parse_arguments(argv=None) -> Namespace:
    return postprocess(build_parser().parse_args(argv))


_same = lambda v: v
# (key, what an args.txt without the key means, normaliser): what the network's output means and what its weights were fitted through
_OURS_MUST_MATCH = (
    ("avo_theta", None, lambda t: None if t is None else [float(x) for x in t]),       # the network's output channels
    ("trace_offsets", None, _same), ("trace_interp", "linear", _same),
    ("wavelet", None, _same), ("wavelet_model", "reflectivity", _same),
    ("moveout", None, _same), ("moveout_interp", "linear", _same),
    # the scanned table: what decides it (window, fold and step only tune the pick; the table itself is saved with the run)
    ("moveout_offset", None, _same), ("moveout_vscan", None, lambda v: None if v is None else [float(x) for x in v]),
    ("moveout_gather", "volume", _same), ("moveout_stretch", None, lambda v: None if v is None else float(v)),
    # the law the table is built from, and where: the device's table may differ from the host's in the rounding of a square root
    ("moveout_smooth", 0.0, float), ("moveout_table", "host", _same),
    ("wavelet_domain", None, _same),                             # which of W and L comes first: what the network's output means
)


def net_args_are_same(args1: Namespace, args2: Namespace) -> bool:
    """Compatibility of a saved args.txt with the current run before loading its weights (parameter.py:133-173)."""
    a, b = vars(args1), vars(args2)
    errors = [k for k in _MUST_MATCH if a[k] != b[k]]
    # ours: args.txt files of older runs lack these keys, which then count as the default (off, or the named kind)
    errors += [k for k, default, norm in _OURS_MUST_MATCH if norm(a.get(k) or default) != norm(b.get(k) or default)]
    warns = [k for k in _OVERRIDDEN if a[k] != b[k]]
    if errors:
        print("The following arguments keys have to be the same:\n\t")
        print(", ".join(errors))
        return False
    if warns:
        print("\nThe following arguments are different, but they are overridden by the network loading:")
        print("\t", ", ".join(warns))
    return True
