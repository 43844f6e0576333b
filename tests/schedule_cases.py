"""The runs tests/test_gpu_schedule_matrix.py repeats under the big-patch stream schedule (weight gradients on the side streams, one join
per step, the ResPath half of a level join on the branch stream) and compares bit for bit with the serial schedule, as pure data (no torch,
no GPU: tests/test_schedule_cases_host.py checks on the CPU that the table names every --net, --optimizer and --upsample choice of
parameter.py, so a net added later without a row fails there).

A row is one Interpolator run:

    Row(name, argv, shape, extra, fields, mode, branch)

 name    the test id
 argv    command-line fragment; COMMON is appended (4 iterations)
 shape   the patch in numpy order, channels last: (T, X, Y, 1) for --datadim 3d, (T, X, 1) for 2d, (T, X, sections) for 2.5d
 extra   data beside the patch, as recipes the device test builds:
           "data": "avo"                  the patch is utils.avo_gathers(shape, THETA) instead of utils.hyperbolic_volume
           "wavelet": (f0, dt, K)         the taps utils.ricker(f0, dt, K), saved as w.npy in --imgdir
           "offsets": seed                trace offsets uniform in [-0.5, 0.5), RandomState(seed), shape (X, Y, 2): the patch's "offsets"
 fields  products the run must have (not None) and that are compared beside what every row compares — every history column the run
         has, out_best, best_iter, every state_dict entry, the optimiser's moment tensors:
           wavelet_model, avo_model       Interpolator.wavelet_model() / avo_model()
           posterior_std, output_selected the sampler's spread and its selected iterate (out_best is the posterior mean there)
           ema_best                       the selected snapshot of the running average
         and history columns that must exist: val_loss, ema_loss, ema_val_loss, reg
 mode    eager | graph: optimize(mode=...).  A graph row's streamed run keeps the side streams inside the captured iteration
         (Schedule.overlap_in_graph); its iteration 0 runs eagerly, branch stream included
 branch  the run must have opened the branch stream: the 3-D MultiRes-UNet whose ResPaths are fusable nodes (ops.skip_begin).  False
         for every other net: they have no level join that runs as one node

Shapes: the smallest each net takes that still give several workgroups per kernel at the finest level — (32, 48, 64) with the narrow
filters of test_gpu_nets.test_branch_stream_schedule_is_bit_identical_to_the_serial_one for the 3-D nets, a 64 x 96 section for the 2-D and
2.5-D ones, and for UNet3D the geometry of NET_CASES in tests/test_gpu_unet3d.py (32 x 16 x 16; widths 2..32, no multiple of 16 below the
coarsest levels, and widths 16 16 32 32 32, whose transposed convolutions all run on MFMA).  Every patch has fewer than 2^20 voxels: the
device test makes it take the big-patch schedule.

ops.sched.side_rr after a streamed run counts the weight-gradient launches that left the main stream in the last iteration: one per k = 1 /
k = 3 convolution weight that received a gradient, in every row (the k = 4 transposed convolutions of --upsample deconv compute their
weight gradient on the main stream and are not counted)."""
from collections import namedtuple

Row = namedtuple("Row", "name argv shape extra fields mode branch")

COMMON = ["--epochs", "4", "--gpu", "0", "--gain", "40"]
THETA = [0.0, 10.0, 20.0, 30.0]          # --avo_theta: four angles
RICKER = (0.12, 1.0, 9)                  # utils.ricker(f0, dt, K)

# --net choices without a row, and why
EXCLUDED_NETS = {
    "part": "never takes the schedule: every `down` convolution is used twice, autograd accumulates its weight gradient on the main stream "
            "(Interpolator.wants_weight_grad_overlap); test_net_part_keeps_the_serial_schedule_at_size holds that rule at 2^20 voxels",
    "load": "builds the net a saved args.txt names, i.e. one of the other choices, from files of an earlier run",
}

M3 = ["--datadim", "3d", "--filters", "6", "12", "24", "40", "--skip", "4", "8", "12", "--inputdepth", "9", "--upsample", "linear"]
A3 = ["--datadim", "3d", "--net", "attmultiunet", "--filters", "6", "12", "24", "--inputdepth", "9"]
M2 = ["--filters", "6", "12", "24", "--skip", "4", "8", "--inputdepth", "9", "--upsample", "linear"]
D2, D25 = ["--datadim", "2d"], ["--datadim", "2.5d", "--slice", "tx", "--imgchannel", "3"]
SK = ["--net", "skip", "--filters", "4", "8", "16", "--skip", "2", "2", "2", "--inputdepth", "8", "--upsample", "linear"]
# --inittype kaiming: the up path of the plain U-Net has no norm, under the default xavier gain of 0.02 its layers pass no gradient
U3 = ["--datadim", "3d", "--net", "unet", "--inittype", "kaiming"]
U3_NARROW = U3 + ["--filters", "2", "4", "8", "16", "32", "--inputdepth", "4"]
U3_MFMA = U3 + ["--filters", "16", "16", "32", "32", "32", "--inputdepth", "8"]
S3, S2, S25, SU = (32, 48, 64, 1), (64, 96, 1), (64, 96, 3), (32, 16, 16, 1)
VAL = ("val_loss", "val_snr")


def _row(name, argv, shape, fields=(), mode="eager", branch=False, **extra):
    return Row(name, list(argv), tuple(shape), dict(extra), tuple(fields), mode, branch)


ROWS = [
    _row("multiunet-3d", M3, S3, branch=True),
    # ---- the nets added since the schedule was written
    _row("attmultiunet-3d-linear", A3 + ["--upsample", "linear"], S3),
    _row("attmultiunet-3d-nearest", A3 + ["--upsample", "nearest"], S3),
    _row("attmultiunet-3d-bf16", A3 + ["--upsample", "linear", "--precision", "bf16"], S3),      # operand rounding only: storage stays fp32
    _row("attmultiunet-25d", D25 + ["--net", "attmultiunet", "--filters", "6", "12", "24", "--inputdepth", "9", "--upsample", "linear"], S25),
    _row("unet-3d-deconv-narrow", U3_NARROW + ["--upsample", "deconv"], SU),
    _row("unet-3d-deconv-mfma", U3_MFMA + ["--upsample", "deconv"], SU),
    _row("unet-3d-linear-narrow", U3_NARROW + ["--upsample", "linear"], SU),
    _row("unet-3d-linear-mfma", U3_MFMA + ["--upsample", "linear"], SU),
    _row("skip-2d", D2 + SK, S2),
    _row("skip-25d", D25 + SK, S25),
    _row("skip-3d", ["--datadim", "3d"] + SK, S3),
    _row("multiunet-2d", D2 + M2, S2),
    _row("multiunet-25d", D25 + M2, S25),
    # ELU: MultiResBlock._fusable() and ResPath._fusable() are false, every layer is a leaf ConvFn / BatchNormFn node and the level joins
    # are plain concats: no branch stream
    _row("multiunet-3d-leaf-nodes", M3 + ["--activation", "ELU"], S3),
    # ---- what stands behind the net's last layer, whose weight gradient is the first launch to leave the main stream
    _row("wavelet-offsets-sinc8", M3 + ["--wavelet", "w.npy", "--wavelet_model", "impedance", "--trace_offsets", "off.npy",
                                         "--trace_interp", "sinc8"], S3, ("wavelet_model",), branch=True, wavelet=RICKER, offsets=11),
    _row("holdout-out_ema", M3 + ["--holdout", "0.25", "--out_ema", "0.9"], S3, VAL + ("ema_loss", "ema_val_loss", "ema_best"), branch=True),
    _row("psgld-holdout", M3 + ["--optimizer", "psgld", "--holdout", "0.25"], S3, VAL + ("posterior_std", "output_selected"), branch=True),
    _row("sgld", M3 + ["--optimizer", "sgld"], S3, ("posterior_std", "output_selected"), branch=True),
    _row("aa_weight", M3 + ["--aa_weight", "0.5", "--aa_smooth", "2"], S3, ("reg",), branch=True),
    # (fp32 storage and two iterations with the data added to the input; the nodes stay fused)
    _row("data-forgetting", M3 + ["--data_forgetting_factor", "2"], S3, branch=True),
    _row("loss-mse", M3 + ["--loss", "mse"], S3, branch=True),
    _row("avo-wavelet-25d", ["--datadim", "2.5d", "--slice", "tx", "--imgchannel", "4", "--avo_theta"] + [str(t) for t in THETA] + M2
         + ["--wavelet", "w.npy"], (64, 96, 4), ("avo_model", "wavelet_model"), data="avo", wavelet=RICKER),
    # ---- the side streams inside a captured iteration
    _row("graph-multiunet-3d", M3, S3, mode="graph", branch=True),
    _row("graph-attmultiunet-3d", A3 + ["--upsample", "linear"], S3, mode="graph"),
]
