"""The convolution launches whose caller-visible contract tests/test_gpu_conv_contract.py checks on a device, as pure data (no torch, no
GPU: tests/test_host_asan.py feeds the same rows to the host driver's `--plan` mode and proves on the CPU that they cover the planner).

A row is one descriptor under one set of knobs:

    Case(launcher, cin, cout, shape, k, kd, stride, precision, io, options, chained, offsets, reaches)

 launcher   fwd | bwd_data | bwd_data_dual | bwd_weight
 cout       output channels; for bwd_data_dual the pair (3x3(x3) layer, 1x1(x1) layer)
 shape      (D, H, W) of the layer's input
 precision  dpi_conv_desc.precision (0 fp32, 1 bf16 operands, 2 three-term split); io: the DPI_IO_* mask (15 = every activation bf16)
 options    dpi_set_option keys that hold for this row only (restored afterwards; the Python side drops its cached workspace sizes)
 chained    forward / backward-weight: the launch that carries a BatchNorm + LeakyReLU chain on x is part of the row
 offsets    element offsets of the INPUT tensors (x, dy) the row is run at besides 0: 1 = one element (4 bytes fp32, 2 bytes bf16),
            2 = two bf16 elements (4 bytes).  Only where the kernel the row reaches is written for that alignment (see the device test).
 reaches    what the planner must answer: launch name of the host driver's table -> kernel family, i.e. the text a failed launch names.
            "packed-weight scratch" is what the bf16 stencil kernels (conv_bf16_mfma.hip) answer on a host without a device: they
            allocate their packed weights before they launch.

PASS1 are the knobs of the driver's second pass: the MFMA, few-output-channel and 4x4x1 families off, which leaves the VALU kernels.
Shapes are the smallest that still reach the family; odd W and odd voxel counts (5x7x9, 3x9x11, 7x9x11) are kept among them because a
channel slice of such a tensor starts at a 4-byte address (2-byte with bf16 storage), which is what the product's concat buffers produce."""
from collections import namedtuple

Case = namedtuple("Case", "launcher cin cout shape k kd stride precision io options chained offsets reaches")

# The library's knobs as it starts, the ONE place the tests and the host driver's `--plan` mode (which is handed them on its first line)
# take them from.  They restate the initialisers in csrc/ (conv_mfma.hip: splitk, bw_pair, mfma_min_cout, bwd_weight_mfma_min_cout;
# conv_direct.hip: dual_bwd_data; conv_fewco_mfma.hip, conv_q4_mfma.hip, conv_bf16_mfma.hip); three of those read the environment.
def knob_defaults(environ):
    return {"splitk": int(environ.get("DPI_SPLITK", 1)), "dual_bwd_data": 0 if "DPI_NO_DUAL" in environ else 1,
            "bw_pair": int(environ.get("DPI_BW_PAIR", 2)), "mfma_min_cout": 8, "bwd_weight_mfma_min_cout": 8, "fewco_mfma": 1, "q4": 1,
            "q4_ck": 0, "bf16_debug": 0}


def options_text(options):
    return ",".join("%s=%d" % kv for kv in sorted(options.items())) or "-"


PASS1 = {"mfma_min_cout": 1 << 20, "bwd_weight_mfma_min_cout": 1 << 20, "fewco_mfma": 0, "q4": 0}
BF = {"bf16_debug": 8}          # bit 3: every 3x3(x3) stride-1 layer of a precision-1 / -2 descriptor through the bf16 stencil kernel
SCRATCH = "packed-weight scratch"


def _fwd(cin, cout, shape, k=3, stride=1, precision=0, io=0, options=None, offsets=(), family="conv_mfma", split=False):
    reaches = {"fwd": family}
    if split:
        reaches["fwd_ws"] = "conv_mfma (split)"
    return Case("fwd", cin, cout, shape, k, 1 if shape[0] == 1 else k, stride, precision, io, dict(options or {}), True, tuple(offsets), reaches)


def _bwd(cin, cout, shape, k=3, stride=1, precision=0, io=0, options=None, offsets=(), family="conv_mfma", split=False):
    reaches = {"bwd_data": family}
    if split:
        reaches["bwd_data_ws"] = "conv_mfma (split)"
    return Case("bwd_data", cin, cout, shape, k, 1 if shape[0] == 1 else k, stride, precision, io, dict(options or {}), False, tuple(offsets), reaches)


def _dual(cin, c3, c1, shape, precision=0, io=0, options=None, family="conv_mfma"):
    return Case("bwd_data_dual", cin, (c3, c1), shape, 3, 1 if shape[0] == 1 else 3, 1, precision, io, dict(options or {}), False, (),
                {"bwd_data_dual": family})


def _bww(cin, cout, shape, k=3, stride=1, precision=0, io=0, options=None, plain="conv_bwd_weight_mfma", chained=None, unaligned=None):
    offsets = (1, 2) if io else (1,)
    reaches = {"bwd_weight": plain, "bwd_weight_chained": chained or plain, "bwd_weight_unaligned": unaligned or plain}
    return Case("bwd_weight", cin, cout, shape, k, 1 if shape[0] == 1 else k, stride, precision, io, dict(options or {}), True, offsets, reaches)


CASES = [
    # ---- forward ---------------------------------------------------------------------------------------------------------------------
    _fwd(71, 20, (5, 7, 9), split=True, offsets=(1,)),                  # fp32 MFMA stencil, input-channel split with a workspace; odd V
    _fwd(133, 17, (3, 9, 11), stride=2, split=True),                    # ... stride 2
    _fwd(17, 26, (6, 6, 6)),                                            # unsplit, small-tile variant, two channel tiles (26 = 16 + 10)
    _fwd(25, 16, (12, 9, 40)),                                          # unsplit, big-tile variant, ragged H
    _fwd(13, 17, (1, 70, 45)),                                          # 2-D (kd = 1)
    _fwd(12, 9, (7, 9, 11), stride=2),                                  # stride 2, odd sizes: element-wise staging
    _fwd(9, 20, (8, 8, 40), stride=2, offsets=(1,)),                                 # stride 2, W % 4 == 0 and V % 4 == 0: the vectorised staging
    _fwd(6, 8, (5, 9, 40), options={"q4": 2, "q4_ck": 2}, offsets=(1,), family="conv_q4_mfma"),   # 4x4x1 MFMA kernel, planar chunks
    _fwd(6, 8, (5, 9, 40), options={"q4": 2, "q4_ck": 4}, offsets=(1,), family="conv_q4_mfma"),   # ... channel-interleaved chunks
    _fwd(4, 8, (32, 64, 192), family="conv_q4_mfma"),                   # ... at its default threshold (W >= 48, 192 tiles): the one large row
    _fwd(9, 3, (32, 33, 47), family="conv_fewco_mfma"),                 # few-output-channel forward kernel, ragged tiles, odd W
    _fwd(137, 51, (5, 7, 9), k=1, family="conv_pw_mfma"),               # 1x1x1 on the MFMA, V % 4 != 0 (scalar paths)
    _fwd(9, 4, (1, 20, 24), k=1, family="conv_pw"),                     # 1x1 VALU
    _fwd(3, 5, (2, 2, 2), family="conv_direct"),                        # VALU stencil, one ragged tile
    _fwd(3, 5, (6, 6, 6), stride=2, family="conv_direct"),              # ... stride 2
    _fwd(17, 26, (6, 6, 6), options=PASS1, family="conv_direct"),       # the fall-back chain: an MFMA row on the VALU stencil
    _fwd(137, 51, (5, 7, 9), k=1, options=PASS1, family="conv_pw"),     # ... and on the VALU 1x1x1
    _fwd(13, 9, (7, 9, 11), io=15),                                     # bf16 tensors, fp32 arithmetic: slices start 2-byte aligned (odd V)
    _fwd(16, 16, (4, 8, 16), io=15),                                    # ... even rows and channels: two voxels per dword store
    _fwd(137, 51, (5, 7, 9), k=1, io=15, family="conv_pw_mfma"),        # ... 1x1x1
    _fwd(7, 3, (5, 7, 9), io=15, family="conv_direct"),                 # ... VALU stencil
    _fwd(17, 26, (6, 6, 6), precision=2),                               # split mode on a shape the fp32 kernel keeps
    _fwd(16, 16, (4, 8, 16), precision=2, options=BF, family=SCRATCH),  # split mode on the bf16 stencil kernel
    _fwd(16, 16, (4, 8, 16), precision=1, io=15, options=BF, family=SCRATCH),           # bf16 stencil kernel, bf16 tensors
    _fwd(16, 16, (4, 6, 16), stride=2, precision=1, io=15, family=SCRATCH),             # bf16 stride-2 forward kernel
    # ---- backward-data -----------------------------------------------------------------------------------------------------------------
    _bwd(20, 71, (5, 7, 9), split=True, offsets=(1,)),                  # the flipped launch splits over the layer's OUTPUT channels
    _bwd(17, 26, (6, 6, 6)),
    _bwd(25, 16, (12, 9, 40)),
    _bwd(13, 17, (1, 70, 45)),
    _bwd(3, 5, (6, 6, 6), stride=2, family="conv_bwd_data_s2"),         # stride 2, Cin < 8: VALU kernel
    _bwd(12, 9, (7, 9, 11), stride=2, family="conv_bwd_data_s2_mfma"),  # stride 2, Cin >= 8, odd W: scalar epilogue
    _bwd(9, 20, (8, 8, 40), stride=2, family="conv_bwd_data_s2_mfma"),  # ... even W and V: float2 epilogue
    _bwd(16, 16, (4, 6, 16), stride=2, precision=1, io=15, offsets=(1,), family=SCRATCH),           # stride 2, bf16 tensors + arithmetic
    _bwd(8, 6, (5, 9, 40), options={"q4": 2}, offsets=(1,), family="conv_q4_mfma"),
    _bwd(8, 4, (32, 64, 192), family="conv_q4_mfma"),
    _bwd(137, 51, (5, 7, 9), k=1, family="conv_pw_mfma"),
    _bwd(4, 9, (1, 20, 24), k=1, family="conv_pw"),
    _bwd(3, 5, (2, 2, 2), family="conv_direct"),
    _bwd(17, 26, (6, 6, 6), options=PASS1, family="conv_direct"),
    _bwd(137, 51, (5, 7, 9), k=1, options=PASS1, family="conv_pw"),
    _bwd(12, 9, (7, 9, 11), stride=2, options=PASS1, family="conv_bwd_data_s2"),
    _bwd(13, 9, (7, 9, 11), io=15),                                     # bf16 tensors, fp32 arithmetic, odd V
    _bwd(12, 9, (7, 9, 11), stride=2, io=15, family="conv_bwd_data_s2_mfma"),
    _bwd(16, 16, (4, 8, 16), precision=1, io=15, options=BF, family=SCRATCH),           # bf16 stencil kernel, flipped
    # ---- the fused pair ------------------------------------------------------------------------------------------------------------------
    _dual(137, 8, 51, (6, 10, 18)),                                     # 1x1x1 term inside the MFMA stencil launch
    _dual(137, 8, 51, (6, 10, 18), options={"dual_bwd_data": 0}, family="conv_pw_mfma"),       # two launches (the first one is named)
    _dual(20, 71, 9, (5, 7, 9), family="conv_pw_mfma"),                 # default knobs, yet two launches: the 3x3x3 launch splits into its workspace
    _dual(13, 9, 7, (1, 20, 24)),
    _dual(13, 9, 7, (1, 20, 24), options={"dual_bwd_data": 0}, family="conv_pw_mfma"),
    _dual(13, 9, 7, (1, 20, 24), options=PASS1, family="conv_pw"),
    _dual(4, 8, 9, (3, 5, 7), family="conv_pw"),                        # Cin < 8: VALU 1x1x1, then the VALU stencil accumulating; odd V
    _dual(16, 16, 16, (4, 8, 16), precision=1, io=15, options=BF, family=SCRATCH),             # extra K blocks of the bf16 stencil kernel
    # ---- backward-weight: each row is four launches (chain or none, x / dy aligned or offset) ------------------------------------------------
    _bww(25, 16, (12, 9, 40)),                                          # MFMA, dY rows x (ci, tap) columns; 25 = 4m + 1 (tail launch)
    _bww(25, 16, (12, 9, 40), options={"bw_pair": 0}),
    _bww(25, 16, (12, 9, 40), options={"bw_pair": 1}),                  # two 4-channel groups per workgroup
    _bww(71, 20, (5, 7, 9)),                                            # odd W and V
    _bww(12, 9, (7, 9, 11), stride=2),
    _bww(16, 4, (1, 40, 48), chained="conv_bwd_weight"),                # 2-D, swapped orientation (needs an input without a chain)
    _bww(13, 4, (32, 32, 40), chained="conv_bwd_weight_smallco"),       # 3-D, swapped; V >= 32768: the few-output-channel kernel with a chain
    _bww(6, 5, (32, 32, 32), plain="conv_bwd_weight_smallco"),          # Cin < 8: the few-output-channel kernel in all four launches
    _bww(137, 51, (5, 7, 9), k=1, plain="conv_pw_bwd_weight_mfma"),
    _bww(9, 4, (1, 20, 24), k=1, plain="conv_bwd_weight"),              # VALU 1x1
    _bww(3, 5, (2, 2, 2), plain="conv_bwd_weight"),                     # VALU stencil
    _bww(25, 16, (12, 9, 40), options=PASS1, plain="conv_bwd_weight"),
    _bww(16, 4, (1, 40, 48), options=PASS1, chained="conv_bwd_weight"),
    _bww(6, 5, (32, 32, 32), options=PASS1, plain="conv_bwd_weight_smallco"),
    _bww(13, 9, (7, 9, 11), precision=1, io=15),                        # bf16 tensors, odd rows: 2-byte pieces in the fp32 MFMA kernel
    _bww(64, 25, (4, 4, 8), k=1, precision=1, io=15, plain="conv_pw_bwd_weight_mfma"),         # 1x1x1: bf16 MFMA when aligned, fp32 else
    _bww(16, 16, (4, 8, 16), precision=1, io=15, plain="conv_bf16_bwd_weight", unaligned="conv_bwd_weight_mfma"),
    _bww(16, 16, (4, 6, 16), stride=2, precision=1, io=15, plain="conv_bf16_bww_s2", chained="conv_bwd_weight_mfma", unaligned="conv_bwd_weight_mfma"),
    _bww(16, 16, (4, 8, 16), precision=1, io=15, options=PASS1, plain="conv_bf16_bwd_weight", unaligned="conv_bwd_weight"),
    _bww(16, 16, (4, 6, 16), stride=2, precision=1, io=15, options=PASS1, plain="conv_bf16_bww_s2", chained="conv_bwd_weight", unaligned="conv_bwd_weight"),
]


def case_id(c):
    cout = "%d+%d" % c.cout if isinstance(c.cout, tuple) else "%d" % c.cout
    opts = "".join("-%s%d" % (k, v) for k, v in sorted(c.options.items())) if c.options != PASS1 else "-pass1"
    return "%s-%dto%s-%dx%dx%d-k%ds%dp%dio%d%s" % ((c.launcher, c.cin, cout) + tuple(c.shape) + (c.k, c.stride, c.precision, c.io, opts))


def plan_line(c):
    """The row in the format `host_asan_driver --plan` reads from stdin."""
    c3, c1 = c.cout if isinstance(c.cout, tuple) else (c.cout, 0)
    return "%s %d %d %d %d %d %d %d %d %d %d %d %s" % ((c.launcher, c.cin, c3, c1) + tuple(c.shape) + (c.k, c.kd, c.stride, c.precision, c.io,
                                                                                                  options_text(c.options)))


def plan_input(environ):
    """What `host_asan_driver --plan` reads: the knobs to return to after every row, then the rows."""
    return "defaults %s\n" % options_text(knob_defaults(environ)) + "".join(plan_line(c) + "\n" for c in CASES)


def planner_pass(c):
    """0 / 1: the row runs under the knobs of that pass of the driver's table; None: under knobs that change the planner's answer
    (q4 = 2, bf16_debug, dual_bwd_data = 0, ...) and therefore says nothing about either pass."""
    forcing = {k: v for k, v in c.options.items() if k in ("mfma_min_cout", "bwd_weight_mfma_min_cout", "fewco_mfma", "q4", "bf16_debug", "splitk",
                                                           "dual_bwd_data")}
    return 0 if not forcing else 1 if forcing == PASS1 else None
