"""Sanitized host build: csrc/ compiled host-only with -fsanitize=address,undefined + tests/host_asan/driver.cpp.
CPU only — GPU AddressSanitizer is not available (and not wanted) on the GPU pool."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "deep_prior_interpolation_amd", "csrc")
EXE = os.path.join(CSRC, "build_asan", "host_asan_driver")
ENV = dict(ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1", HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
needs_hipcc = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs the ROCm compiler")

# `host_asan_driver --dump`: "pass<n> <launcher> [<kernel family the failed launch names, or the error text>]" -> count, the number of table
# lines and the FNV-1a digest of the table.  pass0 = the library's defaults, pass1 = fp32 MFMA, few-output-channel and q4 families off.
PLANNER_LINES = 63666
PLANNER_DIGEST = "13856febc2e2c1fd"
PLANNER_COUNTS = {
    "pass0 bwd_data [conv: 1x1 convolution supports stride 1 only]": 855,
    "pass0 bwd_data [conv_bwd_data_s2]": 117,
    "pass0 bwd_data [conv_bwd_data_s2_mfma]": 630,
    "pass0 bwd_data [conv_direct]": 67,
    "pass0 bwd_data [conv_mfma]": 404,
    "pass0 bwd_data [conv_pw]": 135,
    "pass0 bwd_data [conv_pw_mfma]": 720,
    "pass0 bwd_data [conv_q4_mfma]": 32,
    "pass0 bwd_data [packed-weight scratch]": 460,
    "pass0 bwd_data_dual [conv_mfma]": 311,
    "pass0 bwd_data_dual [conv_pw]": 104,
    "pass0 bwd_data_dual [conv_pw_mfma]": 217,
    "pass0 bwd_data_dual [packed-weight scratch]": 223,
    "pass0 bwd_data_ws [conv_mfma (split)]": 50,
    "pass0 bwd_weight [conv: 1x1 convolution supports stride 1 only]": 855,
    "pass0 bwd_weight [conv_bf16_bwd_weight]": 270,
    "pass0 bwd_weight [conv_bf16_bww_s2]": 95,
    "pass0 bwd_weight [conv_bwd_weight]": 571,
    "pass0 bwd_weight [conv_bwd_weight_mfma]": 971,
    "pass0 bwd_weight [conv_bwd_weight_smallco]": 28,
    "pass0 bwd_weight [conv_pw_bwd_weight_mfma]": 630,
    "pass0 bwd_weight_chained [conv: 1x1 convolution supports stride 1 only]": 855,
    "pass0 bwd_weight_chained [conv_bf16_bwd_weight]": 270,
    "pass0 bwd_weight_chained [conv_bwd_weight]": 693,
    "pass0 bwd_weight_chained [conv_bwd_weight_mfma]": 917,
    "pass0 bwd_weight_chained [conv_bwd_weight_smallco]": 55,
    "pass0 bwd_weight_chained [conv_pw_bwd_weight_mfma]": 630,
    "pass0 bwd_weight_unaligned [conv: 1x1 convolution supports stride 1 only]": 855,
    "pass0 bwd_weight_unaligned [conv_bwd_weight]": 687,
    "pass0 bwd_weight_unaligned [conv_bwd_weight_mfma]": 1209,
    "pass0 bwd_weight_unaligned [conv_bwd_weight_smallco]": 39,
    "pass0 bwd_weight_unaligned [conv_pw_bwd_weight_mfma]": 630,
    "pass0 fwd [conv: 1x1 convolution supports stride 1 only]": 855,
    "pass0 fwd [conv_direct]": 280,
    "pass0 fwd [conv_fewco_mfma]": 12,
    "pass0 fwd [conv_mfma]": 858,
    "pass0 fwd [conv_pw]": 225,
    "pass0 fwd [conv_pw_mfma]": 630,
    "pass0 fwd [conv_q4_mfma]": 64,
    "pass0 fwd [packed-weight scratch]": 496,
    "pass0 fwd_ws [conv_mfma (split)]": 346,
    "pass1 bwd_data [conv: 1x1 convolution supports stride 1 only]": 855,
    "pass1 bwd_data [conv_bwd_data_s2]": 747,
    "pass1 bwd_data [conv_direct]": 503,
    "pass1 bwd_data [conv_pw]": 855,
    "pass1 bwd_data [packed-weight scratch]": 460,
    "pass1 bwd_data_dual [conv_pw]": 632,
    "pass1 bwd_data_dual [packed-weight scratch]": 223,
    "pass1 bwd_weight [conv: 1x1 convolution supports stride 1 only]": 855,
    "pass1 bwd_weight [conv_bf16_bwd_weight]": 270,
    "pass1 bwd_weight [conv_bf16_bww_s2]": 95,
    "pass1 bwd_weight [conv_bwd_weight]": 2019,
    "pass1 bwd_weight [conv_bwd_weight_mfma]": 153,
    "pass1 bwd_weight [conv_bwd_weight_smallco]": 28,
    "pass1 bwd_weight_chained [conv: 1x1 convolution supports stride 1 only]": 855,
    "pass1 bwd_weight_chained [conv_bf16_bwd_weight]": 270,
    "pass1 bwd_weight_chained [conv_bwd_weight]": 2240,
    "pass1 bwd_weight_chained [conv_bwd_weight_smallco]": 55,
    "pass1 bwd_weight_unaligned [conv: 1x1 convolution supports stride 1 only]": 855,
    "pass1 bwd_weight_unaligned [conv_bwd_weight]": 2331,
    "pass1 bwd_weight_unaligned [conv_bwd_weight_mfma]": 195,
    "pass1 bwd_weight_unaligned [conv_bwd_weight_smallco]": 39,
    "pass1 fwd [conv: 1x1 convolution supports stride 1 only]": 855,
    "pass1 fwd [conv_direct]": 1214,
    "pass1 fwd [conv_pw]": 855,
    "pass1 fwd [packed-weight scratch]": 496,
}


@needs_hipcc
def test_host_logic_under_asan_and_ubsan():
    """Descriptor validation, launch planning and workspace sizing of every conv entry point over ~3400 edge-case descriptors
    (bench patch, field-scale patch, 2^29-voxel limit, degenerate sizes, stale layouts), with AddressSanitizer and
    UndefinedBehaviorSanitizer (signed overflow in the 32-bit narrowing arithmetic, out-of-bounds table reads) active."""
    subprocess.check_call(["make", "-C", CSRC, "-j4", "asan"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=900)
    exe = os.path.join(CSRC, "build_asan", "host_asan_driver")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1",
                                HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES=""))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "0 failures" in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr


@needs_hipcc
def test_planner_table_is_pinned():
    """Which kernel family every descriptor of the driver's grid gets (forward, backward-data, the fused pair, backward-weight with and
    without a chain / aligned tensors), the BatchNorm partial rows and the three workspace sizes: the counts per family and the digest of
    the whole table are those of the commit BEFORE the launch planners (conv_plan, bw_plan) were introduced, so the planners provably
    choose and size as the hand-copied chains did.  A host without a device fails every planned launch in dpi_check_launch, and the error
    text names the family.

    When a later change alters a choice or a size ON PURPOSE: build the sanitizer driver (`make -C deep_prior_interpolation_amd/csrc
    asan`), run `HIP_VISIBLE_DEVICES= ROCR_VISIBLE_DEVICES= build_asan/host_asan_driver --dump` with no DPI_* variable set, diff the table
    against the one of the parent commit (its csrc/ objects link with this driver.cpp too: only the public ABI and the hidden setters are
    used) to see that exactly the intended lines moved, then copy the `count`, `lines` and `digest` lines at its end into the constants
    above."""
    subprocess.check_call(["make", "-C", CSRC, "-j4", "asan"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=900)
    env = {k: v for k, v in os.environ.items() if not k.startswith("DPI_")}      # the getenv knobs of the planners stay at their defaults
    r = subprocess.run([EXE, "--dump"], capture_output=True, text=True, timeout=300, env=dict(env, **ENV))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    tail = [ln for ln in r.stdout.splitlines() if ln.startswith(("count ", "lines ", "digest "))]
    counts = {ln[6:].rsplit(" ", 1)[0]: int(ln.rsplit(" ", 1)[1]) for ln in tail if ln.startswith("count ")}
    assert counts == PLANNER_COUNTS, sorted(set(counts.items()) ^ set(PLANNER_COUNTS.items()))
    assert "lines %d" % PLANNER_LINES in tail
    assert "digest " + PLANNER_DIGEST in tail


@needs_hipcc
def test_contract_cases_cover_the_planner():
    """tests/conv_contract_cases.py — the rows tests/test_gpu_conv_contract.py launches on a device — against the planner itself
    (`host_asan_driver --plan`: each row's family as the failed launch names it, under the row's own knobs):
     (1) every row reaches the family the table claims for each of its launches, and the row ids are unique;
     (2) every kernel family of PLANNER_COUNTS — every bracketed text that names a kernel, for every launcher, in both passes — is
         reached by at least one row that runs under that pass's knobs.  Not kernels: the `conv: ...` argument errors and
         `packed-weight scratch`, which is what the bf16 stencil kernels answer without a device (the table has rows for them too).
    The driver cannot see the variants a family chooses from a pointer's address (vectorised staging, pair / float2 epilogues, the
    aligned q4 kernel, ...): the error text names the family only.  Their coverage rests on the shape conditions read from the code and
    stated next to each row of ADDRESS_CASES in the device test."""
    import collections
    import conv_contract_cases as T
    ids = [T.case_id(c) for c in T.CASES]
    assert len(set(ids)) == len(ids), [i for i, n in collections.Counter(ids).items() if n > 1]
    subprocess.check_call(["make", "-C", CSRC, "-j4", "asan"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=900)
    env = {k: v for k, v in os.environ.items() if not k.startswith("DPI_")}
    r = subprocess.run([EXE, "--plan"], input=T.plan_input(env), capture_output=True, text=True, timeout=300, env=dict(env, **ENV))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    assert "rows %d" % len(T.CASES) in r.stdout.splitlines()
    got = collections.defaultdict(dict)
    for ln in r.stdout.splitlines():
        f = ln.split(" ", 3)
        if f[0] == "plan" and f[3].startswith("["):
            got[int(f[1])][f[2]] = f[3][1:-1]
    reached = set()
    for i, c in enumerate(T.CASES):
        assert got[i] == c.reaches, (ids[i], got[i], c.reaches)
        if T.planner_pass(c) is not None:
            reached.update("pass%d %s [%s]" % (T.planner_pass(c), launch, family) for launch, family in got[i].items())
    kernels = {k for k in PLANNER_COUNTS if "[conv: " not in k and "[packed-weight scratch]" not in k}
    assert len(kernels) == 50
    assert not kernels - reached, sorted(kernels - reached)
