// Host-side sanitizer run ("-fsanitize=address host build").  Every .cpp / .hip of csrc/ is compiled HOST-ONLY with
// -fsanitize=address,undefined (no device code, no GPU needed) and linked with this driver, which walks the host logic of the C ABI —
// descriptor validation, launch planning, workspace sizing, the 32-bit narrowing guards — over edge-case descriptors: the shapes of
// tests/test_gpu_bench_size.py (256x128x128 bench patch, the 512x256x256 field-scale patch), volumes at and beyond the 2^29-voxel
// limit of the kernels' 32-bit byte offsets, degenerate sizes, every (k, kd, stride, precision) combination, stale descriptor layouts.
// With no device present a planned launch comes back as DPI_E_LAUNCH from the HIP runtime; everything before it (the code under
// test) has run under the sanitizers.  Exit code 0 = no sanitizer report and every expectation met.
//
// `--dump` prints the planner table instead: for every descriptor of the grid the sizing queries and, for each launcher, the return
// code and the kernel family that the failed launch names (the text of dpi_last_error() up to its first colon: what follows is the HIP
// runtime's wording).  A second pass repeats the grid with the MFMA families switched off, which shows the fallback chain.  Per-family
// counts and a 64-bit digest of the whole table follow; tests/test_host_asan.py pins them.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>
#include "../../include/dpi_hip.h"
#include "../../deep_prior_interpolation_amd/csrc/dpi_hip_internal.h"

static int failures = 0;
#define EXPECT(cond, ...) do { if (!(cond)) { ++failures; std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

static dpi_conv_desc desc(int cin, int cout, int D, int H, int W, int k, int kd, int stride, int precision = 0, int io = 0) {
  dpi_conv_desc d;
  d.size = (int)sizeof(dpi_conv_desc);
  d.Cin = cin; d.Cout = cout; d.D = D; d.H = H; d.W = W; d.k = k; d.kd = kd; d.stride = stride; d.precision = precision; d.io = io;
  return d;
}

static const int channels[][2] = {{64, 4}, {4, 8}, {8, 13}, {25, 16}, {67, 4}, {25, 1}, {25, 25}, {51, 32}, {137, 8}, {105, 64}, {212, 128}, {554, 35},
                                  {142, 213}, {1, 1}, {3, 5}, {426, 554}, {64, 25}, {67, 25}, {17, 26}};
static const int shapes[][3] = {{256, 128, 128}, {512, 256, 256}, {128, 64, 64}, {64, 64, 64}, {16, 8, 8}, {4, 4, 4}, {1, 1, 1}, {2, 3, 5}, {9, 17, 33},
                                {1, 170, 100}, {1, 1, 7}, {33, 31, 50}, {1024, 1024, 256}, {8, 8, 68}, {7, 25, 60}};

// ---- --dump: the planner table ------------------------------------------------------------------------------------------------------
static uint64_t g_digest = 1469598103934665603ull;      // FNV-1a over every table line, newline included
static std::map<std::string, long> g_family;            // "pass<n> <launcher> [<text>]" -> count
static long g_lines = 0;
static void emit(const dpi_conv_desc& d, int pass, const char* what, const std::string& value) {
  char id[160];
  std::snprintf(id, sizeof(id), "pass%d %d->%d %dx%dx%d k%d kd%d s%d p%d io%d ", pass, d.Cin, d.Cout, d.D, d.H, d.W, d.k, d.kd, d.stride, d.precision, d.io);
  const std::string line = std::string(id) + what + " " + value + "\n";
  for (unsigned char c : line) { g_digest ^= c; g_digest *= 1099511628211ull; }
  std::fputs(line.c_str(), stdout);
  ++g_lines;
}
static void emit_rc(const dpi_conv_desc& d, int pass, const char* what, int rc) {
  std::string text = rc == DPI_OK ? "" : dpi_last_error();
  if (rc == DPI_E_LAUNCH) text = text.substr(0, text.find(':'));
  ++g_family["pass" + std::to_string(pass) + " " + what + " [" + text + "]"];
  emit(d, pass, what, "rc " + std::to_string(rc) + " " + text);
}
static void dump_pass(int pass, float* p) {
  long n_desc = 0;
  for (auto& ch : channels)
    for (auto& sh : shapes)
      for (int k : {1, 3})
        for (int stride : {1, 2})
          for (int prec : {0, 1, 2}) {
            const int kd = sh[0] == 1 ? 1 : k;
            const int io = (prec < 2 && ((n_desc / 3) & 1)) ? 15 : 0;
            const dpi_conv_desc d = desc(ch[0], ch[1], sh[0], sh[1], sh[2], k, kd, stride, prec, io);
            ++n_desc;
            const size_t fws = dpi_conv_fwd_ws_floats(&d), bws = dpi_conv_bwd_data_ws_floats(&d), wws = dpi_conv_bwd_weight_ws_floats(&d);
            emit(d, pass, "fwd_stat_blocks", std::to_string(dpi_conv_fwd_stat_blocks(&d)));
            emit(d, pass, "fwd_ws_floats", std::to_string(fws));
            emit(d, pass, "bwd_data_ws_floats", std::to_string(bws));
            emit(d, pass, "bwd_weight_ws_floats", std::to_string(wws));
            emit_rc(d, pass, "fwd", dpi_conv_fwd(&d, p, nullptr, p, nullptr, p, nullptr, nullptr));
            emit_rc(d, pass, "bwd_data", dpi_conv_bwd_data(&d, p, p, p, 1, nullptr));
            // with the workspace the sizing query asks for, the launches that split their input channels say so
            if (fws) emit_rc(d, pass, "fwd_ws", dpi_conv_fwd_ws(&d, p, nullptr, p, nullptr, p, nullptr, p, fws, nullptr));
            if (bws) emit_rc(d, pass, "bwd_data_ws", dpi_conv_bwd_data_ws(&d, p, p, p, 1, p, bws, nullptr));
            if (k == 3 && stride == 1) {
              const dpi_conv_desc d1 = desc(ch[0], ch[1] + 9, sh[0], sh[1], sh[2], 1, 1, 1, prec);
              emit_rc(d, pass, "bwd_data_dual", dpi_conv_bwd_data_dual(&d, p, p, &d1, p, p, p, 0, bws ? p : nullptr, bws, nullptr));
            }
            emit_rc(d, pass, "bwd_weight", dpi_conv_bwd_weight(&d, p, nullptr, p, p, p, wws, nullptr));
            // the launch-time facts the backward-weight choice depends on: a chain on x, tensors that are not 16-byte aligned
            emit_rc(d, pass, "bwd_weight_chained", dpi_conv_bwd_weight(&d, p, p, p, p, p, wws, nullptr));
            emit_rc(d, pass, "bwd_weight_unaligned", dpi_conv_bwd_weight(&d, p + 1, nullptr, p + 1, p, p, wws, nullptr));
          }
}
static int dump() {
  std::vector<float> tiny(4, 0.f);
  dump_pass(0, tiny.data());
  // the fallback chain: fp32 MFMA, few-output-channel and q4 families off (the library's defaults are restored below)
  dpi_set_mfma_min_cout(1 << 20); dpi_set_bwd_weight_mfma_min_cout(1 << 20); dpi_set_fewco_mfma(0); dpi_set_q4(0, -1);
  dump_pass(1, tiny.data());
  dpi_set_mfma_min_cout(8); dpi_set_bwd_weight_mfma_min_cout(8); dpi_set_fewco_mfma(1); dpi_set_q4(1, -1);
  for (const auto& kv : g_family) std::printf("count %s %ld\n", kv.first.c_str(), kv.second);
  std::printf("lines %ld\ndigest %016llx\n", g_lines, (unsigned long long)g_digest);
  return 0;
}

// ---- --plan: the planner's answers for descriptor rows read from stdin -----------------------------------------------------------------
// One row per line (tests/conv_contract_cases.py writes them):
//   <launcher> <Cin> <Cout> <C1> <D> <H> <W> <k> <kd> <stride> <precision> <io> <key>=<value>,... | -
// launcher = fwd | bwd_data | bwd_data_dual | bwd_weight; C1 = output channels of the 1x1(x1) layer of bwd_data_dual (0 elsewhere); the
// last field lists dpi_set_option keys that hold for this row only (they reach the hidden setters through dpi_set_option's table; the
// library's defaults are restored after the row).  Printed per row: "plan <row> <what> <value>" with the three size queries and, for every
// launch the launcher's device test makes, "<launch> [<family>]" — the family exactly as emit_rc derives it.
// The first line, "defaults <key>=<value>,...", names the knobs the library starts with (tests/conv_contract_cases.py holds them).
// Applies such a list; returns the token that dpi_set_option refused, or nullptr.
static const char* set_options(const std::string& list) {
  static std::string bad;
  if (list == "-") return nullptr;
  for (size_t at = 0; at < list.size();) {
    const size_t end = std::min(list.find(',', at), list.size()), eq = list.find('=', at);
    bad = list.substr(at, end - at);
    if (eq == std::string::npos || eq >= end) return bad.c_str();
    if (dpi_set_option(list.substr(at, eq - at).c_str(), std::atoi(list.c_str() + eq + 1)) != DPI_OK) return bad.c_str();
    at = end + 1;
  }
  return nullptr;
}
static std::string family_of(int rc) {
  std::string text = rc == DPI_OK ? "" : dpi_last_error();
  if (rc == DPI_E_LAUNCH) text = text.substr(0, text.find(':'));
  return "[" + text + "]";
}
static int plan() {
  std::vector<float> tiny(4, 0.f);
  float* p = tiny.data();
  char line[1024], defaults[768];
  if (!std::fgets(line, sizeof(line), stdin) || std::sscanf(line, "defaults %767s", defaults) != 1 || set_options(defaults)) {
    std::printf("plan error: the first line must be 'defaults <key>=<value>,...'\n");
    return 2;
  }
  long row = 0;
  for (; std::fgets(line, sizeof(line), stdin); ++row) {
    char launcher[32], opts[768];
    int cin, cout, c1, D, H, W, k, kd, stride, prec, io;
    if (std::sscanf(line, "%31s %d %d %d %d %d %d %d %d %d %d %d %767s", launcher, &cin, &cout, &c1, &D, &H, &W, &k, &kd, &stride, &prec, &io, opts) != 13) {
      std::printf("plan %ld error malformed row\n", row);
      return 2;
    }
    if (const char* bad = set_options(opts)) { std::printf("plan %ld error bad option %s\n", row, bad); return 2; }
    const dpi_conv_desc d = desc(cin, cout, D, H, W, k, kd, stride, prec, io);
    const size_t fws = dpi_conv_fwd_ws_floats(&d), bws = dpi_conv_bwd_data_ws_floats(&d), wws = dpi_conv_bwd_weight_ws_floats(&d);
    std::printf("plan %ld fwd_stat_blocks %d\nplan %ld fwd_ws_floats %zu\nplan %ld bwd_data_ws_floats %zu\nplan %ld bwd_weight_ws_floats %zu\n",
                row, dpi_conv_fwd_stat_blocks(&d), row, fws, row, bws, row, wws);
    const std::string what = launcher;
    if (what == "fwd") {
      std::printf("plan %ld fwd %s\n", row, family_of(dpi_conv_fwd(&d, p, nullptr, p, nullptr, p, nullptr, nullptr)).c_str());
      if (fws) std::printf("plan %ld fwd_ws %s\n", row, family_of(dpi_conv_fwd_ws(&d, p, nullptr, p, nullptr, p, nullptr, p, fws, nullptr)).c_str());
    } else if (what == "bwd_data") {
      std::printf("plan %ld bwd_data %s\n", row, family_of(dpi_conv_bwd_data(&d, p, p, p, 1, nullptr)).c_str());
      if (bws) std::printf("plan %ld bwd_data_ws %s\n", row, family_of(dpi_conv_bwd_data_ws(&d, p, p, p, 1, p, bws, nullptr)).c_str());
    } else if (what == "bwd_data_dual") {
      const dpi_conv_desc d1 = desc(cin, c1, D, H, W, 1, 1, 1, prec, io);
      std::printf("plan %ld bwd_data_dual %s\n", row, family_of(dpi_conv_bwd_data_dual(&d, p, p, &d1, p, p, p, 0, bws ? p : nullptr, bws, nullptr)).c_str());
    } else if (what == "bwd_weight") {
      std::printf("plan %ld bwd_weight %s\n", row, family_of(dpi_conv_bwd_weight(&d, p, nullptr, p, p, p, wws, nullptr)).c_str());
      std::printf("plan %ld bwd_weight_chained %s\n", row, family_of(dpi_conv_bwd_weight(&d, p, p, p, p, p, wws, nullptr)).c_str());
      std::printf("plan %ld bwd_weight_unaligned %s\n", row, family_of(dpi_conv_bwd_weight(&d, p + 1, nullptr, p + 1, p, p, wws, nullptr)).c_str());
    } else {
      std::printf("plan %ld error unknown launcher %s\n", row, launcher);
      return 2;
    }
    set_options(defaults);
  }
  std::printf("rows %ld\n", row);
  return 0;
}

int main(int argc, char** argv) {
  if (argc > 1 && std::strcmp(argv[1], "--dump") == 0) return dump();
  if (argc > 1 && std::strcmp(argv[1], "--plan") == 0) return plan();
  EXPECT(dpi_version() >= 400, "version %d", dpi_version());
  EXPECT(dpi_conv_desc_size() == (int)sizeof(dpi_conv_desc), "desc size");
  // a buffer that is big enough for the few bytes host code may legitimately read from "device" pointers: none — host code must never
  // dereference them, ASAN would flag reads of this 16-byte allocation past its end
  std::vector<float> tiny(4, 0.f);
  float* p = tiny.data();
  long n_desc = 0, n_planned = 0, n_split = 0;
  for (auto& ch : channels)
    for (auto& sh : shapes)
      for (int k : {1, 3})
        for (int stride : {1, 2})
          for (int prec : {0, 1, 2}) {
            const int kd = sh[0] == 1 ? 1 : k;
            // storage types (ABI 400): fp32 everywhere, and for the fp32 / bf16 arithmetic modes bf16 activations + gradients
            // (the planners pick other kernels then: no 4x4x1 / pair kernels, the bf16 kernel on every big-tile shape)
            const int io = (prec < 2 && ((n_desc / 3) & 1)) ? 15 : 0;
            dpi_conv_desc d = desc(ch[0], ch[1], sh[0], sh[1], sh[2], k, kd, stride, prec, io);
            ++n_desc;
            const bool valid = !(k == 1 && stride == 2);
            const int nblk = dpi_conv_fwd_stat_blocks(&d);
            const size_t ws = dpi_conv_bwd_weight_ws_floats(&d);
            if (!valid) { EXPECT(nblk == 0 && ws == 0, "invalid desc must plan nothing (k1 s2)"); continue; }
            EXPECT(nblk > 0, "stat blocks %d for %d->%d %dx%dx%d k%d s%d p%d", nblk, ch[0], ch[1], sh[0], sh[1], sh[2], k, stride, prec);
            EXPECT(ws > 0 && ws < ((size_t)1 << 34), "bwd-weight workspace %zu floats for %d->%d %dx%dx%d k%d s%d p%d", ws, ch[0], ch[1], sh[0], sh[1], sh[2], k, stride, prec);
            // the launchers: planning runs, the launch itself fails without a device (or succeeds on a GPU box: both fine here)
            int rc = dpi_conv_fwd(&d, p, nullptr, p, nullptr, p, nullptr, nullptr);
            EXPECT(rc == DPI_OK || rc == DPI_E_LAUNCH, "conv_fwd rc %d: %s", rc, dpi_last_error());
            rc = dpi_conv_bwd_data(&d, p, p, p, 1, nullptr);
            EXPECT(rc == DPI_OK || rc == DPI_E_LAUNCH, "conv_bwd_data rc %d: %s", rc, dpi_last_error());
            // input-channel split (ABI 301): sizing, the split launch planning, a short workspace refused before any launch
            const size_t fws = dpi_conv_fwd_ws_floats(&d), bws = dpi_conv_bwd_data_ws_floats(&d);
            EXPECT(fws < ((size_t)1 << 32) && bws < ((size_t)1 << 32), "split workspace %zu / %zu floats", fws, bws);
            if (fws) {
              ++n_split;
              rc = dpi_conv_fwd_ws(&d, p, nullptr, p, p, p, nullptr, p, fws, nullptr);
              EXPECT(rc == DPI_OK || rc == DPI_E_LAUNCH, "conv_fwd_ws rc %d: %s", rc, dpi_last_error());
              rc = dpi_conv_fwd_ws(&d, p, nullptr, p, p, p, nullptr, p, fws / 2, nullptr);
              EXPECT(rc == DPI_E_ARG || rc == DPI_E_WORKSPACE, "short split workspace accepted (rc %d)", rc);
            }
            if (bws) {
              rc = dpi_conv_bwd_data_ws(&d, p, p, p, 1, p, bws, nullptr);
              EXPECT(rc == DPI_OK || rc == DPI_E_LAUNCH, "conv_bwd_data_ws rc %d: %s", rc, dpi_last_error());
            }
            EXPECT(dpi_conv_fwd_ws(&d, p, nullptr, p, p, p, nullptr, nullptr, 16, nullptr) == DPI_E_ARG, "workspace size without a workspace accepted");
            if (k == 3 && stride == 1) {      // the 3x3(x3) + 1x1(x1) pair that reads one tensor: fused or two launches, both plan here
              dpi_conv_desc d1 = desc(ch[0], ch[1] + 9, sh[0], sh[1], sh[2], 1, 1, 1, prec);
              rc = dpi_conv_bwd_data_dual(&d, p, p, &d1, p, p, p, 0, bws ? p : nullptr, bws, nullptr);
              EXPECT(rc == DPI_OK || rc == DPI_E_LAUNCH, "conv_bwd_data_dual rc %d: %s", rc, dpi_last_error());
              dpi_conv_desc dbad = desc(ch[0] + 1, ch[1], sh[0], sh[1], sh[2], 1, 1, 1, prec);
              EXPECT(dpi_conv_bwd_data_dual(&d, p, p, &dbad, p, p, p, 0, nullptr, 0, nullptr) == DPI_E_ARG, "dual: mismatched layers accepted");
            }
            rc = dpi_conv_bwd_weight(&d, p, nullptr, p, p, p, ws, nullptr);
            EXPECT(rc == DPI_OK || rc == DPI_E_LAUNCH, "conv_bwd_weight rc %d: %s", rc, dpi_last_error());
            rc = dpi_conv_bwd_weight(&d, p, nullptr, p, p, p, ws / 2, nullptr);       // short workspace must be refused before any launch
            EXPECT(ws < 2 || rc == DPI_E_WORKSPACE, "short workspace accepted (rc %d)", rc);
            ++n_planned;
          }
  // the 32-bit byte-offset limit of the stencil kernels: 2^29 voxels per channel
  {
    dpi_conv_desc d = desc(4, 4, 1024, 1024, 512, 3, 3, 1);
    EXPECT(dpi_conv_fwd(&d, p, nullptr, p, nullptr, p, nullptr, nullptr) == DPI_E_ARG, "2^29-voxel patch must be refused");
    d = desc(4, 4, 2047, 2047, 2047, 3, 3, 1);
    EXPECT(dpi_conv_fwd_stat_blocks(&d) == 0 && dpi_conv_bwd_weight_ws_floats(&d) == 0, "8.6e9-voxel patch must be refused");
    d = desc(4, 4, 1023, 1024, 512, 3, 3, 1);
    EXPECT(dpi_conv_fwd_stat_blocks(&d) > 0, "just below the limit must plan");
  }
  // malformed descriptors
  {
    dpi_conv_desc d = desc(4, 4, 8, 8, 8, 3, 3, 1);
    d.size = 36;
    EXPECT(dpi_conv_fwd(&d, p, nullptr, p, nullptr, p, nullptr, nullptr) == DPI_E_ARG && std::strstr(dpi_last_error(), "size"), "stale size field");
    EXPECT(dpi_conv_bwd_weight_ws_floats(&d) == 0, "stale size field must size nothing");
    for (int bad = 0; bad < 8; ++bad) {
      d = desc(4, 4, 8, 8, 8, 3, 3, 1);
      switch (bad) {
        case 0: d.Cin = 0; break; case 1: d.Cout = -1; break; case 2: d.k = 5; break; case 3: d.kd = 2; break; case 4: d.stride = 3; break;
        case 5: d.precision = 7; break; case 6: d.W = 0; break; case 7: d.kd = 1; break;      /* 2-D kernel on D = 8 */
      }
      EXPECT(dpi_conv_fwd(&d, p, nullptr, p, nullptr, p, nullptr, nullptr) == DPI_E_ARG, "bad descriptor %d accepted", bad);
      EXPECT(dpi_conv_bwd_data(&d, p, p, p, 0, nullptr) == DPI_E_ARG, "bad descriptor %d accepted by bwd_data", bad);
      EXPECT(dpi_conv_bwd_weight(&d, p, nullptr, p, p, p, 1 << 20, nullptr) == DPI_E_ARG, "bad descriptor %d accepted by bwd_weight", bad);
    }
    EXPECT(dpi_conv_fwd(nullptr, p, nullptr, p, nullptr, p, nullptr, nullptr) == DPI_E_ARG, "null descriptor");
    d = desc(4, 4, 8, 8, 8, 3, 3, 1);
    EXPECT(dpi_conv_fwd(&d, nullptr, nullptr, p, nullptr, p, nullptr, nullptr) == DPI_E_ARG, "null tensor");
  }
  // the other sizing functions: monotone, non-zero, no overflow at field scale
  {
    const size_t Vs[] = {1, 63, 64, 65, 1u << 20, (size_t)256 * 128 * 128, (size_t)512 * 256 * 256, (size_t)1 << 31, ((size_t)1 << 33) + 5};
    for (size_t V : Vs) {
      for (int C : {1, 4, 25, 67, 554}) EXPECT(dpi_stat_blocks(C, V) >= 1, "stat_blocks(%d, %zu)", C, V);
      EXPECT(dpi_loss_ws_doubles(V) >= 8, "loss ws %zu", V);
      EXPECT(dpi_max_ws_floats(V) >= 1, "max ws %zu", V);
    }
    EXPECT(dpi_upsample2x_bwd_ws_floats(426, 16, 8, 8, 32, 16, 16, 1) > 0, "upsample ws");
    EXPECT(dpi_upsample2x_bwd_ws_floats(51, 128, 64, 64, 256, 128, 128, 1) > 0, "upsample ws full size");
    EXPECT(dpi_upsample2x_bwd_ws_floats(51, 128, 64, 64, 255, 127, 127, 1) > 0, "upsample ws cropped");
  }
  EXPECT(n_split > 0, "no descriptor exercised the input-channel split");
  std::printf("host sanitizer driver: %ld descriptors, %ld planned launch triples (%ld with an input-channel split), %d failures\n", n_desc, n_planned, n_split, failures);
  return failures ? 1 : 0;
}
