// Host interface between the convolution kernel files: every function that one file of csrc/ defines and another calls, declared once, under
// the file that defines it.  The dispatchers (conv_plan in conv_direct.hip, bw_plan in conv_bwd_weight.hip) call the families, and a family
// answers for its own geometry: *_usable = it can take the launch, *_stat_blocks = BatchNorm partial rows {sum, sum^2} its epilogue writes per
// channel (its spatial tiles), *_ws_floats = workspace it needs.  `flip` = backward-data of a stride-1 convolution (dy passed as x, channel roles swapped).
#pragma once
#include "common.h"

// optional second input of the MFMA stencil kernels (conv_mfma.hip, conv_bf16_mfma.hip): y += W2 * x2 through a 1x1(x1) kernel at the output positions
struct MfmaSecond { const float* x2; const float* w2; int C2; long w2_co_stride, w2_c_stride; };
// ---- conv_direct.hip ------------------------------------------------------------------------------------------------------------------
void dpi_conv_out_dims(const dpi_conv_desc* d, int* Do, int* Ho, int* Wo);
// ---- conv_mfma.hip: fp32 MFMA stencil family (k = 3, enough output channels to fill a 16-row MFMA tile) --------------------------------
int dpi_conv_mfma_stat_blocks(const dpi_conv_desc* d, bool flip);
// floats of the input-channel-split workspace (0: the launch does not split)
size_t dpi_conv_mfma_ws_floats(const dpi_conv_desc* d, bool flip);
// whether dpi_conv_mfma_run can add a 1x1x1 second input of C2 channels in the same pass (MfmaSecond)
bool dpi_conv_mfma_second_ok(const dpi_conv_desc* d, bool flip, int C2, bool have_ws);
// a launch that gets no workspace (ws = nullptr) or a second input runs unsplit
int dpi_conv_mfma_run(const dpi_conv_desc* d, const float* x, const float* chain, const float* w, const float* bias, float* y,
                      double* partials, bool flip, int accumulate, float* ws, size_t ws_floats, hipStream_t st, const MfmaSecond* sec = nullptr);
// backward-data of the stride-2 convolutions
int dpi_conv_bwd_data_s2_mfma_run(const dpi_conv_desc* d, const float* dy, const float* w, float* dx, int accumulate, hipStream_t st);
// backward-weight; sized for either orientation (the swapped one, X rows x (co, tap) columns, needs an input without a chain)
size_t dpi_conv_bwd_weight_mfma_ws_floats(const dpi_conv_desc* d);
bool dpi_conv_bwd_weight_mfma_swapped(const dpi_conv_desc* d, bool chained);
int dpi_conv_bwd_weight_mfma_run(const dpi_conv_desc* d, const float* x, const float* chain, const float* dy, float* dw, float* ws, hipStream_t st);
// few-output-channel backward-weight (3-D, stride 1, Cout <= 5)
size_t dpi_conv_bwd_weight_smallco_ws_floats(const dpi_conv_desc* d);
int dpi_conv_bwd_weight_smallco_run(const dpi_conv_desc* d, const float* x, const float* chain, const float* dy, float* dw, float* ws, hipStream_t st);
// ---- conv_pw_mfma.hip: 1x1(x1) convolution on the fp32 MFMA -----------------------------------------------------------------------------
int dpi_conv_pw_mfma_stat_blocks(const dpi_conv_desc* d);
int dpi_conv_pw_mfma_run(const dpi_conv_desc* d, const float* x, const float* chain, const float* w, const float* bias, float* y,
                         double* partials, bool flip, int accumulate, hipStream_t st);
size_t dpi_conv_pw_bwd_weight_mfma_ws_floats(const dpi_conv_desc* d);
int dpi_conv_pw_bwd_weight_mfma_run(const dpi_conv_desc* d, const float* x, const float* chain, const float* dy, float* dw, float* ws, hipStream_t st);
// ---- conv_fewco_mfma.hip: forward 3x3x3 stride 1 with <= 4 output channels, fp32 tensors ------------------------------------------------
bool dpi_conv_fewco_usable(const dpi_conv_desc* d);
int dpi_conv_fewco_stat_blocks(const dpi_conv_desc* d);
int dpi_conv_fewco_mfma_run(const dpi_conv_desc* d, const float* x, const float* chain, const float* w, const float* bias, float* y,
                            double* partials, hipStream_t st);
// ---- conv_q4_mfma.hip: 3x3x3 stride 1 with <= 8 output channels on the 4x4x1 MFMA, fp32 tensors -----------------------------------------
bool dpi_conv_q4_usable(const dpi_conv_desc* d, bool flip);
int dpi_conv_q4_stat_blocks(const dpi_conv_desc* d);
int dpi_conv_q4_run(const dpi_conv_desc* d, const float* x, const float* chain, const float* w, const float* bias, float* y,
                    double* partials, bool flip, int accumulate, hipStream_t st);
// ---- conv_bf16_mfma.hip: the bf16 arithmetic modes (precision 1 / 2) ----------------------------------------------------------------------
bool dpi_bf16_force_all();      // test switch: every shape the bf16 kernels can run, not only where they pay
// 3x3(x3) stride 1
bool dpi_conv_bf16_usable(const dpi_conv_desc* d, bool flip);
int dpi_conv_bf16_stat_blocks(const dpi_conv_desc* d);
// whether dpi_conv_bf16_run adds a 1x1x1 second input in the same pass: bf16 arithmetic mode, 3-D, backward-data
bool dpi_conv_bf16_second_ok(const dpi_conv_desc* d, bool flip);
int dpi_conv_bf16_run(const dpi_conv_desc* d, const float* x, const float* chain, const float* w, const float* bias, float* y,
                      double* partials, bool flip, int accumulate, hipStream_t st, const MfmaSecond* sec = nullptr);
// 3x3x3 stride-2 forward, bf16 x and y, bf16 arithmetic
bool dpi_conv_bf16_s2_usable(const dpi_conv_desc* d);
int dpi_conv_bf16_s2_stat_blocks(const dpi_conv_desc* d);
int dpi_conv_bf16_s2_run(const dpi_conv_desc* d, const float* x, const float* chain, const float* w, const float* bias, float* y, double* partials,
                         hipStream_t st);
// 3x3x3 stride-2 backward-data, bf16 dy and dx, bf16 arithmetic (8-byte pieces of dy, dword stores of dx: the caller checks the alignment)
bool dpi_conv_bf16_s2_bwd_usable(const dpi_conv_desc* d);
int dpi_conv_bf16_s2_bwd_run(const dpi_conv_desc* d, const float* dy, const float* w, float* dx, int accumulate, hipStream_t st);
// ---- conv_bf16_bww.hip: backward-weight of 3x3x3 stride 1 in the bf16 arithmetic modes -----------------------------------------------------
bool dpi_conv_bf16_bww_usable(const dpi_conv_desc* d);
size_t dpi_conv_bf16_bww_ws_floats(const dpi_conv_desc* d);
int dpi_conv_bf16_bww_run(const dpi_conv_desc* d, const float* x, const float* chain, const float* dy, float* dw, float* ws, hipStream_t st);
// ---- conv_bf16_bww_s2.hip: backward-weight of 3x3x3 stride 2, x and dy bf16, bf16 arithmetic, no chain --------------------------------------
bool dpi_conv_bf16_bww_s2_usable(const dpi_conv_desc* d);
size_t dpi_conv_bf16_bww_s2_ws_floats(const dpi_conv_desc* d);
int dpi_conv_bf16_bww_s2_run(const dpi_conv_desc* d, const float* x, const float* dy, float* dw, float* ws, hipStream_t st);
