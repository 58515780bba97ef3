// Host-side interface of the unified pre-split contraction kernel (pp_gemm_u.hip), used by the dispatch in pp_gemm.hip.
#ifndef PP_GEMM_U_H
#define PP_GEMM_U_H
#include <hip/hip_runtime.h>
#include "../../include/picopose_hip.h"

// block tiles the kernel is instantiated for
enum { PP_U_128x64 = 0, PP_U_128x128 = 1, PP_U_256x128 = 2, PP_U_256x256 = 3, PP_F_256x192 = 4 /* fp32 engine only */,
       PP_U_256x192 = 5 /* pre-split engine: vector epilogue, modes 0 - 2 */ };

// A-delivery mode the kernel will use for this problem: 0 dense, 1 convolution in channel-slice-major K order, 2 natural order
int pp_gemm_u_mode(const PpGemmDesc& d, int terms);
// Launch on `st`: d.A_hl / d.B_hl (+ a_hl_bytes / b_hl_bytes) in the operand format hl (t2) or h (t1), persistent over
// min(tiles, slots) workgroups, on the tile, mode and epilogue (vec) pp_gemm.hip gemm_plan chose.  Returns PP_OK / PP_E*.
int pp_gemm_u_launch_t1(const PpGemmDesc& d, int tile, int mode, bool vec, int cus, hipStream_t st);
int pp_gemm_u_launch_t2(const PpGemmDesc& d, int tile, int mode, bool vec, int cus, hipStream_t st);
// 3x3 / stride 1 / pad 1 convolutions on the 256x256 tile with row-shared A delivery (see pp_gemm_u.hip); shape test + launch
bool pp_gemm_uh_shape_ok(const PpGemmDesc& d, int terms);
bool pp_gemm_u_vec_ok(const PpGemmDesc& d);
// epilogue kind (PP_EPI_*, pp_gemm_dev.h) of a vector-epilogue launch; the dense launches of the 256-wide hl tiles use it
int pp_gemm_epi_kind(const PpGemmDesc& d);
int pp_gemm_uh_launch(const PpGemmDesc& d, int terms, int cus, hipStream_t st);
// The fp32-operand engine (pp_gemm_f.hip: LDS-DMA ring + v_mfma_f32_32x32x2_f32, the same tile ids): eligibility test, A-delivery
// mode (0 dense, 1 / 2 convolution) and launch on exactly `tile` in `mode` (mode 2 has no 256x256 instantiation: gemm_plan)
bool pp_gemm_f_ok(const PpGemmDesc& d);
int pp_gemm_f_mode(const PpGemmDesc& d);
int pp_gemm_f_launch(const PpGemmDesc& d, int tile, int mode, int cus, hipStream_t st);

// Bytes of the A / B buffers a launch reads at eb bytes per element (the operand extents a_hl_bytes / b_hl_bytes: the engines'
// buffer loads take 32-bit byte offsets): a convolution's input images, not its im2col; a grouped batch's weights of every group.
static inline void pp_gemm_extents(const PpGemmDesc& d, int eb, long long& a, long long& b) {
    const long long per = (long long)d.conv_ho * d.conv_wo;
    a = eb * (d.conv_kh != 0 ? ((d.M + per - 1) / per - 1) * d.conv_bstride + (long long)d.conv_h * d.conv_w * d.lda : (long long)(d.M - 1) * d.lda + d.K);
    b = eb * ((long long)(d.N - 1) * d.ldb + d.K + (d.grp_rows != 0 ? (long long)(d.M / d.grp_rows - 1) * d.b_bs0 : 0));
}
#endif
