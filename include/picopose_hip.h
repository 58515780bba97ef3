/*
 * picopose_hip.h — C ABI of libpicopose_hip.so (gfx950 / MI355X).
 *
 * This is the drop-in boundary of the PicoPose correspondence hot path.  The
 * reference (foollh/PicoPose) is pure Python and has no FFI of its own; every
 * entry point below replaces the stock-torch arithmetic of one reference
 * function (cited as file:line relative to the reference tree) and is bound
 * from Python with ctypes (picopose_amd/_lib.py).  INTEGRATION.md shows the
 * binding a maintainer of the reference would add.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer (tensor.data_ptr()), fp32 unless the
 *     name says otherwise, dense row-major in the layout given per argument;
 *   - the caller owns all buffers (inputs, outputs, workspace); inputs are
 *     never written;
 *   - work is enqueued on `stream` (a hipStream_t passed as void*) and the
 *     call returns without synchronising;
 *   - return value: PP_OK (0) or a negative PP_E* code; nothing throws across
 *     the ABI.  pp_strerror() maps a code to text.
 */
#ifndef PICOPOSE_HIP_H
#define PICOPOSE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PP_OK 0
#define PP_EINVAL (-1)     /* unsupported shape / null pointer / bad mode      */
#define PP_EWORKSPACE (-2) /* workspace too small or misaligned (256 B)        */
#define PP_ELAUNCH (-3)    /* hipGetLastError() != hipSuccess after a launch   */

/* arithmetic used for the 256x256xC similarity contraction of stage 1 */
#define PP_MATCH_EXACT 0 /* v_mfma_f32_32x32x2_f32: bit-for-bit an fp32 fma chain */
#define PP_MATCH_FAST 1  /* v_mfma_f32_32x32x16_f16 + exact fp32 re-evaluation of  \
                            every row/column whose index-0 decision is within eps */

const char* pp_strerror(int code);
int pp_version(void);

/* Measurement hooks (bench.py): after pp_prof_enable(n) every call that launches a
 * roofline kernel (stage 1: the fused similarity kernel) brackets exactly that launch with
 * two hipEvents on the caller's stream, up to n records; pp_prof_collect waits for them and
 * returns the durations in ms.  pp_prof_enable(0) switches the hooks off. */
int pp_prof_enable(int max_records);
int pp_prof_collect(float* out_ms, int max_out, int* count);
/* The same for the contraction engine: after pp_prof_gemm_enable(n) every pp_gemm launch (up to n; the
 * autotuner's trial launches excluded) is bracketed by two hipEvents on its stream and its 2*M*N*K*batch flop
 * count is kept.  pp_prof_gemm_collect sums durations (ms), flops and launches into 2-element arrays:
 * [0] = launches of the pre-split f16x3 kernel (the dominant kernel of the full path), [1] = all other
 * GEMM kernels.  pp_prof_gemm_enable(0) switches the hooks off. */
int pp_prof_gemm_enable(int max_records);
int pp_prof_gemm_collect(double* ms, double* flops, int* launches);
/* Per-launch view of the same records (call BEFORE pp_prof_gemm_collect, which resets them): for record i < *count,
 * shape[6 i ..] = {M, N, K, conv kernel size (0: dense), tile configuration the launch used (PP_GEMM_FORCE_CFG numbering, as
 * resolved by the one launch plan of csrc/pp_gemm.hip gemm_plan: what ran, not what was requested),
 * kind (0 = both operands pre-split, 1 = other)}, ms[i] its duration, flops[i] = 2 M N K batch. */
int pp_prof_gemm_records(int max_records, int* shape, float* ms, double* flops, int* count);
/* The same with 8 ints per record — shape[8 i ..] = {M, N, K, conv kernel size, cfg, kind, A-delivery mode of the pre-split kernel
 * (0 dense, 1 convolution in channel-slice-major K order, 2 natural order), 0} — plus bytes[i] = the launch's ALGORITHMIC bytes: every element of A (a convolution: of its input image, not of the im2col),
 * B, the output(s) and the residual(s) once, in the format the launch reads / writes them (4 B fp32; 4 B per element of a 2-term
 * operand, 2 B of a 1-term one) — what a per-kernel traffic ratio (PMC FETCH + WRITE over this) is taken against. */
int pp_prof_gemm_records2(int max_records, int* shape, float* ms, double* flops, double* bytes, int* count);
/* The contraction engine's autotuner (pp_gemm: per problem shape the fastest tile configuration, measured once per process) as a
 * table that can be written and read back, so that separate processes — the passes of one profiling set, a serving fleet — run the
 * SAME configuration per shape: pp_gemm_tune_save writes "key cfg" lines and returns the entry count, pp_gemm_tune_load merges a
 * file into the table (shapes it lacks are still tuned on first use) and returns the entries read (PP_EINVAL: unreadable);
 * the environment variable PP_GEMM_TUNE_FILE loads a file before the first pp_gemm call.  Results do not depend on the table
 * (every configuration accumulates in the same order), only speed does. */
int pp_gemm_tune_save(const char* path);
int pp_gemm_tune_load(const char* path);
int pp_gemm_tune_entries(void);
/* The pre-split kernel's epilogue has straight-line bodies for the flag sets of the hot dense launches (the qkv / fc1 / proj / fc2
 * linears, the Winograd products) next to one generic body that reads every flag at run time; both give the same bits.
 * pp_gemm_generic_epilogue(1) makes every later launch of the process take the generic body, (0) restores the default.
 * Returns the previous setting, PP_EINVAL for any other argument.  For tests and A/B timing. */
int pp_gemm_generic_epilogue(int on);

/* ------------------------------------------------------------------------- *
 * Stage 1: template matching — utils/matching.py:29-69 (matching_templates)
 * called from model/picopose.py:102-104.
 *
 *   bank   (B,N,C,16,16)  template patch features (un-normalised is fine)
 *   query  (B,C,16,16)    query patch features
 *   mask   (B,mh,mw)      query mask; sampled nearest to 16x16 exactly as
 *                         F.interpolate(mask, size=(16,16)) does
 *   sim_avg (B,N)         out: masked mean of the best-match scores
 *
 * pp_stage1_scores computes sim_avg (matching.py:38-66); pp_topk performs
 * torch.topk(sim_avg, k, dim=1) (matching.py:68) with ties broken toward the
 * lower template id; pp_stage1_match is scores followed by topk.
 * `eps` is the half-width of the fast mode's re-evaluation band (ignored in
 * exact mode; <=0 selects the default 2e-4).
 * stats (optional, may be NULL): device int32[4] = {rows re-evaluated on their
 * candidate columns, rows re-evaluated in full, columns re-evaluated, 0}.
 * ------------------------------------------------------------------------- */
int pp_stage1_workspace_bytes(int B, int N, int C, size_t* bytes);

int pp_stage1_scores(const float* bank, const float* query, const float* mask,
                     int mask_h, int mask_w, int B, int N, int C, int mode,
                     float eps, void* workspace, size_t workspace_bytes,
                     float* sim_avg, int32_t* stats, void* stream);

/* The same with the bank's storage type as an argument (BASELINE configs[4]: a template bank kept in half precision —
 * half the HBM bytes per template).  bank_dtype = PP_BANK_F32: bank is float (B,N,C,16,16), exactly pp_stage1_scores;
 * PP_BANK_F16: bank is IEEE half (B,N,C,16,16) and the result is what pp_stage1_scores returns on those values
 * widened to float (the rounding to half happened when the bank was stored, outside this library). */
#define PP_BANK_F32 0
#define PP_BANK_F16 1
int pp_stage1_scores_ex(const void* bank, int bank_dtype, const float* query, const float* mask,
                        int mask_h, int mask_w, int B, int N, int C, int mode,
                        float eps, void* workspace, size_t workspace_bytes,
                        float* sim_avg, int32_t* stats, void* stream);

int pp_topk(const float* scores, int B, int N, int k, float* out_score,
            int64_t* out_index, void* stream);

int pp_stage1_match(const float* bank, const float* query, const float* mask,
                    int mask_h, int mask_w, int B, int N, int C, int k, int mode,
                    float eps, void* workspace, size_t workspace_bytes,
                    float* sim_avg, float* out_score, int64_t* out_index,
                    int32_t* stats, void* stream);
/* pp_stage1_match with the bank's storage type as an argument: one ABI call for scores + top-k (the host mirror's
 * matching_templates).  With fewer than two (crop, template) items per CU the main kernel runs its 4-wave shape on template
 * halves (shorter tail round: BASELINE configs[1] 73.2 -> 68.7 us per call).  Three launch fusions were built, measured SLOWER at
 * configs[1] and are off by default (profiles/r04/stage1_small.txt): PP_S1_QPREP=1 (query pre-pack as one launch),
 * PP_S1_TOPK_SMALL=1 (one wave per crop), PP_S1_FUSE_TOPK=1 (the last resolve workgroup of a crop ranks its scores through an
 * agent-scope arrival counter).  Same results as pp_stage1_scores_ex + pp_topk, bit for bit, in every form. */
int pp_stage1_match_ex(const void* bank, int bank_dtype, const float* query, const float* mask,
                       int mask_h, int mask_w, int B, int N, int C, int k, int mode,
                       float eps, void* workspace, size_t workspace_bytes, float* sim_avg,
                       float* out_score, int64_t* out_index, int32_t* stats, void* stream);

/* Indexed bank: the evaluator's per-object template bank without a per-crop copy.  run_test.py:159-162 hands every detection
 * its own copy of the bank, templates_data[key][obj_idx]; here
 *   bank      (n_obj,N,C,16,16)  per-object banks, float or half (bank_dtype as in pp_stage1_scores_ex)
 *   obj_index (B,)               device int64: crop b is matched against bank[obj_index[b]]
 * and everything else is as in pp_stage1_scores_ex / pp_stage1_match_ex (utils/matching.py:29-69).  The results are those of
 * the _ex entries on the gathered bank bank[obj_index], bit for bit, in both modes and for both bank types.  The crops are
 * grouped by object on the device and the crops of one object stream each of its templates together, so a template read by
 * several crops comes from HBM about once.  An index outside [0, n_obj) is clamped on the device (it never reads outside the
 * bank); checking the range is the caller's business.  PP_S1_CPX=<n> pins the number of crops that share a template's
 * stream (default 8; for A/B timing).
 * Argument errors, returned before any launch: obj_index NULL, n_obj < 1 or n_obj * N >= 2^23, and every error of the _ex
 * entries (PP_EINVAL); a workspace smaller than pp_stage1_indexed_workspace_bytes (PP_EWORKSPACE). */
int pp_stage1_indexed_workspace_bytes(int B, int N, int C, size_t* bytes);
int pp_stage1_scores_indexed(const void* bank, int bank_dtype, const int64_t* obj_index, int n_obj,
                             const float* query, const float* mask, int mask_h, int mask_w, int B, int N,
                             int C, int mode, float eps, void* workspace, size_t workspace_bytes,
                             float* sim_avg, int32_t* stats, void* stream);
int pp_stage1_match_indexed(const void* bank, int bank_dtype, const int64_t* obj_index, int n_obj,
                            const float* query, const float* mask, int mask_h, int mask_w, int B, int N,
                            int C, int k, int mode, float eps, void* workspace, size_t workspace_bytes,
                            float* sim_avg, float* out_score, int64_t* out_index, int32_t* stats,
                            void* stream);


/* ------------------------------------------------------------------------- *
 * Stage 2/3 glue around the networks (picopose_amd/csrc/pp_geom.hip).
 * ------------------------------------------------------------------------- */

/* utils/matching.py:6-26 matching_features_similarity (model/picopose.py:81).
 * src_feat/tar_feat (B,C,16,16) template/query features, src_mask (B,mh,mw) template mask;
 * out (B,256,16,16): out[b,s,h,w] = relu(cos(query patch t=w*16+h, template patch s) * mask_s). */
int pp_similarity_volume(const float* src_feat, const float* tar_feat, const float* src_mask,
                         int mask_h, int mask_w, int B, int C, float* out, void* stream);

/* utils/torch_utils.py:39-51 calc_pred_Ms (model/picopose.py:84): pred_scale (B), pred_inplane
 * (B,2) cos/sin, pred_translation (B,2), tem_pose (B,4,4), tem_K/tem_M (B,3,3) -> pred_Ms (B,3,3). */
int pp_calc_pred_Ms(const float* pred_scale, const float* pred_inplane, const float* pred_translation,
                    const float* tem_pose, const float* tem_K, const float* tem_M, int B,
                    float trans_scale, float* pred_Ms, void* stream);

/* utils/pose_recovery.py:9-65 pose_recovery_2d_prediction (model/picopose.py:86-89) -> (B,4,4).
 * Contract (asserted on the host by the reference, torch_utils.py:100-101): query_M is a crop
 * affine with M01 = M10 = 0 and M00 = M11. */
int pp_pose_recovery_2d(const float* query_M, const float* query_K, const float* pred_Ms,
                        const float* tem_K, const float* tem_M, const float* tem_pose, int B,
                        float* pred_pose, void* stream);

/* utils/correspondence.py:10-26 compute_init_correspondences (model/picopose.py:91):
 * pred_Ms (B,3,3), tem_mask (B,mh,mw) square -> init_flow (B,2,16,16) [ch0 = x], init_certainty
 * (B,1,16,16). */
int pp_init_correspondences(const float* pred_Ms, const float* tem_mask, int mask_h, int mask_w, int B,
                            float* init_flow, float* init_certainty, void* stream);

/* utils/correspondence.py:28-59 compute_stage3_correspondences (model/picopose.py:93):
 * pred_flow (B,2,H,W), pred_certainty (B,1,H,W) -> tar_pts, src_pts (B,H*W,2) int64, entry
 * k = w*H + h = (x,y) or (-1,-1). */
int pp_stage3_correspondences(const float* pred_flow, const float* pred_certainty, int B, int H, int W,
                              float threshold, int64_t* tar_pts, int64_t* src_pts, void* stream);

/* utils/torch_utils.py:257-284 gather, as used at utils/pose_recovery.py:76-77: features
 * (B,C,H,W), index_patches (B,N,2) int64 (x,y) with -1 padding -> out (B,N,C) whose first count[b]
 * rows are features[b,:,y,x] of the valid entries in order; count (B) int32. */
int pp_gather_valid(const float* features, const int64_t* index_patches, int B, int C, int H, int W,
                    int N, float* out, int32_t* count, void* stream);

/* ------------------------------------------------------------------------- *
 * Network engine (picopose_amd/csrc/pp_gemm.hip): fp32 MFMA GEMM / implicit-GEMM convolution
 * and the row-wise kernels around it.  Device tensors are token-major / NHWC: a row is a token
 * or a pixel, channels are contiguous.  These entries replace the stock torch ops (nn.Linear,
 * nn.Conv2d, nn.ConvTranspose2d, nn.LayerNorm, softmax, nn.GroupNorm) the reference's modules
 * call: model/stage1/layers/{attention.py:44-62,mlp.py:30-41,patch_embed.py:66-82,block.py:56-106},
 * model/stage2/affine_regressor.py:72-84, model/stage3/{dpt.py:252-272,flow_decoder.py:58-94,
 * raft_decoder.py:147-161,287-289}.
 * ------------------------------------------------------------------------- */
#define PP_ACT_NONE 0
#define PP_ACT_RELU 1
#define PP_ACT_GELU 2    /* exact erf GELU (nn.GELU default) */
#define PP_ACT_LEAKY01 3 /* LeakyReLU(0.1) */
#define PP_ACT_TANH 4

/* arithmetic of the GEMM engine */
#define PP_PREC_F32 0   /* v_mfma_f32_32x32x2_f32: exact fp32 products, fp32 accumulate                       */
#define PP_PREC_F16X3 1 /* operands scaled and split into 2 fp16 terms, 3 x v_mfma_f32_16x16x32_f16, fp32 acc. */
#define PP_PREC_F16 2   /* plain fp16 operands f16(4 x) [rows][ld] ("h" format), ONE v_mfma_f32_16x16x32_f16 per product, fp32
                           accumulate — the arithmetic BASELINE configs[4] names; pre-split operands only (A_hl / B_hl / C_hl
                           then hold the h format) */

/* C[m,n] = residual[m,n] + gamma[n] * act(alpha * sum_k A(m,k) * B(n,k) + bias[n])
 * for every batch index z = z0*batch1 + z1 (operand offsets z0*bs0 + z1*bs1, in floats). */
typedef struct PpGemmDesc {
    const float* A;        /* dense: [M][lda]; conv: NHWC image (conv_b, conv_h, conv_w, lda>=conv_cin) */
    const float* B;        /* [N][ldb] (k contiguous) or, if b_kn, [K][ldb] (n contiguous)            */
    float* C;              /* [M][ldc]; with shuffle_r: NHWC image (b, h*r, w*r, ldc)                 */
    const float* bias;     /* [N] or NULL */
    const float* gamma;    /* [N] or NULL (LayerScale) */
    const float* residual; /* laid out like C, or NULL */
    const float* residual2; /* second addend laid out like C, or NULL (FeatureFusionBlock, dpt.py:139-141) */
    int M, N, K;
    int lda, ldb, ldc;
    int b_kn;
    int batch0, batch1;
    long long a_bs0, a_bs1, b_bs0, b_bs1, c_bs0, c_bs1;
    float alpha;
    int act;
    int relu_in;           /* apply ReLU to A while loading (ResidualConvUnit, dpt.py:82-86)           */
    /* implicit im2col (conv_kh == 0: dense A): k = (ky*conv_kw + kx)*conv_cin + ci                    */
    int conv_kh, conv_kw, conv_cin, conv_stride, conv_pad, conv_h, conv_w, conv_ho, conv_wo;
    long long conv_bstride; /* floats between consecutive images of A (0: conv_h*conv_w*lda)           */
    /* ConvTranspose2d(kernel = stride = shuffle_r): rows are the pixels of (b, shuffle_h, shuffle_w),
     * column n = (dy*r + dx)*Cout + co is stored at pixel (y*r+dy, x*r+dx), channel co               */
    int shuffle_r, shuffle_h, shuffle_w;
    int prec;              /* PP_PREC_*                                                               */
    /* Pre-split f16x3 operands ("hl" format): a matrix [rows][ld] of fp32 becomes fp16 [rows][ld/8][2][8] —
     * for every group of 8 consecutive k the 8 hi terms then the 8 lo terms (32 contiguous bytes), so that a K
     * tile of 32 is one 128-byte segment per row.  element (r, k), term p: r*2*ld + (k/8)*16 + p*8 + k%8.
     * ld % 8 == 0; the buffers are indexed exactly like the fp32 operand would be (dense / NHWC image).   */
    const void* B_hl;      /* optional pre-split weights for PP_PREC_F16X3 ([N][ldb], pp_split_f16x3)  */
    float b_scale;         /* power-of-two scale the pre-split weights were multiplied by             */
    const void* A_hl;      /* optional pre-split activation operand (pp_split_activation); A may be NULL */
    long long a_hl_bytes, b_hl_bytes; /* filled in by pp_gemm (extent of the buffers)                  */
    void* C_hl;            /* optional: ALSO (or, with C == NULL, only) write the output as an hl operand */
    int ldc_h;             /* [M][ldc_h] for the next GEMM (no pixel shuffle, no batch); ldc_h % 8 == 0  */
    int c_relu;            /* C_hl holds split(max(out, 0)): the consumer's input ReLU folded in        */
    const float* alpha_dev;  /* optional DEVICE scalars: alpha is multiplied by alpha_dev[0] (and alpha_dev2[0]) when the kernel   */
    const float* alpha_dev2; /* runs — the inverse range scales of backward operands, chosen on the device (pp_pow2_scale_ws)      */
    /* K slices (weight gradients: few output tiles over a very long K leave most CUs idle).  ksplit = S > 1, both operands pre-split,
     * dense, M % 256 == 0, K % (64 S) == 0: C holds S*M rows — rows s*M .. of it receive the product over k in [s K/S, (s+1) K/S)
     * (one launch of S * tiles work items); add the S slices in index order (pp_sum_slices).  No bias / activation / residual.  */
    int ksplit;
    int ks_rows;             /* filled in by pp_gemm (the rows of one slice)                                                       */
    /* filled in by pp_gemm — a batch of fp32 products whose A and C blocks lie one behind the other (a_bs0 = M lda, c_bs0 = M ldc,
     * batch1 = 1, M % 256 == 0, no residual: the sixteen products of a Winograd convolution) runs as ONE persistent launch of the fp32
     * engine over batch0 * M rows; row tile r reads the weights of group r BM / grp_rows, grp_b_bytes further on.                     */
    int grp_rows;
    long long grp_b_bytes;
} PpGemmDesc;

int pp_gemm(const PpGemmDesc* desc, void* stream);
/* Split n fp32 weights (rows of a multiple of 8 elements) once at load time into an hl buffer of 2n halfs:
 * scale[0] = 2^k with max|scale*w| in [512,1024) (device float), hi = f16(scale*w), lo = f16(scale*w - hi). */
int pp_split_f16x3(const float* w, long long n, void* hl, float* scale, void* stream);
/* The same split with the scale left ON THE DEVICE: scale2[0] = 2^k, scale2[1] = 2^-k (pass scale2 + 1 as PpGemmDesc.alpha_dev with
 * b_scale = 1: no host read-back — the training step re-splits every parameter after every optimizer step); partials: 1024 floats of
 * scratch; two launches. */
int pp_split_weights_ws(const float* w, long long n, int terms, void* out, float* scale2, float* partials, void* stream);
/* Split an activation tensor x (B, P, C) fp32 (batch / row strides in floats, channels contiguous, C % 8 == 0)
 * once into a contiguous hl buffer (B*P rows, ld = C) for PP_PREC_F16X3 (activation scale 4; optional ReLU first). */
int pp_split_activation(const float* x, long long batch_stride, int B, int P, int row_stride, int C, int relu,
                        void* hl, void* stream);
/* The same into C columns of a wider hl operand whose rows hold ld_h elements (hl = address of the first column's
 * group: a multiple of 8 columns into the row): the channel concatenation of operands without an fp32 concat buffer. */
int pp_split_activation_ld(const float* x, long long batch_stride, int B, int P, int row_stride, int C, int relu,
                           void* hl, int ld_h, void* stream);
/* Backward-product operands (picopose_amd/autograd.py): gradients span 1e-9 .. 1, so an operand is multiplied by a power of two chosen
 * on the DEVICE from its max before it is split, and the product is scaled back through PpGemmDesc.alpha_dev — no host sync, and
 * (round 4) no separate scaling / transposing passes:
 *   pp_pow2_scale_ws   scale2[0] = 2^k with max|2^k x| in [512, 1024), scale2[1] = 2^-k; partials: >= 1024 floats of scratch
 *                      (two launches: per-workgroup maxima, one fold — no atomics, no init launch);
 *   pp_split_scaled_t  x (rows, C) fp32 with row pitch ld -> contiguous operand (rows, C) of scale[0] * x;
 *   pp_split_transpose_t  x (rows, cols) fp32 with row pitch ld -> contiguous operand (cols, rows) of scale[0] * x^T (scale NULL = 1;
 *                      rows % 8 == 0): the K-major operands of dW = dz^T x in ONE pass instead of scale copy + transposed copy + split. */
int pp_pow2_scale_ws(const float* x, long long n, float* scale2, float* partials, void* stream);
int pp_split_scaled_t(const float* x, long long rows, int ld, int C, const float* scale, void* out, int terms, void* stream);
int pp_split_transpose_t(const float* x, long long rows, int cols, int ld, const float* scale, void* out, int terms, void* stream);
/* ... with an operand row pitch ld_out >= rows (% 8 == 0), the k in [rows, ld_out) zero: K padded to a multiple of the K slices */
int pp_split_transpose_ld(const float* x, long long rows, int cols, int ld, const float* scale, void* out, long long ld_out, int terms,
                          void* stream);
/* The K-major im2col of an NHWC image (pp_im2col_t_nhwc below) written straight as the engine operand: (ksize^2 C) operand rows with
 * K = B Ho Wo pixels (a multiple of 8) — the B operand of a convolution's weight gradient dW = dz^T colT without the fp32 matrix. */
int pp_im2col_t_operand(const float* x, int B, int H, int W, int C, int ksize, int stride, int pad, void* out, int terms, void* stream);
/* Second half of a split-K linear layer (a few rows against a long K — stage 2's fc1, affine_regressor.py:77: 160 x 16384 x
 * 1024 fills 8 workgroups as one GEMM): part (S, M, N) fp32 = the S K-slices' products from one batched pp_gemm;
 * out[m, n] = act(sum_s part[s, m, n] + bias[n]), slices added in index order. */
int pp_sum_slices(const float* part, int S, int M, int N, const float* bias, int act, float* out, void* stream);
/* Columns col0 .. col0 + c - 1 (any alignment, c <= 64) of every row of an existing hl operand with rows of ld_h channels
 * <- x (rows, c) fp32 with row pitch ld_x: the narrow member of a channel concatenation (raft_decoder.py:161, [out | flow]). */
int pp_hl_patch_columns(const float* x, int ld_x, int c, long long rows, void* hl, int ld_h, int col0, void* stream);

/* ---- operand-format ("terms") forms of the producers above.  terms = 2: the hl format of PP_PREC_F16X3 (fp16 [rows][ld/8][2][8]);
 * terms = 1: the h format of PP_PREC_F16 (plain fp16 f16(4 x) [rows][ld]) — BASELINE configs[4]'s "fp16 storage / MFMA with fp32
 * accumulate".  Same arguments as the entries they generalise, which are these with terms = 2. */
int pp_split_weights_t(const float* w, long long n, int terms, void* out, float* scale, void* stream);
int pp_split_activation_t(const float* x, long long batch_stride, int B, int P, int row_stride, int C, int relu, void* out,
                          int ld_h, int terms, void* stream);
int pp_hl_patch_columns_t(const float* x, int ld_x, int c, long long rows, void* out, int ld_h, int col0, int terms, void* stream);
int pp_layernorm_t(const float* x, const float* gamma, const float* beta, int rows, int C, float eps, float* y, void* out, int terms,
                   void* stream);
int pp_resize_bilinear_nhwc_t(const float* in, int B, int H, int W, int C, int Ho, int Wo, float mul, void* out, int terms,
                              void* stream);
/* ... the same resize with BOTH results: the fp32 map `out` (B, Ho, Wo, C) and its operand form `out_operand` (the DPT fusion block's
 * path map, dpt.py:150-155 with out_conv moved in front of the interpolation: an output and the flow decoder's projection input). */
int pp_resize_bilinear_nhwc_dual(const float* in, int B, int H, int W, int C, int Ho, int Wo, float mul, float* out, void* out_operand,
                                 int terms, void* stream);
int pp_warp_nhwc_t(const float* feat, int feat_batch, const float* flow, int B, int H, int W, int C, int ld_flow, void* out,
                   int ld_h, int terms, void* stream);
/* attention on the operand the qkv GEMM wrote, result as fp32 (out) and / or as an operand (out_operand), both optional */
int pp_attention_t(const void* qkv_operand, int terms, int B, int T, int heads, int head_dim, float scale, float* out,
                   void* out_operand, void* stream);

/* Fused multi-head self-attention (model/stage1/layers/attention.py:49-62): qkv (B,T,3,heads,64) as the qkv
 * linear produces it -> out (B,T,heads*64) = softmax((q*scale) k^T) v per head; exact fp32 MFMA, flash style. */
int pp_attention(const float* qkv, int B, int T, int heads, int head_dim, float scale, float* out, void* stream);
/* Same, writing the output (also) as an hl operand (B*T rows, ld = heads*head_dim) for the projection GEMM;
 * out may be NULL. */
int pp_attention_split(const float* qkv, int B, int T, int heads, int head_dim, float scale, float* out, void* out_hl,
                       void* stream);
/* General form: prec = PP_PREC_F32 (exact fp32 products, as the two entries above) or PP_PREC_F16X3 (q, k, v and
 * the probabilities split into 2 fp16 terms, 3 fp16 MFMAs per product, fp32 soft-max statistics and accumulation);
 * out and/or the hl operand out_hl. */
int pp_attention_ex(const float* qkv, int B, int T, int heads, int head_dim, float scale, int prec, float* out, void* out_hl,
                    void* stream);
/* PP_PREC_F16X3 attention whose input is already the hl operand (B*T rows, ld = 3*heads*head_dim) that the qkv GEMM
 * wrote (PpGemmDesc.C_hl): no split work inside the kernel; bit-identical to pp_attention_ex on the fp32 qkv. */
int pp_attention_hl(const void* qkv_hl, int B, int T, int heads, int head_dim, float scale, float* out, void* out_hl,
                    void* stream);
/* Training forward of the same attention (PP_PREC_F16X3): out as above plus lse2 (B*heads, T), the base-2 log-sum-exp of every
 * query's scaled scores — all pp_attention_backward needs; the T x T probabilities are never stored. */
int pp_attention_train(const float* qkv, int B, int T, int heads, int head_dim, float scale, float* out, float* lse2, void* stream);
/* Adjoint of attention.py:49-62 (what torch.autograd derives for the reference): dqkv (B*T, 3*heads*64) from qkv, the forward's out
 * and lse2, and dout (B*T, heads*64).  gpair = device (2^k, 2^-k) with max|dout| 2^k in [512, 1024) (pp_pow2_scale_ws); Dws = B*heads*T
 * floats of scratch.  Scores and probabilities are recomputed tile by tile; two kernels (dq | dk, dv), no atomics: bit-reproducible.
 * T = 1 (the soft-max of one key is constant): dq = dk = 0 and dv = dout, exactly. */
int pp_attention_backward(const float* qkv, const float* out, const float* dout, const float* lse2, const float* gpair, int B, int T,
                          int heads, int head_dim, float scale, float* Dws, float* dqkv, void* stream);

/* nn.LayerNorm(C, eps) over rows of a [rows][C] matrix. */
int pp_layernorm(const float* x, const float* gamma, const float* beta, int rows, int C, float eps,
                 float* y, void* stream);
/* Same, writing the result (also) as an hl operand (rows, ld = C; C % 8 == 0); y may be NULL. */
int pp_layernorm_split(const float* x, const float* gamma, const float* beta, int rows, int C, float eps, float* y,
                       void* hl, void* stream);
/* softmax(dim=-1) in place over rows of a [rows][ld] matrix (n valid columns). */
int pp_softmax_rows(float* x, int rows, int n, int ld, void* stream);
/* nn.GroupNorm(groups, C, eps) (+ReLU when relu != 0) on an NHWC tensor (B, HW, C). */
int pp_groupnorm_nhwc(const float* x, const float* gamma, const float* beta, int B, int HW, int C,
                      int groups, float eps, int relu, float* y, void* stream);
/* out[b, c, col_off + r] = in[b, r, c]: (B,R,C) -> (B,C,ld_out); NCHW <-> NHWC at the API boundary.
 * Batch strides in floats (0: dense). */
int pp_transpose_batched(const float* in, long long in_batch_stride, int B, int R, int C, float* out,
                         long long out_batch_stride, int ld_out, int col_off, void* stream);
/* vision_transformer.py:209-216: tokens (B,T+1,C) = [cls; patches (B,T,C)] + pos (T+1,C). */
int pp_assemble_tokens(const float* patches, const float* cls_token, const float* pos, int B, int T, int C,
                       float* tokens, void* stream);
/* F.normalize(x, dim=1) for [rows][n<=64]. */
int pp_normalize_rows(const float* x, int rows, int n, float eps, float* y, void* stream);

/* ------------------------------------------------------------------------- *
 * Stage-3 sampling kernels (picopose_amd/csrc/pp_sample.hip), NHWC.
 * ------------------------------------------------------------------------- */
/* F.interpolate(mode="bilinear", align_corners=True) (dpt.py:150-152, flow_decoder.py:88-92); the
 * result is multiplied by `mul` (the 2x of the flow up-sampling). */
int pp_resize_bilinear_nhwc(const float* in, int B, int H, int W, int C, int Ho, int Wo, float mul,
                            float* out, void* stream);
/* Same, writing the result only as an hl operand (B*Ho*Wo rows, ld = C, C % 8 == 0) for the convolution that follows. */
int pp_resize_bilinear_nhwc_hl(const float* in, int B, int H, int W, int C, int Ho, int Wo, float mul, void* out_hl,
                               void* stream);
/* FlowDecoder.feature_sample (flow_decoder.py:49-56): out[b,p,:] = bilinear(feat[b % feat_batch], p + flow[b,p]),
 * zeros padding, align_corners=True.  flow rows have ld_flow floats (x, y first), out rows ld_out.  feat holds
 * feat_batch images (= B, or the query maps given once for the B / feat_batch hypotheses of a hypothesis-major batch). */
int pp_warp_nhwc(const float* feat, int feat_batch, const float* flow, int B, int H, int W, int C, int ld_flow,
                 float* out, int ld_out, void* stream);
/* Same, writing the result only as C columns of an hl operand with rows of ld_h elements (C % 8 == 0). */
int pp_warp_nhwc_hl(const float* feat, int feat_batch, const float* flow, int B, int H, int W, int C, int ld_flow,
                    void* out_hl, int ld_h, void* stream);
/* nn.AvgPool2d(2,2) on NHWC. */
int pp_avgpool2_nhwc(const float* in, int B, int H, int W, int C, float* out, void* stream);
/* dst[i] = src[index[i]] for i < n: rows of row_floats fp32 (a multiple of 4; both buffers 16-byte aligned), index int64
 * into the n_src_rows rows of src — the selection of the top-k templates' rgb / mask / pts3d / pose / K / M rows
 * (model/picopose.py:55-62). */
int pp_gather_rows(const float* src, const long long* index, long long n_src_rows, long long row_floats, int n, float* dst,
                   void* stream);
/* Rows of the feature bank as token rows: tokens[(j T + skip + p) ld + c] = bank[(index[j] C + c) P + p] for j < n, p < P, c < C.
 * bank: n_bank_rows rows of (C, P) fp32 — `template_feature.flatten(0, 1)`, which run_test.py:120-134 builds as
 * feature_extractor(tem_rgb)[-1] and run_test.py:161-162 gathers per crop; index: int64 on the device (an index outside
 * [0, n_bank_rows) leaves its image untouched, as in pp_gather_rows); tokens: the (rows, ld) fp32 buffer of a ViT level with T rows per
 * image (ld >= C, skip + P <= T).  The `skip` leading rows of every image (the cls row) are written as zeros; rows past skip + P and
 * columns past C are not written.  One launch: the gather fused with the (C, P) -> (P, C) transpose through an LDS tile. */
int pp_bank_rows_to_tokens(const float* bank, long long n_bank_rows, int C, int P, const long long* index, int n, float* tokens, int ld,
                           int T, int skip, void* stream);
/* The patch-embed operand straight from the image bank: image j < n_front of the result is front[j] ((n_front, 3, H, W) contiguous fp32;
 * NULL with n_front = 0), image n_front + i is bank[index[i]] (bank: n_bank_rows rows of (3, H, W) fp32 — `tem_rgb.flatten(0, 1)`; index:
 * n int64 on the device).  out: ((n_front + n) H W, 8) operand rows in the format pp_split_activation_t writes (terms = 2: hl, 1: h),
 * channels 0..2 = the pixel's three planes, 3..7 zero; a value beyond the operand range sets the saturation word as there.  The bits are
 * those of pp_gather_rows -> concatenation -> NCHW to NHWC-8 (pp_transpose_batched into a zeroed map) -> pp_split_activation_t, in one pass
 * (NCHW -> pixel-major through an LDS tile).  bank, front and out 16-byte aligned; an index outside [0, n_bank_rows) leaves its image's
 * rows unwritten and the call returns PP_OK, as in pp_gather_rows. */
int pp_patch_operand(const float* bank, long long n_bank_rows, const long long* index, int n, const float* front, int n_front, int H, int W,
                     void* out, int terms, void* stream);
/* A flow map as the operand of flow_net[0] (raft_decoder.py:141-147): flow (rows, ld_flow >= 2) fp32, x and y first; out8: (rows, 8)
 * operand (16-byte aligned) with channels 0, 1 = the flow and 2..7 zero.  One launch for a zeroed 8-channel map, the copy of the flow
 * into it and its pp_split_activation_t — the same bits and the same saturation report. */
int pp_flow_operand(const float* flow, int ld_flow, long long rows, void* out8, int terms, void* stream);

/* -------------------------------------------------------------------------
 * Crop preprocessing of one detection (provider/bop_test_dataset.py:162-177, utils/data_utils.py:231-250):
 * image (H, W, 3) uint8 as loaded, optional full-frame binary mask (H, W) uint8 (device pointers); crop rows [y1, y2),
 * columns [x1, x2); out_rgb (3, S, S) fp32 = (cv2-style INTER_LINEAR resize of the channel-flipped crop / 255
 * [* (mask > 0) if rgb_mask_flag] - mean) / std (mean3 / std3: host pointers to 3 doubles, in output-channel order);
 * out_mask (S, S) fp32 = INTER_NEAREST resize of the cropped mask (may be NULL).  cv2 is not available to pin the
 * interpolation bit-for-bit: it follows OpenCV's published definition (oracle/preprocess.py).
 * ------------------------------------------------------------------------- */
int pp_crop_resize_normalize(const unsigned char* image, int H, int W, const unsigned char* mask, int y1, int y2, int x1,
                             int x2, int S, int rgb_mask_flag, const double* mean3, const double* std3, float* out_rgb,
                             float* out_mask, void* stream);
/* Template lookup points (bop_test_dataset.py:233-235, data_utils.py:97-115): depth (H, W) fp32 metres -> out (P, P, 3):
 * the back-projection ((x-cx) z/fx, (y-cy) z/fy, z) of the crop rows [y1,y2) x columns [x1,x2), INTER_NEAREST-resized. */
int pp_depth_points_nearest(const float* depth_m, int H, int W, int y1, int y2, int x1, int x2, int P, float fx, float fy,
                            float cx, float cy, float* out_pts, void* stream);
/* CorrelationPyramid (raft_decoder.py:30-53) + CorrLookup (corr_lookup.py:100-134) without the
 * (B*HW, HW) volume: f1 (B,H,W,C) with rows of ld_f1 floats, f2_l{0,1,2} = f2 and its 2x2 average pools holding
 * f2_batch images (image b reads f2[b % f2_batch]), flow (B,H,W,ld_flow);
 * out (B,H,W,ld_out) with channel l*(2r+1)^2 + a*(2r+1) + b = corr_l sampled at x offset a-r,
 * y offset b-r around (p + flow)/2^l; ld_out is the channel count of the result: the channels from levels*(2r+1)^2 up to ld_out
 * (padding to the next layer's multiple of 8) are written as zeros by these entries and by pp_corr_lookup_nhwc_hl.
 * When H, W are multiples of 8 and C of 32 the local correlations of an 8x8 pixel tile against a 16x16 region of f2
 * are computed on the matrix cores in the engine's f16x3 arithmetic (22 operand bits, fp32 accumulation; values with
 * |x| >= 16376 saturate); otherwise (and with PP_CORR_TILED=0 in the environment) by exact fp32 fmas, one lane per
 * neighbour position. */
int pp_corr_lookup_nhwc(const float* f1, int ld_f1, const float* f2_l0, const float* f2_l1, const float* f2_l2,
                        int f2_batch, const float* flow, int B, int H, int W, int C, int levels, int radius,
                        int ld_flow, float* out, int ld_out, void* stream);
/* The same with the arithmetic as an argument: PP_PREC_F16X3 = the default above, PP_PREC_F32 = exact fp32 products and sums
 * whatever the shape — what `ops.PRECISION = "f32"` / `bench.py --mode exact` runs — PP_PREC_F16 = plain fp16 operands, one MFMA
 * per product, fp32 accumulation (`--mode fp16`: the arithmetic of that mode's convolutions). */
int pp_corr_lookup_nhwc_ex(const float* f1, int ld_f1, const float* f2_l0, const float* f2_l1, const float* f2_l2,
                           int f2_batch, const float* flow, int B, int H, int W, int C, int levels, int radius,
                           int ld_flow, int prec, float* out, int ld_out, void* stream);

/* Convolution with ONE or TWO output channels on an hl operand (the flow / certainty predict layers of the decoder heads,
 * raft_decoder.py:287-289): x_hl (B,H,W) pixels with rows of ld_x channels (C of them read, C % 32 == 0), stride 1,
 * padding ksize / 2, ksize 1 or 3, W in {16, 32, 64} and H a multiple of 256 / W; weight (n_out, ksize*ksize*C) fp32 in the
 * engine's k order (tap-major, then channel), bias (n_out) or NULL, residual (B,H,W,n_out) or NULL added to the result;
 * out (B,H,W,n_out) fp32.  Exact fp32 products of the operand's value (hi + lo) with the fp32 filters, fp32 accumulation —
 * at least the accuracy of the f16x3 engine, independent of the batch size. */
int pp_conv_narrow_hl(const void* x_hl, int ld_x, int B, int H, int W, int C, const float* weight, const float* bias, int ksize,
                      int n_out, const float* residual, float* out, void* stream);
/* The same layers on the fp32 NHWC map itself (x: (B,H,W) pixels with rows of ld_x floats, ld_x % 4 == 0, 16-byte aligned; images
 * contiguous) — the strict-fp32 mode's form (PP_PREC_F32 networks: raft_decoder.py:287-289 in the reference's own arithmetic):
 * every product and sum fp32, taps walked in the engine's k order. */
int pp_conv_narrow_f32(const float* x, int ld_x, int B, int H, int W, int C, const float* weight, const float* bias, int ksize,
                       int n_out, const float* residual, float* out, void* stream);

/* Winograd F(2x2, 3x3) for the 3x3 / stride 1 / padding 1 convolutions of the strict-fp32 mode (raft_decoder.py:251-289, dpt.py:72-95 in
 * the reference's own arithmetic; csrc/pp_winograd.hip): 16 dense products Y_xi (P, Cout) = U_xi (P, Cin) V_xi (Cout, Cin)^T over the
 * P = B H W / 4 output tiles run through pp_gemm (PP_PREC_F32, dense); these are the three fp32 transforms around them.
 *   pp_winograd_input_f32   x: NHWC image (B, H, W) with rows of ld_x floats (C of them read; H, W even, C % 4 == 0, 16-byte aligned,
 *                           images batch_stride floats apart), relu != 0: max(x, 0) first (ResidualConvUnit)  ->  U (16, P, C)
 *   pp_winograd_weight_f32  w: (Cout, 9 Cin) in the engine's k order (tap-major, then channel), rows of ldw floats  ->  V (16, Cout, Cin)
 *   pp_winograd_output_f32  Y (16, P, Cout)  ->  out (B, H, W) with rows of ldc floats: A^T Y A + bias, act (none / ReLU / LeakyReLU),
 *                           + residual + residual2 (laid out like out) */
int pp_winograd_input_f32(const float* x, int ld_x, long long batch_stride, int B, int H, int W, int C, int relu, float* U, void* stream);
int pp_winograd_weight_f32(const float* w, int Cout, int Cin, int ldw, float* V, void* stream);
int pp_winograd_output_f32(const float* Y, int B, int H, int W, int Cout, const float* bias, int act, const float* residual,
                           const float* residual2, float* out, int ldc, void* stream);

/* Winograd F(4x4, 3x3) on the f16x3 engine (PP_PREC_F16X3; round 6) for the large 3x3 / stride 1 / padding 1 convolutions of the flow
 * decoder's heads (raft_decoder.py:251-289): 36 dense products Y_xi (P, Cout) = U_xi (P, Cin) V_xi (Cout, Cin)^T over the P = B H W / 16
 * tiles — four times fewer multiplications than the direct convolution — run by pp_gemm as a batch of pre-split products (A_hl, B_hl,
 * batch0 = the frequencies of the launch, a_bs0 = P lda, b_bs0 = Cout Cin, c_bs0 = P ldc, alpha = 64: ONE persistent launch).
 *   pp_winograd4_input_hl    x_hl: hl operand image (B, H, W), rows of ld_x channels (C of them read from the pointer's column on; H, W
 *                            % 4 == 0, C % 8 == 0); batch_stride in ELEMENTS  ->  U_hl (36, P, C) hl operand of (B^T d B) / 16
 *   pp_winograd4_weight_f32  w (Cout, 9 Cin) in the engine's k order, rows of ldw floats  ->  V (36, Cout, Cin) fp32 (split it with
 *                            pp_split_weights_t as ONE matrix of 36 Cout rows)
 *   pp_winograd4_output      Y (36, P, Cout) fp32  ->  A^T Y A + bias, act (none / ReLU / LeakyReLU): as fp32 NHWC map `out` (rows of ldc
 *                            floats; + residual + residual2 laid out like out) and / or as hl operand `out_hl` (rows of ld_h channels,
 *                            the pointer at the first column's group; of max(., 0) with c_relu).  Cout % 4 == 0 (% 8 for out_hl).
 * ld_y >= Cout: the row pitch of Y in floats (Y may be a column slice of a wider product: two layers that read the same U, fused along N).
 * P_pad >= P: the rows of one frequency block of U and Y (P rounded up to a multiple of 256, the engine's row tile, so that a row tile
 * lies inside one frequency; the pad rows are never read by the output transform). */
int pp_winograd4_input_hl(const void* x_hl, int ld_x, long long batch_stride, int B, int H, int W, int C, int relu, void* U_hl, long long P_pad,
                          void* stream);
int pp_winograd4_weight_f32(const float* w, int Cout, int Cin, int ldw, float* V, void* stream);
int pp_winograd4_output(const float* Y, int ld_y, int B, int H, int W, int Cout, const float* bias, int act, const float* residual,
                        const float* residual2, float* out, int ldc, void* out_hl, int ld_h, int c_relu, long long P_pad, void* stream);

/* Output transform of a Winograd F(4x4, 3x3) layer CHAINED into the input transform of the next one (conv 3x3 -> ReLU -> conv 3x3,
 * raft_decoder.py:251-289): Y (36, P_pad, C) fp32 of the first layer -> U_hl (36, P_pad, C) hl operand of B^T relu'(A^T Y A + bias) B / 16 of the
 * second, the hidden map never stored; bit-identical to pp_winograd4_output (operand output, c_relu) followed by pp_winograd4_input_hl.
 * W in {16, 32, 64}, H % 4 == 0, C % 32 == 0; act none / ReLU / LeakyReLU, then (c_relu) the consumer's input ReLU. */
int pp_winograd4_chain(const float* Y, int ld_y, int B, int H, int W, int C, const float* bias, int act, int c_relu, void* U_hl, long long P_pad,
                       void* stream);

/* The same chain for the strict-fp32 mode's F(2x2, 3x3): Y (16, P, C) fp32 of layer k -> U (16, P, C) fp32 of layer k + 1 (P = B H W / 4),
 * h = act(A^T Y A + bias), then max(h, 0) with relu_next (the next layer's input ReLU: dpt.py:82-86), never stored; bit-identical to
 * pp_winograd_output_f32 followed by pp_winograd_input_f32.  W in {16, 32, 64}, H even, C % 32 == 0. */
int pp_winograd_chain_f32(const float* Y, int B, int H, int W, int C, const float* bias, int act, int relu_next, float* U, void* stream);

/* Sticky operand-saturation word.  The f16x3 / f16 operand formats clamp at the fp16 range (|4 x| >= 65504): a clamped term is finite but
 * WRONG.  The Winograd F(4x4, 3x3) transforms (pp_winograd4_input_hl, pp_winograd4_output, pp_winograd4_chain) do NOT clamp: there a value
 * beyond the fp16 range is stored as +-inf in the hi term and NaN in the lo term, and everything computed from it is +-inf / NaN.  Either
 * way the result is wrong and is reported the same way.  With a device word registered here, every kernel that writes operand terms ORs bit 0 into it when a term hit the clamp (one
 * atomic per wave that saw one; nothing when none did) — the host reads the word together with its results (no extra synchronisation)
 * and raises.  word = NULL switches the reporting off.  Per device (the current one).  block.py:104-106 / layer_scale.py:27-28: trained
 * DINOv2 residual streams hold a few very large channels. */
int pp_set_saturation_word(unsigned int* word);

/* Stream-ordered snapshot of a saturation word: enqueued on `stream`, one lane does *slot = atomicExch(word, 0).  Taken right after a
 * forward on that forward's stream, the slot holds the flag of exactly the producers enqueued since the previous take (one batch's own
 * verdict, however many batches are in flight) and the word is clear for the next one.  word: the registered device word
 * (pp_set_saturation_word); slot: a device uint32.  Null pointers: PP_EINVAL.  Does not synchronise. */
int pp_saturation_take(unsigned int* word, unsigned int* slot, void* stream);


/* The tiled lookup on operands the producers already hold in the engine's hl format (fp16 [pixels][2 ld]: per 8 channels
 * the 8 hi then the 8 lo terms; include "hl" above): f1_hl with rows of ld_f1 channels (a column block of a wider operand
 * is fine), f2_hl_l{0,1,2} contiguous (f2_batch, H >> l, W >> l, C).  H, W multiples of 8 and C of 32 (else PP_EINVAL: use
 * pp_corr_lookup_nhwc).  Same values as pp_corr_lookup_nhwc on the fp32 maps, without the split work per staged chunk. */
int pp_corr_lookup_nhwc_hl(const void* f1_hl, int ld_f1, const void* f2_hl_l0, const void* f2_hl_l1, const void* f2_hl_l2,
                           int f2_batch, const float* flow, int B, int H, int W, int C, int levels, int radius, int ld_flow,
                           float* out, int ld_out, void* stream);
/* The same lookup with the choice of output: exactly one of `out` (the fp32 map, rows of ld_out floats) and `out_hl` (the result
 * as an hl operand with rows of ld_out_h channels, ld_out_h % 8 == 0 and >= levels (2 radius + 1)^2: the operand of the 1x1
 * convolution that reads the map, pad channels zero — the bits and the saturation report of the fp32 map going through
 * pp_split_activation, with no fp32 map stored).  Both entries take the ring-staged kernel (per-level regions of the query map,
 * chunks moved into LDS by LDS-DMA) unless PP_CORR_RING=0 (read per call), which keeps the register-staged kernel: the same bits. */
int pp_corr_lookup_nhwc_hl_op(const void* f1_hl, int ld_f1, const void* f2_hl_l0, const void* f2_hl_l1, const void* f2_hl_l2,
                              int f2_batch, const float* flow, int B, int H, int W, int C, int levels, int radius, int ld_flow,
                              float* out, int ld_out, void* out_hl, int ld_out_h, void* stream);
/* pp_avgpool2_nhwc with the pooled map's hl operand written by the same kernel (C % 8 == 0; in and out 16-byte aligned): out_hl
 * (B (H/2) (W/2), 2 C) holds the bits of pp_split_activation on the pooled map (same sum order, same saturation report); out may be
 * null (a pyramid level whose fp32 form nothing reads). */
int pp_avgpool2_hl(const float* in, int B, int H, int W, int C, float* out, void* out_hl, void* stream);

/* ------------------------------------------------------------------------- *
 * utils/pose_recovery.py:68-105 pose_recovery_ransac_pnp, batched over P = instances x hypotheses
 * (run_test.py:168-184 calls it once per pair): gather of the valid 2D/3D correspondences, object-frame
 * transform, RANSAC (5-point samples, `iterations`, squared reprojection error <= threshold^2) with EPnP
 * as the model solver and an EPnP refit on the inliers (picopose_amd/csrc/pp_pnp.hip).  One 512-thread workgroup per
 * problem, fp64; hypothesis h of problem p draws its sample from a counter-based hash of (p, h), so a problem's result
 * depends on its index in the batch (as OpenCV's depends on its RNG state), not on the launch configuration.
 *   tar_pts_2d (P,2,H,W), src_pts_3d (P,3,H,W), K (P,3,3), tem_pose (P,4,4) fp32;
 *   tar_pts, src_pts (P,N,2) int64 (x,y) with -1 padding, N <= 4096;
 *   out: rot (P,3,3) f64, tvec (P,3) f64, inlier_ratio (P) f64, success (P) int32 (0: the reference's
 *   failure outputs I, [0,0,1], 0.0), num_points (P) int32.
 * ------------------------------------------------------------------------- */
int pp_pnp_ransac(const float* tar_pts_2d, const float* src_pts_3d, const float* K, const float* tem_pose,
                  const int64_t* tar_pts, const int64_t* src_pts, int P, int H, int W, int N, int iterations,
                  float reproj_threshold, double* rot, double* tvec, double* inlier_ratio, int32_t* success,
                  int32_t* num_points, void* stream);

/* pp_pnp_ransac with one more output for parity work: refit_branches (P, 40) f64 = for the final EPnP refit on the consensus
 * set, the candidate pose of each of EPnP's three beta initialisations (N = 1 / 2 / 3 null-space vectors; OpenCV's epnp.cpp
 * find_betas_approx_1 / _2 / _3 behind cv2.solvePnPRansac, utils/pose_recovery.py:93-95) as [R (9, row-major), t (3), mean
 * reprojection error in px (1e300: the branch gave no pose)] x 3, then the index of the branch the refit kept (-1: none, the
 * RANSAC winner's pose is returned).  Two correct EPnP implementations may keep different branches when their errors are
 * within rounding of each other; compared branch by branch they must agree to solver accuracy (tests/test_e2e.py). */
int pp_pnp_ransac_debug(const float* tar_pts_2d, const float* src_pts_3d, const float* K, const float* tem_pose,
                        const int64_t* tar_pts, const int64_t* src_pts, int P, int H, int W, int N, int iterations,
                        float reproj_threshold, double* rot, double* tvec, double* inlier_ratio, int32_t* success,
                        int32_t* num_points, double* refit_branches, void* stream);

/* pp_pnp_ransac followed by a Levenberg-Marquardt refinement of each pose on its RANSAC consensus set: what
 * cv2.solvePnPRefineLM(inlier object points, inlier image points, K, None, rvec, tvec, criteria) does after
 * cv2.solvePnPRansac(..., SOLVEPNP_EPNP) (OpenCV's default criteria: 20 iterations, FLT_EPSILON).  The consensus set
 * (inlier_ratio), success and num_points are those of pp_pnp_ransac, computed by the same code; only rot / tvec move.
 *   Cost: sum over the consensus set of the squared pixel reprojection error, in the object frame of pp_pnp_ransac (points
 *   after the tem_pose transform, fp32 values evaluated in fp64) and K's fu, fv, uc, vc.  Parameters: a local so(3)
 *   perturbation w applied on the left through the Cayley map (R <- cay(w) R, first-order equal to exp([w]x) R) and a
 *   translation increment; analytic 2x6 Jacobian, fp64.
 *   Start: the pose pp_pnp_ransac returns (the EPnP refit, or the RANSAC winner when the refit gave no pose).
 *   Step: (J^T J + lambda diag(J^T J)) dx = -J^T r by Cholesky, lambda = 0 at the start (a Gauss-Newton step).  The trial
 *   pose is accepted iff its cost is lower than the current cost and every point of the set has Z > 0; lambda is then divided
 *   by 10, otherwise it becomes max(10 lambda, 1e-3) (also when the damped matrix is not positive definite).  The returned
 *   cost is never above the starting cost.
 *   Stop: after max_iters iterations (each is one pass over the points), after an ACCEPTED step whose cost decrease is
 *   <= eps * the previous cost, or after any step with |dx|_2 <= eps (radians and the object's length unit).
 *   Skipped (start pose returned, 0 iterations) when the set has fewer than 6 points or the start or its cost is not finite.
 *   The sums of a pass are reduced in a fixed order: the result does not change from one launch to the next.
 * Extra outputs: rms_before / rms_after (P) f64 = RMS reprojection error over the consensus set at the start / the returned
 * pose in px; lm_iterations (P) int32 = accepted steps; for failed problems (success 0: the reference's failure outputs) 0, 0,
 * 0.  inlier_mask (P, N) uint8 or null: 1 for a consensus-set member, in the order of the valid (no -1) entries of tar_pts /
 * src_pts (cv2's `inliers`), 0 in the remaining N - num_points slots and for failed problems.
 * PP_EINVAL (before any launch): what pp_pnp_ransac rejects, a null rms_before / rms_after / lm_iterations, max_iters <= 0,
 * eps < 0 or NaN. */
int pp_pnp_ransac_refine(const float* tar_pts_2d, const float* src_pts_3d, const float* K, const float* tem_pose,
                         const int64_t* tar_pts, const int64_t* src_pts, int P, int H, int W, int N, int iterations,
                         float reproj_threshold, int max_iters, double eps, double* rot, double* tvec, double* inlier_ratio,
                         int32_t* success, int32_t* num_points, double* rms_before, double* rms_after, int32_t* lm_iterations,
                         uint8_t* inlier_mask, void* stream);

/* cv2.solvePnPRefineLM(object_points, image_points, K, None, rvec, tvec) over a ragged batch of P problems, one 512-thread
 * workgroup each, with the refinement (cost, parameters, step, stopping rule) of pp_pnp_ransac_refine.
 *   object_points (P, Nmax, 3), image_points (P, Nmax, 2) f64: problem p uses its first count[p] rows (count (P) int32,
 *   clamped to [0, Nmax]); K (P, 3, 3) f64 (fu, fv, uc, vc; the skew entry is not used); rot_init (P, 3, 3) row-major,
 *   tvec_init (P, 3) f64: the start.
 *   out: rot (P, 3, 3), tvec (P, 3) f64 (may alias rot_init / tvec_init), rms_before, rms_after (P) f64 in px,
 *   lm_iterations (P) int32.  A problem with count < 6 (or a non-finite start) returns its start and 0 iterations.
 * PP_EINVAL (before any launch): a null pointer, P <= 0, Nmax <= 0 or > 4096, max_iters <= 0, eps < 0 or NaN. */
int pp_pnp_refine_lm(const double* object_points, const double* image_points, const int32_t* count, const double* K,
                     const double* rot_init, const double* tvec_init, int P, int Nmax, int max_iters, double eps, double* rot,
                     double* tvec, double* rms_before, double* rms_after, int32_t* lm_iterations, void* stream);

/* ------------------------------------------------------------------------- *
 * RGB-D POSE RECOVERY (picopose_amd/csrc/pp_rgbd_pose.hip; restated in numpy by tests/rgbd_pose_oracle.py)
 * The correspondences of pp_pnp_ransac, each lifted to a 3D-3D pair by the test depth image, RANSAC over three-point rigid
 * fits, a rigid refit on the consensus set: a metric pose from one launch, one 512-thread workgroup per problem, no host wait.
 * This is the project's own algorithm — the project it was modelled on recovers poses from RGB alone — so it is defined by the
 * contract below, not by parity with anything.
 *   The first ten arguments are pp_pnp_ransac's (same layouts, N <= 4096).  depth (n_images, dH, dW) fp32 in the length unit
 *   of src_pts_3d; image_index (P) int32: the depth image each problem reads; inlier_dist (P) fp32: the inlier radius in the
 *   same unit.  out: rot (P,3,3) f64, tvec (P,3) f64, inlier_ratio (P) f64, success, num_points, num_listed (P) int32,
 *   rms (P) f64, inlier_mask (P, N) uint8 or null.
 * Gather.  The entries of tar_pts / src_pts with no -1, in list order, and the object-frame source point (X - t_tem) @ R_tem
 *   in fp32, exactly as pp_pnp_ransac walks and forms them; num_listed is their count (at most 4096).  For each, (u, v) is the
 *   fp32 pair of tar_pts_2d and the pixel is (xi, yi) = (floor(u + 0.5), floor(v + 0.5)), evaluated in fp32.  The entry is
 *   dropped if the pixel lies outside [0, dW) x [0, dH) (a NaN coordinate does) or if z = depth[image, yi, xi] is not finite or
 *   is <= 0.  Otherwise the camera point is q = ((u - cx) z / fx, (v - cy) z / fy, z), evaluated in fp64 from the fp32 values in
 *   that order, with fx, fy, cx, cy = K[0], K[4], K[2], K[5].  num_points is the number kept.  Kept pairs are STORED AS FP32:
 *   the source point as formed, q rounded once from its fp64 value (z is exact); everything below reads those fp32 values and
 *   works in fp64.  An image_index outside [0, n_images) reads no depth: every entry is dropped (num_points 0).
 *   Fewer than 3 kept pairs, or an inlier_dist that is not > 0 (a NaN is not), give the failure outputs of pp_pnp_ransac:
 *   rot = I, tvec = (0, 0, 1), inlier_ratio 0, success 0, rms 0, an all-zero mask; num_listed and num_points are still reported.
 * Hypotheses.  nh = min(iterations, 256).  Hypothesis h of problem p draws 3 distinct indices in [0, num_points) by
 *   pp_pnp_ransac's rule with a sample of 3: s = mix(0x9E3779B9 (p + 1) ^ (h 7919 + 17)), then per index s = mix(s + 0x6D2B79F5),
 *   c = s % num_points, drawn again while c repeats an earlier index (mix: the 32-bit finaliser x ^= x >> 16, x *= 0x7feb352d,
 *   x ^= x >> 15, x *= 0x846ca68b, x ^= x >> 16; uint32 arithmetic).  A sample is degenerate if, in its source or its target
 *   triangle, |a x b|^2 <= 1e-6 |a|^2 |b|^2 for the two edges a, b from its first point; a degenerate sample scores 0.
 *   Otherwise its pose is the least-squares rigid fit q ~ R p + t of the 3 pairs (Horn's quaternion form: the 4x4 symmetric
 *   matrix of the centred cross-covariance, its largest eigenvector by cyclic Jacobi in fp64, t = qm - R pm: a proper rotation
 *   by construction).  Its score is the number of kept pairs with |R p + t - q|^2 <= inlier_dist^2 (fp64; a non-finite residual
 *   is no inlier).  The winner has the highest score, the lowest h among equals; a winning score below 3 is a failure.
 * Refit.  The same rigid fit over the winner's consensus set, its sums (centroids first, then the centred cross-covariance and
 *   the source scatter) reduced in a fixed order: two launches give the same bits.  The refit is returned unless it is not
 *   finite or the set's source points are collinear: l2 <= 1e-6 l1 for the two largest eigenvalues l1 >= l2 of their centred
 *   3x3 scatter matrix; then the winner's pose is returned.  inlier_ratio = winner's score / num_points; rms = sqrt of the mean
 *   squared 3-D residual of the consensus set at the returned pose; inlier_mask = membership of the winner's consensus set in
 *   the order of the listed entries (0 for dropped entries, for the N - num_listed padding slots and for failed problems).
 * PP_EINVAL (before any launch): what pp_pnp_ransac rejects, a null pointer other than inlier_mask, n_images <= 0, dH or
 * dW <= 0, iterations <= 0.  image_index and inlier_dist are device data: a bad value fails its problem (above), nothing is
 * read out of bounds.
 * ------------------------------------------------------------------------- */
int pp_rgbd_ransac(const float* tar_pts_2d, const float* src_pts_3d, const float* K, const float* tem_pose,
                   const int64_t* tar_pts, const int64_t* src_pts, int P, int H, int W, int N,
                   const float* depth, int n_images, int dH, int dW, const int32_t* image_index,
                   const float* inlier_dist, int iterations,
                   double* rot, double* tvec, double* inlier_ratio, int32_t* success,
                   int32_t* num_points, int32_t* num_listed, double* rms, uint8_t* inlier_mask, void* stream);

/* ------------------------------------------------------------------------- *
 * Training forward (model/picopose.py:114-137 — losses only, no gradients; csrc/pp_train.hip)
 * ------------------------------------------------------------------------- */
/* KeyPointSampler.sample_pts (utils/keypoints.py:120-205, Keypoint :47-92, torch_utils.py unproject_points :138-151,
 * project_points :154-161) for B (template = "src", real = "tar") pairs: crop masks (B, mask_h, mask_w), full depth images
 * (B, depth_h, depth_w), crop affines M and their inverses (torch_utils.inverse_affine :93-111), intrinsics K and their
 * inverses, the rigid motions between the two cameras (B,4,4), all fp32 row-major.  The small matrix inverses are the
 * caller's (the reference's torch.inverse); every per-point step is evaluated here as the reference evaluates it,
 * including the comparison of re-projections in CROP pixels with grid points in IMAGE pixels against 1000 px.
 * out: src_pts, tar_pts (B, 4096, 2) fp32 patch coordinates (integer pixel / 3.5), -1 where invalid. */
size_t pp_train_keypoints_workspace_bytes(int B);
int pp_train_keypoints(const float* src_mask, const float* tar_mask, int mask_h, int mask_w, const float* src_depth,
                       const float* tar_depth, int depth_h, int depth_w, const float* src_Minv, const float* tar_Minv,
                       const float* src_M, const float* tar_M, const float* src_Kinv, const float* tar_Kinv, const float* src_K,
                       const float* tar_K, const float* T_src2tar, const float* T_tar2src, int B, float* src_pts, float* tar_pts,
                       void* workspace, size_t workspace_bytes, void* stream);
/* nn.BatchNorm2d in TRAINING mode (model/stage3/dpt.py:64-66,84-90, flow_decoder.py:22) on an NHWC map viewed as
 * (rows, C), C % 4 == 0: y = relu?((x - mean_batch) / sqrt(var_batch + eps) * gamma + beta) + residual + residual2
 * (residuals may be NULL); running_mean / running_var (may both be NULL) get the momentum update with the unbiased
 * variance, as the module does.  Statistics are summed in fp64. */
size_t pp_batchnorm_train_workspace_bytes(int rows, int C);
int pp_batchnorm_train(const float* x, const float* gamma, const float* beta, int rows, int C, float eps, float momentum,
                       float* running_mean, float* running_var, int relu, const float* residual, const float* residual2, float* y,
                       void* workspace, size_t workspace_bytes, void* stream);
/* compute_stage_one_loss (utils/loss_utils.py:144-175): out[i] = F.normalize(src[index[i] * row_stride ...][:C]) — the
 * gather of torch_utils.gather (:257-284) on a token-major feature map and the normalisation of :169-170 in one pass */
int pp_gather_normalize_rows(const float* src, long long row_stride, const int64_t* index, int n, int C, float eps, float* out,
                             void* stream);
/* ... and F.cross_entropy(scale * logits, arange(n)) per row (:171-174): row_loss[i] = logsumexp_j - the diagonal entry */
int pp_xent_diag_rows(const float* logits, int n, int ld, float scale, float* row_loss, void* stream);
/* compute_stage_three_loss for one level (utils/loss_utils.py:188-202 with compute_flow_loss :119-125, RAFTLoss :24-39):
 * flow (B,H,W,2), certainty logits (B,H,W) NHWC, tar_pts (B,4096,2) from pp_train_keypoints.  Writes
 * pp_flow_loss_blocks() x 3 doubles: per workgroup [sum of BCE-with-logits terms, sum over valid pixels with
 * |gt flow| < max_flow of |flow - gt|_1, number of those pixels]; the caller adds the rows and forms the two means. */
int pp_flow_loss_blocks(void);
int pp_flow_loss_sums(const float* flow, const float* certainty, const float* tar_pts, int B, int H, int W, float max_flow,
                      double* partial_sums, void* stream);

/* ------------------------------------------------------------------------- *
 * First backward slice of the training path (utils/lite.py:33-49 -> loss.backward()): the row-wise /
 * element-wise adjoints whose matrix products run on pp_gemm (picopose_amd/autograd.py: dgrad = dz W, wgrad = dz^T x).  Scope:
 * InfoNCE (utils/loss_utils.py:144-175) -> the last ViT block (layers/block.py:82-107); the stage-2 losses (:177-186) -> the
 * AffineRegressor (model/stage2/affine_regressor.py:72-84).  Deterministic (fixed-order reductions, no atomics); csrc/pp_backward.hip.
 * ------------------------------------------------------------------------- */
/* out[c] = sum_r x[r][c] over `rows` rows of ld floats (bias / LayerScale / norm-parameter gradients) */
size_t pp_colsum_workspace_bytes(long long rows, int cols);
int pp_colsum(const float* x, long long rows, int cols, int ld, float* out, void* workspace, size_t workspace_bytes, void* stream);
/* y = act(z) and dz = dy * act'(z) for the PP_ACT_* activations (exact erf GELU, as nn.GELU) */
int pp_act_forward(const float* z, long long n, int act, float* y, void* stream);
int pp_act_backward(const float* z, const float* dy, long long n, int act, float* dz, void* stream);
/* op 0: out = a * b; 1: out = a * b[col] (b a vector of `cols`); 2: out = a + b — n elements, rows of `cols` */
int pp_elementwise(int op, const float* a, const float* b, long long n, int cols, float* out, void* stream);
/* nn.LayerNorm backward: dx (rows, C) and gx = dy * xhat (dgamma = column sums of gx, dbeta = column sums of dy) */
int pp_layernorm_backward(const float* x, const float* gamma, const float* dy, int rows, int C, float eps, float* dx, float* gx, void* stream);
/* nn.GroupNorm(groups, C) (+ReLU when relu != 0) backward on NHWC (B, HW, C): dx, gx = d * xhat and gy = d with d = dy masked by the
 * ReLU (dgamma / dbeta = their column sums) */
int pp_groupnorm_backward_nhwc(const float* x, const float* gamma, const float* beta, const float* dy, int B, int HW, int C, int groups,
                               float eps, int relu, float* dx, float* gx, float* gy, void* stream);
/* softmax backward per row: ds = p * (dp - sum_j dp_j p_j) */
int pp_softmax_backward_rows(const float* p, const float* dp, long long rows, int n, float* ds, void* stream);
/* gradient of pp_xent_diag_rows's mean: dlogits[i][j] = upstream[0] * scale / n * (softmax_j(scale * logits[i]) - [i == j]) */
int pp_xent_diag_backward(const float* logits, int n, int ld, float scale, const float* upstream, float* dlogits, void* stream);
/* dst[index[i]][0..C) += src[i][0..C) for i = 0 .. n-1 — the backward of a row gather (torch.gather under autograd,
 * utils/torch_utils.py:257-283 as used by InfoNCE, utils/loss_utils.py:163-175).  `index` may repeat (several key-points in one
 * feature-grid cell): their rows are added in ascending i, no atomics, so the result does not depend on the launch.  dst (rows, C)
 * contiguous, zeroed or holding a sum to extend; every index must be a valid row of dst. */
int pp_scatter_add_rows(const float* src, const int64_t* index, int n, int C, float* dst, void* stream);
/* F.normalize backward for the rows x[index[i] * row_stride ...] (index NULL: row i): dx (rows, C) contiguous */
int pp_normalize_rows_backward(const float* x, long long row_stride, const int64_t* index, const float* dq, int rows, int C, float eps,
                               float* dx, void* stream);
/* im2col of an NHWC image for a ksize x ksize / stride / pad convolution (k order (ky, kx, ci), as pack_conv_weight) and its adjoint */
int pp_im2col_nhwc(const float* x, int B, int H, int W, int C, int ksize, int stride, int pad, float* col, void* stream);
int pp_col2im_nhwc(const float* col, int B, int H, int W, int C, int ksize, int stride, int pad, float* dx, void* stream);
/* pp_split_weights_t with a GIVEN scale (device scalar; a power of two): the operand of a weight whose scale the host already knows
 * (the training graph re-splits every weight each step with the scale read back one step earlier: no host wait) */
int pp_split_with_scale_t(const float* w, long long n, int terms, const float* scale, void* out, void* stream);
/* scale2[0] = the power of two s with max|x| s in [512, 1024) (1 for an all-zero x), scale2[1] = 1 / s — the range normalisation of a
 * gradient operand before a backward product (picopose_amd/autograd.py: _ranged); device scalars, no host sync */
int pp_pow2_scale(const float* x, long long n, float* scale2, void* stream);
/* im2col written transposed: colT (ksize^2 C, rows), rows = B Ho Wo — the K-major operand of the weight-gradient product */
int pp_im2col_t_nhwc(const float* x, int B, int H, int W, int C, int ksize, int stride, int pad, float* colT, void* stream);
/* adjoint of pp_similarity_volume's tail (mask, clamp at 0, the [s][h][w] layout with t = w 16 + h; utils/matching.py:21-25):
 * out / dout (B,256,16,16) -> dS (B, t = 256, s = 256), the gradient of the cosine matrix <tar_hat[t], src_hat[s]> */
int pp_simvol_backward(const float* out, const float* dout, const float* src_mask, int mask_h, int mask_w, int B, float* dS, void* stream);

/* ---- adjoints of stage 3's training path (csrc/pp_backward3.hip; each restates its forward kernel's coordinate arithmetic) ---- */
/* nn.BatchNorm2d in training mode (pp_batchnorm_train: batch statistics, biased variance) on (rows, C), y = relu?(bn(x)):
 * dx, dgamma, dbeta from dy; the ReLU mask is recomputed from x (beta is needed for it) */
size_t pp_batchnorm_train_backward_workspace_bytes(long long rows, int C);
int pp_batchnorm_train_backward(const float* x, const float* gamma, const float* beta, const float* dy, long long rows, int C, float eps,
                                int relu, float* dx, float* dgamma, float* dbeta, void* workspace, size_t workspace_bytes, void* stream);
/* adjoint of pp_resize_bilinear_nhwc (align_corners = True, result scaled by mul): dy (B,Ho,Wo,C) -> dx (B,H,W,C), gather form */
int pp_resize_bilinear_backward_nhwc(const float* dy, int B, int H, int W, int C, int Ho, int Wo, float mul, float* dx, void* stream);
/* adjoint of pp_avgpool2_nhwc: dy (B,H/2,W/2,C) -> dx (B,H,W,C) (accumulate != 0: added to dx) */
int pp_avgpool2_backward_nhwc(const float* dy, int B, int H, int W, int C, int accumulate, float* dx, void* stream);
/* adjoint of pp_warp_nhwc (FlowDecoder.feature_sample): dfeat (B,H,W,C) must be ZERO on entry (atomic scatter), dflow (B,H,W,2) */
int pp_warp_backward_nhwc(const float* feat, const float* flow, const float* dy, int B, int H, int W, int C, int ld_flow, float* dfeat,
                          float* dflow, void* stream);
/* adjoint of pp_corr_lookup_nhwc (correlation pyramid + lookup): f2_levels[l] = the query map pooled l times (B, H>>l, W>>l, C);
 * df1 (B,H,W,C) is written, df2_levels[l] must be ZERO on entry (atomic scatter), dflow (B,H,W,2).  C <= 256, levels <= 3 */
int pp_corr_lookup_backward_nhwc(const float* f1, const float* const* f2_levels, const float* flow, const float* dout, int B, int H, int W,
                                 int C, int levels, int radius, int ld_flow, int ld_dout, float* df1, float* const* df2_levels, float* dflow,
                                 void* stream);
/* The deterministic forms of the two scatter adjoints: the scattered sums (dfeat; df2 per level) accumulate in 64-bit FIXED POINT
 * (2^-40 units, integer atomics: the same bits whatever order the workgroups arrive in) into caller-zeroed long long buffers of the
 * same element counts; pp_fixed_to_float turns them into the fp32 gradients.  df1 / dflow are written directly as before. */
int pp_warp_backward_nhwc_fixed(const float* feat, const float* flow, const float* dy, int B, int H, int W, int C, int ld_flow,
                                long long* dfeat_acc, float* dflow, void* stream);
int pp_corr_lookup_backward_nhwc_fixed(const float* f1, const float* const* f2_levels, const float* flow, const float* dout, int B, int H,
                                       int W, int C, int levels, int radius, int ld_flow, int ld_dout, float* df1,
                                       long long* const* df2_acc_levels, float* dflow, void* stream);
int pp_fixed_to_float(const long long* acc, long long n, float* out, void* stream);
/* adjoint of pp_flow_loss_sums for one level: g_flow[0] = upstream * flow_weight / (count + eps), g_cert[0] = upstream * mask_weight /
 * (B H W) (device scalars) -> dflow (B,H,W,2), dcertainty (B,H,W) */
int pp_flow_loss_backward(const float* flow, const float* certainty, const float* tar_pts, int B, int H, int W, float max_flow,
                          const float* g_flow, const float* g_cert, float* dflow, float* dcertainty, void* stream);


/* ---- fused optimizer step (csrc/pp_optim.hip) ----
 * Replaces the reference's `optim.AdamW` / `optim.Adam` step (run_train.py:79-85, config/base.yaml:9-20), i.e. torch's
 * `_single_tensor_adam` per parameter, with two launches over ALL tensors: pass 1 updates p, exp_avg (m) and exp_avg_sq (v) in chunks of
 * PP_ADAM_CHUNK elements; pass 2 (only when some tensor has an `hl` buffer and terms > 0) re-splits those tensors into the engine's weight
 * operand — bit for bit what pp_split_weights_ws writes for the updated weight (hl layout, scale2 = [2^e, 2^-e]).
 * The table (PpAdamTensor[], stable across steps: updates are in place) is laid out in the workspace when `rebuild` != 0 (the call then
 * waits for the stream once); every step passes the per-tensor step record array `steps` (device memory, PpAdamStep[ntensors]).
 * Per element, in fp32 and in torch's order:  mode 1 (AdamW): p *= decay;  mode 2 (Adam + weight decay): g += decay * p;
 *   m = lerp(m, g, lerp_w);  v = v * beta2 + one_minus_beta2 * g * g;  p += neg_step_size * (m / (sqrt(v) * inv_bc2_sqrt + eps)),
 * each torch op rounded on its own.  The host forms neg_step_size = -lr / (1 - beta1^step) and bc2_sqrt = sqrt(1 - beta2^step) in
 * double, like torch, and inv_bc2_sqrt = 1 / bc2_sqrt in double, rounded to fp32 (ATen's division by a scalar).
 * Tensors with n % 8 != 0 are updated and never split.  Null pointers, n <= 0, ntensors <= 0, terms not in {0,1,2}: PP_EINVAL. */
#define PP_ADAM_CHUNK 65536
typedef struct PpAdamTensor {
    float* p;          /* parameter (n,) contiguous fp32, updated in place                                      */
    float* m;          /* exp_avg (n,)                                                                           */
    float* v;          /* exp_avg_sq (n,)                                                                        */
    void* hl;          /* operand buffer pass 2 writes (fp16, terms * n halfs), or NULL: not split               */
    float* scale2;     /* [2^e, 2^-e] of that split (NULL when hl is NULL)                                       */
    long long n;
} PpAdamTensor;
/* PpAdamStep arrays live in DEVICE memory: the Python binding passes `steps` as a raw address (picopose_amd/_lib.py _DEVICE_STRUCTS
 * names the struct; a further device-resident struct is added there). */
typedef struct PpAdamStep {
    const float* g;    /* gradient (n,) contiguous fp32 (may move between steps)                                 */
    float neg_step_size, inv_bc2_sqrt, decay, lerp_w, beta2, one_minus_beta2, eps;
    int mode;          /* 0: no weight decay, 1: decoupled (decay = 1 - lr wd), 2: L2 (decay = wd)                 */
} PpAdamStep;
int pp_adam_workspace_bytes(const PpAdamTensor* tensors, int ntensors, size_t* bytes);
int pp_adam_multi_tensor(const PpAdamTensor* tensors, int ntensors, const PpAdamStep* steps, int terms, int rebuild, void* workspace,
                         size_t workspace_bytes, void* stream);

/* -------------------------------------------------------------------------
 * Training-pair assembly (provider/training_dataset.py:173-316; picopose_amd/provider/training_batch.py plans every call).
 *
 * Frames: buffer 0 = real views, (H_f, W_f, 3) uint8 RGB as load_im gives it plus the visible mask (H_f, W_f) uint8;
 * buffer 1 = template views, (H_f, W_f, 4) RGBA.  Crops live in two ragged "ping-pong" buffers of 4-byte pixels, the colour
 * BGR-ordered (image[..., ::-1]) and byte 3 the mask / alpha, carried along.
 *
 * images: n_images descriptors of PP_AUG_IMG_WORDS int32:
 *   [0] frame buffer (0: frames0, 1: frames1)  [1] pixel offset of the frame  [2] W_f  [3] y1  [4] x1  [5] h  [6] w
 *   [7] pixel offset of the crop in the ragged buffers  [8] seed (uint32 bits)  [9] index of the image's first op record
 *   [10] nseg = passes the image takes (1..4)  [11 + s] first op of pass s, s = 0..nseg ([11 + nseg] = op count)
 *   [16] mask mode (0: real, mask value out; 1: alpha, out = (alpha == 255))  [17..19] 0
 * ops: records of PP_AUG_OP_WORDS int32, word 0 the recipe row (1..13), then (floats as their bit patterns):
 *   1 CoarseDropout: -               2 GaussianBlur: radius, taps q0..q4 (sum q0 + 2 (q1..q4) = 256), sigma
 *   3-6 Sharpness / Contrast / Brightness / Color: factor   7 Add: three ints   8 Invert: three 0/1 flags
 *   9, 10 Multiply: three factors    11 AdditiveGaussianNoise: -   12 LinearContrast: three alphas   13 Grayscale: alpha
 * Pass s > 0 of an image starts with its Blur, Sharpness or Contrast op and runs the pointwise ops up to the next one; pass 0
 * crops the frame.  Pass p writes buf0 when p is even, buf1 when odd; an image's result is in buffer (nseg - 1) & 1.
 * Random ops use the counter-based hash h(seed, a, b) = mix(seed ^ mix(a ^ mix(b + 0x9e3779b9))), mix = the
 * "lowbias32" finalizer (x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16):
 *   dropout drops cell c (grid max(h*5/100, 3) x max(w*5/100, 3), nearest) when h(seed, c, 0xd0) < PP_AUG_DROP_THRESHOLD;
 *   noise of pixel p (= y w + x), channel c is ((2 sum of the 12 bytes of h(seed, 3p + c, k), k < 3) - 3060) * 10 + 256) >> 9
 *   (an Irwin-Hall sum scaled to std ~10, not a true normal and not imgaug's stream).
 * ------------------------------------------------------------------------- */
#define PP_AUG_OP_WORDS 8
#define PP_AUG_IMG_WORDS 20
#define PP_AUG_MAX_OPS 13
#define PP_AUG_MAX_PASSES 4
#define PP_AUG_DROP_THRESHOLD 858993459u /* 0.2 * 2^32 */
/* Runs every pass: tiles = int4 {image, y0, x0, 0} of 16 x 16 pixels, pass p's tiles at [pass_tiles[p], pass_tiles[p+1])
 * (pass_tiles: HOST array of n_passes + 1 ints, pass_tiles[0] = 0, pass 0 non-empty); n_frame*_px / n_buf_px: uchar4 counts
 * of the buffers (descriptors outside them are skipped); lsum: n_images uint32 workspace (zeroed here). */
int pp_augment_execute(const unsigned char* rgb0, const unsigned char* mask0, long long n_frame0_px, const unsigned char* rgba1,
                       long long n_frame1_px,
                       const int* images, int n_images, const int* ops, int n_ops, const int* tiles, const int* pass_tiles,
                       int n_passes, unsigned char* buf0, unsigned char* buf1, long long n_buf_px, unsigned int* lsum,
                       void* stream);
/* The executor's results -> out_rgb (n_images, 3, S, S) fp32 = Normalize(resize(crop [* (mask > 0) if rgb_mask_flag]) / 255)
 * in double, out_mask (n_images, S, S) fp32 = INTER_NEAREST of the mask byte.  The resize is OpenCV's cv::resize on CV_8U,
 * INTER_LINEAR fixed-point path in its scalar form (11-bit coefficients saturate_cast<short>((1 - f) 2048), integer
 * horizontal pass, (v + 2^21) >> 22 vertical; the SIMD vertical pass of OpenCV rounds in two steps and may differ by 1 LSB),
 * switching to INTER_AREA ((a + b + c + d + 2) >> 2) for an exact 2x downscale (h = w = 2 S).  mean3 / std3: host. */
int pp_augment_resize(const unsigned char* buf0, const unsigned char* buf1, long long n_buf_px, const int* images, int n_images,
                      int S, int rgb_mask_flag, const double* mean3, const double* std3, float* out_rgb, float* out_mask,
                      void* stream);
/* real depth (training_dataset.py:227-228): out = f32(d) * scale[frame] / 1000 in float32; depth (n_frames, n_per_frame)
 * uint16 (8-byte aligned), scale: device fp32 per frame, out 16-byte aligned. */
int pp_depth_u16_scaled(const unsigned short* depth, long long n_per_frame, int n_frames, const float* scale, float* out,
                        void* stream);
/* template depth (training_dataset.py:294): out = (float)(d * 0.1 / 1000.0) in double. */
int pp_depth_u16_template(const unsigned short* depth, long long n, float* out, void* stream);

/* -------------------------------------------------------------------------
 * Detection batch of one test image (provider/bop_test_dataset.py:112-207; picopose_amd/provider/test_batch.py plans the call):
 * pp_crop_resize_normalize for n detections of one frame in one launch, the masks given as COCO run lengths instead of frames.
 * THE RUN TABLES (run_ends, run_offset, run_offset_host) are stated here once; pp_rle_pack_bits reads and pp_components_rle writes the
 * same tables.  picopose_amd/masks.py builds them; csrc/pp_runs_dev.h holds the checks and the search that their readers share.
 *
 * image (H, W, 3) uint8 as loaded (H * W < 2^31).  run_ends: the detections' cumulative run ends, concatenated — detection d owns
 * run_ends[run_offset[d] .. run_offset[d + 1]), the inclusive prefix sums of its COCO counts (column-major over (H, W), runs
 * alternate 0-run, 1-run, ..., so they are non-decreasing and the last one is H * W).  Pixel (y, x) is in the mask when an odd
 * number of ends are <= x * H + y.  window[d] = {y1, y2, x1, x2}: crop rows [y1, y2), columns [x1, x2).
 * out_rgb (n, 3, S, S), out_mask (n, S, S) fp32: per detection exactly what pp_crop_resize_normalize writes for the decoded mask
 * (same arithmetic, bit for bit); mean3 / std3 host pointers.
 * run_ends, run_offset (n + 1 ints) and window (4 n ints) are device pointers; run_offset_host / window_host are the HOST copies
 * of the two tables, validated here before the launch.  PP_EINVAL: a null pointer, n <= 0 or > 65535, S <= 0 or > 4096, n_runs <= 0,
 * H * W >= 2^31, run_offset_host decreasing, negative or past n_runs, a window that is empty or leaves the frame.  A workgroup
 * stages the ends that touch its source columns in LDS when they are at most 2048, and searches global memory otherwise.
 * ------------------------------------------------------------------------- */
int pp_detections_crop(const unsigned char* image, int H, int W, const int* run_ends, int n_runs, const int* run_offset,
                       const int* window, const int* run_offset_host, const int* window_host, int n, int S, int rgb_mask_flag,
                       const double* mean3, const double* std3, float* out_rgb, float* out_mask, void* stream);

/* -------------------------------------------------------------------------
 * Template rendering: a mesh to its rendered template views and their bank entries (picopose_amd/provider/template_bank.py plans
 * every call).  Replaces the offline renderer rendering/src/custom_megapose/call_panda3d.py:48-98 (ambient light of colour 1:
 * a pixel is the surface colour, unshaded; K and the 480 x 640 frame of :48-54; RGBA + 16-bit depth in mm of :87-98) for
 * vertex-coloured meshes.  Parity with Panda3D / BlenderProc pixels is UNPINNED (neither can be run next to this library);
 * the conventions below are the places where it could differ.
 *
 * THE RASTER CONTRACT (tests/render_oracle.py restates it in numpy; the kernels equal it bit for bit).  All float operations
 * are IEEE float32, one rounding each, never contracted, in the order written.
 *  1. Camera space of vertex (X, Y, Z) under the row-major pose P (4, 4) (object -> camera, t in the vertices' unit):
 *       Xc = ((P00 X + P01 Y) + P02 Z) + P03, Yc and Zc likewise from rows 1 and 2.
 *     A triangle with a vertex whose Zc > near is false is dropped whole and counted in *near_count (no geometric clipping).
 *  2. Projection u = (fx Xc) / Zc + cx, v = (fy Yc) / Zc + cy.  Pixel (x, y) is sampled at (u, v) = (x, y): integer coordinates
 *     are pixel centres — the convention of get_point_cloud_from_depth (utils/data_utils.py:97-115), so a rendered depth
 *     back-projects onto the surface point that produced it.  (Whether Panda3D samples at x or x + 1/2 is unpinned.)
 *  3. Snap: xs = (int) rint(clamp(256 u, -2^28, 2^28)) (round half to even), ys likewise: 1/256 pixel fixed point.
 *  4. area2 = (xs1 - xs0)(ys2 - ys0) - (ys1 - ys0)(xs2 - xs0) in 64-bit integers.  area2 = 0: the triangle covers nothing.
 *     area2 < 0: vertices 1 and 2 are exchanged (both windings are drawn, there is no back-face culling), so area2 > 0 below.
 *  5. Edge function of a -> b at the sample (256 x, 256 y): E = (xb - xa)(256 y - ya) - (yb - ya)(256 x - xa), 64-bit exact.
 *     w0 = E(1 -> 2), w1 = E(2 -> 0), w2 = E(0 -> 1); w0 + w1 + w2 = area2.  The sample is covered when every w_k >= 0 and
 *     every edge with w_k = 0 is a left edge (yb < ya) or a top edge (yb = ya and xb > xa) — the top-left fill rule, y down:
 *     two triangles sharing an edge cover each sample of it exactly once.  Samples are taken for 0 <= x < W, 0 <= y < H
 *     inside the triangle's box only (clipping by the box, not by geometry).
 *  6. Perspective weights p_k = ((float) w_k / (float) area2) * (1 / Zc_k), q = (p0 + p1) + p2, depth Z = 1 / q: camera Z
 *     (not ray length), 1 / Z linear in screen space.  Colour channel c = min(255, max(0, floor(((p0 c0 + p1 c1) + p2 c2) / q + 0.5)))
 *     with c_k the vertex colours as floats; alpha = 255 where covered, the pixel is (0, 0, 0, 0) elsewhere.
 *  7. Depth test: the fragment with the smallest Z wins a sample; equal Z: the lowest face index.  The result does not depend
 *     on launch order, stream or chunking: it is a 64-bit unsigned atomic minimum over (bits of Z) << 32 | face.
 *  8. depth_mm = (uint16) min(65535, rint(1000 * Z)) (round half to even), 0 on background: what `*_depth.png` holds when the
 *     vertices are in metres.  (bop_toolkit's save_depth is recalled to round with np.round; not verifiable here.)
 *     depth_m = Z (0 on background), face_id = the winning face (-1 on background).
 *
 * vertices (Nv, 3) fp32, faces (Nf, 3) int32, colors (Nv, 3) uint8 RGB, poses (V, 4, 4) fp32: device.  faces_host: the HOST copy
 * of faces, range-checked here before any launch (the kernels skip a triangle whose device indices are out of range anyway).
 * rgba (V, H, W, 4) uint8 (4-byte aligned), depth_mm (V, H, W) uint16; depth_m (V, H, W) fp32 and face_id (V, H, W) int32 may be
 * NULL; near_count: one device uint32, zeroed here.  The views are rendered in chunks of as many views as the workspace holds
 * (pp_render_workspace_bytes(H, W, Nf, chunk) = 256 + chunk (H W + Nf) 8 bytes: a 64-bit depth/face word per sample and a queue
 * slot per triangle); any chunk size gives the same bytes.  All work is enqueued on `stream`; nothing synchronises.
 * PP_EINVAL: null pointer, V / Nv / Nf / H / W <= 0, H W >= 2^31, near <= 0, fx or fy = 0, an index of faces_host outside
 * [0, Nv).  PP_EWORKSPACE: workspace misaligned (256 B) or smaller than one view needs.
 * ------------------------------------------------------------------------- */
int pp_render_workspace_bytes(int H, int W, int n_faces, int chunk_views, size_t* bytes);
int pp_render_views(const float* vertices, int n_vertices, const int* faces, const int* faces_host, int n_faces,
                    const unsigned char* colors, const float* poses, int n_views, float fx, float fy, float cx, float cy, int H,
                    int W, float near, void* workspace, size_t workspace_bytes, unsigned char* rgba, unsigned short* depth_mm,
                    float* depth_m, int* face_id, unsigned int* near_count, void* stream);
/* -------------------------------------------------------------------------
 * THE TEXTURE CONTRACT: the same render for a UV-textured mesh (BOP's `obj_NNNNNN.ply` with `texture_u texture_v` and a
 * `comment TextureFile`).  The reference's recipe is textured and unshaded: rendering/src/custom_megapose/panda3d_scene_renderer.py:70-73
 * sets `texture-minfilter mipmap` and call_panda3d.py:57-62 lights the object with ambient light of colour 1, so a pixel is the
 * filtered texture colour.  Items 1-5, 7 and 8 of THE RASTER CONTRACT (coverage, depth, alpha, depth_mm, face_id) hold unchanged;
 * only the colour of item 6 changes, to T3-T5.  tests/texture_oracle.py restates T2-T5 in numpy; the kernels equal it bit for bit.
 * Float operations are IEEE float32, one rounding each, never contracted, in the order written.
 *  T1. Inputs.  The texture is (Ht, Wt, 3) uint8 RGB, row 0 the top row of the image file, 1 <= Wt, Ht <= PP_TEXTURE_MAX.  UVs are
 *      per corner: face_uv (Nf, 3, 2) float32 = (u, v) of corner k of face f, in the order of `faces`; u runs to the right, v runs
 *      UP (v = 0 is the bottom row of the image: the PLY / OBJ / Panda3D convention).  Per-corner UVs are the only device layout;
 *      per-vertex UVs are expanded by the caller (uv[faces]).
 *  T2. Mip pyramid (pp_texture_build_mips, once per texture).  Level 0 is the image.  Level l + 1 has W' = max(1, W_l >> 1) by
 *      H' = max(1, H_l >> 1) texels; texel (x, y) is (a + b + c + d + 2) >> 2 per channel over the four taps
 *      (min(2x, W_l - 1) | min(2x + 1, W_l - 1), min(2y, H_l - 1) | min(2y + 1, H_l - 1)) of level l.  Levels go down to 1 x 1.
 *      Integer arithmetic: the pyramid equals a numpy one bit for bit.  Storage: uchar4 texels {r, g, b, 255}, row-major, the
 *      levels back to back from level 0 (pp_texture_mips_bytes gives the size and the number of levels), so each of a sample's
 *      four texels is one 4-byte load.
 *  T3. Level of detail: one level per (view, face), constant over the triangle, recomputed for the winning face by the resolve pass
 *      (nothing is stored per triangle).  With the corner UVs in the order item 4 left the corners in,
 *        A_t = (fabsf(((u1 - u0) (v2 - v0)) - ((v1 - v0) (u2 - u0))) * (float) Wt) * (float) Ht     (twice the texel area)
 *        A_p = (float) area2 / 65536                                                                (twice the pixel area)
 *      the level is the smallest l >= 0 with A_t <= (2 A_p) 4^l, capped at the last level; (2 A_p) 4^l is formed by repeated
 *      multiplication by 4, which is exact — no log2.  A_t that is zero or NaN gives level 0.  A linear footprint (texels per pixel)
 *      of 1 therefore samples level 0, 2 level 1, 4 level 2: the switch points lie at sqrt(2) 2^k.  Exchanging corners 1 and 2
 *      negates the determinant exactly, so the level does not depend on the winding.
 *  T4. Coordinates at a covered sample: u = ((p0 u0 + p1 u1) + p2 u2) / q and v likewise, p_k and q of item 6 (perspective
 *      correct).  Wrap mode repeat on both axes: u' = u - floorf(u), v' = v - floorf(v).
 *  T5. Bilinear sample of level l (W_l x H_l): x = u' W_l - 0.5, y = (1 - v') H_l - 0.5 (texel centres at half-integer texture
 *      coordinates, v flipped); x0 = floorf(x), fx = x - x0, y0 = floorf(y), fy = y - y0; taps x0, x0 + 1 and y0, y0 + 1 reduced by
 *      a positive modulo of W_l / H_l (u', v' in [0, 1] put x0 in [-1, W_l - 1]: -1 wraps to W_l - 1 and W_l to 0).  Per channel,
 *      with c_yx the texels as floats: a = c00 + fx (c01 - c00), b = c10 + fx (c11 - c10), val = a + fy (b - a),
 *      out = min(255, max(0, floorf(val + 0.5))); alpha = 255.  A coordinate that is not finite (UVs that are, or overflow) reads
 *      texels inside the level and gives an unspecified colour, never a fault.
 *  T6. OUT OF SCOPE: anisotropic filtering and trilinear blending between levels (one level per face, chosen by area); clamp and
 *      mirror wrap modes; texture alpha (a texel's alpha is ignored: convert to RGB first); more than one texture per mesh.
 *      Silhouettes of this entry are single-sampled as in item 5; multisampled edges (the reference enables 4x MSAA) are THE
 *      MULTISAMPLE CONTRACT below, through pp_render_views_ms.  Shading is THE SHADING CONTRACT below; what it leaves out is S9.
 *      Parity with Panda3D's pixels stays UNPINNED, as for the rest of the render.
 *
 * pp_texture_mips_bytes: *bytes = 4 * the texels of all levels, *levels (may be NULL) = their number.  PP_EINVAL: bytes NULL, Wt or
 * Ht outside [1, PP_TEXTURE_MAX].
 * pp_texture_build_mips: rgb (Ht, Wt, 3) uint8 and mips (4-byte aligned, mips_bytes >= pp_texture_mips_bytes) on the device; packs
 * level 0 and builds every further level, one launch per level, on `stream`.  PP_EINVAL: null pointer, size out of range, mips
 * misaligned or too small.
 * pp_render_views_textured: pp_render_views with `colors` replaced by face_uv (Nf, 3, 2) fp32, the pyramid and the texture's size;
 * the coverage launches are the same, the resolve pass implements T3-T5.  Everything said of pp_render_views' other arguments,
 * chunking and errors holds; also PP_EINVAL: face_uv or mips NULL or not 4-byte aligned, Wt or Ht outside [1, PP_TEXTURE_MAX].
 * ------------------------------------------------------------------------- */
#define PP_TEXTURE_MAX 16384
int pp_texture_mips_bytes(int Wt, int Ht, size_t* bytes, int* levels);
int pp_texture_build_mips(const unsigned char* rgb, int Wt, int Ht, void* mips, size_t mips_bytes, void* stream);
int pp_render_views_textured(const float* vertices, int n_vertices, const int* faces, const int* faces_host, int n_faces,
                             const float* face_uv, const void* mips, int Wt, int Ht, const float* poses, int n_views, float fx,
                             float fy, float cx, float cy, int H, int W, float near, void* workspace, size_t workspace_bytes,
                             unsigned char* rgba, unsigned short* depth_mm, float* depth_m, int* face_id, unsigned int* near_count,
                             void* stream);
/* -------------------------------------------------------------------------
 * THE SHADING CONTRACT: the same render, lit.  The reference renders T-LESS and ITODD from their untextured CAD meshes with
 * BlenderProc under eight point lights (rendering/scripts/render_bop_templates.py:131, rendering/src/lib3d/blenderproc.py:29-39,
 * :54-57); unlit, such a mesh is a flat silhouette.  pp_render_views_lit multiplies the base colour of a covered sample by
 * ambient + Lambert diffuse.  tests/shading_oracle.py restates S2-S8 in numpy; the kernels equal it bit for bit.  Float operations
 * are IEEE float32, one rounding each, never contracted, in the order written; only `/` and sqrtf (both correctly rounded) are
 * used besides + - *: no reciprocal square root, no fast intrinsic, no powf.
 *  S1. Inputs.  n_lights in [0, PP_MAX_LIGHTS]; light k is (x, y, z, I_k) float32 in camera space (the frame of item 1: x right,
 *      y down, z forward) in the vertices' unit, finite, I_k >= 0.  ambient >= 0.  Base colour of a covered sample: the uchar4
 *      the UNLIT render writes there (vertex colours by item 6, or the texture by T3-T5), or a constant RGB triple when one is
 *      given (a constant overrides both).  Normal mode flat or smooth.  Optional tone table: T uint8 entries on the device,
 *      2 <= T <= PP_TONE_MAX.
 *  S2. Position P = ((p0 C0 + p1 C1) + p2 C2) / q per coordinate: C_k the camera-space corners of item 1 in the order item 4
 *      left them, p_k and q of item 6.
 *  S3. Normal.  Flat: e1 = C1 - C0, e2 = C2 - C0, n = e1 x e2 with every component formed as (a b) - (c d):
 *        nx = (e1y e2z) - (e1z e2y), ny = (e1z e2x) - (e1x e2z), nz = (e1x e2y) - (e1y e2x).
 *      Exchanging corners 1 and 2 negates n exactly, so the result after the facing step does not depend on the winding.
 *      Smooth: o = (p0 N0 + p1 N1) + p2 N2 per component, N_k the object-space vertex normals (S8, or the model's own) of those
 *      corners; rotated by the pose's 3 x 3 block, assumed orthonormal: nx = ((P00 ox + P01 oy) + P02 oz), ny and nz from rows 1, 2.
 *      Both: len2 = (nx nx + ny ny) + nz nz.  When len2 > 0 is false the sample gets s = 0 (ambient only).  Otherwise
 *      n = n / sqrtf(len2) per component, then facing (two-sided, matching "no back-face culling"): when
 *      ((nx Px + ny Py) + nz Pz) > 0, n = -n.
 *  S4. Lights in index order, s starting at 0: L = L_k - P; d2 = (Lx Lx + Ly Ly) + Lz Lz; ndl = (nx Lx + ny Ly) + nz Lz;
 *      when ndl > 0 and d2 > 0: s = s + (I_k ndl) / (d2 sqrtf(d2)).  (Inverse-square fall-off times the cosine.)
 *  S5. m = ambient + s.  Per channel val = (float) base_c * m.
 *  S6. Output.  Without a table: out = min(255, max(0, floorf(val + 0.5))).  With a table: idx = (int) rintf(fminf(val / 255, 1) * (float)(T - 1))
 *      (round half to even), clamped to [0, T - 1] (a no-op for the inputs of S1), out = table[idx].  Alpha = 255.
 *  S7. Coverage, depth, depth_mm, depth_m, face_id and alpha are items 1-5, 7 and 8, unchanged: shading moves colour only.
 *  S8. Vertex normals (pp_vertex_normals, once per mesh).  For vertex v: the sum, over the entries vf_faces[vf_offsets[v] ..
 *      vf_offsets[v + 1]) in that order, of the object-space (V1 - V0) x (V2 - V0) of the face (area-weighted, un-normalised,
 *      the face's own corner order, components as in S3), every component accumulated sequentially in float32 from 0; then
 *      normalised as in S3 (zeros when len2 > 0 is false: an unreferenced vertex, or faces without area).  The adjacency is a
 *      CSR pair built on the host: a stable sort of faces.reshape(-1) by vertex, so a vertex's faces come in ascending face
 *      index (a face that names v twice is listed twice and adds zero).  No float atomics: the bytes do not depend on launch order.
 *  S9. OUT OF SCOPE: specular terms, shadows, coloured or spot lights, decoding base colours from sRGB, angle-threshold "auto
 *      smooth".  (4x multisampling is THE MULTISAMPLE CONTRACT below, through pp_render_views_ms; this entry is single-sampled.)
 *      Parity with Cycles / pyrender pixels stays UNPINNED, as for the rest of the render.
 *
 * pp_vertex_normals: vertices (Nv, 3) fp32, faces (Nf, 3) int32, vf_offsets (Nv + 1) int32, vf_faces (3 Nf) int32, normals (Nv, 3)
 * fp32 out: device.  One launch on `stream`, nothing synchronises.  An entry of the lists that is out of range is skipped, never a
 * fault.  PP_EINVAL: null or misaligned (4 B) pointer, Nv or Nf <= 0, 3 Nf >= 2^31.
 * pp_render_views_lit: the arguments of pp_render_views and pp_render_views_textured together, then the shading.  Colour source:
 * `colors`, or face_uv + mips (+ Wt, Ht), or neither (NULL, NULL, NULL, 0, 0) with base_color_host.  lights_host: n_lights x 4 floats
 * on the HOST, copied into the kernel arguments; base_color_host: 3 bytes on the HOST or NULL; normals (Nv, 3) fp32 on the device
 * (needed for PP_NORMALS_SMOOTH only); tone_table: tone_entries bytes on the device, or NULL with tone_entries = 0.  The coverage
 * launches, the workspace (pp_render_workspace_bytes), chunking and everything pp_render_views rejects are unchanged; all work is
 * enqueued on `stream`, nothing synchronises.  Also PP_EINVAL, before any launch: n_lights outside [0, PP_MAX_LIGHTS] or lights_host
 * NULL with n_lights > 0; a light that is not finite or has I < 0; ambient negative or not finite; normal_mode not one of the two;
 * smooth without normals; no colour source (and no constant); both colour sources; face_uv without mips or the reverse; Wt / Ht out
 * of range with a texture; tone_entries outside [2, PP_TONE_MAX] with a table, or != 0 without; lights_host, normals, face_uv or mips
 * not 4-byte aligned.
 * ------------------------------------------------------------------------- */
#define PP_MAX_LIGHTS 16
#define PP_TONE_MAX 65536
#define PP_NORMALS_FLAT 0
#define PP_NORMALS_SMOOTH 1
int pp_vertex_normals(const float* vertices, int n_vertices, const int* faces, int n_faces, const int* vf_offsets, const int* vf_faces,
                      float* normals, void* stream);
int pp_render_views_lit(const float* vertices, int n_vertices, const int* faces, const int* faces_host, int n_faces,
                        const unsigned char* colors, const float* face_uv, const void* mips, int Wt, int Ht, const float* poses,
                        int n_views, float fx, float fy, float cx, float cy, int H, int W, float near, void* workspace,
                        size_t workspace_bytes, unsigned char* rgba, unsigned short* depth_mm, float* depth_m, int* face_id,
                        unsigned int* near_count, const float* lights_host, int n_lights, float ambient, int normal_mode,
                        const float* normals, const unsigned char* base_color_host, const unsigned char* tone_table, int tone_entries,
                        void* stream);
/* -------------------------------------------------------------------------
 * THE MULTISAMPLE CONTRACT: the same render with 4x anti-aliased colour and alpha.  The reference renders its templates with
 * `framebuffer-multisample 1` / `multisamples 4` (rendering/src/megapose/panda3d_renderer/panda3d_scene_renderer.py:72-73 and
 * set_antialias(MAuto) at :99), so its PNGs hold partial alpha along silhouettes; pp_template_extents (alpha != 0) and
 * pp_templates_crop (mask from alpha == 255, colour mask from alpha > 0) already treat such frames as `_get_template` does.
 * tests/multisample_oracle.py restates M1-M5 in numpy; the kernels equal it bit for bit.  Pixel parity with Panda3D stays
 * UNPINNED, and the effect of the option on pose accuracy is UNMEASURED (no trained weights were available to measure it).
 * A multisampled render of a view has S = 4 SAMPLE PLANES and one CENTRE PLANE.
 *  M1. Sample positions.  Plane s of pixel (x, y) is sampled at the sub-pixel position (256 x + ox_s, 256 y + oy_s) in the 1/256
 *      pixel fixed point of item 3, (ox, oy) = (-32, -96), (96, -32), (-96, 32), (32, 96) for s = 1 .. 4: the standard rotated-grid
 *      4x pattern in 1/16 pixel, times 16.  The centre plane (plane 0) has offset (0, 0).  Which pattern the reference's GL driver
 *      used is unpinned.
 *  M2. Each plane is a full render under THE RASTER CONTRACT: items 1-7 hold with the sample point of item 5 moved by the offset.
 *      The edge functions only see differences, so this is exactly the single-sample render of the triangle whose SNAPPED
 *      coordinates are (xs - ox, ys - oy): area2, the winding exchange and 1 / Zc are unchanged; the sample box of item 5 is
 *      recomputed from the shifted coordinates; the top-left rule applies per sample; the weights p_k, q, Z and the colour are
 *      evaluated at that sample.  Consequently the centre plane is the single-sample render, bit for bit.  A triangle dropped at
 *      the near plane is counted ONCE in *near_count, not once per plane.
 *  M3. Colour.  Each covered sample's colour is that of the unlit (item 6), textured (T3-T5, the level per face as there) or lit
 *      (S2-S6) contract evaluated at that sample: 4x SUPERSAMPLING at the MSAA positions, interior pixels included.  Hardware
 *      MSAA shades once per pixel and triangle (at the centre or centroid) and only tests coverage and depth per sample; here
 *      every sample is shaded, so interior pixels are the mean of four shaded samples, not the centre's colour.
 *  M4. Resolve, in integer arithmetic: per channel out = (c_1 + c_2 + c_3 + c_4 + 2) >> 2 over the four sample planes.  An
 *      uncovered sample contributes (0, 0, 0, 0), a covered one has alpha 255: alpha is one of 0, 64, 128, 191, 255 and colour is
 *      blended towards black at silhouettes — what a multisample resolve over a (0, 0, 0, 0) clear gives and what the reference's
 *      PNGs hold (colour premultiplied by coverage).
 *  M5. Geometry outputs come from the centre plane alone: depth_mm, depth_m and face_id equal the samples = 1 render bit for bit;
 *      multisampling moves colour and alpha only (the analogue of S7).  Pixels with alpha > 0 and depth 0 (a sample is covered,
 *      the centre is not) and pixels with depth > 0 and alpha < 255 (the centre is covered, a sample is not) therefore exist.
 *  M6. OUT OF SCOPE: sample counts other than 1 and 4; centroid or per-pixel shading; alpha-to-coverage; multisampling of the
 *      windowed depth raster (VSD, verify, refine, scene ground truth: single-sampled by definition) and of
 *      synth_scenes.render_scenes, whose composite picks one layer per pixel.
 *
 * pp_render_ms_workspace_bytes: samples = 1 gives pp_render_workspace_bytes; samples = 4 gives 256 + chunk 5 (H W + Nf) 8 bytes:
 * per view (1 + S) planes of H W 64-bit words, and a queue slot per triangle and plane (a triangle's box is recomputed per plane,
 * so each plane queues its own large triangles).  PP_EINVAL: samples not 1 or 4, what pp_render_workspace_bytes rejects, and
 * with samples = 4 a chunk_views whose size does not fit a size_t.
 * pp_render_views_ms: the argument list of pp_render_views_lit with `int shaded` in front of the shading arguments and `int
 * samples` behind them.  shaded = 1: the colour source and shading of pp_render_views_lit, with all its checks.  shaded = 0, the
 * UNLIT render: the colour source is `colors` (pp_render_views) or face_uv + mips (+ Wt, Ht; pp_render_views_textured), exactly
 * one of the two; the shading arguments (lights_host ... tone_entries) are not read.  samples = 1 gives the bytes of those three
 * entries, through the same kernels and the same workspace.  samples = 4: the coverage launches run over the 5 planes of every
 * view of a chunk, the resolve pass shades the four samples of a pixel and applies M4 and M5; the views are rendered in chunks of
 * as many views as the workspace holds and any chunk size gives the same bytes; all work is enqueued on `stream`, nothing
 * synchronises.  PP_EINVAL, before any launch: samples not 1 or 4, shaded not 0 or 1, and everything the entry it stands for
 * rejects (unlit: no colour source, both, or a bad texture argument).  PP_EWORKSPACE: workspace misaligned (256 B) or smaller than
 * pp_render_ms_workspace_bytes(H, W, Nf, 1, samples).
 * ------------------------------------------------------------------------- */
int pp_render_ms_workspace_bytes(int H, int W, int n_faces, int chunk_views, int samples, size_t* bytes);
int pp_render_views_ms(const float* vertices, int n_vertices, const int* faces, const int* faces_host, int n_faces,
                       const unsigned char* colors, const float* face_uv, const void* mips, int Wt, int Ht, const float* poses,
                       int n_views, float fx, float fy, float cx, float cy, int H, int W, float near, void* workspace,
                       size_t workspace_bytes, unsigned char* rgba, unsigned short* depth_mm, float* depth_m, int* face_id,
                       unsigned int* near_count, int shaded, const float* lights_host, int n_lights, float ambient, int normal_mode,
                       const float* normals, const unsigned char* base_color_host, const unsigned char* tone_table, int tone_entries,
                       int samples, void* stream);
/* Per view the first / last row and column with alpha != 0 — the np.any / np.where of get_bbox (utils/data_utils.py:131-137) on
 * rgba[..., 3]: extents (V, 4) int32 = {rmin, rmax, cmin, cmax} (inclusive; -1 each for a view that covers nothing);
 * counts (V) int32 covered samples, may be NULL. */
int pp_template_extents(const unsigned char* rgba, int n_views, int H, int W, int* extents, int* counts, void* stream);
/* `_get_template` (provider/bop_test_dataset.py:222-240) for V frames in one launch.  boxes (V, 4) int32 {y1, y2, x1, x2} on the
 * device, boxes_host its HOST copy, validated here.  Per view: out_rgb (V, 3, S, S) = pp_crop_resize_normalize of the frame's
 * colours (masked by alpha > 0 when rgb_mask_flag), out_mask (V, S, S) = its nearest-resized mask of alpha == 255, out_pts
 * (V, P, P, 3) = pp_depth_points_nearest of the depth in metres — the same device functions, bit-equal to the per-view calls.
 * depth: (V, H, W) uint16 millimetres, converted as (float)((double) d / 1000.0) (:230), or fp32 metres when depth_is_f32.
 * PP_EINVAL: null pointer, V <= 0 or > 65535, S or P outside 1..4096, fx or fy = 0, a box that is empty or leaves the frame. */
int pp_templates_crop(const unsigned char* rgba, const void* depth, int depth_is_f32, int n_views, int H, int W, const int* boxes,
                      const int* boxes_host, float fx, float fy, float cx, float cy, int S, int P, int rgb_mask_flag,
                      const double* mean3, const double* std3, float* out_rgb, float* out_mask, float* out_pts, void* stream);

/* -------------------------------------------------------------------------
 * Pose errors against ground truth (picopose_amd/evaluation.py plans every call): MSSD, MSPD (Hodan et al., "BOP Challenge 2020
 * on 6D Object Localization", section 2.2), ADD and ADD-S (Hinterstoisser et al. 2012) of n_pairs (estimate, ground truth) pairs
 * that may mix objects, in one launch sequence: one compose launch (when MSSD or MSPD is asked for), one launch per kind, one
 * finalize launch (the minimum over symmetries of MSSD / MSPD and the tile sums of ADD-S).
 *
 * THE ARITHMETIC (tests/pose_error_oracle.py restates it in numpy; MSSD, MSPD and their indices equal it bit for bit).  float32,
 * one rounding per operation, never contracted, in the order written, unless float64 is named:
 *  1. compose, per (pair p, symmetry s of its object): G = f32(R_gt R_s), g = f32(R_gt t_s + t_gt), every entry evaluated in float64
 *     as ((a0 b0 + a1 b1) + a2 b2) [+ t] from the float32 inputs and rounded once.
 *  2. a point under a map (R, t): X = ((R00 x + R01 y) + R02 z) + t0, and Y, Z alike.
 *  3. MSSD_s = sqrt(max over the object's vertices of (dx dx + dy dy) + dz dz), d = est(x) - (G, g)(x).  A squared distance that is
 *     NaN (a pose that holds a NaN or an infinity) counts as +inf: such a pair has MSSD +inf, never a small value.
 *  4. MSPD_s = sqrt(max of du du + dv dv), u = (fx X) (1 / Z), v = (fy Y) (1 / Z), d = est - gt.  The principal point cancels in the
 *     difference and is not added.  A squared distance is +inf when a point of either side has Z <= 0 (or when it is NaN).
 *  5. mssd / mspd = the minimum over s, *_sym = its index within the object's symmetry list (the lowest on a tie; 0 when all are +inf).
 *     (ADD of a pair with a non-finite pose is NaN or +inf, ADD-S +inf or NaN: never a finite value.)
 *  6. ADD = f32(sum / Nv): the distances sqrt((dx dx + dy dy) + dz dz) against (R_gt, t_gt) itself, added in float64: lane l of 256
 *     adds vertices l, l + 256, ... in order, the 64 lanes of a wave combine by xor-shuffles 32, 16, ... 1, the 4 waves in order.
 *  7. ADD-S = f32(sum / Nv'): per estimate-side vertex the square root of the minimum over the ground-truth-side vertices of the
 *     squared distance in difference form, over the ADD-S vertex set; tiles of PP_EVAL_ADDS_TILE vertices (lane l holds vertices
 *     l, l + 256, l + 512, l + 768 of its tile) are summed as in 6 and the tiles added in order.
 * Every result is independent of launch order, stream, pair order and of how the caller splits the pairs over calls.  No atomics.
 *
 * vertices / adds_vertices: every object's (Nv, 3) fp32 vertices concatenated (millimetres), object o at rows
 * [vert_off[o], vert_off[o + 1]) / [adds_off[o], adds_off[o + 1]) (adds_vertices: the set ADD-S runs on, e.g. a subsample; it may be
 * the same buffer).  sym_R (S, 9) / sym_t (S, 3) fp32: every object's symmetry transforms concatenated, object o at
 * [sym_off[o], sym_off[o + 1]), at least one each.  The three *_off tables (n_objects + 1 ints) are device pointers, *_off_host
 * their HOST copies, validated here.  pair_obj (n_pairs) int32 object index per pair, device, pair_obj_host its HOST copy.
 * R_est, R_gt (n_pairs, 9), t_est, t_gt (n_pairs, 3) fp32, translations in millimetres; focal (n_pairs, 2) fp32 {fx, fy}, needed
 * for PP_EVAL_MSPD only.  kinds: an OR of PP_EVAL_*; outputs of kinds not asked for may be NULL.  mssd, mspd, add, adds (n_pairs)
 * fp32, mssd_sym, mspd_sym (n_pairs) int32.
 * Workspace (256-byte aligned): pp_pose_errors_workspace_bytes(n_pairs, max_syms, max_adds_vertices, kinds), where max_syms /
 * max_adds_vertices are the largest symmetry count / ADD-S vertex count among the objects of the call's pairs: 12 floats per
 * (pair, symmetry) for the composed maps, one per (pair, symmetry) and requested symmetric kind, one double per (pair, ADD-S tile).
 * PP_EINVAL (before any launch): a null pointer that is needed, n_pairs / n_objects <= 0, kinds 0 or with an unknown bit, an offset
 * table that does not start at 0 or has an empty object, a pair_obj_host entry outside [0, n_objects), n_pairs max_syms >= 2^31.
 * PP_EWORKSPACE: workspace misaligned or smaller than pp_pose_errors_workspace_bytes says.
 * ------------------------------------------------------------------------- */
#define PP_EVAL_MSSD 1
#define PP_EVAL_MSPD 2
#define PP_EVAL_ADD 4
#define PP_EVAL_ADDS 8
#define PP_EVAL_ADDS_TILE 1024
int pp_pose_errors_workspace_bytes(int n_pairs, int max_syms, int max_adds_vertices, int kinds, size_t* bytes);
int pp_pose_errors(const float* vertices, const int* vert_off, const float* adds_vertices, const int* adds_off, const float* sym_R,
                   const float* sym_t, const int* sym_off, const int* vert_off_host, const int* adds_off_host,
                   const int* sym_off_host, int n_objects, const int* pair_obj, const int* pair_obj_host, const float* R_est,
                   const float* t_est, const float* R_gt, const float* t_gt, const float* focal, int n_pairs, int kinds,
                   void* workspace, size_t workspace_bytes, float* mssd, int* mssd_sym, float* mspd, int* mspd_sym, float* add,
                   float* adds, void* stream);

/* -------------------------------------------------------------------------
 * VSD, the Visible Surface Discrepancy of BOP (picopose_amd/evaluation.py plans every call): per (estimate, ground truth) pair two
 * depth renders of the object's mesh and a three-image comparison with the test depth image.  This is the BOP toolkit's
 * pose_error.vsd with visib_mode = "bop19" and cost_type = "step", WRITTEN FROM MEMORY: the toolkit cannot be run next to this
 * library, so parity with its pixels is UNPINNED.  Known places where it can differ: its renderer's sampling convention (here pixel
 * centres at integer coordinates, raster contract item 2) and its geometric near-plane clipping (here a triangle with a vertex at
 * Zc <= near is dropped whole and counted).
 *
 * THE DEFINITION.  Z_est, Z_gt: camera-Z depth renders (mm, 0 = background) of the mesh under the two poses; Z_test: the test depth
 * in mm, "missing" where Z_test > 0 is false (zero, negative, NaN).  Per pixel (x, y) with the image's fx, fy, cx, cy:
 *   r = sqrt(((x - cx) / fx)^2 + ((y - cy) / fy)^2 + 1),  D_* = Z_* r                                   (distance along the ray)
 *   visib_gt  = D_gt  > 0 and (missing or D_gt  - D_test <= delta)
 *   visib_est = D_est > 0 and (missing or D_est - D_test <= delta or visib_gt)
 *   inter = visib_gt and visib_est, union = visib_gt or visib_est;  on inter: dd = |D_gt - D_est| / diameter, n_t = #{dd >= tau_t}
 *   e_t = (n_t + |union| - |inter|) / |union|, and e_t = 1 when |union| = 0.
 *
 * THE DEPTH RASTER.  Items 1-5 and 7 of THE RASTER CONTRACT above apply unchanged and item 6 for Z only (no colour), with the
 * vertices in millimetres, the camera of the view's image and sampling clipped to the view's WINDOW {x0, y0, x1, y1}
 * (x0 <= x < x1, y0 <= y < y1, inside the frame) instead of the frame.  A window that contains every sample the full-frame render
 * covers gives the full-frame render's bits (tests/vsd_oracle.py restates the windowed render; the kernels equal it bit for bit).
 * A view with an empty window renders nothing and counts nothing.  A triangle whose clipped box holds at most 64 samples is walked
 * by one lane, a larger one goes through a queue to 16 x 16 tiles, as in pp_render_views.
 *
 * THE PAIR REDUCTION, float32, one rounding per operation, never contracted, in this order:
 *   xr = ((float) x - cx) / fx, yr = ((float) y - cy) / fy;  r = sqrtf((xr xr + yr yr) + 1);  D = Z r for est, gt and test;
 *   the compares are D_model - D_test <= delta;  dd = fabsf(D_gt - D_est) / diameter, then dd >= tau_t.
 * One workgroup per pair walks the union box of the two windows (outside a view's window its Z is 0).  |union|, |inter| and n_t
 * are INTEGER counters per lane, reduced by xor-shuffles within a wave and through LDS across waves (no atomics), then
 *   e_t = f32((double)(n_t + union - inter) / (double) union), or 1 when union = 0.
 * Integers make the result independent of order, stream, pair order and of how the caller splits the pairs over calls.
 *
 * THE SCENE (PpScene, below) is what pp_vsd_errors, pp_depth_refine and pp_scene_gt share: the objects, cameras and views of a call.
 * Objects: vertices (millimetres) and faces (indices LOCAL to their object) of every object concatenated, object o at rows
 * [vert_off[o], vert_off[o + 1]) / [face_off[o], face_off[o + 1]); diameters (n_objects) fp32.  cams (n_images, 4) fp32 = fx, fy, cx, cy.
 * Views: view_obj, view_img (n_views) int32, poses (n_views, 4, 4) fp32 row-major object -> camera, windows (n_views, 4) int32,
 * view_zoff (n_views + 1) int64: the prefix sums of the windows' sample counts — view v owns z-buffer words
 * [view_zoff[v], view_zoff[v + 1]).  H, W: the frame the windows lie in; near: the near plane (mm).
 * Every table is a device pointer; the *_host members are HOST copies of the offset, window and index tables (and of faces,
 * diameters, cams), validated by every entry before any launch.  A device table an entry does not read may be NULL (pp_scene_gt:
 * diameters); every other member pointer is needed.  The struct is read during the call only: the caller may reuse or free it after.
 * THE SCENE CHECKS, PP_EINVAL (before any launch) from every entry: a NULL scene or a needed member pointer that is null; n_objects /
 * n_images / n_views / H / W <= 0, H W >= 2^31; near or a diameter not positive and finite; fx or fy = 0, a camera entry that is not
 * finite; an offset table that does not start at 0, an object without vertices, a view whose object has no faces; a face index
 * outside its object; a view's object or image index out of range; a window outside the frame or with x1 < x0 / y1 < y0; view_zoff
 * not the prefix sums of the windows; view_faces (the sum over the views of their object's face count) >= 2^32.
 *
 * pp_vsd_errors.  Pairs: pair_est, pair_gt (n_pairs) int32 view indices, device pointers with *_host copies validated here.
 * depth (n_images, H, W) fp32 millimetres.  taus_host: n_taus floats on the host (they travel as kernel arguments).
 * Outputs: vsd (n_pairs, n_taus) fp32, counts (n_pairs, 2 + n_taus) int32 = {union, inter, n_1 .. n_T}, near_count (n_views) uint32
 * (zeroed here): the triangles of each view dropped at the near plane; depth_out (n_views, H, W) fp32 (0 = background) or NULL.
 * n_pairs = 0 with depth_out renders only (the pair tables, depth, vsd and counts may then be NULL).
 * Workspace (256-byte aligned): pp_vsd_workspace_bytes(window_samples, view_faces) = 256 + roundup256(8 window_samples) + 8 view_faces
 * with window_samples = view_zoff[n_views] and view_faces = the sum over the views of their object's face count (one queue slot per
 * (view, triangle)).  One call is one launch sequence over all its views: the caller (evaluation.vsd_errors) splits the PAIRS into
 * groups whose views fit its workspace bound, one call per group, with identical results.  All work is enqueued on `stream`;
 * nothing synchronises.
 * PP_EINVAL (before any launch): THE SCENE CHECKS; a null pointer that is needed; n_pairs < 0, n_pairs = 0 without depth_out; n_taus
 * outside 1..PP_VSD_MAX_TAUS, a NaN tau; delta not positive and finite; a pair index out of range; a pair whose two views differ in
 * image or object.  PP_EWORKSPACE: workspace misaligned or smaller than pp_vsd_workspace_bytes says.
 * ------------------------------------------------------------------------- */
typedef struct PpScene {
    /* device tables */
    const float* vertices;
    const int* vert_off;
    const int* faces;
    const int* face_off;
    const float* diameters;
    const float* cams;
    const int* view_obj;
    const int* view_img;
    const float* poses;
    const int* windows;
    const long long* view_zoff;
    /* host copies, validated before any launch */
    const int* vert_off_host;
    const int* faces_host;
    const int* face_off_host;
    const float* diameters_host;
    const float* cams_host;
    const int* view_obj_host;
    const int* view_img_host;
    const int* windows_host;
    const long long* view_zoff_host;
    int n_objects, n_images, H, W, n_views;
    float near;
} PpScene;

#define PP_VSD_MAX_TAUS 16
int pp_vsd_workspace_bytes(long long window_samples, long long view_faces, size_t* bytes);
int pp_vsd_errors(const PpScene* scene, const int* pair_est, const int* pair_gt, const int* pair_est_host, const int* pair_gt_host,
                  int n_pairs, const float* depth, float delta, const float* taus_host, int n_taus, void* workspace,
                  size_t workspace_bytes, float* vsd, int* counts, unsigned int* near_count, float* depth_out, void* stream);

/* -------------------------------------------------------------------------
 * DEPTH REFINEMENT: projective point-to-plane ICP of n_views poses of mixed objects against the test depth images
 * (picopose_amd/depth_refine.py plans every call; tests/depth_refine_oracle.py restates this text in numpy float64).  This is THIS
 * library's own algorithm.  The project it was modelled on refines with OpenCV's ppf_match_3d ICP after a centroid shift; that code
 * cannot be run next to this library and sub-samples its points, so PARITY WITH IT IS UNPINNED AND NOT ATTEMPTED.
 * Millimetres throughout.
 *
 * THE ALGORITHM.  Per pose, at most `iterations` times:
 *  1. Render.  THE DEPTH RASTER of the VSD block, unchanged: the object under the CURRENT float32 pose into the view's window of the
 *     ragged z-buffer, word = (bits of Z) << 32 | face, 64-bit unsigned atomic minimum.  The window is fixed for the whole call (the
 *     caller plans it once from the input pose: scene.plan_window grown by a margin and clipped to the frame); a sample that
 *     leaves it is not rendered and therefore not associated.
 *  2. Associate and accumulate.  For every window sample (x, y) with a z-buffer hit (Z_r, face f):
 *       Z_t = the test depth at (x, y); the sample is skipped unless Z_t > 0 (zero, negative, NaN: missing);
 *       the gate, in float32, never contracted: fabsf(Z_t - Z_r) <= max_distance, otherwise skipped;
 *     from here float64, computed from the float32 inputs (fx, fy, cx, cy, the pose, the vertices, Z_r, Z_t):
 *       xr = (x - cx) / fx, yr = (y - cy) / fy;  p_m = Z_r (xr, yr, 1), p_t = Z_t (xr, yr, 1);
 *       m = R ((v1 - v0) x (v2 - v0)) with v0, v1, v2 the face's vertices in the order of the faces table; a face whose cross product
 *       is the zero vector (or whose |m| is not > 0) is skipped;  n = m / |m|, negated when n . p_m > 0 (so that n . p_m <= 0);
 *       skipped when -(n . p_m) / |p_m| < min_cos (grazing);
 *       residual r = n . (p_t - p_m);  row J = [ ((p_m - c) x n) / rho , n ] with c = R (centre of the object's vertex box) + t,
 *       the centre = ((double) lo + (double) hi) / 2 of `boxes`, and rho = (double) diameter / 2: the unknowns (rho theta, v) are mm.
 *     Sums (PP_DEPTH_REFINE_SUMS = 29 doubles): the 21 upper entries of J^T J row by row ((0,0), (0,1) .. (0,5), (1,1) ..), the 6 of
 *     J^T r, sum r^2, and the count N (an integer held in a double).  A workgroup of 256 lanes owns one STRIP of
 *     PP_DEPTH_REFINE_STRIP_ROWS window rows: lane l adds samples l, l + 256, .. of the strip (row-major) in order, the 64 lanes of a
 *     wave combine by xor-shuffles 32, 16 .. 1, the 4 waves are added in wave order, and the strips of a view in index order.  No
 *     floating-point atomics: the sums are the same bits for any stream, pose order, batch composition and grouping.
 *  3. Solve and update.  The symmetric 6 x 6 matrix is decomposed by cyclic Jacobi rotations (12 sweeps, float64).  With lambda_max
 *     the largest eigenvalue, a direction is KEPT when lambda > 0 and lambda >= rcond lambda_max; rank = the directions kept;
 *     x = sum over the kept directions of e (e . J^T r) / lambda: the pseudo-inverse step.  Directions the depth does not constrain
 *     (a plate's in-plane motion, a sphere's rotation) are left where the input pose put them.  theta = x[0..3] / rho, v = x[3..6];
 *     Exp(theta) = I + A K + B K K (K the cross-product matrix of theta, a = |theta|, A = sin a / a, B = (1 - cos a) / a^2; for
 *     a^2 < 1e-12: A = 1 - a^2 / 6, B = 1/2 - a^2 / 24);  R <- Exp(theta) R,  t <- c + Exp(theta) (t - c) + v, each entry rounded once
 *     to float32: the rasteriser's input format.
 *  4. Stop.  status per pose, decided after every linearisation in this order:
 *       2  N < min_points in this linearisation                                              -> the INPUT pose is returned
 *       3  |t - t_in| > max_translation or angle(R R_in^T) > max_rotation for the updated float32 pose (the angle is
 *          acos(clamp((trace - 1) / 2, -1, 1)); a non-finite value counts as exceeding)       -> the INPUT pose is returned
 *       0  max(|rho theta|, |v|) < eps: converged                                             -> the updated pose
 *       1  none of these after `iterations` linearisations                                   -> the updated pose
 *       4  (before the first) an input pose whose first three rows hold a NaN or an infinity, or an empty window -> the input pose
 *     A stopped pose is frozen: later launches neither render it nor move it, and nothing of another pose depends on it.
 *
 * Objects, cams, views, windows and view_zoff are THE SCENE (PpScene, the VSD block); scene->poses are the INPUT poses ("poses_in"
 * below), (n_views, 4, 4) fp32 row-major object -> camera.  boxes (n_objects, 6) fp32 = the lower and the upper corner of each
 * object's vertex box, view_soff (n_views + 1) int32: the prefix sums of the views' strip counts, ceil(window height /
 * PP_DEPTH_REFINE_STRIP_ROWS), 0 for an empty window; both are device pointers with *_host copies validated here.
 * depth (n_images, H, W) fp32 millimetres.  max_distance, min_cos, rcond, eps, max_translation
 * (mm), max_rotation (rad) are float32 arguments, converted to float64 where they are compared with float64.
 * Outputs (device): poses_out (n_views, 4, 4) fp32 (also the working poses; it must not be poses_in); active (n_views) int32 work
 * table; status, n_iterations (linearisations performed), rank and n_points (of the last linearisation; rank 0 when it stopped with
 * status 2) (n_views) int32; rms_before, rms_after (n_views) fp32 = sqrt(sum r^2 / N) of the first and the last linearisation (NaN
 * without one, or when N = 0); near_count (n_views) uint32: the triangles dropped at the near plane, over all iterations.
 * Optional (NULL: off): trajectory (n_views, iterations + 1, 4, 4) fp32, entry 0 the input pose and entry k + 1 the pose after
 * round k (a stopped pose repeats its result); sums (n_views, iterations, 29) fp64, the sums of each linearisation (0 where none).
 * Workspace (256-byte aligned): pp_depth_refine_workspace_bytes(window_samples, view_faces, strips) = 256 + roundup256(8
 * window_samples) + roundup256(8 view_faces) + 232 strips.  All `iterations` rounds (clear, two raster launches, accumulate, solve)
 * are enqueued on `stream`; nothing synchronises with the host.
 * PP_EINVAL (before any launch): THE SCENE CHECKS; a null pointer that is needed; poses_out = scene->poses; a box that is not finite
 * or has hi < lo; view_soff not the prefix sums of the strip counts; iterations outside 1..PP_DEPTH_REFINE_MAX_ITERATIONS;
 * min_points < 1; max_distance, max_translation or max_rotation not positive and finite; min_cos or rcond outside [0, 1); eps
 * negative or not finite.  PP_EWORKSPACE: workspace misaligned or smaller than pp_depth_refine_workspace_bytes says.
 * ------------------------------------------------------------------------- */
#define PP_DEPTH_REFINE_STRIP_ROWS 8
#define PP_DEPTH_REFINE_SUMS 29
#define PP_DEPTH_REFINE_MAX_ITERATIONS 1000
int pp_depth_refine_workspace_bytes(long long window_samples, long long view_faces, long long strips, size_t* bytes);
int pp_depth_refine(const PpScene* scene, const float* boxes, const float* boxes_host, const int* view_soff, const int* view_soff_host,
                    const float* depth, int iterations, float max_distance, int min_points, float min_cos, float rcond, float eps,
                    float max_translation, float max_rotation, void* workspace, size_t workspace_bytes, float* poses_out,
                    int* active, int* status, int* n_iterations, int* rank, int* n_points, float* rms_before, float* rms_after,
                    unsigned int* near_count, float* trajectory, double* sums, void* stream);

/* -------------------------------------------------------------------------
 * SCENE GROUND TRUTH: per ground-truth view the pixel counts, boxes and masks of BOP's scene_gt_info.json, mask and mask_visib, and per
 * image the composite of its views (picopose_amd/scene_gt.py plans every call; tests/scene_gt_oracle.py restates this text in numpy).
 * This is the BOP toolkit's calc_gt_info / calc_gt_masks WRITTEN FROM MEMORY: the toolkit cannot be run next to this library, so
 * parity with its pixels is UNPINNED.  Known places where it can differ: its renderer's sampling convention (here pixel centres at
 * integer coordinates, raster contract item 2), its geometric near-plane clipping (here a triangle with a vertex at Zc <= near is
 * dropped whole and counted), and its box convention (here boxes are INCLUSIVE corners; scene_gt.format_gt_info turns them into
 * the file's [x, y, w, h]).  Millimetres throughout.
 *
 * THE CANVAS.  A frame is H x W with camera (fx, fy, cx, cy).  Views are rasterised on a canvas of (H + 2 pad_y) x (W + 2 pad_x)
 * samples whose camera is (fx, fy, f32(cx + pad_x), f32(cy + pad_y)): the sums are taken in float32 and rounded once.  Items 1-5 and 7
 * of THE RASTER CONTRACT and the Z of item 6 apply with the canvas as the frame (THE DEPTH RASTER of the VSD block); windows are
 * planned on, and clipped to, the canvas.  Canvas sample (xc, yc) is frame pixel (x, y) = (xc - pad_x, yc - pad_y), IN-FRAME iff
 * 0 <= x < W and 0 <= y < H.  pad = (0, 0) gives the bits of a pp_vsd_errors depth render.  A padded render does NOT in general:
 * the principal point changes the float32 projection (shifting cx by W changes one of the twelve ground-truth views of
 * tests/vsd_oracle.py's mixed scene).  The toolkit's own canvas, from memory, is pad = (W, H).
 *
 * PER VIEW, with Z the view's render and Z_test the test depth of its image, "missing" where Z_test > 0 is false:
 *   px_count_all   = #{canvas samples with Z > 0}
 *   px_count_valid = #{in-frame samples with Z > 0 and Z_test > 0}
 *   visible        = in-frame and Z > 0 and (missing or D - D_test <= delta), with D = Z r, D_test = Z_test r,
 *                    xr = ((float) x - cx) / fx, yr = ((float) y - cy) / fy, r = sqrtf((xr xr + yr yr) + 1) from the FRAME pixel and
 *                    the FRAME camera; float32, one rounding per operation, never contracted: visib_gt of the VSD block, operation
 *                    for operation
 *   px_count_visib = #{visible samples}
 *   bbox_obj       = inclusive corners {x_min, y_min, x_max, y_max} of the samples with Z > 0, in FRAME coordinates (they may be negative
 *                    or reach past the frame);  bbox_visib = the same of the visible samples;  an empty set gives {0, 0, -1, -1}.
 *
 * THE COMPOSITE.  Per frame pixel the minimum of (bits of Z_v) << 32 | v over the views v of that image that cover it, v the view's
 * index in the call: scene_depth = that Z (background 0), instance_map = view_label[v] (v itself without the table; background -1);
 * on equal depth the lower v wins.  Without a test depth (depth = NULL) Z_test := scene_depth: nothing is missing where a model
 * covers, and an instance is hidden exactly by the other instances of its image; delta = 0 is then exact mutual occlusion.
 * The composite runs when scene_depth or instance_map is asked for or depth is NULL.
 *
 * DETERMINISM.  Counts are integer sums (three counters and eight extrema per lane, xor-shuffles within a wave, LDS across the four
 * waves, then integer atomicAdd / atomicMin / atomicMax per workgroup of a view), the composite is a 64-bit integer atomic minimum;
 * there is no floating-point atomic.  Every output is the same bits for any stream, view order, window, and grouping of the views
 * over calls (the map: up to the tie rule, which is stated on the call's view order).
 *
 * Objects, views, windows (on the canvas) and view_zoff are THE SCENE (PpScene, the VSD block); the device table `diameters` is not
 * read and may be NULL.  scene->cams, H and W are the FRAME cameras and the frame size; the canvas is derived here, and THE SCENE
 * CHECKS run on a copy of the scene with the canvas cameras and the canvas size in their place.  canvas_cams (n_images, 4), device
 * pointer with a host copy: the canvas cameras, which must be the float32 sums above.  depth (n_images, H, W) fp32 mm or NULL.
 * view_label (n_views) int32, used when use_view_label != 0.  Outputs (device): counts (n_views, 3) int32 = {all, valid, visib};
 * boxes (n_views, 8) int32 = bbox_obj, bbox_visib; near_count (n_views) uint32 (zeroed here).  Optional (NULL: off): mask_all,
 * mask_visib (n_views, H, W) uint8, 0 / 255, in-frame only, mask_all = Z > 0 (zeroed here); scene_depth (n_images, H, W) fp32;
 * instance_map (n_images, H, W) int32.
 * Workspace (256-byte aligned): pp_scene_gt_workspace_bytes(window_samples, view_faces, composite_pixels) = the header, z-buffer and
 * queue of pp_vsd_workspace_bytes, and when composite_pixels = n_images H W > 0 (the composite runs) that rounded up to 256 plus
 * 8 composite_pixels.  All work is enqueued on `stream`; nothing synchronises.
 * PP_EINVAL (before any device call): THE SCENE CHECKS, with the canvas as the frame (so a canvas of 2^31 samples or more); a needed
 * pointer that is null; pad_x or pad_y < 0; delta negative or not finite; a canvas camera that is not the stated sum;
 * use_view_label with view_label NULL.  PP_EWORKSPACE: as pp_vsd_errors.
 * ------------------------------------------------------------------------- */
int pp_scene_gt_workspace_bytes(long long window_samples, long long view_faces, long long composite_pixels, size_t* bytes);
int pp_scene_gt(const PpScene* scene, const float* canvas_cams, const float* canvas_cams_host, int pad_x, int pad_y, const float* depth,
                float delta, const int* view_label, int use_view_label, void* workspace, size_t workspace_bytes, int* counts, int* boxes,
                unsigned int* near_count, unsigned char* mask_all, unsigned char* mask_visib, float* scene_depth, int* instance_map,
                void* stream);

/* -------------------------------------------------------------------------
 * MODEL INFO: what a models_info.json entry needs from the vertices alone (picopose_amd/model_info.py plans every call;
 * tests/model_info_oracle.py restates this text in numpy; every output equals it bit for bit).  Two all-pairs measurements:
 * the BOP diameter — the largest distance between two vertices, with the pair that attains it — and the directed Hausdorff distance
 * of a vertex set under candidate rigid transforms, which is what a symmetry search measures.  The search itself (which
 * transforms to try, what passes) is the host's; these entries only measure.  Millimetres throughout.
 *
 * THE ARITHMETIC.  float32, one rounding per operation, never contracted, in the order written:
 *  1. the squared distance of two points p, q, in difference form: dx = p.x - q.x, dy = p.y - q.y, dz = p.z - q.z,
 *     d2 = (dx dx + dy dy) + dz dz.
 *  2. pp_model_diameter, per object with vertices v_0 .. v_(n-1): d2max = the maximum over the pairs i < j of d2(v_i, v_j); pair =
 *     the lexicographically lowest (i, j), indices LOCAL to the object, among the pairs that attain it.  One vertex: d2max = 0,
 *     pair = (0, 0).  The square root is the caller's (model_info.py takes it in float64 from the two vertices of the pair).
 *  3. a point under a candidate T (12 floats: R row-major, then t — the layout of the composed maps of pp_pose_errors):
 *     X = ((T0 x + T1 y) + T2 z) + T9, Y = ((T3 x + T4 y) + T5 z) + T10, Z = ((T6 x + T7 y) + T8 z) + T11 (item 2 of that block).
 *  4. pp_transform_hausdorff, per candidate c of object o: h[c] = sqrtf(max over x in query(o) of min over y in full(o) of
 *     d2(T_c(x), y)), the minimum by fminf from +inf, the maximum by fmaxf from 0; y is NOT transformed.  The distance is DIRECTED
 *     (query under T towards the full set): the caller asks for T and for its inverse when it wants the symmetric one.
 * A maximum, a minimum and an index tie rule do not depend on the order of evaluation: every output is the same bits for any stream,
 * object order, candidate order and any split of the candidates over calls.  No atomics.
 *
 * THE WORK.  Tiles of PP_MODEL_INFO_TILE = 1024 points, 4 per lane of a 256-lane workgroup held in registers (lane l holds points
 * l, l + 256, l + 512, l + 768 of its tile); the other side goes through LDS 256 points at a time.  Diameter: one workgroup per
 * (object, i-tile, range of 2 j-tiles at or beyond the i-tile), so only the upper triangle is visited; every lane keeps its best
 * (d2, i, j), the lanes combine by xor-shuffles 32 .. 1, the waves through LDS, the workgroups of an object in a finalize launch, all
 * with the tie rule of item 2.  Hausdorff: one workgroup per (candidate, query tile), then one finalize lane per candidate.
 *
 * vertices: every object's (Nv, 3) fp32 vertices concatenated, object o at rows [vert_off[o], vert_off[o + 1]), as
 * evaluation.ObjectModels lays them out; q_vertices / q_off: the query sets alike (e.g. a sub-sample; it may be the same buffers).
 * The *_off tables (n_objects + 1 ints) are device pointers, *_off_host their HOST copies, validated here.
 * pp_model_diameter: d2max (n_objects) fp32, pair (n_objects, 2) int32, device.  Workspace (256-byte aligned):
 * pp_model_diameter_workspace_bytes(vert_off_host, n_objects) = roundup256(4 (n_objects + 1)) + roundup256(16 work items), an object
 * of T tiles having T ceil(T / 2) work items.
 * pp_transform_hausdorff: cand_obj (n_candidates) int32 object index per candidate, device, cand_obj_host its HOST copy; cand_T
 * (n_candidates, 12) fp32, device; h (n_candidates) fp32, device.  Workspace (256-byte aligned):
 * pp_transform_hausdorff_workspace_bytes(n_candidates, max_query_vertices) = roundup256(4 n_candidates ceil(max_query_vertices /
 * 1024)), max_query_vertices the largest query set among the objects of the call's candidates; a caller with a bound on its workspace
 * splits the candidates into consecutive groups, one call each, with identical results.
 * All work is enqueued on `stream`; nothing synchronises.
 * PP_EINVAL (before any device call): a null pointer; n_objects <= 0 (pp_model_diameter: or > 65535); n_candidates <= 0; an offset table that does not
 * start at 0 or does not increase (an object without vertices); a cand_obj_host entry outside [0, n_objects); more than 2^31 - 1
 * diameter work items; a query set of more than 65535 tiles.  PP_EWORKSPACE: workspace misaligned or smaller than stated.
 * ------------------------------------------------------------------------- */
#define PP_MODEL_INFO_TILE 1024
int pp_model_diameter_workspace_bytes(const int* vert_off_host, int n_objects, size_t* bytes);
int pp_model_diameter(const float* vertices, const int* vert_off, const int* vert_off_host, int n_objects, void* workspace,
                      size_t workspace_bytes, float* d2max, int* pair, void* stream);
int pp_transform_hausdorff_workspace_bytes(int n_candidates, int max_query_vertices, size_t* bytes);
int pp_transform_hausdorff(const float* vertices, const int* vert_off, const float* q_vertices, const int* q_off,
                           const int* vert_off_host, const int* q_off_host, int n_objects, const int* cand_obj,
                           const int* cand_obj_host, const float* cand_T, int n_candidates, void* workspace, size_t workspace_bytes,
                           float* h, void* stream);

/* -------------------------------------------------------------------------
 * THE SCENE COMPOSITE: rendered object layers over a background -> the colour frame, 16-bit depth, instance map and per-instance
 * visibility of a synthetic training scene (csrc/pp_synth.hip; picopose_amd/provider/synth_scenes.py plans every call;
 * tests/synth_oracle.py restates this text in numpy; every output equals it bit for bit).  A LAYER is one object instance rendered
 * into a full frame by pp_render_views*: layers_rgba (L, H, W, 4) uint8 and layers_depth (L, H, W) fp32 metres (that entry's
 * depth_m: 0 on its background).  layer_off (n_images + 1 int32, non-decreasing, device; layer_off_host its HOST copy): the layers of
 * image i are [layer_off[i], layer_off[i + 1]); an image may have none.
 *
 * PER FRAME PIXEL of image i.  Layer l COVERS the pixel when its depth Z_l > 0 is true (a NaN, a negative value and +-0 do not
 * cover; +inf does).  The coverage test is on depth alone: alpha is never read.  The WINNER is the l of the minimum of
 * (bits of Z_l) << 32 | l over the covering layers of the image, l the layer's index in the call: the nearest layer, on equal depth
 * the lower l.  Then
 *   rgb      (n_images, H, W, 3) uint8  = bytes 0..2 of the winner's layers_rgba pixel, or the background pixel (below);
 *   depth    (n_images, H, W) uint16    = min(65535, rintf((1000.0f * Z) / depth_scale[i])) of the winner's Z — float32, one rounding
 *                                         per operation in the order written, never contracted, rintf = round half to even (the
 *                                         value a depth PNG with the camera's depth_scale would hold) — or 0 on background;
 *   instance (n_images, H, W) int32     = the winner l, or -1.
 * PER LAYER l:
 *   counts (L, 2) int32 = {px_all, px_visib}: the pixels l covers, and the pixels l wins;
 *   boxes  (L, 4) int32 = inclusive {x_min, y_min, x_max, y_max} of the pixels l wins; none: {0, 0, -1, -1} (as pp_scene_gt);
 *   mask_visib (L, H, W) uint8 (optional, NULL: off) = 255 where l wins, else 0 (every byte is written).
 *
 * THE BACKGROUND.  background (n_images, PP_SYNTH_BG_WORDS) int32 descriptors {mode, a, b, 0} (device; background_host the HOST copy):
 *   mode 0  a constant: R = a & 255, G = (a >> 8) & 255, B = (a >> 16) & 255;
 *   mode 1  the pixel of bg_images (n_images, H, W, 3) uint8, image i of the CALL;
 *   mode 2  a lattice in integer arithmetic: seed = a (its uint32 bits), s = b in 2..7, S = 2^s the cell.  Pixel (x, y):
 *           gx = x >> s, fx = x & (S - 1), gy = y >> s, fy = y & (S - 1); node (u, v) has the colour bytes 0..2 (channel c = byte c,
 *           (h >> 8 c) & 255) of h(seed, u, v), h the counter hash of the training-pair assembly block above (one device function,
 *           csrc/pp_hash_dev.h); channel c of the pixel =
 *           (n00 (S - fx)(S - fy) + n10 fx (S - fy) + n01 (S - fx) fy + n11 fx fy + 2^(2s-1)) >> 2s, n_uv the byte of node
 *           (gx + u, gy + v).  At a node (fx = fy = 0) it is the node's colour; elsewhere it lies within the four.
 * depth_scale (n_images) fp32 (device; depth_scale_host the HOST copy): the camera's depth_scale, millimetres per depth unit.
 *
 * DETERMINISM.  The composite is a loop over the image's layers per pixel: no atomics.  counts and boxes are integer sums and integer
 * extrema: per workgroup (PP_SYNTH_TILE consecutive pixels of one image) ballots and xor-shuffles within a wave and LDS across the four
 * waves give one record of six integers per layer of the image, written to the workspace; a second launch reduces the records of a
 * layer in a fixed order.  There is no atomic and no floating-point reduction anywhere.  Every output is the same bits for any
 * stream, any split of the images over calls and any order of the images (instance and the layer order of the per-layer outputs:
 * up to the call's layer indices, which the tie rule is stated on).
 *
 * Workspace (256-byte aligned; may be NULL when 0 bytes are needed): pp_scene_composite_workspace_bytes(n_layers, H, W) =
 * roundup256(24 n_layers ceil(H W / PP_SYNTH_TILE)).  All work is enqueued on `stream`; nothing synchronises.
 * The layers are read with 16-byte loads and the outputs written four pixels per lane when W % 4 == 0 and every buffer is 16-byte
 * aligned, one pixel per access otherwise; the results do not depend on which.
 * PP_EINVAL (before any device call): a needed pointer that is null (layers_* with n_layers > 0, layer_off*, background*,
 * depth_scale*, rgb, depth, instance; counts and boxes with n_layers > 0); n_images, H or W <= 0; n_layers < 0; n_layers H W or
 * n_images H W >= 2^31; layer_off_host decreasing, not starting at 0 or not ending at n_layers; a depth_scale_host entry that is not
 * positive and finite; a mode outside 0..2; mode 2 with s outside 2..7; mode 1 with bg_images NULL.  PP_EWORKSPACE: workspace
 * misaligned or smaller than stated.  n_layers = 0 is legal: every image is its background.
 *
 * pp_depth_quantize_u16: out[k] = Z > 0 ? min(65535, rintf(units_per_metre * Z)) : 0 for k < n, Z = depth_m[k] (float32, rintf = round
 * half to even; not (Z > 0) — background, NaN, negative — gives 0).  The template frames use it with 10000: the 0.1 mm unit of the
 * template depth files that pp_depth_u16_template reads back.  PP_EINVAL: a null pointer, n < 0, units_per_metre not positive and
 * finite.  n = 0 launches nothing.
 * ------------------------------------------------------------------------- */
#define PP_SYNTH_BG_WORDS 4
#define PP_SYNTH_TILE 1024
int pp_scene_composite_workspace_bytes(int n_layers, int H, int W, size_t* bytes);
int pp_scene_composite(const unsigned char* layers_rgba, const float* layers_depth, const int* layer_off, const int* layer_off_host,
                       int n_layers, int n_images, int H, int W, const int* background, const int* background_host,
                       const unsigned char* bg_images, const float* depth_scale, const float* depth_scale_host, void* workspace,
                       size_t workspace_bytes, unsigned char* rgb, unsigned short* depth, int* instance, int* counts, int* boxes,
                       unsigned char* mask_visib, void* stream);
int pp_depth_quantize_u16(const float* depth_m, long long n, float units_per_metre, unsigned short* out, void* stream);

/* -------------------------------------------------------------------------
 * PROPOSAL LABELLING: which onboarded object a class-agnostic mask proposal is, and how sure (csrc/pp_proposals.hip;
 * picopose_amd/proposals.py plans every call; tests/proposal_oracle.py restates this text in numpy float64).  CNOS's matching stage,
 * written from its published description: cls-token descriptors, cosine similarity to every template of every object, the mean of
 * the top-k templates per object, arg-max over objects, then mask NMS on the host from the intersection table below.  Parity with
 * CNOS's own code is unpinned.  All pointers are device pointers unless named *_host; all work is enqueued on `stream`, nothing
 * synchronises; no entry uses atomics.  Finite inputs are the caller's contract everywhere: a NaN or an infinity in a descriptor
 * gives unspecified scores, labels and views (never an access outside the buffers).
 *
 * pp_descriptor_normalize: y[r] = x[r] / max(||x[r]||_2, eps) for the n rows of x (n, C) fp32 (y is another buffer).  The sum of squares of a
 * row is accumulated in THE ROW ORDER: lane l of the row's wave adds the elements l, l + 64, ... in ascending order with one fma
 * each, and the 64 lane sums are folded by a butterfly over the lane masks 32, 16, 8, 4, 2, 1; then one sqrtf, one maximum and one
 * division per element.  A zero row gives a zero row.  PP_EINVAL: a null pointer, n or C <= 0, eps not positive.
 *
 * pp_proposal_match: query (P, C) and bank (sum T, C) hold unit rows (pp_descriptor_normalize's); offsets (O + 1 int32): the
 * templates of object o are the bank rows [offsets[o], offsets[o + 1]), T_o >= 1 of them; offsets_host is the HOST copy, validated
 * before the launch.  cos(p, t) = the dot product of query row p and a template row in THE DOT ORDER: lane l adds the products of
 * the elements 4 c .. 4 c + 3 of its 16-byte chunks c = l, l + 64, ... in ascending element order, one fma each, starting from 0;
 * the 64 lane sums are folded by the butterfly above.  The order depends on C alone — not on P, O, T, the proposal's place in its
 * tile or the wave that computes it — so bit-equal rows give bit-equal cosines.  With k = min(topk, T_o):
 *   score (P, O) fp32  = (the k largest cos(p, t) of object o, added largest first) / k   (one division);
 *   view  (P, O) int32 = the t - offsets[o] of the largest cos(p, t); among equal ones the lowest;
 *   label (P) int32    = the o of the largest score[p][o]; among equal ones the lowest;
 *   best  (P) fp32     = score[p][label[p]].
 * One workgroup of four waves per (tile of PP_MATCH_TILE proposals, object) stages the tile's rows in LDS (PP_MATCH_TILE * C * 4
 * bytes: 64 KB at PP_MATCH_MAX_C, the largest C the staging holds); a second small launch takes the arg-max over objects.
 * PP_EINVAL (before any launch): a null pointer; P, O or C <= 0; O > 65535; C not a multiple of 4 or above PP_MATCH_MAX_C; topk < 1
 * or > PP_MATCH_MAX_TOPK; query or bank not 16-byte aligned; offsets_host not starting at 0, decreasing or leaving an object empty.
 *
 * pp_rle_pack_bits: the run-end tables of pp_detections_crop (run_ends, run_offset, run_offset_host: cumulative COCO run ends over
 * the column-major mask of hw = H * W pixels) -> bits (n, words) uint32, words = ceil(hw / 32): bit i of word w of mask d is pixel
 * 32 w + i in column-major order (x * H + y), the bits past hw in the last word are 0; area (n) int32 = the mask's pixel count.
 * PP_EINVAL: a null pointer, n <= 0 or > PP_MASK_MAX_N, n_runs <= 0, hw <= 0, words != ceil(hw / 32), run_offset_host decreasing,
 * negative or past n_runs.
 *
 * pp_mask_intersections: bits (n, words) -> inter (n, n) int32, inter[i][j] = the sum over the words of popcount(bits[i][w] &
 * bits[j][w]): symmetric, its diagonal is the area.  A workgroup owns 8 x 8 pairs, four threads per pair, and stages 64 words of its 16 rows
 * per step in LDS, the rows 68 words apart (conflict-free 4-byte reads).  PP_EINVAL: a null pointer, n <= 0 or > PP_MASK_MAX_N, words <= 0.
 *
 * THE APPEARANCE SCORE (csrc/pp_appearance.hip; tests/appearance_oracle.py restates it): the appearance term of SAM-6D's
 * instance-segmentation stage (Lin et al., "SAM-6D: Segment Anything Model Meets Zero-Shot 6D Object Pose Estimation", 2024), WRITTEN
 * FROM ITS PUBLISHED DESCRIPTION, NOT FROM ITS CODE: for every foreground patch of a proposal's crop the best cosine to any
 * foreground patch of the best-matching template, averaged over the crop's foreground patches.  Parity with SAM-6D's code is
 * unpinned.  Its geometric score and box NMS are not here.
 *
 * pp_patch_valid: mask (n, S, S) fp32 (out_mask of pp_detections_crop, or a tem_mask) and the ViT's patch size p, S % p == 0,
 * w0 = S / p, N = w0 w0 -> valid (n, N) uint8, n_valid (n) int32.  Patch i = py w0 + px (the ViT's token order: row-major over
 * the patch grid, cls token excluded) covers the pixels [py p, py p + p) x [px p, px p + p); count = its pixels with
 * mask > 0.5f (a NaN is not counted); valid[i] = 1 iff 2 count >= p p, else 0; n_valid = the number of valid patches.  Integers
 * only.  One workgroup per mask.  PP_EINVAL: a null pointer; n, S or p <= 0; S > PP_APP_MAX_S; S % p != 0.
 *
 * pp_appearance_match: query (P, N, C) and bank (R, N, C) hold unit rows (pp_descriptor_normalize's), q_valid (P, N) and t_valid
 * (R, N) uint8 (non-zero: valid; pp_patch_valid's), pair_row (P) int32 with its HOST copy pair_row_host, validated before the
 * launch: proposal p is compared with bank view pair_row[p] (a device entry outside [0, R) that the host copy does not show is
 * answered like a view without a valid patch: 0 and -1, nothing is read).  cos(i, j) of query patch i and template patch j is computed in THE
 * CHAIN ORDER: acc = 0, then acc = fmaf(q[i][k], t[j][k], acc) for k = 0 .. C - 1 ascending (v_mfma_f32_32x32x2_f32 is bit for bit
 * that chain; the K tail is padded with zeros, fma(0, 0, acc) = acc).  The order depends on C alone - not on P, N, R, the
 * proposal's place in the batch or the wave that computes it - so bit-equal rows give bit-equal cosines.
 *   patch_sim (P, N) fp32 = for EVERY query patch i, valid or not, the largest cos(i, j) over the valid template patches j of view
 *                           pair_row[p]; 0 when that view has no valid patch;
 *   patch_arg (P, N) int32 = the j of that maximum, among equal maxima the lowest; -1 when the view has no valid patch;
 *   n_valid (P) int32     = the number of valid query patches;
 *   app (P) fp32          = (the sum of patch_sim[p][i] over the valid i in THE ROW ORDER above: lane l adds i = l, l + 64, ...
 *                           ascending starting from 0, then the butterfly) / n_valid[p], one division; 0 when n_valid[p] == 0 or
 *                           the view has no valid patch.
 * One workgroup of four waves per (proposal, PP_APP_TILE query patches): the template's patches go over the waves in chunks of 256
 * (2 x 2 tiles of 32 x 32 per wave, the template the A operand: a lane's column is one query patch), K is staged through LDS 16
 * channels at a time; the masked (value, index) maximum is taken in the lane, across the lane halves and across the waves
 * through LDS.  A second launch, one wave per proposal, takes the masked sum and the division.  No atomics, no scratch.
 * PP_EINVAL (before any launch): a null pointer; P, R, N or C <= 0; N > PP_APP_MAX_N; C not a multiple of 4 or above
 * PP_MATCH_MAX_C; query or bank not 16-byte aligned; a pair_row_host entry outside [0, R).
 * ------------------------------------------------------------------------- */
#define PP_MATCH_TILE 16
#define PP_MATCH_MAX_C 1024
#define PP_MATCH_MAX_TOPK 8
#define PP_APP_TILE 64
#define PP_APP_MAX_N 1024 /* patches of a crop: a 448 crop at patch 14 */
#define PP_APP_MAX_S 16384
#define PP_MASK_MAX_N 4096
int pp_descriptor_normalize(const float* x, int n, int C, float eps, float* y, void* stream);
int pp_proposal_match(const float* query, int P, const float* bank, const int* offsets, const int* offsets_host, int O, int C,
                      int topk, float* score, int* view, int* label, float* best, void* stream);
int pp_rle_pack_bits(const int* run_ends, int n_runs, const int* run_offset, const int* run_offset_host, int n, int hw, int words,
                     unsigned* bits, int* area, void* stream);
int pp_mask_intersections(const unsigned* bits, int n, int words, int* inter, void* stream);
int pp_patch_valid(const float* mask, int n, int S, int p, unsigned char* valid, int* n_valid, void* stream);
int pp_appearance_match(const float* query, const unsigned char* q_valid, int P, const float* bank, const unsigned char* t_valid, int R,
                        const int* pair_row, const int* pair_row_host, int N, int C, float* patch_sim, int* patch_arg, int* n_valid,
                        float* app, void* stream);

/* -------------------------------------------------------------------------
 * POSE VERIFICATION: per pose hypothesis, how well its depth render explains the image: eight integer counts of the render held
 * against the detection's mask and, when there is one, the test depth image (csrc/pp_verify.hip; picopose_amd/verify.py plans every
 * call and turns the counts into scores; tests/verify_oracle.py restates this text in numpy; counts equal it bit for bit).  This is
 * the project's own rule, not a published protocol's.  Millimetres throughout.
 *
 * Objects, views, windows and view_zoff are THE SCENE (PpScene, the VSD block): one view per hypothesis, rendered by THE DEPTH RASTER
 * inside its window; the device table `diameters` is not read and may be NULL.  mask_bits (n_masks, words) uint32 is what
 * pp_rle_pack_bits writes for the frame: words = ceil(H W / 32), bit x * H + y (word (x H + y) / 32, bit (x H + y) % 32) is pixel
 * (x, y).  view_mask (n_views) int32, device pointer with a host copy: the mask of each view, so that the hypotheses of one detection
 * share one mask.  depth (n_images, H, W) fp32 or NULL (RGB only).
 *
 * PER VIEW, over the window samples (x, y) with a rendered depth (z-buffer word != all ones, Z > 0), with in_mask the sample's mask
 * bit and Z_test = depth[view_img][y][x]:
 *   counts[0] render     every such sample
 *   counts[1] inter      in_mask
 *   counts[2] valid      depth given and Z_test > 0 (a NaN or a non-positive Z_test is missing)
 *   counts[3] agree      valid, not front, not behind
 *   counts[4] front      valid and e > delta    (the scene is closer: the model is occluded here)
 *   counts[5] behind     valid and -e > delta   (the sensor sees through the model)
 *   counts[6] vis        not front              (a missing depth counts as visible: the rule of SCENE GROUND TRUTH)
 *   counts[7] vis_inter  not front and in_mask
 * e = D - D_test with xr = ((float) x - cx) / fx, yr = ((float) y - cy) / fy, r = sqrtf((xr xr + yr yr) + 1), D = Z r,
 * D_test = Z_test r: float32, one rounding per operation, never contracted — the operations of SCENE GROUND TRUTH's `visible`.
 * With depth = NULL the counts are {render, inter, 0, 0, 0, 0, render, inter}.  A view with an empty window has all-zero counts.
 *
 * DETERMINISM.  Only integers are summed (eight counters per lane, xor-shuffles within a wave, LDS across the four waves, one integer
 * atomicAdd per counter and workgroup into the cleared counts); there is no floating-point atomic.  Every output is the same bits
 * for any stream, view order, window and grouping of the views over calls.
 *
 * Outputs (device): counts (n_views, PP_VERIFY_COUNTS) int32 and near_count (n_views) uint32, both zeroed here.  Workspace (256-byte
 * aligned): pp_vsd_workspace_bytes(window_samples, view_faces), nothing added.  All work is enqueued on `stream` (two clears, the
 * raster, one reduction launch); nothing synchronises.
 * PP_EINVAL (before any launch): THE SCENE CHECKS; a null mask_bits, view_mask, view_mask_host, workspace, counts or near_count;
 * n_masks <= 0; words != ceil(H W / 32); a view_mask_host entry outside [0, n_masks); delta negative, NaN or infinite.
 * PP_EWORKSPACE: a workspace that is misaligned or short.
 * ------------------------------------------------------------------------- */
#define PP_VERIFY_COUNTS 8
int pp_pose_verify(const PpScene* scene, const unsigned* mask_bits, int n_masks, int words, const int* view_mask,
                   const int* view_mask_host, const float* depth, float delta, void* workspace, size_t workspace_bytes, int* counts,
                   unsigned int* near_count, void* stream);

/* -------------------------------------------------------------------------
 * DEPTH PROPOSALS: class-agnostic mask proposals from the depth image alone: the dominant plane of each image by consensus, the pixels
 * that stand off it labelled into 4-connected components, per-component records, and the COCO run lengths of the kept components
 * (csrc/pp_depth_proposals.hip; picopose_amd/depth_proposals.py plans every call; tests/depth_proposals_oracle.py restates this text in
 * numpy).  THIS IS THE PROJECT'S OWN ALGORITHM, as POSE VERIFICATION, RGB-D POSE RECOVERY and the depth refinement are; it claims parity
 * with no published segmenter, and its accuracy on real depth images is unmeasured.  What is exact: given a depth image, every
 * integer output (scores, winner, labels, records, run ends) equals the restatement bit for bit; the refit plane is a float64 fit.
 * All pointers are device pointers unless named *_host; all work is enqueued on `stream`, nothing synchronises; only integers meet
 * in atomics, so every output is the same bits for any stream and launch order.  Millimetres throughout.
 *
 * depth (B, H, W) fp32; cams (B, 4) fp32 {fx, fy, cx, cy}, fx and fy non-zero.  A pixel is VALID when 0 < z < infinity (a NaN is
 * not).  THE POINT of pixel (u, v), float32, one rounding per operation, never contracted:
 *   X = ((float(u) - cx) * z) / fx,  Y = ((float(v) - cy) * z) / fy,  Z = z.
 * THE HEIGHT of a point over the plane (nx, ny, nz, d):  s = ((nx * X + ny * Y) + nz * Z) + d, float32 in exactly this order.
 *
 * pp_depth_plane.  Hypothesis h < n_hyp (<= PP_PLANE_MAX_HYP) of image b samples the pixels i_k = (aug_hash(seed, b, 3 h + k) * H W)
 * >> 32 (64-bit product; aug_hash as in "Training-pair assembly"), k = 0, 1, 2, row-major (v = i / W, u = i % W), with points p_k.
 * With a = p_1 - p_0, e = p_2 - p_0 (componentwise float32), c = (ay ez - az ey, az ex - ax ez, ax ey - ay ex) (each product rounded,
 * then the difference), len2 = (cx cx + cy cy) + cz cz: the hypothesis is DEAD — it scores 0 and cannot win over a live one —
 * if any i_k is invalid, or len2 <= PP_PLANE_MIN_CROSS2 (mm^4) or is not finite.  Otherwise inv = 1 / sqrtf(len2) (both correctly
 * rounded), n = c * inv, d = -((nx p0x + ny p0y) + nz p0z).  Its score is the INTEGER count of valid pixels with |s| <= tau.  The
 * winner is the highest score, the lowest h among equals.  An image whose best score is below min_inliers has NO PLANE.
 * Refit: over the winner's consensus set (the same pixels), with q = p - p_0 in float64, the sums of q and of q q^T and the count are
 * accumulated per strip of PP_PLANE_STRIP pixels (per lane in pixel order, a butterfly over the lane masks 32 .. 1, the four waves in
 * order) and the strips added in a fixed order (lane l of one wave takes strips l, l + 64, ... ascending, then the same butterfly).
 * The normal is the eigenvector of the smallest eigenvalue of sum(q q^T) / N - m m^T, m = sum(q) / N, by the cyclic Jacobi of the pose
 * solvers, normalised; d = -n . (p_0 + m); the sign is chosen so that d >= 0 (the camera is on the positive side).
 * Outputs: plane64 (B, 4) float64, plane (B, 4) fp32 = its cast, info (B, 4) int32 = {has_plane, winner, its score, the refit's
 * consensus count}; an image with no plane has a zero plane row and refit count 0 (winner and score are still reported).
 * Workspace (256-byte aligned): pp_depth_plane_workspace_bytes = roundup256(4 B n_hyp) + roundup256(80 B ceil(H W / PP_PLANE_STRIP)).
 * PP_EINVAL (before any launch): a null pointer; B, H or W <= 0; B > 65535; H W >= 2^31; n_hyp outside [1, PP_PLANE_MAX_HYP]; tau
 * negative, NaN or infinite; min_inliers < 3.  PP_EWORKSPACE: a workspace that is misaligned or short.
 *
 * pp_depth_components.  plane (B, 4) fp32 and has_plane (B) int32 as above (any plane may be given).  A valid pixel is FOREGROUND when
 * Z <= max_range and, where has_plane[b] != 0, min_height < s < max_height (both strict).  Two 4-neighbours that are both foreground
 * are CONNECTED when |z_p - z_q| <= max_step: one float32 subtraction, equality connects.  labels (B, H, W) int32: -1 for background,
 * otherwise the smallest row-major pixel index (y W + x, within the image) of the pixel's component.  Union by smaller index: the
 * result does not depend on the order of the unions.  One workgroup per 32 x 128 tile (labels and depth in LDS), then the pairs
 * across tile edges in global memory, then a pass that replaces every label by its root.  pp_depth_components_workspace_bytes is 0
 * today (the labels are the parent array); workspace may be NULL.
 * PP_EINVAL: a null depth, cams, plane, has_plane or labels; the frame limits above; H > 32 * 65535; a NaN height bound; max_range not
 * positive; max_step negative, NaN or infinite.
 *
 * pp_component_stats.  Per root (a pixel whose label is its own index): area, the inclusive box xmin, ymin, xmax, ymax, and border = 1
 * when a pixel of the component lies in the first or last row or column.  The roots with min_area <= area <= max_area (and border = 0
 * when drop_border) QUALIFY: n_qualified (B) int32 counts them all; the first min(n_qualified[b], cap) rows of comps (B, cap,
 * PP_COMPONENT_FIELDS) int32 = {root, area, xmin, ymin, xmax, ymax, border} hold qualifiers in an UNSPECIFIED order (which ones when
 * n_qualified > cap is unspecified too); the other rows are not written.  Lanes of a wave that share a root are reduced by ballots
 * and shuffles before one integer atomic per value (at most four roots per wave this way, the rest lane by lane).
 * Workspace (256-byte aligned): pp_component_stats_workspace_bytes = roundup256(24 B H W); it is not cleared.
 * PP_EINVAL: a null pointer; the frame limits; min_area < 1; max_area < min_area; cap < 1.  PP_EWORKSPACE as above.
 *
 * pp_components_rle.  sel (n, PP_RLE_SEL_FIELDS) int32 with a host copy = {image, root, xmin, ymin, xmax, ymax}: the mask of entry k
 * is labels[image] == root inside the box (a box that holds the whole component gives the component).  With run_ends NULL (the COUNT
 * pass): n_runs[k] = the number of cumulative run ends of the mask in COCO's column-major order (position x H + y): a leading 0 when
 * pixel 0 is set, every position f >= 1 whose pixel differs from pixel f - 1, and H W.  With run_ends (the EMIT pass): those ends,
 * ascending, at run_ends[run_offset[k] ..]; run_offset (n + 1) with its host copy is the exclusive sum of the counts, ending in
 * n_runs_total — the tables pp_rle_pack_bits and pp_detections_crop read.  Nothing is written at or past run_offset[k + 1].
 * One workgroup per entry walks the columns of the box; no dense mask is built.
 * PP_EINVAL: a null labels, sel or sel_host; the frame limits; n <= 0 or > PP_MASK_MAX_N; a sel_host row with an image outside [0, B), a
 * root outside [0, H W) or a box that is empty or leaves the frame; count pass: n_runs NULL; emit pass: a null run_offset or
 * run_offset_host, n_runs_total <= 0, run_offset_host not starting at 0, decreasing or not ending in n_runs_total.
 * ------------------------------------------------------------------------- */
#define PP_PLANE_MAX_HYP 1024
#define PP_PLANE_STRIP 1024
#define PP_PLANE_MIN_CROSS2 1.0f
#define PP_COMPONENT_FIELDS 7
#define PP_RLE_SEL_FIELDS 6
int pp_depth_plane_workspace_bytes(int B, int H, int W, int n_hyp, size_t* bytes);
int pp_depth_plane(const float* depth, const float* cams, int B, int H, int W, int n_hyp, unsigned seed, float tau, int min_inliers,
                   void* workspace, size_t workspace_bytes, float* plane, double* plane64, int* info, void* stream);
int pp_depth_components_workspace_bytes(int B, int H, int W, size_t* bytes);
int pp_depth_components(const float* depth, const float* cams, const float* plane, const int* has_plane, int B, int H, int W,
                        float min_height, float max_height, float max_range, float max_step, void* workspace, size_t workspace_bytes,
                        int* labels, void* stream);
int pp_component_stats_workspace_bytes(int B, int H, int W, size_t* bytes);
int pp_component_stats(const int* labels, int B, int H, int W, int min_area, int max_area, int drop_border, int cap, void* workspace,
                       size_t workspace_bytes, int* n_qualified, int* comps, void* stream);
int pp_components_rle(const int* labels, int B, int H, int W, const int* sel, const int* sel_host, int n, const int* run_offset,
                      const int* run_offset_host, int n_runs_total, int* n_runs, int* run_ends, void* stream);

/* -------------------------------------------------------------------------
 * DETECTION SCORING: COCO-style average precision and recall of 2D detections and masks — what BOP's detection and segmentation
 * tasks are scored by (csrc/pp_det_eval.hip; picopose_amd/detection_eval.py plans every call and accumulates on the host;
 * tests/detection_eval_oracle.py restates this text in numpy loops; every device output equals it bit for bit).  The protocol is
 * COCOeval AS REMEMBERED: neither pycocotools nor the BOP toolkit's eval_bop22_coco.py can be run next to this library, so parity
 * with both is UNPINNED.  All pointers are device pointers unless named *_host; all work is enqueued on `stream`, nothing
 * synchronises; no entry uses atomics or accumulates in floating point.
 *
 * RECORDS.  A detection is a CNOS record: scene_id, image_id, category_id, bbox [x, y, w, h], score, segmentation (COCO RLE).  A
 * ground-truth annotation is the same record without a score, plus ignore (bool) and iscrowd (bool, default false); its area is the
 * pixel count of its mask.  A crowd annotation is ignored as well (COCOeval's _prepare as remembered; the Python layer sets the flag,
 * the kernels take the two flags as given).  iou_type is "segm" or "bbox".  An image is one (scene_id, image_id); a GROUP is one
 * (image, category).
 *
 * ORDER WITHIN A GROUP.  Detections are sorted by descending score, stably (the lower input index first among equal scores), and cut
 * to the largest max_dets (default (1, 10, 100)).  For each area range [lo, hi] a ground truth is IGNORED if its ignore flag is set
 * or its area is < lo or > hi; the ground truths are ordered with the non-ignored ones first, stably.
 *
 * OVERLAP.  segm, from pixel counts: iou = inter / (area_d + area_g - inter); for a crowd ground truth inter / area_d.  bbox, in
 * float64, one rounding per operation, never contracted: iw = max(0, min(xd + wd, xg + wg) - max(xd, xg)), ih likewise,
 * iou = (iw ih) / ((wd hd + wg hg) - iw ih); for a crowd ground truth the denominator is wd hd.  Every IoU is ONE IEEE float64
 * division; a denominator that is not positive gives 0.
 *
 * MATCHING, per group, area range and threshold t of iou_thrs (default np.linspace(.5, .95, 10)), the detections visited in order:
 * best = min(t, 1 - 1e-10), m = -1; the ground truths are scanned in group order: one that is already matched at this t is skipped
 * unless it is a crowd; the scan stops if m >= 0, m is not ignored and this ground truth is ignored; one with iou < best is skipped;
 * otherwise best = iou, m = this.  If m >= 0 the detection is matched, takes m's ignore flag, and m is marked matched.  An unmatched
 * detection whose own area (the mask area for segm, w h for bbox) lies outside [lo, hi] is ignored.
 * THE CLOSED FORM (what pp_det_match computes): the winner is the largest IoU >= min(t, 1 - 1e-10) among the eligible (unmatched, or
 * crowd) NON-IGNORED ground truths, on equal IoU the LAST one in group order; only if no non-ignored one qualifies does the same
 * rule apply among the ignored ones.  Inside each class the group order is the input order, so "last" is the highest input index:
 * the group order is computed in the wave, implicitly — it is never materialised and the host hands none in.
 *
 * ACCUMULATION is the host's, numpy float64 (detection_eval.accumulate states it): per category, area range and max_dets value the
 * first max_det detections of every image are concatenated and sorted by descending score (mergesort); tp / fp are cumulative sums
 * of (matched / unmatched) and not ignored; rc = tp / npig, pr = tp / (tp + fp + spacing(1)); recall = rc[-1]; pr is made
 * non-increasing from the right and sampled at the 101 recalls np.linspace(0, 1, 101) by searchsorted(rc, r, "left").  A cell
 * without a non-ignored ground truth stays -1; a summary is the mean of the cells > -1.
 *
 * THE TABLES OF A CALL.  n_det detections and n_gt ground truths, each side with its groups contiguous: the detections in group-sorted
 * order (sorted and cut by the host), the ground truths in the order the annotations were given.  groups (n_groups,
 * PP_DET_GROUP_FIELDS) int32 with a host copy = {first detection, D_g, first ground truth, G_g, offset of the group's block}: the
 * block is D_g x G_g row-major (detection-major) inside the ragged arrays of n_pairs entries.  An empty side (D_g = 0 or G_g = 0) is
 * legal.  gt_flags (n_gt) uint8: PP_DET_GT_IGNORE | PP_DET_GT_CROWD.
 *
 * pp_det_overlaps.  segm: bits (n_det + n_gt, words) uint32 and area (n_det + n_gt) int32 as pp_rle_pack_bits writes them for the
 * chunk's frame, the detections' rows first; boxes NULL.  bbox: boxes (n_det + n_gt, 4) float64 {x, y, w, h}, the detections' rows
 * first, finite with w, h >= 0 (the caller's contract); bits, area and inter NULL.  tiles (n_tiles, 3) int32 with a host copy =
 * {group, first detection of the tile within the group, first ground truth within the group}, both multiples of PP_DET_TILE and
 * inside the group: the host lists the tiles that hold a pair, one workgroup each.  Outputs: inter (n_pairs) int32 (segm) and iou
 * (n_pairs) float64.  segm stages 64 words of the tile's 8 + 8 rows per step in LDS, the rows 68 words apart, four threads per pair
 * (pp_mask_intersections' staging).  No pair outside a group is computed, and there is no cap on the pairs or the masks: only the
 * pp_rle_pack_bits call that produced `bits` is capped, and the Python layer chunks for it.  n_tiles = 0: no launch.
 * PP_EINVAL (before any launch, no GPU needed): a null groups, groups_host, gt_flags or iou; both or neither of bits and boxes;
 * segm with a null area or inter or words <= 0; n_det, n_gt, n_tiles or n_pairs negative; n_groups <= 0; tiles without both copies;
 * a groups_host row with a negative field, a range past n_det / n_gt or a block past n_pairs; a tiles_host row with a group outside
 * [0, n_groups), a start that is negative, no multiple of PP_DET_TILE or outside the group.
 *
 * pp_det_match.  iou as above; det_area (n_det) and gt_area (n_gt) float64; area_ranges (A, 2) and iou_thrs (T) float64, each
 * with a host copy.  One wave per (group, area range, threshold): the detections are walked in order, the group's ground truths are
 * spread over the lanes (j = lane + 64 k), the matched, ignore and crowd flags of a lane's ground truths are bits of three 64-bit
 * registers (hence G_g <= PP_DET_MAX_GT), and the winner under THE CLOSED FORM is found by two wave reductions (the largest IoU bit
 * pattern, then the highest index that holds it), the non-ignored class first.  Outputs, the detection axis in the call's (group-
 * sorted) order and the ground-truth axis in the call's (input) order:
 *   dt_match  (A, T, n_det) int32  the call-wide index of the matched ground truth, or -1;
 *   dt_ignore (A, T, n_det) uint8  the matched ground truth's ignore flag; unmatched: area outside [lo, hi];
 *   gt_match  (A, T, n_gt)  int32  the call-wide index of the detection matched to it (the last one, for a crowd), or -1;
 *   gt_ignore (A, n_gt)     uint8.
 * Every element of a group of the table is written; detections and ground truths outside every group are not.
 * PP_EINVAL (before the launch, no GPU needed): a null pointer; n_pairs, n_det or n_gt negative; n_groups, A or T <= 0; a
 * threshold outside (0, 1] or NaN; an area range with lo > hi or a NaN; the groups_host checks above; G_g > PP_DET_MAX_GT.
 * ------------------------------------------------------------------------- */
#define PP_DET_GROUP_FIELDS 5
#define PP_DET_TILE 8
#define PP_DET_MAX_GT 4096
#define PP_DET_GT_IGNORE 1
#define PP_DET_GT_CROWD 2
int pp_det_overlaps(const unsigned* bits, const int* area, int words, const double* boxes, int n_det, int n_gt, const int* groups,
                    const int* groups_host, int n_groups, const int* tiles, const int* tiles_host, int n_tiles,
                    const unsigned char* gt_flags, int n_pairs, int* inter, double* iou, void* stream);
int pp_det_match(const double* iou, int n_pairs, const int* groups, const int* groups_host, int n_groups, int n_det, int n_gt,
                 const double* det_area, const double* gt_area, const unsigned char* gt_flags, const double* area_ranges,
                 const double* area_ranges_host, int A, const double* iou_thrs, const double* iou_thrs_host, int T, int* dt_match,
                 unsigned char* dt_ignore, int* gt_match, unsigned char* gt_ignore, void* stream);

/* -------------------------------------------------------------------------
 * 6D DETECTION SCORING: average precision of pose estimates against ground truth under MSSD and MSPD, where every estimate counts
 * and a false positive is punished — the task the chain depth_proposals -> label_proposals -> infer_proposals -> verify / refine
 * solves (an unknown number of instances per image) — and the suppression of duplicate poses of one instance
 * (csrc/pp_pose_det.hip; picopose_amd/pose_detection_eval.py plans every call and accumulates on the host;
 * tests/pose_detection_oracle.py restates this text in numpy loops; every device output equals it bit for bit).  This is the BOP
 * 2024 6D-detection protocol AS REMEMBERED: the BOP toolkit cannot be run next to this library, so parity with it is UNPINNED.
 * The suppression rule is the project's own.  All pointers are device pointers unless named *_host; all work is enqueued on
 * `stream`, nothing synchronises; no entry uses atomics, accumulates in floating point or needs scratch or LDS.
 *
 * RECORDS.  An estimate is a row of a BOP results file (evaluation.read_bop_results): scene_id, im_id, obj_id, score, R, t.  A
 * ground truth is an instance of scene_gt.json (evaluation.read_scene_gt) with an IGNORE flag: set when its visib_fract (of
 * scene_gt_info.json) is below min_visib_fract (default 0.1, as remembered): it is neither required nor does a match to it count.
 * An image is one (scene_id, im_id); a GROUP is one (image, obj_id) that holds at least one record of either side.
 *
 * ORDER.  Within an image only the max_per_image best-scored estimates are kept (default 100, as remembered; none dropped when
 * the caller asks for all): by descending score, the lower row first among equal scores, across all objects of the image.  Within
 * a group the kept estimates go by descending score, the lower row first among equal scores; the ground truths stay in scene_gt
 * order.
 *
 * THE TABLES OF A CALL.  n_est estimates and n_gt ground truths, each side with its groups contiguous and in the order above.
 * groups (n_groups, PP_DET_GROUP_FIELDS) int32 with a host copy = {first estimate, E_g, first ground truth, G_g, offset of the
 * group's block}: DETECTION SCORING's row.  err (M, n_pairs) float32, one row of n_pairs entries per metric: a group's block is
 * E_g x G_g row-major (estimate-major), so an estimate's errors to the group's ground truths are contiguous.  An empty side
 * (E_g = 0 or G_g = 0) is legal.  gt_ignore (n_gt) uint8, non-zero = ignored.  limits (n_groups, M, T) float64 with a host copy:
 * what an error must stay BELOW at threshold t of metric m in that group (the Python layer: MSSD threshold x the object's
 * diameter, MSPD threshold x image_width / 640).  A pair QUALIFIES when (double)err < limit, strictly, as evaluation.score_pairs
 * has it; a NaN and +inf never qualify, and neither does an entry whose sign bit is set: an error is a distance.
 *
 * MATCHING, per group, metric m and threshold t, the group's estimates visited in order: among the group's ground truths that are
 * not yet matched at this (m, t) and qualify, the winner is the lowest error among the NON-IGNORED ones, the lowest index among
 * equal errors; only if no non-ignored one qualifies does the same rule apply among the ignored ones.  A matched estimate takes
 * the winner's ignore flag and the winner is marked matched; an estimate without a winner is unmatched — a false positive, never
 * ignored.
 *
 * ACCUMULATION is the host's, numpy float64, with the formulae of DETECTION SCORING's ACCUMULATION paragraph: per object, metric
 * and threshold the estimates of all images are concatenated (groups in sorted (image, object) order) and sorted by descending score
 * (mergesort); tp / fp are cumulative sums of (matched / unmatched) and not ignored; npig = the object's non-ignored ground truths;
 * rc = tp / npig, pr = tp / (tp + fp + spacing(1)); pr is made non-increasing from the right and sampled at the 101 recalls
 * np.linspace(0, 1, 101) by searchsorted(rc, r, "left"); the recall reported is rc[-1] (0 without estimates).  An object without a
 * non-ignored ground truth stays -1.  SUMMARY: AP_MSSD = the mean over the objects (those > -1) of the mean over thresholds and
 * recall samples, AP_MSPD likewise, AP = (AP_MSSD + AP_MSPD) / 2; -1 when no object counts.
 *
 * pp_pose_match.  One wave per (group, m, t): the group's ground truths are spread over the lanes (j = lane + 64 k), the matched and
 * ignore flags of a lane's ground truths are bits of two 64-bit registers (hence G_g <= PP_POSE_MAX_GROUP), the estimates are
 * walked in order, each reading its contiguous row of G_g errors, and the winner is found by two wave reductions (the smallest
 * error bit pattern — non-negative floats order as unsigned integers — then the lowest index that holds it), the non-ignored
 * class first.  Outputs:
 *   est_match  (M, T, n_est) int32  the call-wide index of the matched ground truth, or -1;
 *   est_ignore (M, T, n_est) uint8  the matched ground truth's ignore flag; unmatched: 0;
 *   gt_match   (M, T, n_gt)  int32  the call-wide index of the estimate matched to it, or -1.
 * Every element of a group of the table is written; records outside every group are not.  1 <= M <= PP_POSE_MAX_METRICS (MSSD and
 * MSPD today; the cap leaves room for VSD).
 * PP_EINVAL (before the launch, no GPU needed): a null pointer; n_pairs, n_est or n_gt negative; n_groups, M or T <= 0; M >
 * PP_POSE_MAX_METRICS; a groups_host row with a negative field, a range past n_est / n_gt or a block past n_pairs; G_g >
 * PP_POSE_MAX_GROUP; a NaN in limits_host.
 *
 * DUPLICATE POSES (the project's own rule; nms_dist is untuned and its effect on real data unmeasured).  Groups and the order
 * within a group as above, without the per-image cut.  For the group's estimates in order, DIST(i, j), i < j, is the MSSD with
 * the earlier estimate i as the ground truth and the later j as the estimate (the object's symmetries included; the roles are
 * fixed because the value is slightly asymmetric).  Visiting j = 0 .. E_g - 1: j is DROPPED when a KEPT earlier i has
 * (double)DIST(i, j) < limit (strict: a distance exactly at the limit keeps j); otherwise j is kept.  A dropped estimate
 * suppresses nothing.  The Python layer's limit is nms_dist x the object's diameter (default 0.1).
 *
 * pp_pose_nms.  groups (n_groups, PP_POSE_NMS_FIELDS) int32 with a host copy = {first estimate, E_g, offset of the group's
 * triangle}; dist (n_tri) float32: DIST(i, j) is at offset + j (j - 1) / 2 + i, so a candidate's earlier partners are contiguous;
 * limit (n_groups) float64 with a host copy.  One wave per group holds the kept bits of the positions lane + 64 k in a 64-bit
 * register (hence E_g <= PP_POSE_MAX_GROUP) and finds a near kept partner by ballot, 64 partners at a time.  Output: keep (n_est)
 * uint8, every element of a group written.
 * PP_EINVAL (before the launch, no GPU needed): a null pointer; n_tri or n_est negative; n_groups <= 0; a groups_host row with a
 * negative field, a range past n_est, E_g > PP_POSE_MAX_GROUP or a triangle past n_tri; a limit_host that is NaN or negative.
 * ------------------------------------------------------------------------- */
#define PP_POSE_MAX_GROUP 4096
#define PP_POSE_MAX_METRICS 4
#define PP_POSE_NMS_FIELDS 3
int pp_pose_match(const float* err, int M, int n_pairs, const int* groups, const int* groups_host, int n_groups, int n_est, int n_gt,
                  const unsigned char* gt_ignore, const double* limits, const double* limits_host, int T, int* est_match,
                  unsigned char* est_ignore, int* gt_match, void* stream);
int pp_pose_nms(const float* dist, int n_tri, const int* groups, const int* groups_host, int n_groups, int n_est, const double* limit,
                const double* limit_host, unsigned char* keep, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PICOPOSE_HIP_H */
