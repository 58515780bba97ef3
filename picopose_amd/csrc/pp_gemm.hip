// fp32 MFMA GEMM / implicit-GEMM convolution engine for the network parts of the path
// (DINOv2 ViT linears and attention products, AffineRegressor, DPT head, flow decoder).
//
//   C[m, n] = epilogue( alpha * sum_k A(m, k) * B(n, k) )
//
// Everything is token-major / NHWC on the device: a "row" m is a token or an output pixel, k
// runs over input channels (times filter taps for a convolution), n over output channels.
// A is either a dense row-major matrix or an implicit im2col view of an NHWC image
// (zero padding, stride), so 1x1 / 3x3 / 7x7 / 14x14 convolutions, nn.Linear and the attention
// products all run on this one kernel; ConvTranspose2d with kernel == stride is the same GEMM
// with a pixel-shuffle store.  Arithmetic: v_mfma_f32_32x32x2_f32 (exact fp32 products and
// accumulation) — the reference computes in fp32 and parity comes first; the fp16/bf16 MFMA
// variants are a later round's lever.
//
// Tiling: 256 threads = 4 waves (2x2), block tile 128x128, K step 32, each wave a 64x64 tile
// (2x2 MFMA tiles, 64 accumulator registers).  LDS tiles are [128][36] floats (row stride 36
// keeps ds_read_b128 fragment reads conflict-free); each lane reads 16 consecutive k per row
// (4 x ds_read_b128), lanes 0-31 the first half of the K step and lanes 32-63 the second, which
// is the k-pair v_mfma_f32_32x32x2 consumes per issue.  Next tile is prefetched into registers
// while the MFMAs of the current one run.

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <atomic>
#include <mutex>
#include <string>
#include <unordered_map>
#include "../../include/picopose_hip.h"
#include "pp_common.h"
#include "pp_reduce_dev.h"
#include "pp_gemm_dev.h"
#include "pp_gemm_u.h"

// The autotuner's table (problem shape -> fastest tile configuration), process-wide.  pp_gemm_tune_save / pp_gemm_tune_load (and
// PP_GEMM_TUNE_FILE at first use) make a run reproducible: every profiling pass of one measurement set loads the SAME table, so the
// kernel trace, the MFMA-busy pass and the two traffic passes see identical launches.
static std::mutex g_tune_mu;
static std::unordered_map<std::string, int> g_tune_best;
static int g_tune_loaded = 0;

static int tune_load_locked(const char* path) {
    FILE* f = fopen(path, "r");
    if (!f) return -1;
    char key[192];
    int cfg, n = 0;
    while (fscanf(f, "%191s %d", key, &cfg) == 2) {
        g_tune_best[key] = cfg;
        ++n;
    }
    fclose(f);
    g_tune_loaded += n;
    return n;
}

namespace {

// One f16x3 term of the kernels that split fp32 operands on the fly: D = A(32 x 16) * B(16 x 32) + C on the matrix cores.
__device__ __forceinline__ f32x16 pp_mfma(const h8 a, const h8 b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0); }

constexpr int BM = 128, BK = 32, LDT = 36;  // BN = 64 * NJ (template): 128x128 or 128x64 block tiles

// one A element group: 4 consecutive k of row m (zero outside the matrix / image)
template <bool VEC4>
__device__ __forceinline__ f4 load_a(const PpGemmDesc& d, const float* __restrict__ A, int m, int k,
                                     int b_img, int oy, int ox) {
    f4 v = {0.f, 0.f, 0.f, 0.f};
    if (m >= d.M) return v;
    if (d.conv_kh == 0) {  // dense rows
        const float* p = A + (size_t)m * d.lda + k;
        if (VEC4) {
            if (k + 3 < d.K) v = *(const f4*)p;
            else {
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (k + i < d.K) v[i] = p[i];
            }
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (k + i < d.K) v[i] = p[i];
        }
    } else {  // implicit im2col of an NHWC image: k = (ky*KW + kx)*Cin + ci
        if (VEC4) {  // Cin % 4 == 0: the 4 elements share a tap
            if (k < d.K) {
                const int tap = k / d.conv_cin, ci = k - tap * d.conv_cin;
                const int ky = tap / d.conv_kw, kx = tap - ky * d.conv_kw;
                const int iy = oy + ky, ix = ox + kx;  // (oy, ox): top-left input pixel of the window
                if (iy >= 0 && iy < d.conv_h && ix >= 0 && ix < d.conv_w)
                    v = *(const f4*)(A + (size_t)b_img * d.conv_bstride + ((size_t)iy * d.conv_w + ix) * d.lda + ci);
            }
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int kk = k + i;
                if (kk < d.K) {
                    const int tap = kk / d.conv_cin, ci = kk - tap * d.conv_cin;
                    const int ky = tap / d.conv_kw, kx = tap - ky * d.conv_kw;
                    const int iy = oy + ky, ix = ox + kx;
                    if (iy >= 0 && iy < d.conv_h && ix >= 0 && ix < d.conv_w)
                        v[i] = A[(size_t)b_img * d.conv_bstride + ((size_t)iy * d.conv_w + ix) * d.lda + ci];
                }
            }
        }
    }
    if (d.relu_in) {
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = v[i] > 0.f ? v[i] : 0.f;
    }
    return v;
}

// OCC = workgroups per CU the register allocation is held to: the 128x128 tile runs ~10 % faster per tile at 2
// (no spills, 200 VGPRs) than at 3 (168 VGPRs); which one wins depends on how the tile count fills the slots.
// Store one output element: out = residual + residual2 + v at (m, n) of C (row-major, or the pixel-shuffled layout
// of a ConvTranspose2d(kernel = stride = r)), and/or as the f16x3 "hl" operand C_hl ([M][ldc_h], with the
// consumer's input ReLU folded in) so the next GEMM needs no separate split pass.
__device__ __forceinline__ void epilogue_store(const PpGemmDesc& d, float* C, const float* R, const float* R2, int m, int n,
                                               float v) {
    size_t off, orow = (size_t)m;
    int ocol = n;
    if (d.shuffle_r == 0) {
        off = (size_t)m * d.ldc + n;
    } else {
        // row m = input pixel (b, y, x) of an (shuffle_h x shuffle_w) image, column n = (dy*r + dx)*Cout + co
        const int r = d.shuffle_r, cout = d.N / (r * r);
        const int sub = n / cout, co = n - sub * cout, dy = sub / r, dx = sub - dy * r;
        const int per = d.shuffle_h * d.shuffle_w;
        const int b = m / per, rem = m - b * per, y = rem / d.shuffle_w, x = rem - y * d.shuffle_w;
        orow = ((size_t)b * d.shuffle_h * r + y * r + dy) * (d.shuffle_w * r) + x * r + dx;   // output pixel
        ocol = co;
        off = orow * d.ldc + co;
    }
    if (R) v += R[off];
    if (R2) v += R2[off];
    if (C) C[off] = v;
    if (d.C_hl) {
        _Float16 h, l;
        pp_split_f16_chk(d.c_relu ? fmaxf(v, 0.f) : v, h, l);
        _Float16* hp = (_Float16*)d.C_hl + orow * 2 * d.ldc_h + pp_hl_col(ocol, 0);
        hp[0] = h;
        hp[8] = l;
    }
}

template <bool VEC4, int NJ, int OCC>
__global__ __launch_bounds__(256, OCC) void gemm_kernel(const PpGemmDesc d) {
    constexpr int BN = 64 * NJ;
    __shared__ __attribute__((aligned(16))) float As[BM * LDT];
    __shared__ __attribute__((aligned(16))) float Bs[BN * LDT];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int wr = w >> 1, wc = w & 1, l31 = lane & 31, lh = lane >> 5;
    const int m0 = blockIdx.y * BM, n0 = blockIdx.x * BN;
    const int z = blockIdx.z, z0 = z / d.batch1, z1 = z - z0 * d.batch1;
    const float* A = d.A + (size_t)z0 * d.a_bs0 + (size_t)z1 * d.a_bs1;
    const float* Bm = d.B + (size_t)z0 * d.b_bs0 + (size_t)z1 * d.b_bs1;
    float* C = d.C + (size_t)z0 * d.c_bs0 + (size_t)z1 * d.c_bs1;
    const float* R = d.residual ? d.residual + (size_t)z0 * d.c_bs0 + (size_t)z1 * d.c_bs1 : nullptr;
    const float* R2 = d.residual2 ? d.residual2 + (size_t)z0 * d.c_bs0 + (size_t)z1 * d.c_bs1 : nullptr;

    // this thread's 4 (row, k-quad) slots of the A and B tiles: idx = tid + 256 j -> row (tid>>3) + 32 j, quad tid&7
    const int arow0 = tid >> 3;
#define AROW(j) (arow0 + 32 * (j))
    int aoy[4], aox[4];
    int abase[4];  // VEC4 conv: element offset of input pixel (oy*stride - pad, ox*stride - pad) of the row's image
    int ab[VEC4 ? 1 : 4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int m = m0 + AROW(j);
        aoy[j] = aox[j] = abase[j] = 0;
        if (!VEC4) ab[j] = 0;
        if (d.conv_kh != 0 && m < d.M) {
            const int per = d.conv_ho * d.conv_wo;
            const int bi = m / per;
            const int r = m - bi * per;
            aoy[j] = r / d.conv_wo;
            aox[j] = r - aoy[j] * d.conv_wo;
            aoy[j] = aoy[j] * d.conv_stride - d.conv_pad;  // top-left input pixel of the window
            aox[j] = aox[j] * d.conv_stride - d.conv_pad;
            abase[j] = (int)((long long)bi * d.conv_bstride + ((long long)aoy[j] * d.conv_w + aox[j]) * d.lda);
            if (!VEC4) ab[j] = bi;
        }
    }
    const int kq = (tid & 7) * 4;
    // VEC4 conv: the tap (ky, kx) and channel ci of this thread's k = k0 + kq, advanced by BK per K step
    // without divisions (all four rows of the thread share k)
    int tky = 0, tkx = 0, tci = 0;
    if (VEC4 && d.conv_kh != 0) {
        const int tap = kq / d.conv_cin;
        tci = kq - tap * d.conv_cin;
        tky = tap / d.conv_kw;
        tkx = tap - tky * d.conv_kw;
    }

    f32x16 acc[2][NJ];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    f4 ra[4], rb[2 * NJ];
    auto fetch = [&](int k0) __attribute__((always_inline)) {
        const int k = k0 + kq;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (VEC4 && d.conv_kh != 0) {
                f4 v = {0.f, 0.f, 0.f, 0.f};
                const int iy = aoy[j] + tky, ix = aox[j] + tkx;
                if (m0 + AROW(j) < d.M && k < d.K && iy >= 0 && iy < d.conv_h && ix >= 0 && ix < d.conv_w)
                    v = *(const f4*)(A + (long long)abase[j] + (tky * d.conv_w + tkx) * d.lda + tci);
                if (d.relu_in) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) v[i] = v[i] > 0.f ? v[i] : 0.f;
                }
                ra[j] = v;
            } else {
                ra[j] = load_a<VEC4>(d, A, m0 + AROW(j), k, ab[VEC4 ? 0 : j], aoy[j], aox[j]);
            }
            if (j >= 2 * NJ) continue;  // the B tile has BN = 64*NJ rows
            f4 v = {0.f, 0.f, 0.f, 0.f};
            const int n = n0 + AROW(j);
            if (n < d.N) {
                if (d.b_kn) {  // B stored [K][N]
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        if (k + i < d.K) v[i] = Bm[(size_t)(k + i) * d.ldb + n];
                } else {
                    const float* p = Bm + (size_t)n * d.ldb + k;
                    if (VEC4 && k + 3 < d.K) v = *(const f4*)p;
                    else {
#pragma unroll
                        for (int i = 0; i < 4; ++i)
                            if (k + i < d.K) v[i] = p[i];
                    }
                }
            }
            rb[j] = v;
        }
        if (VEC4 && d.conv_kh != 0) {  // advance the tap by BK channels
            tci += BK;
            while (tci >= d.conv_cin) {
                tci -= d.conv_cin;
                if (++tkx == d.conv_kw) {
                    tkx = 0;
                    ++tky;
                }
            }
        }
    };

    const int nk = (d.K + BK - 1) / BK;
    fetch(0);
    for (int kt = 0; kt < nk; ++kt) {
        __syncthreads();  // previous tile fully consumed
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            *(f4*)(As + AROW(j) * LDT + kq) = ra[j];
            if (j < 2 * NJ) *(f4*)(Bs + AROW(j) * LDT + kq) = rb[j];
        }
        __syncthreads();
        if (kt + 1 < nk) fetch((kt + 1) * BK);
#pragma unroll
        for (int q = 0; q < 4; ++q) {  // 4 k-pairs per fragment read: keeps only 4 fragment registers sets live
            f4 af[2], bf[NJ];
#pragma unroll
            for (int i = 0; i < 2; ++i) af[i] = *(const f4*)(As + (wr * 64 + i * 32 + l31) * LDT + lh * 16 + 4 * q);
#pragma unroll
            for (int j = 0; j < NJ; ++j)
                bf[j] = *(const f4*)(Bs + (wc * 32 * NJ + j * 32 + l31) * LDT + lh * 16 + 4 * q);
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < NJ; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i][e], bf[j][e], acc[i][j], 0, 0, 0);
        }
    }

    // ---- epilogue: out = residual + residual2 + gamma * act(alpha * acc + bias)
    const float alpha_ = pp_alpha(d);
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int n = n0 + wc * 32 * NJ + j * 32 + l31;
        if (n >= d.N) continue;
        const float bias = d.bias ? d.bias[n] : 0.f;
        const float gamma = d.gamma ? d.gamma[n] : 1.f;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int m = m0 + wr * 64 + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * lh;
                if (m >= d.M) continue;
                float v = act_apply(acc[i][j][e] * alpha_ + bias, d.act) * gamma;
                epilogue_store(d, C, R, R2, m, n, v);
            }
    }
}

// ---------------------------------------------------------------------------
// Split-precision variant ("f16x3"): every fp32 operand v is scaled by a power of two s and split on the
// fly into two fp16 numbers   hi = f16(s v),  lo = f16(s v - hi)   (s v - hi is exact in fp32), and the
// product a*b is evaluated as hi_a*hi_b + hi_a*lo_b + lo_a*hi_b on v_mfma_f32_32x32x16_f16 — fp16 x fp16
// products are exact in the fp32 accumulator, the dropped lo*lo term is 2^-22 relative.  For |s v| >= 2^-3
// lo is a normal fp16 and 22 operand bits survive; below that lo is subnormal and the operand keeps an
// ABSOLUTE accuracy of 2^-25 / s — what fp32 gives an element of magnitude ~0.25/s — so the scales are
// chosen to put the bulk of the data above 2^-3: activations s_a = 4 (|v| up to 16376 before hi saturates;
// no NaN, the excess stays in lo), weights s_b = 2^k per tensor with max |s_b w| in [512, 1024).  The result
// is multiplied by 1/(s_a s_b) in the epilogue (exact).  Three MFMAs at 16x the fp32-MFMA rate.  Weights
// can be handed over pre-split (d.B_hl / d.b_scale from pp_split_f16x3).
// LDS: hi/lo planes of [rows][32 k] halfs with an 80-byte row stride (conflict-free ds_read_b128).
// ---------------------------------------------------------------------------
constexpr float A_SCALE = PP_A_SCALE;  // activation operand scale of the f16x3 engine

// largest magnitude of 8 values (producers of operand buffers: the saturation report, pp_common.h)
__device__ __forceinline__ float top4(const f4 a, const f4 b) {
    float t = fmaxf(fmaxf(fabsf(a[0]), fabsf(a[1])), fabsf(a[2]));
    t = fmaxf(fmaxf(t, fabsf(a[3])), fabsf(b[0]));
    t = fmaxf(fmaxf(t, fabsf(b[1])), fabsf(b[2]));
    return fmaxf(t, fabsf(b[3]));
}

// an element of 4 the activation split clamps (or a NaN): the on-the-fly kernel's saturation report (pp_common.h)
__device__ __forceinline__ bool over4(const f4 v) {
    return !(fabsf(v[0]) * A_SCALE < 65504.f) | !(fabsf(v[1]) * A_SCALE < 65504.f) | !(fabsf(v[2]) * A_SCALE < 65504.f) |
           !(fabsf(v[3]) * A_SCALE < 65504.f);
}

template <bool WEIGHT = false>
__device__ __forceinline__ void split_f16x4(const f4 v, float s, h4& hi, h4& lo) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float x = v[i] * s;
        const _Float16 h = (_Float16)fminf(fmaxf(x, -65504.f), 65504.f);
        hi[i] = h;
        lo[i] = (_Float16)fminf(fmaxf(x - (float)h, -65504.f), 65504.f);
#ifdef PP_STUDY_ACT_LO_ZERO   // (precision study builds, pp_common.h)
        if (!WEIGHT) lo[i] = (_Float16)0.f;
#endif
#ifdef PP_STUDY_W_LO_ZERO
        if (WEIGHT) lo[i] = (_Float16)0.f;
#endif
    }
}

template <int NJ, int OCC, bool BSPLIT>
__global__ __launch_bounds__(256, OCC) void gemm_f16x3_kernel(const PpGemmDesc d) {
    constexpr bool VEC4 = true;
    constexpr int BN = 64 * NJ;
    constexpr int LDH = 40;  // halfs per LDS row (32 used): 80-byte stride
    __shared__ __attribute__((aligned(16))) _Float16 Ah[BM * LDH], Al[BM * LDH], Bh[BN * LDH], Bl[BN * LDH];

    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int wr = w >> 1, wc = w & 1, l31 = lane & 31, lh = lane >> 5;
    const int m0 = blockIdx.y * BM, n0 = blockIdx.x * BN;
    const int z = blockIdx.z, z0 = z / d.batch1, z1 = z - z0 * d.batch1;
    const float* A = d.A + (size_t)z0 * d.a_bs0 + (size_t)z1 * d.a_bs1;
    const float* Bm = d.B + (size_t)z0 * d.b_bs0 + (size_t)z1 * d.b_bs1;
    constexpr bool bsplit = BSPLIT;  // pre-split weights: [N][ldb] halfs, no batch
    const _Float16* Bhl = (const _Float16*)d.B_hl;
    float* C = d.C + (size_t)z0 * d.c_bs0 + (size_t)z1 * d.c_bs1;
    const float* R = d.residual ? d.residual + (size_t)z0 * d.c_bs0 + (size_t)z1 * d.c_bs1 : nullptr;
    const float* R2 = d.residual2 ? d.residual2 + (size_t)z0 * d.c_bs0 + (size_t)z1 * d.c_bs1 : nullptr;

    // this thread's 4 (row, k-quad) slots of the A and B tiles: idx = tid + 256 j -> row (tid>>3) + 32 j, quad tid&7
    const int arow0 = tid >> 3;
#define AROW(j) (arow0 + 32 * (j))
    int aoy[4], aox[4];
    int abase[4];  // VEC4 conv: element offset of input pixel (oy*stride - pad, ox*stride - pad) of the row's image
    int ab[VEC4 ? 1 : 4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int m = m0 + AROW(j);
        aoy[j] = aox[j] = abase[j] = 0;
        if (!VEC4) ab[j] = 0;
        if (d.conv_kh != 0 && m < d.M) {
            const int per = d.conv_ho * d.conv_wo;
            const int bi = m / per;
            const int r = m - bi * per;
            aoy[j] = r / d.conv_wo;
            aox[j] = r - aoy[j] * d.conv_wo;
            aoy[j] = aoy[j] * d.conv_stride - d.conv_pad;  // top-left input pixel of the window
            aox[j] = aox[j] * d.conv_stride - d.conv_pad;
            abase[j] = (int)((long long)bi * d.conv_bstride + ((long long)aoy[j] * d.conv_w + aox[j]) * d.lda);
            if (!VEC4) ab[j] = bi;
        }
    }
    const int kq = (tid & 7) * 4;
    // VEC4 conv: the tap (ky, kx) and channel ci of this thread's k = k0 + kq, advanced by BK per K step
    // without divisions (all four rows of the thread share k)
    int tky = 0, tkx = 0, tci = 0;
    if (VEC4 && d.conv_kh != 0) {
        const int tap = kq / d.conv_cin;
        tci = kq - tap * d.conv_cin;
        tky = tap / d.conv_kw;
        tkx = tap - tky * d.conv_kw;
    }

    f32x16 acc[2][NJ];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    const float b_scale = bsplit ? d.b_scale : A_SCALE;  // on-the-fly B operands are activations
    const float descale = 1.0f / (A_SCALE * b_scale);

    f4 ra[4], rb[BSPLIT ? 1 : 2 * NJ];
    h4 rbh[BSPLIT ? 2 * NJ : 1], rbl[BSPLIT ? 2 * NJ : 1];  // pre-split B
    auto fetch = [&](int k0) __attribute__((always_inline)) {
        const int k = k0 + kq;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (VEC4 && d.conv_kh != 0) {
                f4 v = {0.f, 0.f, 0.f, 0.f};
                const int iy = aoy[j] + tky, ix = aox[j] + tkx;
                if (m0 + AROW(j) < d.M && k < d.K && iy >= 0 && iy < d.conv_h && ix >= 0 && ix < d.conv_w)
                    v = *(const f4*)(A + (long long)abase[j] + (tky * d.conv_w + tkx) * d.lda + tci);
                if (d.relu_in) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) v[i] = v[i] > 0.f ? v[i] : 0.f;
                }
                ra[j] = v;
            } else {
                ra[j] = load_a<VEC4>(d, A, m0 + AROW(j), k, ab[VEC4 ? 0 : j], aoy[j], aox[j]);
            }
            if (j >= 2 * NJ) continue;  // the B tile has BN = 64*NJ rows
            f4 v = {0.f, 0.f, 0.f, 0.f};
            const int n = n0 + AROW(j);
            if (bsplit) {
                h4 vh = {0, 0, 0, 0}, vl = {0, 0, 0, 0};
                if (n < d.N && k < d.K) {  // K % 8 == 0 is checked on the host for pre-split weights
                    const _Float16* bp = Bhl + (size_t)n * 2 * d.ldb + pp_hl_col(k, 0);
                    vh = *(const h4*)bp;
                    vl = *(const h4*)(bp + 8);
                }
                rbh[BSPLIT ? j : 0] = vh;
                rbl[BSPLIT ? j : 0] = vl;
                continue;
            }
            if (n < d.N) {
                if (d.b_kn) {  // B stored [K][N]
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        if (k + i < d.K) v[i] = Bm[(size_t)(k + i) * d.ldb + n];
                } else {
                    const float* p = Bm + (size_t)n * d.ldb + k;
                    if (VEC4 && k + 3 < d.K) v = *(const f4*)p;
                    else {
#pragma unroll
                        for (int i = 0; i < 4; ++i)
                            if (k + i < d.K) v[i] = p[i];
                    }
                }
            }
            rb[BSPLIT ? 0 : j] = v;
        }
        if (VEC4 && d.conv_kh != 0) {  // advance the tap by BK channels
            tci += BK;
            while (tci >= d.conv_cin) {
                tci -= d.conv_cin;
                if (++tkx == d.conv_kw) {
                    tkx = 0;
                    ++tky;
                }
            }
        }
    };

    const int nk = (d.K + BK - 1) / BK;
    bool sat = false;   // an fp32 operand element beyond the split's range (|v| >= 16376): reported once per thread after the K loop
    fetch(0);
    for (int kt = 0; kt < nk; ++kt) {
        __syncthreads();  // previous tile fully consumed
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            h4 hh, ll;
            sat |= over4(ra[j]);
            split_f16x4(ra[j], A_SCALE, hh, ll);
            *(h4*)(Ah + AROW(j) * LDH + kq) = hh;
            *(h4*)(Al + AROW(j) * LDH + kq) = ll;
            if (j < 2 * NJ) {
                if (bsplit) {
                    hh = rbh[BSPLIT ? j : 0];
                    ll = rbl[BSPLIT ? j : 0];
                } else {
                    sat |= over4(rb[BSPLIT ? 0 : j]);
                    split_f16x4<true>(rb[BSPLIT ? 0 : j], A_SCALE, hh, ll);
                }
                *(h4*)(Bh + AROW(j) * LDH + kq) = hh;
                *(h4*)(Bl + AROW(j) * LDH + kq) = ll;
            }
        }
        __syncthreads();
        if (kt + 1 < nk) fetch((kt + 1) * BK);
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {  // two 16-deep MFMA steps per K tile; lane half lh holds k = 8 lh .. 8 lh + 7
            h8 ah[2], al[2], bh[NJ], bl[NJ];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                ah[i] = *(const h8*)(Ah + (wr * 64 + i * 32 + l31) * LDH + ks * 16 + lh * 8);
                al[i] = *(const h8*)(Al + (wr * 64 + i * 32 + l31) * LDH + ks * 16 + lh * 8);
            }
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                bh[j] = *(const h8*)(Bh + (wc * 32 * NJ + j * 32 + l31) * LDH + ks * 16 + lh * 8);
                bl[j] = *(const h8*)(Bl + (wc * 32 * NJ + j * 32 + l31) * LDH + ks * 16 + lh * 8);
            }
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < NJ; ++j) {
                    acc[i][j] = pp_mfma(al[i], bh[j], acc[i][j]);
                    acc[i][j] = pp_mfma(ah[i], bl[j], acc[i][j]);
                    acc[i][j] = pp_mfma(ah[i], bh[j], acc[i][j]);
                }
        }
    }
    pp_sat_flag(sat);
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] *= descale;

    // ---- epilogue: out = residual + residual2 + gamma * act(alpha * acc + bias)
    const float alpha_ = pp_alpha(d);
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int n = n0 + wc * 32 * NJ + j * 32 + l31;
        if (n >= d.N) continue;
        const float bias = d.bias ? d.bias[n] : 0.f;
        const float gamma = d.gamma ? d.gamma[n] : 1.f;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int m = m0 + wr * 64 + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * lh;
                if (m >= d.M) continue;
                float v = act_apply(acc[i][j][e] * alpha_ + bias, d.act) * gamma;
                epilogue_store(d, C, R, R2, m, n, v);
            }
    }
}

}  // namespace

namespace {

// activation pre-split: x (B, P, C) fp32 with batch / row strides -> contiguous hl operand (B*P rows, ld = C):
// one thread = 8 channels = 32 bytes in, 32 contiguous bytes (8 hi + 8 lo) out
__global__ __launch_bounds__(256) void split_act_kernel(const float* __restrict__ x, long long bstride, int P, int ld,
                                                        int C, long long total8, int relu, _Float16* __restrict__ hl,
                                                        int ldh, int terms) {
    // terms = 2: hl format, 32 bytes per 8 channels (ldh = 2 ld_h halfs per row); terms = 1: h format, 16 bytes (ldh = ld_h)
    const int c8n = C >> 3;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total8; i += (long long)gridDim.x * 256) {
        const long long row = i / c8n;
        const int c = (int)(i - row * c8n) * 8;
        const long long b = row / P, p = row - b * P;
        const float* xp = x + b * bstride + p * ld + c;
        f4 v0 = *(const f4*)xp, v1 = *(const f4*)(xp + 4);
        if (relu) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                v0[k] = v0[k] > 0.f ? v0[k] : 0.f;
                v1[k] = v1[k] > 0.f ? v1[k] : 0.f;
            }
        }
        h4 h0, l0, h1, l1;
        pp_sat_flag(!(top4(v0, v1) * A_SCALE < 65504.f));
        split_f16x4(v0, A_SCALE, h0, l0);
        split_f16x4(v1, A_SCALE, h1, l1);
        _Float16* o = hl + row * ldh + terms * c;
        *(h4*)o = h0;
        *(h4*)(o + 4) = h1;
        if (terms == 2) {
            *(h4*)(o + 8) = l0;
            *(h4*)(o + 12) = l1;
        }
    }
}

// ---------------------------------------------------------------------------
// Row-wise kernels around the GEMMs
// ---------------------------------------------------------------------------

// nn.LayerNorm(eps) over the last dimension: one wave per row (model/stage1 block.py:56,68).  A lane owns NG groups of 8
// consecutive channels (two 16-byte loads; the row is read once and stays in registers), mean and variance are the
// two-pass forms over the registers, and the f16x3 operand of the following linear layer leaves as one 32-byte
// [8 hi | 8 lo] group per store.  NG = 0: any C, the row is re-read from cache (not used by the ViT widths).
template <int NG>
__global__ __launch_bounds__(256) void layernorm_kernel(const float* __restrict__ x, const float* __restrict__ g,
                                                        const float* __restrict__ b, int rows, int C, float eps,
                                                        float* __restrict__ y, _Float16* __restrict__ hl, int terms) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= rows) return;
    const float* xr = x + (size_t)row * C;
    if constexpr (NG > 0) {
        const int ngrp = C >> 3;
        f4 v[NG][2];
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < NG; ++j) {
            const int gi = lane + 64 * j;
            if (gi < ngrp) {
                v[j][0] = *(const f4*)(xr + gi * 8);
                v[j][1] = *(const f4*)(xr + gi * 8 + 4);
            } else {
                v[j][0] = f4{0.f, 0.f, 0.f, 0.f};
                v[j][1] = v[j][0];
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) s += v[j][0][k] + v[j][1][k];
        }
        s = wave_sum(s);
        const float mean = s / (float)C;
        float q = 0.f;
#pragma unroll
        for (int j = 0; j < NG; ++j) {
            if (lane + 64 * j < ngrp) {
#pragma unroll
                for (int h = 0; h < 2; ++h)
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const float dlt = v[j][h][k] - mean;
                        q = fmaf(dlt, dlt, q);
                    }
            }
        }
        q = wave_sum(q);
        const float rstd = 1.0f / sqrtf(q / (float)C + eps);
#pragma unroll
        for (int j = 0; j < NG; ++j) {
            const int gi = lane + 64 * j;
            if (gi >= ngrp) continue;
            f4 o[2];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const f4 gg = *(const f4*)(g + gi * 8 + 4 * h), bb = *(const f4*)(b + gi * 8 + 4 * h);
#pragma unroll
                for (int k = 0; k < 4; ++k) o[h][k] = (v[j][h][k] - mean) * rstd * gg[k] + bb[k];
            }
            if (y) {
                *(f4*)(y + (size_t)row * C + gi * 8) = o[0];
                *(f4*)(y + (size_t)row * C + gi * 8 + 4) = o[1];
            }
            if (hl) {
                h4 h0, l0, h1, l1;
                pp_sat_flag(!(top4(o[0], o[1]) * A_SCALE < 65504.f));
                split_f16x4(o[0], A_SCALE, h0, l0);
                split_f16x4(o[1], A_SCALE, h1, l1);
                _Float16* hp = hl + ((size_t)row * C + gi * 8) * terms;
                *(h4*)hp = h0;
                *(h4*)(hp + 4) = h1;
                if (terms == 2) {
                    *(h4*)(hp + 8) = l0;
                    *(h4*)(hp + 12) = l1;
                }
            }
        }
    } else {
        float s = 0.f;
        for (int c = lane; c < C; c += 64) s += xr[c];
        s = wave_sum(s);
        const float mean = s / (float)C;
        float v = 0.f;
        for (int c = lane; c < C; c += 64) {
            const float dlt = xr[c] - mean;
            v = fmaf(dlt, dlt, v);
        }
        v = wave_sum(v);
        const float rstd = 1.0f / sqrtf(v / (float)C + eps);
        for (int c = lane; c < C; c += 64) {
            const float o = (xr[c] - mean) * rstd * g[c] + b[c];
            if (y) y[(size_t)row * C + c] = o;
            if (hl) {  // f16x3 operand of the following linear layer
                _Float16 h, l;
                pp_split_f16_chk(o, h, l);
                if (terms == 2) {
                    _Float16* hp = hl + (size_t)row * 2 * C + pp_hl_col(c, 0);
                    hp[0] = h;
                    hp[8] = l;
                } else {
                    hl[(size_t)row * C + c] = h;
                }
            }
        }
    }
}

static void launch_layernorm(const float* x, const float* gamma, const float* beta, int rows, int C, float eps, float* y,
                             _Float16* hl, hipStream_t st, int terms = 2) {
    const dim3 grid((rows + 3) / 4), block(256);
    const bool vec = C % 8 == 0 && ((uintptr_t)x % 16 == 0) && ((uintptr_t)gamma % 16 == 0) &&
                     ((uintptr_t)beta % 16 == 0) && (!y || (uintptr_t)y % 16 == 0) && (!hl || (uintptr_t)hl % 16 == 0);
    if (vec && C <= 512)
        hipLaunchKernelGGL(layernorm_kernel<1>, grid, block, 0, st, x, gamma, beta, rows, C, eps, y, hl, terms);
    else if (vec && C <= 1024)
        hipLaunchKernelGGL(layernorm_kernel<2>, grid, block, 0, st, x, gamma, beta, rows, C, eps, y, hl, terms);
    else
        hipLaunchKernelGGL(layernorm_kernel<0>, grid, block, 0, st, x, gamma, beta, rows, C, eps, y, hl, terms);
}

// softmax over the last dimension, in place: one wave per row (layers/attention.py:57)
__global__ __launch_bounds__(256) void softmax_kernel(float* __restrict__ x, int rows, int n, int ld) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= rows) return;
    float* xr = x + (size_t)row * ld;
    float mx = -INFINITY;
    for (int c = lane; c < n; c += 64) mx = fmaxf(mx, xr[c]);
    mx = wave_max(mx);
    float s = 0.f;
    for (int c = lane; c < n; c += 64) {
        const float e = expf(xr[c] - mx);
        xr[c] = e;
        s += e;
    }
    s = wave_sum(s);
    const float inv = 1.0f / s;
    for (int c = lane; c < n; c += 64) xr[c] *= inv;
}

// nn.GroupNorm(G, C, eps) on an NHWC image (+ optional ReLU): one workgroup per (image, group)
__global__ __launch_bounds__(256) void groupnorm_kernel(const float* __restrict__ x, const float* __restrict__ g,
                                                        const float* __restrict__ b, int HW, int C, int G, float eps,
                                                        int relu, float* __restrict__ y) {
    __shared__ float red[8];
    const int img = blockIdx.x / G, grp = blockIdx.x % G, cg = C / G, tid = threadIdx.x;
    const float* xi = x + (size_t)img * HW * C + grp * cg;
    float* yi = y + (size_t)img * HW * C + grp * cg;
    const int n = HW * cg;
    float s = 0.f;
    for (int i = tid; i < n; i += 256) s += xi[(size_t)(i / cg) * C + (i % cg)];
    const float mean = block_reduce_all<4>(s, red, op_sum{}) / (float)n;
    float v = 0.f;
    for (int i = tid; i < n; i += 256) {
        const float dlt = xi[(size_t)(i / cg) * C + (i % cg)] - mean;
        v = fmaf(dlt, dlt, v);
    }
    const float rstd = 1.0f / sqrtf(block_reduce_all<4>(v, red + 4, op_sum{}) / (float)n + eps);
    for (int i = tid; i < n; i += 256) {
        const int c = i % cg;
        const size_t off = (size_t)(i / cg) * C + c;
        float o = (xi[off] - mean) * rstd * g[grp * cg + c] + b[grp * cg + c];
        if (relu) o = o > 0.f ? o : 0.f;
        yi[off] = o;
    }
}

// (B, C, H*W) <-> (B, H*W, C) through a 32x33 LDS tile
__global__ __launch_bounds__(256) void transpose_kernel(const float* __restrict__ in, long long in_bs, int R,
                                                        int Cc, float* __restrict__ out, long long out_bs,
                                                        int ld_out, int col_off) {
    __shared__ float t[32][33];
    const int b = blockIdx.z, r0 = blockIdx.y * 32, c0 = blockIdx.x * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
    const float* ib = in + (size_t)b * in_bs;
    float* ob = out + (size_t)b * out_bs;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int r = r0 + ty + 8 * i, c = c0 + tx;
        if (r < R && c < Cc) t[ty + 8 * i][tx] = ib[(size_t)r * Cc + c];
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c = c0 + ty + 8 * i, r = r0 + tx;
        if (r < R && c < Cc) ob[(size_t)c * ld_out + col_off + r] = t[tx][ty + 8 * i];
    }
}

// DinoVisionTransformer.prepare_tokens_with_masks (vision_transformer.py:209-216):
// tokens[b,0] = cls + pos[0]; tokens[b,1+p] = patch[b,p] + pos[1+p]
__global__ __launch_bounds__(256) void assemble_tokens_kernel(const float* __restrict__ patches,
                                                              const float* __restrict__ cls,
                                                              const float* __restrict__ pos, int T, int C,
                                                              float* __restrict__ tokens) {
    const int t = blockIdx.x, b = blockIdx.y;
    const float* src = t == 0 ? cls : patches + ((size_t)b * T + (t - 1)) * C;
    float* dst = tokens + ((size_t)b * (T + 1) + t) * C;
    for (int c = threadIdx.x; c < C; c += 256) dst[c] = src[c] + pos[(size_t)t * C + c];
}

// F.normalize(x, dim=1) for short rows (affine_regressor.py:83)
__global__ void normalize_rows_kernel(const float* __restrict__ x, int rows, int n, float eps,
                                      float* __restrict__ y) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= rows) return;
    float s = 0.f;
    for (int i = 0; i < n; ++i) s = fmaf(x[(size_t)r * n + i], x[(size_t)r * n + i], s);
    const float d = fmaxf(sqrtf(s), eps);
    for (int i = 0; i < n; ++i) y[(size_t)r * n + i] = x[(size_t)r * n + i] / d;
}

// (The maxima below begin at 0.f and meet absolute values through fmaxf, which drops a NaN: no operand is NaN or -0, so fmaxf is
// exact on them and their order does not show in the bits.)
// max |w| -> power-of-two scale with max |s w| in [512, 1024): init / grid-wide max (the bit pattern of a non-negative float
// orders like an unsigned integer: one atomicMax per workgroup) / finish, three small launches without a workspace
__global__ void absmax_init_kernel(float* __restrict__ scale) { ((unsigned*)scale)[0] = 0u; }

__global__ __launch_bounds__(256) void absmax_kernel(const float* __restrict__ w, long long n, float* __restrict__ scale) {
    __shared__ float red[4];
    float m = 0.f;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) m = fmaxf(m, fabsf(w[i]));
    m = block_reduce_to<4>(m, red, op_max{});
    if (threadIdx.x == 0) {
        if (m == m) atomicMax((unsigned*)scale, __float_as_uint(m));   // (a NaN never enters the maximum)
    }
}

__global__ void absmax_finish_kernel(float* __restrict__ scale, int with_inverse, int emax) {
    const float m = scale[0];
    int e = 0;
    if (m > 0.f && m < INFINITY) {
        (void)frexpf(m, &e);  // m = f * 2^e, f in [0.5, 1)
        e = 10 - e;           // s m in [512, 1024)
    }
    e = e > emax ? emax : (e < -emax ? -emax : e);
    scale[0] = ldexpf(1.f, e);
    if (with_inverse) scale[1] = ldexpf(1.f, -e);
}

// two launches, no atomics, 16-byte loads: every workgroup leaves its maximum in partial[blockIdx.x], one workgroup folds them
__global__ __launch_bounds__(256) void absmax_part_kernel(const float* __restrict__ w, long long n, float* __restrict__ partial) {
    __shared__ float red[4];
    float m = 0.f;
    const long long n4 = ((uintptr_t)w & 15) == 0 ? n >> 2 : 0;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
        const f4 v = ((const f4*)w)[i];
        m = fmaxf(fmaxf(m, fmaxf(fabsf(v[0]), fabsf(v[1]))), fmaxf(fabsf(v[2]), fabsf(v[3])));
    }
    for (long long i = 4 * n4 + (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) m = fmaxf(m, fabsf(w[i]));
    m = block_reduce_to<4>(m, red, op_max{});
    if (threadIdx.x == 0) partial[blockIdx.x] = m;   // (fmaxf drops a NaN operand)
}

__global__ __launch_bounds__(256) void absmax_fold_kernel(const float* __restrict__ partial, int np, float* __restrict__ scale, int with_inverse, int emax) {
    __shared__ float red[4];
    float m = 0.f;
    for (int i = threadIdx.x; i < np; i += 256) m = fmaxf(m, partial[i]);
    m = block_reduce_to<4>(m, red, op_max{});
    if (threadIdx.x == 0) {
        int e = 0;
        if (m > 0.f && m < INFINITY) {
            (void)frexpf(m, &e);
            e = 10 - e;
        }
        e = e > emax ? emax : (e < -emax ? -emax : e);
        scale[0] = ldexpf(1.f, e);
        if (with_inverse) scale[1] = ldexpf(1.f, -e);
    }
}

static void launch_pow2_scale(const float* w, long long n, float* scale, int with_inverse, int emax, hipStream_t st) {
    hipLaunchKernelGGL(absmax_init_kernel, dim3(1), dim3(1), 0, st, scale);
    const int grid = (int)((n + 2047) / 2048 < 1024 ? (n + 2047) / 2048 : 1024);
    hipLaunchKernelGGL(absmax_kernel, dim3(grid), dim3(256), 0, st, w, n, scale);
    hipLaunchKernelGGL(absmax_finish_kernel, dim3(1), dim3(1), 0, st, scale, with_inverse, emax);
}

__global__ void split_f16x3_kernel(const float* __restrict__ w, long long n, const float* __restrict__ scale,
                                   _Float16* __restrict__ hl, int terms) {
    const float s = scale[0];
    if (terms == 1) {   // h format: f16(s w)
        for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
            hl[i] = (_Float16)fminf(fmaxf(w[i] * s, -65504.f), 65504.f);
        return;
    }
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const float x = w[i] * s;
        const _Float16 h = (_Float16)fminf(fmaxf(x, -65504.f), 65504.f);
        _Float16* p = hl + ((i >> 3) << 4) + (i & 7);  // rows are multiples of 8 long: groups never straddle rows
        p[0] = h;
#ifdef PP_STUDY_W_LO_ZERO   // (precision study builds, pp_common.h)
        p[8] = (_Float16)0.f;
#else
        p[8] = (_Float16)(x - (float)h);
#endif
    }
}

// pp_split_weights_ws: the fold of absmax_part_kernel's maxima inside the split launch (every workgroup folds the <= 1024 partial
// maxima itself, workgroup 0 leaves the scale pair) — two launches per weight instead of four, nothing read back by the host
__global__ __launch_bounds__(256) void split_fold_kernel(const float* __restrict__ w, long long n, const float* __restrict__ partial, int np, int emax,
                                                         float* __restrict__ scale2, _Float16* __restrict__ hl, int terms) {
    __shared__ float red[4];
    __shared__ float s_sh;
    float m = 0.f;
    for (int i = threadIdx.x; i < np; i += 256) m = fmaxf(m, partial[i]);
    m = block_reduce_to<4>(m, red, op_max{});
    if (threadIdx.x == 0) {
        int e = 0;
        if (m > 0.f && m < INFINITY) {
            (void)frexpf(m, &e);
            e = 10 - e;
        }
        e = e > emax ? emax : (e < -emax ? -emax : e);
        s_sh = ldexpf(1.f, e);
        if (blockIdx.x == 0) {
            scale2[0] = ldexpf(1.f, e);
            scale2[1] = ldexpf(1.f, -e);
        }
    }
    __syncthreads();
    const float s = s_sh;
    if (terms == 1) {
        for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
            hl[i] = (_Float16)fminf(fmaxf(w[i] * s, -65504.f), 65504.f);
        return;
    }
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const float x = w[i] * s;
        const _Float16 h = (_Float16)fminf(fmaxf(x, -65504.f), 65504.f);
        _Float16* p = hl + ((i >> 3) << 4) + (i & 7);
        p[0] = h;
        p[8] = (_Float16)(x - (float)h);
    }
}

}  // namespace

extern "C" {

int pp_split_weights_t(const float* w, long long n, int terms, void* out, float* scale, void* stream) {
    if (!w || !out || !scale || n <= 0 || n % 8 != 0 || (terms != 1 && terms != 2)) return PP_EINVAL;
    launch_pow2_scale(w, n, scale, 0, 30, (hipStream_t)stream);
    const int grid = (int)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096);
    hipLaunchKernelGGL(split_f16x3_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, w, n, scale, (_Float16*)out, terms);
    return pp_last_launch();
}

int pp_split_weights_ws(const float* w, long long n, int terms, void* out, float* scale2, float* partials, void* stream) {
    if (!w || !out || !scale2 || !partials || n <= 0 || n % 8 != 0 || (terms != 1 && terms != 2)) return PP_EINVAL;
    const int gp = (int)((n + 8191) / 8192 < 1024 ? (n + 8191) / 8192 : 1024);
    hipLaunchKernelGGL(absmax_part_kernel, dim3(gp), dim3(256), 0, (hipStream_t)stream, w, n, partials);
    const int grid = (int)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096);
    hipLaunchKernelGGL(split_fold_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, w, n, (const float*)partials, gp, 30, scale2, (_Float16*)out, terms);
    return pp_last_launch();
}

int pp_split_f16x3(const float* w, long long n, void* hl, float* scale, void* stream) { return pp_split_weights_t(w, n, 2, hl, scale, stream); }

int pp_split_with_scale_t(const float* w, long long n, int terms, const float* scale, void* out, void* stream) {
    if (!w || !out || !scale || n <= 0 || n % 8 != 0 || (terms != 1 && terms != 2)) return PP_EINVAL;
    const int grid = (int)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096);
    hipLaunchKernelGGL(split_f16x3_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, w, n, scale, (_Float16*)out, terms);
    return pp_last_launch();
}

int pp_pow2_scale(const float* x, long long n, float* scale2, void* stream) {
    if (!x || !scale2 || n <= 0) return PP_EINVAL;
    launch_pow2_scale(x, n, scale2, 1, 100, (hipStream_t)stream);
    return pp_last_launch();
}

int pp_pow2_scale_ws(const float* x, long long n, float* scale2, float* partials, void* stream) {
    if (!x || !scale2 || !partials || n <= 0) return PP_EINVAL;
    const int grid = (int)((n + 8191) / 8192 < 1024 ? (n + 8191) / 8192 : 1024);
    hipLaunchKernelGGL(absmax_part_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, x, n, partials);
    hipLaunchKernelGGL(absmax_fold_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const float*)partials, grid, scale2, 1, 100);
    return pp_last_launch();
}

// split_act_kernel with a device-side scale: the operand of s x (s = scale[0], a power of two chosen on the device from max|x|)
__global__ __launch_bounds__(256) void split_act_scaled_kernel(const float* __restrict__ x, long long rows, int ld, int C, const float* __restrict__ scale,
                                                               _Float16* __restrict__ hl, int terms) {
    const int c8n = C >> 3;
    const long long total8 = rows * c8n;
    const float s = scale[0] * A_SCALE;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total8; i += (long long)gridDim.x * 256) {
        const long long row = i / c8n;
        const int c = (int)(i - row * c8n) * 8;
        const float* xp = x + row * ld + c;
        const f4 v0 = *(const f4*)xp, v1 = *(const f4*)(xp + 4);
        h4 h0, l0, h1, l1;
        split_f16x4(v0, s, h0, l0);
        split_f16x4(v1, s, h1, l1);
        _Float16* o = hl + (row * C + c) * terms;
        *(h4*)o = h0;
        *(h4*)(o + 4) = h1;
        if (terms == 2) {
            *(h4*)(o + 8) = l0;
            *(h4*)(o + 12) = l1;
        }
    }
}

int pp_split_scaled_t(const float* x, long long rows, int ld, int C, const float* scale, void* hl, int terms, void* stream) {
    if (!x || !hl || !scale || rows <= 0 || C <= 0 || C % 8 != 0 || ld % 4 != 0 || ld < C || ((uintptr_t)x & 15) != 0 || ((uintptr_t)hl & 15) != 0 ||
        (terms != 1 && terms != 2))
        return PP_EINVAL;
    const long long total8 = rows * (C / 8);
    const int grid = (int)((total8 + 255) / 256 < 8192 ? (total8 + 255) / 256 : 8192);
    hipLaunchKernelGGL(split_act_scaled_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, x, rows, ld, C, scale, (_Float16*)hl, terms);
    return pp_last_launch();
}

int pp_split_activation_t(const float* x, long long batch_stride, int B, int P, int row_stride, int C, int relu, void* hl,
                          int ld_h, int terms, void* stream) {
    if (!x || !hl || B <= 0 || P <= 0 || C <= 0 || C % 8 != 0 || row_stride % 4 != 0 || batch_stride % 4 != 0 ||
        ((uintptr_t)x % 16) != 0 || ((uintptr_t)hl % 16) != 0 || ld_h < C || ld_h % 8 != 0 || (terms != 1 && terms != 2))
        return PP_EINVAL;
    const long long total8 = (long long)B * P * (C / 8);
    const int grid = (int)((total8 + 255) / 256 < 8192 ? (total8 + 255) / 256 : 8192);
    hipLaunchKernelGGL(split_act_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, x, batch_stride, P, row_stride, C,
                       total8, relu, (_Float16*)hl, terms * ld_h, terms);
    return pp_last_launch();
}

int pp_split_activation_ld(const float* x, long long batch_stride, int B, int P, int row_stride, int C, int relu, void* hl,
                           int ld_h, void* stream) {
    return pp_split_activation_t(x, batch_stride, B, P, row_stride, C, relu, hl, ld_h, 2, stream);
}

// Second half of a split-K linear layer: out[m, n] = act(sum_s part[s, m, n] + bias[n]) (fixed summation order s = 0, 1, ...)
__global__ __launch_bounds__(256) void sum_slices_kernel(const float* __restrict__ part, int S, long long mn, int N,
                                                         const float* __restrict__ bias, int act, float* __restrict__ out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= mn) return;
    float v = 0.f;
    for (int s = 0; s < S; ++s) v += part[(long long)s * mn + i];
    out[i] = act_apply(v + (bias ? bias[i % N] : 0.f), act);
}

int pp_sum_slices(const float* part, int S, int M, int N, const float* bias, int act, float* out, void* stream) {
    if (!part || !out || S <= 0 || M <= 0 || N <= 0 || act < 0 || act > PP_ACT_TANH) return PP_EINVAL;
    const long long mn = (long long)M * N;
    hipLaunchKernelGGL(sum_slices_kernel, dim3((unsigned)((mn + 255) / 256)), dim3(256), 0, (hipStream_t)stream, part, S, mn, N, bias, act, out);
    return pp_last_launch();
}

// A few columns of an existing hl operand (channel concatenation with a narrow tensor: the flow decoder's [out_net | flow],
// raft_decoder.py:161): columns col0 .. col0 + c - 1 of every row <- x[row][0 .. c-1]; any alignment, one element per thread.
__global__ __launch_bounds__(256) void hl_patch_kernel(const float* __restrict__ x, int ld_x, int c, long long rows, _Float16* __restrict__ hl,
                                                       int ldh, int col0, int terms) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= rows * c) return;
    const long long row = i / c;
    const int j = (int)(i - row * c);
    _Float16 h, l;
    pp_split_f16_chk(x[row * ld_x + j], h, l);
    if (terms == 2) {
        _Float16* hp = hl + row * ldh + pp_hl_col(col0 + j, 0);
        hp[0] = h;
        hp[8] = l;
    } else {
        hl[row * ldh + col0 + j] = h;
    }
}

int pp_hl_patch_columns_t(const float* x, int ld_x, int c, long long rows, void* hl, int ld_h, int col0, int terms, void* stream) {
    if (!x || !hl || c <= 0 || c > 64 || rows <= 0 || ld_x < c || col0 < 0 || col0 + c > ld_h || ld_h % 8 != 0 || (terms != 1 && terms != 2))
        return PP_EINVAL;
    const long long n = rows * c;
    hipLaunchKernelGGL(hl_patch_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, ld_x, c, rows,
                       (_Float16*)hl, terms * ld_h, col0, terms);
    return pp_last_launch();
}

int pp_hl_patch_columns(const float* x, int ld_x, int c, long long rows, void* hl, int ld_h, int col0, void* stream) {
    return pp_hl_patch_columns_t(x, ld_x, c, rows, hl, ld_h, col0, 2, stream);
}

int pp_split_activation(const float* x, long long batch_stride, int B, int P, int row_stride, int C, int relu, void* hl,
                        void* stream) {
    return pp_split_activation_ld(x, batch_stride, B, P, row_stride, C, relu, hl, C, stream);
}

}  // extern "C"
PP_SAT_SETTER(pp_sat_set_gemm)

// pp_gemm_generic_epilogue: every launch takes the generic epilogue body (tests compare the kinds against it)
static std::atomic<int> g_epi_generic{0};

// Epilogue kind of a vector-epilogue launch of the pre-split kernel (pp_gemm_dev.h): a kind only where the descriptor is exactly
// its flag set, the generic body otherwise
int pp_gemm_epi_kind(const PpGemmDesc& d) {
    if (g_epi_generic.load(std::memory_order_relaxed)) return PP_EPI_GENERIC;
    if (d.residual2 || d.shuffle_r != 0) return PP_EPI_GENERIC;
    if (!d.C && d.C_hl && d.bias && !d.gamma && !d.residual && !d.c_relu) {
        if (d.act == PP_ACT_NONE) return PP_EPI_HL_LIN;
        if (d.act == PP_ACT_GELU) return PP_EPI_HL_GELU;
        return PP_EPI_GENERIC;
    }
    if (d.C && !d.C_hl && d.act == PP_ACT_NONE) {
        if (d.bias && d.gamma && d.residual) return PP_EPI_C_BGR;
        if (!d.bias && !d.gamma && !d.residual) return PP_EPI_C_PLAIN;
    }
    return PP_EPI_GENERIC;
}

// The launch view of a pp_gemm call (gemm_normalise): the descriptor as the kernels take it, and what it says about the operands.
struct GemmView {
    PpGemmDesc d;   // grouped batches as one launch (grp_rows), K slices as extra rows (ks_rows), operand extents filled in
    long long z;    // products in the batch (batch0 * batch1)
    int terms;      // operand terms: 1 for plain fp16 operands (PP_PREC_F16), 2 otherwise
    bool vec;       // 16-byte operand loads: K-contiguous operands with lda / ldb / Cin % 4 == 0
    bool asplit;    // both operands pre-split: pp_gemm_u_kernel / pp_gemm_uh_kernel
    bool split;     // fp32 operands split on the fly: gemm_f16x3_kernel (unaligned (tiny) layers stay on the fp32 kernel)
    bool fvec;      // fp32 operands the fp32 engine takes: pp_gemm_f_kernel
    bool u_vec;     // pre-split: the vector epilogue's conditions hold
    bool h_shape;   // pre-split: a 3x3 convolution the row-shared kernel takes
};

// Validate *desc and rewrite it into the launch view v: PP_OK, or PP_EINVAL for a descriptor no kernel takes.
static int gemm_normalise(const PpGemmDesc* desc, GemmView& v) {
    // (B may be NULL when BOTH operands arrive pre-split: products of two transient operands, picopose_amd/ops.matmul_operands)
    if (!desc || (!desc->A && !desc->A_hl) || (!desc->B && !(desc->A_hl && desc->B_hl)) || (!desc->C && !desc->C_hl)) return PP_EINVAL;
    {   // operand output: rows of ldc_h elements holding the N columns (pixel-shuffle stores: the N / r^2 channels of a pixel)
        const int r2 = desc->shuffle_r > 0 ? desc->shuffle_r * desc->shuffle_r : 1;
        if (desc->C_hl && (desc->ldc_h < desc->N / r2 || desc->ldc_h % 8 != 0 || desc->batch0 * desc->batch1 != 1 ||
                           (desc->shuffle_r != 0 && (desc->N / r2) % 8 != 0)))
            return PP_EINVAL;
    }
    PpGemmDesc& d = v.d;
    d = *desc;
    if (d.M <= 0 || d.N <= 0 || d.K <= 0 || d.batch0 <= 0 || d.batch1 <= 0) return PP_EINVAL;
    if (d.act < 0 || d.act > PP_ACT_TANH) return PP_EINVAL;
    if (d.conv_kh != 0) {
        if (d.conv_kw <= 0 || d.conv_cin <= 0 || d.conv_stride <= 0 || d.conv_h <= 0 || d.conv_w <= 0 ||
            d.conv_ho <= 0 || d.conv_wo <= 0 || d.K != d.conv_kh * d.conv_kw * d.conv_cin)
            return PP_EINVAL;
    }
    if (d.shuffle_r != 0 && (d.N % (d.shuffle_r * d.shuffle_r) != 0 || d.shuffle_h * d.shuffle_w <= 0))
        return PP_EINVAL;
    if (d.conv_kh != 0 && d.conv_bstride == 0) d.conv_bstride = (long long)d.conv_h * d.conv_w * d.lda;
    if (d.conv_kh != 0) {  // the conv loader keeps 32-bit element offsets per row
        const long long imgs = (d.M + (long long)d.conv_ho * d.conv_wo - 1) / ((long long)d.conv_ho * d.conv_wo);
        if (imgs * d.conv_bstride >= (1LL << 31)) return PP_EINVAL;
    }
    // 16-byte vector loads need aligned rows: K-contiguous operands with lda/ldb/Cin % 4 == 0
    bool vec = (d.A_hl || (uintptr_t)d.A % 16 == 0) && ((uintptr_t)d.B % 16 == 0) && d.lda % 4 == 0 &&
               (d.b_kn || d.ldb % 4 == 0) && d.a_bs0 % 4 == 0 && d.a_bs1 % 4 == 0 && d.b_bs0 % 4 == 0 &&
               d.b_bs1 % 4 == 0;
    if (d.conv_kh != 0 && (d.conv_cin % 4 != 0 || d.conv_bstride % 4 != 0)) vec = false;
    v.vec = vec;
    static const bool dbg = getenv("PP_GEMM_DEBUG") != nullptr;
    if (dbg && !vec)
        fprintf(stderr, "[pp_gemm] scalar path: M=%d N=%d K=%d lda=%d ldb=%d conv=%dx%d cin=%d b_kn=%d batch=%d A%%16=%d B%%16=%d\n", d.M, d.N, d.K, d.lda,
                d.ldb, d.conv_kh, d.conv_kw, d.conv_cin, d.b_kn, d.batch0 * d.batch1, (int)((uintptr_t)d.A % 16), (int)((uintptr_t)d.B % 16));
    static const bool f_engine_on = [] { const char* e = getenv("PP_F32_ENGINE"); return !(e && e[0] == '0'); }();
    static const bool f_group_on = [] { const char* e = getenv("PP_F32_GROUPED"); return !(e && e[0] == '0'); }();
    d.grp_rows = 0;
    d.grp_b_bytes = 0;
    // A batch of fp32 products with A and C blocks one behind the other (the sixteen products of a Winograd convolution): ONE persistent
    // launch of the fp32 engine over all the row tiles — a row tile lies inside one group (M % 256 == 0) and reads that group's weights.
    if (f_engine_on && f_group_on && d.prec == PP_PREC_F32 && d.batch0 > 1 && d.batch1 == 1 && vec && !d.A_hl && d.conv_kh == 0 && !d.b_kn &&
        d.shuffle_r == 0 && !d.residual && !d.residual2 && d.ksplit <= 1 && d.M % 256 == 0 && d.a_bs0 == (long long)d.M * d.lda &&
        d.c_bs0 == (long long)d.M * d.ldc && (long long)d.M * d.batch0 < (1LL << 31) && d.b_bs0 >= 0) {
        PpGemmDesc g = d;
        g.grp_rows = d.M;
        g.grp_b_bytes = d.b_bs0 * 4;
        g.M = d.M * d.batch0;
        g.batch0 = 1;
        if (pp_gemm_f_ok(g)) d = g;
    }
    // The same for a batch of PRE-SPLIT products (the 36 frequencies of a Winograd F(4x4, 3x3) convolution on the f16x3 engine): A_hl /
    // C blocks one behind the other, the weights of group g b_bs0 ELEMENTS further on — one persistent launch of pp_gemm_u_kernel.
    if (d.A_hl && d.B_hl && d.batch0 > 1 && d.batch1 == 1 && d.conv_kh == 0 && !d.b_kn && d.shuffle_r == 0 && !d.residual && !d.residual2 &&
        d.ksplit <= 1 && !d.C_hl && d.M % 256 == 0 && d.a_bs0 == (long long)d.M * d.lda && d.c_bs0 == (long long)d.M * d.ldc &&
        (long long)d.M * d.batch0 < (1LL << 31) && d.b_bs0 >= 0 && d.b_bs0 % 8 == 0) {
        d.grp_rows = d.M;
        d.grp_b_bytes = d.b_bs0 * (d.prec == PP_PREC_F16 ? 2 : 4);
        d.M *= d.batch0;
        d.batch0 = 1;
    }
    const long long z = v.z = (long long)d.batch0 * d.batch1;
    const bool f16 = d.prec == PP_PREC_F16;          // plain fp16 operands: pre-split kernels only
    const int terms = v.terms = f16 ? 1 : 2;         // operand terms
    const bool split = v.split = d.prec == PP_PREC_F16X3 && vec;
    const bool asplit = v.asplit = d.A_hl != nullptr;
    if (f16 && !asplit) return PP_EINVAL;
    if (asplit) {
        const bool ok = d.B_hl && (d.prec == PP_PREC_F16X3 || f16) && z == 1 && !d.b_kn && !d.relu_in &&
                        d.K % 8 == 0 && d.lda % 8 == 0 && d.ldb % 8 == 0 && d.b_scale > 0.f &&
                        (d.conv_kh == 0 || (d.conv_cin % 8 == 0 && d.conv_bstride % 8 == 0)) &&
                        ((uintptr_t)d.A_hl % 16 == 0) && ((uintptr_t)d.B_hl % 16 == 0);
        if (!ok) return PP_EINVAL;
        pp_gemm_extents(d, 2 * terms, d.a_hl_bytes, d.b_hl_bytes);
        // (32-bit byte offsets; 0xFFFFFFFF is the "reads zero" marker)
        if (d.a_hl_bytes >= 0xFFFFFF00LL || d.b_hl_bytes >= 0xFFFFFF00LL) return PP_EINVAL;
    }
    d.ks_rows = 0;
    if (d.ksplit > 1) {   // K slices as extra tile rows (include/picopose_hip.h): from here on d is the launch's view, M = S rows-blocks of K / S
        if (!asplit || d.conv_kh != 0 || d.M % 256 != 0 || d.K % (64 * d.ksplit) != 0 || d.bias || d.gamma || d.residual || d.residual2 ||
            d.act != 0 || d.C_hl || d.shuffle_r != 0 || !d.C || (long long)d.M * d.ksplit >= (1LL << 31))
            return PP_EINVAL;
        d.ks_rows = d.M;
        d.M *= d.ksplit;
        d.K /= d.ksplit;
    }
    if (d.B_hl && (d.b_kn || d.ldb % 8 != 0 || d.K % 8 != 0 || z != 1 || !(d.b_scale > 0.f))) return PP_EINVAL;
    if (d.B_hl && !split && !f16) {                  // unaligned layer: the fp32 kernel reads d.B
        // ... whose epilogue knows nothing of a weight scale handed over as a device scalar (ops._weight_args cache="dev": b_scale = 1,
        // alpha_dev = 2^-k for weights pre-multiplied by 2^k): refusing beats a result that is off by 2^-k without an error
        if (d.alpha_dev || d.alpha_dev2) return PP_EINVAL;
        d.B_hl = nullptr;
    }
    v.fvec = f_engine_on && !asplit && !split && vec && z == 1 && pp_gemm_f_ok(d);
    if (v.fvec) pp_gemm_extents(d, 4, d.a_hl_bytes, d.b_hl_bytes);
    v.u_vec = asplit && pp_gemm_u_vec_ok(d);
    v.h_shape = v.u_vec && pp_gemm_uh_shape_ok(d, terms);
    return PP_OK;
}

// TAIL SPLIT (round 6; configurations 9 = 256x256 + tail, 10 = 256x128 + tail).  A persistent launch of T tiles on S slots takes
// ceil(T / S) rounds; the ViT linears at M = 49 344 leave the last round of 256-row tiles 5-50 % filled (fc1: 9.05 rounds -> 10,
// proj / fc2: 2.26 -> 3).  The rows of the full rounds run on the big tile, the remaining rows as a second launch on 128x128 tiles
// (two workgroups per CU: a short round of quarter-size tiles).  Dense launches only (a row's address is base + m * pitch: the tail is the
// same descriptor with shifted pointers); every tile configuration accumulates in the same order, so the split leaves no trace in the bits.
static int tail_rows(const GemmView& v, int big_bn, int cus) {   // r: rows [0, r) on the 256 x big_bn tile, [r, M) on 128x128; 0: no split
    const PpGemmDesc& d = v.d;
    if (!((v.asplit || v.fvec) && d.conv_kh == 0 && d.shuffle_r == 0 && d.ks_rows == 0 && d.grp_rows == 0 && v.z == 1)) return 0;
    const long long gx = (d.N + big_bn - 1) / big_bn, gy = (d.M + 255) / 256, tiles = gx * gy, full = tiles / cus;
    if (full < 1 || tiles % cus == 0) return 0;
    const long long r = full * cus / gx * 256;
    return (r > 0 && r < d.M && d.M - r >= 128) ? (int)r : 0;
}

// What one pp_gemm call launches.  Its cfg, amode and engine are the launch record's fields (bench.py gemm_per_kernel decodes them).
enum { GE_U, GE_UH, GE_F, GE_FLY, GE_R1 };   // pp_gemm_u_kernel, pp_gemm_uh_kernel, pp_gemm_f_kernel, gemm_f16x3_kernel, gemm_kernel
struct GemmPlan {
    int engine;      // GE_*
    int cfg;         // the configuration that runs, canonical (PP_GEMM_FORCE_CFG numbering; a tail split: its big tile)
    int tile;        // PP_U_* block tile of the pre-split / fp32 engine
    int amode;       // MODE of pp_gemm_u_kernel (1: pp_gemm_uh_kernel), 16 + MODE of pp_gemm_f_kernel, others 8 + vec + 2 (on the fly)
    bool vec;        // pre-split: the vector epilogue; gemm_kernel: 16-byte loads
    int tail_rows;   // > 0: rows [0, tail_rows) on `tile`, the rest as a second launch on 128x128 tiles
};

// Tile configurations ("cfg", PP_GEMM_FORCE_CFG numbering): the one place a requested configuration becomes a kernel and a tile.
// Both operands pre-split (pp_gemm_u_kernel.h): 0 = 128x128 tile, two workgroups per CU; 2 = 128x64, two per CU; 4 = 256x128 (3,
// the former one-shot launch of it, is an alias); 5 = 256x256; 6 = 256x256 with row-shared A delivery (3x3 convolutions); 7 / 8 (the
// former two / three-workgroups-per-CU K-16 kernels) are aliases of 0.  All of them persistent (a launch with fewer tiles than slots
// is one tile per workgroup) and bit-identical in their results.  fp32 operands (split on the fly, or fp32 MFMA): 0 / 1 = 128x128 at
// 2 / 3 workgroups per CU, 2 = 128x64.  fp32 operands on aligned shapes: the fp32 engine (pp_gemm_f.hip; configurations 3 = 128x128,
// 4 = 256x128, 5 = 256x256, 6 = 128x64, 7 = 256x192 — every one of them accumulates in the same order).  The round-1 gemm_kernel
// keeps batched products, B [K][N], unaligned rows.  9 / 10: the tail split (tail_rows) of 5 / 4.  11: the pre-split engine's 256x192
// tile (vector epilogue, modes 0 - 2; the same accumulation order, the same bits) — for the fp32 engine 11 is not a configuration.
static GemmPlan gemm_plan(const GemmView& v, int cfg, int cus) {
    const PpGemmDesc& d = v.d;
    GemmPlan p{};
    if (cfg == 9 || cfg == 10) {
        p.tail_rows = cfg == 10 || d.N > 128 ? tail_rows(v, cfg == 9 ? 256 : 128, cus) : 0;
        cfg = cfg == 9 ? 5 : 4;
    }
    if (v.asplit) {
        cfg = cfg == 3 ? 4 : (cfg == 1 || cfg == 7 || cfg == 8) ? 0 : cfg;   // aliases
        if (cfg == 6 && !(v.h_shape && d.N > 128)) cfg = 5;
        if (cfg == 5 && d.N <= 128) cfg = 4;
        if (!v.u_vec && cfg != 2) cfg = 0;   // the element-wise epilogue exists for the two 128-row tiles
        p.engine = cfg == 6 ? GE_UH : GE_U;
        p.amode = cfg == 6 ? 1 : pp_gemm_u_mode(d, v.terms);
        if (cfg == 11 && p.amode == 3) cfg = 4;   // (K slices: no 256x192 instantiation)
        p.tile = cfg == 11 ? PP_U_256x192 : cfg == 5 ? PP_U_256x256 : cfg == 4 ? PP_U_256x128 : cfg == 2 ? PP_U_128x64 : PP_U_128x128;
        p.vec = v.u_vec;
    } else if (v.fvec && (cfg >= 3 || d.grp_rows != 0)) {
        if (cfg < 3) cfg = 3;   // a grouped batch exists on the engine only (the round-1 kernel would read group 0's weights for every row)
        const int mode = pp_gemm_f_mode(d);
        if (mode == 2 && (cfg == 5 || cfg == 7)) cfg = 4;   // (natural-order convolutions: the 256x128 tile, pp_f_launch_tile)
        p.engine = GE_F;
        p.tile = cfg == 7 ? PP_F_256x192 : cfg == 5 ? PP_U_256x256 : cfg == 4 ? PP_U_256x128 : cfg == 3 ? PP_U_128x128 : PP_U_128x64;
        p.amode = 16 + mode;
    } else {
        p.engine = v.split ? GE_FLY : GE_R1;
        p.amode = 8 + (v.vec ? 1 : 0) + (v.split ? 2 : 0);
        p.vec = v.vec;
    }
    p.cfg = cfg;
    return p;
}

// gemm_f16x3_kernel / gemm_kernel: 2 = the 128x64 tile, 0 / otherwise 128x128 at 2 / 3 workgroups per CU (2 without vector loads)
static int gemm_r1_launch(const GemmPlan& p, const PpGemmDesc& d, long long z, hipStream_t st) {
    const bool narrow = p.cfg == 2, occ2 = p.cfg == 0;
    void (*k)(PpGemmDesc);
    if (p.engine == GE_FLY && d.B_hl) k = narrow ? gemm_f16x3_kernel<1, 4, true> : occ2 ? gemm_f16x3_kernel<2, 2, true> : gemm_f16x3_kernel<2, 3, true>;
    else if (p.engine == GE_FLY) k = narrow ? gemm_f16x3_kernel<1, 4, false> : occ2 ? gemm_f16x3_kernel<2, 2, false> : gemm_f16x3_kernel<2, 3, false>;
    else if (!p.vec) k = narrow ? gemm_kernel<false, 1, 2> : gemm_kernel<false, 2, 2>;   // scalar loads (Cin % 4 != 0: 7x7 / 1x1 / patch embed)
    else k = narrow ? gemm_kernel<true, 1, 4> : occ2 ? gemm_kernel<true, 2, 2> : gemm_kernel<true, 2, 3>;
    const dim3 grid((d.N + (narrow ? 63 : 127)) / (narrow ? 64 : 128), (unsigned)((d.M + BM - 1) / BM), (unsigned)z);
    void* args[] = {(void*)&d};
    (void)hipLaunchKernel((const void*)k, grid, dim3(256), args, 0, st);
    return PP_OK;
}

// The plan's launches (a tail split: the head on the plan's tile, then the tail on 128x128); PP_OK or the first error
static int gemm_launch(const GemmPlan& p, const GemmView& v, int cus, hipStream_t st) {
    auto one = [&](const PpGemmDesc& d, int tile) {
        switch (p.engine) {
            case GE_U: return (v.terms == 2 ? pp_gemm_u_launch_t2 : pp_gemm_u_launch_t1)(d, tile, p.amode, p.vec, cus, st);
            case GE_UH: return pp_gemm_uh_launch(d, v.terms, cus, st);
            case GE_F: return pp_gemm_f_launch(d, tile, p.amode - 16, cus, st);
            default: return gemm_r1_launch(p, d, v.z, st);
        }
    };
    if (p.tail_rows == 0) return one(v.d, p.tile);
    auto rows = [&](int r0, int m) {   // rows [r0, r0 + m) of the dense launch as a launch of its own
        PpGemmDesc t = v.d;
        t.M = m;
        const size_t eb = v.terms == 1 ? 2 : 4;
        if (t.A_hl) t.A_hl = (const char*)t.A_hl + (size_t)r0 * t.lda * eb;
        if (t.A) t.A += (size_t)r0 * t.lda;
        if (t.C) t.C += (size_t)r0 * t.ldc;
        if (t.C_hl) t.C_hl = (char*)t.C_hl + (size_t)r0 * t.ldc_h * eb;
        if (t.residual) t.residual += (size_t)r0 * t.ldc;
        if (t.residual2) t.residual2 += (size_t)r0 * t.ldc;
        pp_gemm_extents(t, (int)eb, t.a_hl_bytes, t.b_hl_bytes);
        return t;
    };
    const int rc = one(rows(0, p.tail_rows), p.tile);
    return rc != PP_OK ? rc : one(rows(p.tail_rows, v.d.M - p.tail_rows), PP_U_128x128);
}

// The configurations the autotuner times for a launch view, in the order it times them, into c[]; returns their count (<= 12).
static int tune_candidates(const GemmView& v, int cus, int* c) {
    static const int tail_env = [] { const char* e = getenv("PP_GEMM_TAIL_SPLIT"); return e ? (e[0] == '1' ? 1 : 0) : -1; }();
    const PpGemmDesc& d = v.d;
    // tail-split candidates: pre-split engine opt-in (PP_GEMM_TAIL_SPLIT=1: measured neutral on the f16x3 step), fp32 engine on unless
    // PP_GEMM_TAIL_SPLIT=0 (fc1 at M = 49 344: 7.18 -> 7.06 ms per burst; exact-mode step +0.5 %) — profiles/r06/README.md
    const bool tail_on = tail_env == 1, tail_on_f = tail_env != 0;
    const long long t4 = (long long)((d.M + 255) / 256) * ((d.N + 127) / 128), t5 = (long long)((d.M + 255) / 256) * ((d.N + 255) / 256);
    int n = 0;
    if (v.asplit) {
        // the 128-row tiles always; the 256-row ones for problems that give at least half the chip a tile of theirs
        c[n++] = 0;
        c[n++] = 2;
        if (t4 >= cus / 2) c[n++] = 4;
        if (t5 >= cus / 2 && d.N > 128) c[n++] = 5;
        if (t5 >= cus / 2 && d.N > 128 && v.h_shape) c[n++] = 6;
        // 256x192: the last 256-wide tile column would be more than a quarter empty (N = 192: corr_net[1] of the flow decoder)
        static const bool tile192 = [] { const char* e = getenv("PP_GEMM_TILE_192"); return !(e && e[0] == '0'); }();   // (A/B switch)
        if (tile192 && d.N % 256 > 128 && d.N % 256 <= 192 && v.u_vec && (long long)((d.M + 255) / 256) * ((d.N + 191) / 192) >= cus / 2) c[n++] = 11;
        if (tail_on && d.N > 128 && tail_rows(v, 256, cus)) c[n++] = 9;
        if (tail_on && tail_rows(v, 128, cus)) c[n++] = 10;
    } else if (v.fvec) {
        c[n++] = 6;
        if (d.N > 64) c[n++] = 3;
        if (t4 >= cus / 2 && d.N > 64) c[n++] = 4;
        if (t5 >= cus / 2 && d.N > 128) c[n++] = 5;
        // 256x192: layers whose N wastes less of a 192-wide tile than of a 128-wide one (the decoder's 192-channel maps)
        if ((d.N + 191) / 192 * 192 - d.N < (d.N + 127) / 128 * 128 - d.N && (long long)((d.M + 255) / 256) * ((d.N + 191) / 192) >= cus / 2) c[n++] = 7;
        if (tail_on_f && d.N > 128 && tail_rows(v, 256, cus)) c[n++] = 9;
        if (tail_on_f && d.N > 64 && tail_rows(v, 128, cus)) c[n++] = 10;
    } else {
        for (int i = 0; i < (v.vec ? 3 : 2); ++i) c[n++] = v.vec ? i : (i == 0 ? 0 : 2);
    }
    return n;
}

// The fastest of the candidates on this call's own launch (timed launches of the same GEMM — idempotent unless the output aliases a
// residual, which the caller excludes).  Round-robin: every round times one burst of four back-to-back launches of EACH candidate, and a
// candidate keeps its best burst.  (Timing the candidates one after the other ranked them by the clock the chip happened to hold: the
// first ones ran on a cool chip, and configurations within ~5-10 % changed places from run to run.)  The winner goes into the table
// under `key` and is launched once more, so that the call leaves its result; a call that tunes records nothing.
static int gemm_tune(const GemmView& v, const char* key, int cus, hipStream_t st) {
    static const bool dbg = getenv("PP_GEMM_DEBUG") != nullptr;
    hipEvent_t e0, e1;
    PP_CHECK_HIP(hipEventCreate(&e0));
    PP_CHECK_HIP(hipEventCreate(&e1));
    int cands[12];
    const int nc = tune_candidates(v, cus, cands);
    GemmPlan plans[12];
    float ms[12];
    for (int i = 0; i < nc; ++i) {
        plans[i] = gemm_plan(v, cands[i], cus);
        ms[i] = 1e30f;
        (void)gemm_launch(plans[i], v, cus, st);  // warm
    }
    for (int rep = 0; rep < 4; ++rep)
        for (int i = 0; i < nc; ++i) {
            (void)hipEventRecord(e0, st);
            for (int k = 0; k < 4; ++k) (void)gemm_launch(plans[i], v, cus, st);
            (void)hipEventRecord(e1, st);
            (void)hipEventSynchronize(e1);
            float t = 0.f;
            (void)hipEventElapsedTime(&t, e0, e1);
            ms[i] = t < ms[i] ? t : ms[i];
        }
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    int best = 0;
    for (int i = 0; i < nc; ++i) {
        if (dbg) fprintf(stderr, "[pp_gemm] autotune %s cfg %d: %.4f ms\n", key, cands[i], ms[i]);
        if (ms[i] < ms[best]) best = i;
    }
    g_tune_best[key] = cands[best];
    const int rc = gemm_launch(plans[best], v, cus, st);
    return rc != PP_OK ? rc : pp_last_launch();
}

extern "C" {

int pp_gemm_generic_epilogue(int on) {
    if (on != 0 && on != 1) return PP_EINVAL;
    return g_epi_generic.exchange(on);
}

int pp_gemm(const PpGemmDesc* desc, void* stream) {
    GemmView v;
    if (const int rc = gemm_normalise(desc, v); rc != PP_OK) return rc;
    const PpGemmDesc& d = v.d;
    hipStream_t st = (hipStream_t)stream;
    const int cus = pp_cu_count();   // cached per device (two runtime calls per GEMM launch otherwise)
    // Which block tile / occupancy is fastest depends on how the tile count fills the CUs (wave quantisation)
    // and on K; it is measured once per problem shape (gemm_tune) and remembered.  PP_GEMM_AUTOTUNE=0 keeps the static choice.
    int cfg = v.fvec ? (d.N <= 64 ? 6 : 3) : (d.N <= 64 ? 2 : 0);
    bool pinned = false;
    if (const char* f = getenv("PP_GEMM_FORCE_CFG")) {  // tests: pin one kernel configuration (recorded like any other launch)
        const int fc = atoi(f);
        if (((fc == 9 || fc == 10) && (v.asplit || v.fvec)) || (fc == 11 && v.asplit) || (fc >= 0 && fc <= 8 && (v.asplit || fc <= 2 || (v.fvec && fc <= 7)))) {
            cfg = fc;
            pinned = true;
        }
    }
    const bool alias = d.C != nullptr && (d.residual == d.C || d.residual2 == d.C);  // (C is null for operand-only outputs)
    static const bool tune = [] { const char* e = getenv("PP_GEMM_AUTOTUNE"); return !(e && e[0] == '0'); }();
    if (!pinned && tune && !alias && (d.N > 64 || v.fvec)) {
        [[maybe_unused]] static const bool env_loaded = [] {
            if (const char* p = getenv("PP_GEMM_TUNE_FILE")) {
                std::lock_guard<std::mutex> lock(g_tune_mu);
                (void)tune_load_locked(p);
            }
            return true;
        }();
        char key[160];
        snprintf(key, sizeof key, "%d.%d.%d.%d.%d.%lld.%d.%d.%d.%d.%d.%d", d.M, d.N, d.K, (int)v.vec, d.b_kn, v.z, d.conv_kh,
                 d.conv_cin, d.conv_stride, d.conv_h, d.shuffle_r,
                 (int)v.split + 2 * (d.B_hl != nullptr) + 4 * (int)v.asplit + 8 * (int)(v.terms == 1) + 16 * (int)v.fvec);
        std::lock_guard<std::mutex> lock(g_tune_mu);
        auto it = g_tune_best.find(key);
        if (it == g_tune_best.end()) return gemm_tune(v, key, cus, st);
        cfg = it->second;
    }
    const GemmPlan p = gemm_plan(v, cfg, cus);
    PpGemmProf* gp = pp_gemm_prof_state();
    const bool rec = gp->capacity > 0 && gp->count < gp->capacity;
    if (rec) (void)hipEventRecord(gp->ev[2 * gp->count], st);
    const int rc = gemm_launch(p, v, cus, st);
    if (rec) {
        (void)hipEventRecord(gp->ev[2 * gp->count + 1], st);
        gp->flops[gp->count] = 2.0 * d.M * d.N * d.K * (double)v.z;
        // algorithmic bytes: every operand and result element once, in the format this launch reads / writes it
        const double eb = 2.0 * v.terms, ea = v.asplit ? eb : 4.0, ew = (v.asplit || d.B_hl) ? eb : 4.0;
        const long long per = (long long)d.conv_ho * d.conv_wo;
        const double a_el = d.conv_kh != 0 ? (double)((d.M + per - 1) / per) * d.conv_h * d.conv_w * d.conv_cin   // the image, not its im2col
                                           : (double)d.M * d.K;
        const double mn = (double)d.M * d.N;
        gp->bytes[gp->count] = (double)v.z * (a_el * ea + (double)d.N * d.K * ew * (d.grp_rows ? d.M / d.grp_rows : 1) + (d.C ? mn * 4.0 : 0.0) +
                                              (d.C_hl ? mn * eb : 0.0) + (d.residual ? mn * 4.0 : 0.0) + (d.residual2 ? mn * 4.0 : 0.0));
        // (pp_prof_gemm_collect: two classes; the fp32 engine is told apart by its mode field, 16 + MODE)
        gp->kind[gp->count] = p.engine == GE_U || p.engine == GE_UH ? 0 : 1;
        // (a tail split is recorded under its big tile; the tail's share of the time rides along)
        int* sh = gp->shape[gp->count];
        sh[0] = d.M, sh[1] = d.N, sh[2] = d.K, sh[3] = d.conv_kh, sh[4] = p.cfg, sh[5] = p.amode;
        gp->count++;
    }
    return rc != PP_OK ? rc : pp_last_launch();
}

int pp_gemm_tune_save(const char* path) {
    if (!path) return PP_EINVAL;
    std::lock_guard<std::mutex> lock(g_tune_mu);
    FILE* f = fopen(path, "w");
    if (!f) return PP_EINVAL;
    for (const auto& kv : g_tune_best) fprintf(f, "%s %d\n", kv.first.c_str(), kv.second);
    fclose(f);
    return (int)g_tune_best.size();
}

int pp_gemm_tune_load(const char* path) {
    if (!path) return PP_EINVAL;
    std::lock_guard<std::mutex> lock(g_tune_mu);
    const int n = tune_load_locked(path);
    return n < 0 ? PP_EINVAL : n;
}

int pp_gemm_tune_entries(void) {
    std::lock_guard<std::mutex> lock(g_tune_mu);
    return (int)g_tune_best.size();
}

int pp_layernorm(const float* x, const float* gamma, const float* beta, int rows, int C, float eps, float* y,
                 void* stream) {
    if (!x || !gamma || !beta || !y || rows <= 0 || C <= 0) return PP_EINVAL;
    launch_layernorm(x, gamma, beta, rows, C, eps, y, nullptr, (hipStream_t)stream);
    return pp_last_launch();
}

int pp_layernorm_t(const float* x, const float* gamma, const float* beta, int rows, int C, float eps, float* y,
                   void* hl, int terms, void* stream) {
    if (!x || !gamma || !beta || !hl || rows <= 0 || C <= 0 || C % 8 != 0 || (terms != 1 && terms != 2)) return PP_EINVAL;
    launch_layernorm(x, gamma, beta, rows, C, eps, y, (_Float16*)hl, (hipStream_t)stream, terms);
    return pp_last_launch();
}

int pp_layernorm_split(const float* x, const float* gamma, const float* beta, int rows, int C, float eps, float* y,
                       void* hl, void* stream) {
    return pp_layernorm_t(x, gamma, beta, rows, C, eps, y, hl, 2, stream);
}

int pp_softmax_rows(float* x, int rows, int n, int ld, void* stream) {
    if (!x || rows <= 0 || n <= 0 || ld < n) return PP_EINVAL;
    hipLaunchKernelGGL(softmax_kernel, dim3((rows + 3) / 4), dim3(256), 0, (hipStream_t)stream, x, rows, n, ld);
    return pp_last_launch();
}

int pp_groupnorm_nhwc(const float* x, const float* gamma, const float* beta, int B, int HW, int C, int groups,
                      float eps, int relu, float* y, void* stream) {
    if (!x || !gamma || !beta || !y || B <= 0 || HW <= 0 || C <= 0 || groups <= 0 || C % groups != 0)
        return PP_EINVAL;
    hipLaunchKernelGGL(groupnorm_kernel, dim3(B * groups), dim3(256), 0, (hipStream_t)stream, x, gamma, beta, HW,
                       C, groups, eps, relu, y);
    return pp_last_launch();
}

int pp_transpose_batched(const float* in, long long in_batch_stride, int B, int R, int C, float* out,
                         long long out_batch_stride, int ld_out, int col_off, void* stream) {
    if (!in || !out || B <= 0 || R <= 0 || C <= 0 || ld_out < R + col_off || col_off < 0) return PP_EINVAL;
    if (in_batch_stride == 0) in_batch_stride = (long long)R * C;
    if (out_batch_stride == 0) out_batch_stride = (long long)C * ld_out;
    hipLaunchKernelGGL(transpose_kernel, dim3((C + 31) / 32, (R + 31) / 32, B), dim3(256), 0,
                       (hipStream_t)stream, in, in_batch_stride, R, C, out, out_batch_stride, ld_out, col_off);
    return pp_last_launch();
}

int pp_assemble_tokens(const float* patches, const float* cls_token, const float* pos, int B, int T, int C,
                       float* tokens, void* stream) {
    if (!patches || !cls_token || !pos || !tokens || B <= 0 || T <= 0 || C <= 0) return PP_EINVAL;
    hipLaunchKernelGGL(assemble_tokens_kernel, dim3(T + 1, B), dim3(256), 0, (hipStream_t)stream, patches,
                       cls_token, pos, T, C, tokens);
    return pp_last_launch();
}

int pp_normalize_rows(const float* x, int rows, int n, float eps, float* y, void* stream) {
    if (!x || !y || rows <= 0 || n <= 0 || n > 64) return PP_EINVAL;
    hipLaunchKernelGGL(normalize_rows_kernel, dim3((rows + 255) / 256), dim3(256), 0, (hipStream_t)stream, x,
                       rows, n, eps, y);
    return pp_last_launch();
}

}  // extern "C"
