// The on-demand local correlation lookup of stage 3 (NHWC), which replaces the reference's materialised correlation pyramid:
// CorrelationPyramid + CorrLookup fused — raft_decoder.py:30-53, corr_lookup.py:100-134.  corr_l[p, q] = <f1[p], pool_l(f2)[q]> / sqrt(C);
// for every pixel p and level l the (2r+1)^2 window around (p + flow[p]) / 2^l is bilinearly sampled (zeros padding; the window order
// and the skeleton that the two kernels tiled on the matrix cores share: pp_corr_dev.h).

#include <stdlib.h>
#include <stdint.h>
#include "pp_corr_dev.h"

namespace {

typedef float f4 __attribute__((ext_vector_type(4)));

// One wave per pixel: the (2r+2)^2 integer neighbours per level are dotted by one lane each (C sequential fmas, f1[p] broadcast from LDS),
// then lanes blend the 4 corners.
__global__ __launch_bounds__(256) void corr_lookup_kernel(const float* __restrict__ f1, int ld_f1, int f2_batch, const float* __restrict__ f2l0,
                                                          const float* __restrict__ f2l1, const float* __restrict__ f2l2,
                                                          const float* __restrict__ flow, int H, int W, int C, int L, int r, int ld_flow,
                                                          float inv_sqrt_c, float* __restrict__ out, int ld_out) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    float* a = sm + (size_t)wv * (C + MAXL * TW * TW);  // f1[p] then the corr tables
    float* tab = a + C;
    const int b = blockIdx.y, p = blockIdx.x * 4 + wv;
    const bool live = p < H * W;
    const int y = live ? p / W : 0, x = live ? p - y * W : 0;
    const int tw = 2 * r + 2, win = 2 * r + 1;
    if (live) {
        const float* src = f1 + ((size_t)b * H * W + p) * ld_f1;
        for (int c = lane * 4; c < C; c += 256) *(f4*)(a + c) = *(const f4*)(src + c);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_s_waitcnt(0xC07F);
    __builtin_amdgcn_wave_barrier();
    float cx[MAXL], cy[MAXL];
    int bx[MAXL], by[MAXL];
    if (live) {
        const float* fl = flow + ((size_t)b * H * W + p) * ld_flow;
        const float gx = (float)x + fl[0], gy = (float)y + fl[1];
        for (int l = 0; l < L; ++l) {
            const int Hl = H >> l, Wl = W >> l;
            const float sc = (float)(1 << l);
            // centre sample (offset 0): its integer corner anchors the table, offsets shift by integers
            // (clamped as floats before the integer conversion: a huge / NaN flow is an out-of-image sample, all zeros; the adjoint's rx == ix test rests on THIS clamp)
            cx[l] = fminf(fmaxf(pp_roundtrip(gx / sc, Wl), -(float)(r + 2)), (float)(Wl + r + 1));
            cy[l] = fminf(fmaxf(pp_roundtrip(gy / sc, Hl), -(float)(r + 2)), (float)(Hl + r + 1));
            bx[l] = (int)floorf(cx[l]) - r;
            by[l] = (int)floorf(cy[l]) - r;
        }
        const int npos = L * tw * tw;
        for (int i = lane; i < npos; i += 64) {
            const int l = i / (tw * tw), rem = i - l * tw * tw, dy = rem / tw, dx = rem - dy * tw;
            const int Hl = H >> l, Wl = W >> l;
            const int qx = bx[l] + dx, qy = by[l] + dy;
            float dot = 0.f;
            // positions outside the (pooled) map: the dot product runs on a clamped position and its VALUE is then replaced
            // by zero (one select, no lane-masked branch around the loads — DESIGN section 6)
            const bool inside = qx >= 0 && qx < Wl && qy >= 0 && qy < Hl;
            const int qxc = min(max(qx, 0), Wl - 1), qyc = min(max(qy, 0), Hl - 1);
            const float* f2 = l == 0 ? f2l0 : (l == 1 ? f2l1 : f2l2);
            const float* q = f2 + (((size_t)(b % f2_batch) * Hl + qyc) * Wl + qxc) * C;
            for (int c = 0; c < C; c += 4) {
                const f4 u = *(const f4*)(a + c), v = *(const f4*)(q + c);
                dot = fmaf(u.x, v.x, dot);
                dot = fmaf(u.y, v.y, dot);
                dot = fmaf(u.z, v.z, dot);
                dot = fmaf(u.w, v.w, dot);
            }
            tab[i] = inside ? dot * inv_sqrt_c : 0.f;
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_s_waitcnt(0xC07F);
    __builtin_amdgcn_wave_barrier();
    if (live) {
        float* o = out + ((size_t)b * H * W + p) * ld_out;
        const int nout = L * win * win;
        for (int i = lane; i < nout; i += 64) {
            const int l = i / (win * win), rem = i - l * win * win, ai = rem / win, bi = rem - ai * win;
            const float wx1 = cx[l] - floorf(cx[l]), wy1 = cy[l] - floorf(cy[l]);
            const float wx0 = 1.f - wx1, wy0 = 1.f - wy1;
            // x offset a-r -> dx = ai, y offset b-r -> dy = bi.  A pooled axis of size 1: the reference's round trip multiplies by size - 1 = 0,
            // so every offset along it samples coordinate 0 — all of them read the column (row) of offset 0 (c = 0 there: weights 1 and 0)
            const int di = (W >> l) == 1 ? r : ai, dj = (H >> l) == 1 ? r : bi;
            const float* t = tab + l * tw * tw + dj * tw + di;
            o[i] = t[0] * (wx0 * wy0) + t[1] * (wx1 * wy0) + t[tw] * (wx0 * wy1) + t[tw + 1] * (wx1 * wy1);
        }
        for (int i = nout + lane; i < ld_out; i += 64) o[i] = 0.f;   // the pad channels of the row (the caller allocates without a fill)
    }
}

// ---- the same lookup, tiled on the matrix cores --------------------------------------------------------------
// With one lane per neighbour position the kernel above streams 108 separate 1 KB rows of f2 per pixel through the
// texture path (64 distinct cache lines per load instruction): 9.4 ms per step once the flows are realistic.  Here a
// workgroup takes an 8 x 8 tile of source pixels.  Their targets lie close together (a flow field is smooth), so the
// 6 x 6 neighbourhoods of all 64 pixels fall into one 16 x 16 REGION of the (pooled) f2 map: the workgroup computes the
// local correlation S[64 pixels][256 region positions] = F1_tile . F2_region^T on the matrix cores — in the engine's
// f16x3 arithmetic: every fp32 value is split into two fp16 terms as it is staged into LDS (hi = f16(4x), lo = f16(4x -
// hi)) and a product is hi.hi + hi.lo + lo.hi on v_mfma_f32_32x32x16_f16 with fp32 accumulation (22 operand bits; 5x
// the rate of the fp32 MFMA, which made this kernel matrix-bound).  K = C in chunks of 32 channels, coalesced 128-byte
// row segments.  S stays in LDS, and every pixel then blends its 25 bilinear samples per level out of S.  Pixels whose
// neighbourhood does not fit the region are served by further passes with a new region (smooth flows need one pass).
// f2 rows outside the image enter as zero rows (grid_sample's zeros padding).
constexpr int CRW = 16, CN = CRW * CRW;   // region of f2 positions
constexpr int CK = 32, CKP = CK + 4;      // channels per chunk; LDS row = 32 hi + 32 lo halfs + pad = 36 dwords (144 B: conflict-free b128 reads)
constexpr int CSP = CN + 4;               // row pitch of S
typedef _Float16 h8_t __attribute__((ext_vector_type(8)));
typedef _Float16 h4_t __attribute__((ext_vector_type(4)));
typedef float f32x16_t __attribute__((ext_vector_type(16)));

// HLIN: f1 / f2 arrive as the engine's hl operand (fp16 [rows][2 ld]: per 8 channels 8 hi then 8 lo terms — what the
// producing convolution's epilogue writes): staging is 16-byte copies, no split arithmetic (it was as long as the MFMAs of a
// chunk).  Same bits either way: the split of a value does not depend on who performs it.
// EXACT (fp32 input only; ops.PRECISION = "f32" / bench.py --mode exact): the chunk is staged as fp32 (a 128-byte row is 32 floats
// instead of 32 hi + 32 lo halfs) and S is accumulated by v_mfma_f32_32x32x2_f32 — exact fp32 products, a k-ordered fma chain per
// entry like the lane-per-position kernel's, 5.3 x the matrix time of the f16x3 form but a third less than that kernel's 108 row
// streams per pixel (9.6 -> measured below, profiles/r05/exact).
// ONE (fp32 input only; ops.PRECISION = "f16" / bench.py --mode fp16): plain fp16 operands — a value is staged as its hi term alone and a
// product is ONE MFMA (the arithmetic of that mode's convolutions: 11 operand bits, fp32 accumulation); a third of the matrix work.
template <bool HLIN, bool EXACT = false, bool ONE = false>
__global__ __launch_bounds__(256, 2) void corr_lookup_mfma_kernel(const void* __restrict__ f1v, int ld_f1, int f2_batch,
                                                                  const void* __restrict__ f2l0, const void* __restrict__ f2l1,
                                                                  const void* __restrict__ f2l2, const float* __restrict__ flow,
                                                                  int B, int H, int W, int C, int L, int r, int ld_flow,
                                                                  float inv_sqrt_c, float* __restrict__ out, int ld_out,
                                                                  _Float16* __restrict__ out_hl) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    float* As = sm;                        // [CM][CKP]
    float* Bs = sm + CM * CKP;             // [CN][CKP]
    float* S = sm;                         // [CM][CSP], aliases As/Bs once the K loop is over
    __shared__ corr_tile_t ts;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, l31 = lane & 31, lh = lane >> 5;
    const int fit = CRW - (2 * r + 2);
    float gx, gy;
    const corr_dst_t d = corr_tile_begin(B, H, W, flow, ld_flow, out, out_hl, ld_out, L, r, gx, gy);
    for (int l = 0; l < L; ++l) {
        const int Hl = H >> l, Wl = W >> l;
        const void* f2v = l == 0 ? f2l0 : (l == 1 ? f2l1 : f2l2);
        const float* f2 = (const float*)f2v + (size_t)(d.b % f2_batch) * Hl * Wl * C;                 // fp32 input
        const _Float16* f2h = (const _Float16*)f2v + (size_t)(d.b % f2_batch) * Hl * Wl * C * 2;      // hl input
        const float* f1 = (const float*)f1v;
        const _Float16* f1h = (const _Float16*)f1v;
        corr_level_begin(ts, d, l, Hl, Wl, gx, gy, r);
        while (ts.todo > 0) {                               // (uniform: read after a barrier, written before the next)
            const int2 org = corr_pass_origin(ts, fit);
            const int ox = org.x, oy = org.y;
            // ---- S = F1_tile . F2_region^T
            f32x16_t acc[2][2];
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
            // Two chunks of register prefetch: chunk kc + 2 is requested as soon as chunk kc has been stored to LDS, so a load has
            // two chunk periods (MFMAs, fragment reads, two barriers each) to arrive; with one chunk ahead the L2 latency showed.
            f4 ra0[2], rb0[8], ra1[2], rb1[8];   // (HLIN: the 16 bytes are 8 halfs — piece `part` of the row's 128-byte chunk)
            const int part = tid & 7, row0 = tid >> 3;
            auto load_chunk = [&](int kc, f4 (&ra)[2], f4 (&rb)[8]) __attribute__((always_inline)) {
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    const size_t px = corr_row(d, row0 + 32 * i);
                    ra[i] = HLIN ? *(const f4*)(f1h + (px * ld_f1 + kc * CK) * 2 + 8 * part) : *(const f4*)(f1 + px * ld_f1 + kc * CK + 4 * part);
                }
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const int n = row0 + 32 * i, qy = oy + (n >> 4), qx = ox + (n & 15);
                    const bool in = qx >= 0 && qx < Wl && qy >= 0 && qy < Hl;
                    const size_t px = (size_t)qy * Wl + qx;
                    rb[i] = !in ? f4{0.f, 0.f, 0.f, 0.f}
                                : (HLIN ? *(const f4*)(f2h + (px * C + kc * CK) * 2 + 8 * part) : *(const f4*)(f2 + px * C + kc * CK + 4 * part));
                }
            };
            // LDS rows hold the chunk in hl order: per 8 channels 8 hi then 8 lo halfs (fp32 input: split here)
            auto put = [&](float* rowp, f4 v) __attribute__((always_inline)) {
                if (EXACT) {
                    *(f4*)(rowp + 4 * part) = v;
                    return;
                }
                if (HLIN) {
                    *(f4*)((_Float16*)rowp + 8 * part) = v;
                    return;
                }
                // (staging into LDS, not an operand buffer: the same maps' saturation is reported by the epilogue that wrote their operand form)
                _Float16* g8 = (_Float16*)rowp + 16 * (part >> 1) + 4 * (part & 1);   // channels 4 part .. + 3 of group part / 2
                if (ONE) {   // the hi plane alone (the lo plane of the row is never read)
                    const h4_t hi = {pp_to_f16(v.x), pp_to_f16(v.y), pp_to_f16(v.z), pp_to_f16(v.w)};
                    *(h4_t*)g8 = hi;
                    return;
                }
                _Float16 h0, h1, h2, h3, l0, l1, l2, l3;
                pp_split_f16(v.x, h0, l0);
                pp_split_f16(v.y, h1, l1);
                pp_split_f16(v.z, h2, l2);
                pp_split_f16(v.w, h3, l3);
                const h4_t hi = {h0, h1, h2, h3}, lo = {l0, l1, l2, l3};
                *(h4_t*)g8 = hi;
                *(h4_t*)(g8 + 8) = lo;
            };
#ifdef PP_STUDY_CORR_NK1   // (timing-only study build: one channel chunk instead of C / 32 — sizes the K loop's share)
            const int nk = 1;
#else
            const int nk = C / CK;
#endif
            auto chunk = [&](int kc, f4 (&ra)[2], f4 (&rb)[8]) __attribute__((always_inline)) {
                __syncthreads();                            // the previous chunk (or the previous pass's S) has been read
#pragma unroll
                for (int i = 0; i < 2; ++i) put(As + (row0 + 32 * i) * CKP, ra[i]);
#pragma unroll
                for (int i = 0; i < 8; ++i) put(Bs + (row0 + 32 * i) * CKP, rb[i]);
                __syncthreads();
                if (kc + 2 < nk) load_chunk(kc + 2, ra, rb);    // in flight under two chunks of MFMAs
                if constexpr (EXACT) {
                    // lane (l31, lh) feeds row / column l31 with channels 16 lh + 4 q .. + 3: MFMA e of quad q multiplies the pair
                    // (4 q + e, 16 + 4 q + e) — the order of the fp32 engine (csrc/pp_gemm_f.hip)
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        f4 af[2], bf[2];
#pragma unroll
                        for (int i = 0; i < 2; ++i) {
                            af[i] = *(const f4*)(As + (i * 32 + l31) * CKP + 16 * lh + 4 * q);
                            bf[i] = *(const f4*)(Bs + (wv * 64 + i * 32 + l31) * CKP + 16 * lh + 4 * q);
                        }
#pragma unroll
                        for (int e = 0; e < 4; ++e)
#pragma unroll
                            for (int i = 0; i < 2; ++i)
#pragma unroll
                                for (int j = 0; j < 2; ++j)
                                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i][e], bf[j][e], acc[i][j], 0, 0, 0);
                    }
                    return;
                }
                // lane (l31, lh) feeds row / column l31 with channels 16 q + 8 lh .. + 7 of the chunk in k-step q
#pragma unroll
                for (int q = 0; q < 2; ++q) {
                    h8_t ah[2], al[2], bh[2], bl[2];
#pragma unroll
                    for (int i = 0; i < 2; ++i) {
                        const _Float16* ar = (const _Float16*)(As + (i * 32 + l31) * CKP) + 16 * (2 * q + lh);
                        const _Float16* br = (const _Float16*)(Bs + (wv * 64 + i * 32 + l31) * CKP) + 16 * (2 * q + lh);
                        ah[i] = *(const h8_t*)ar;
                        bh[i] = *(const h8_t*)br;
                        if (!ONE) {
                            al[i] = *(const h8_t*)(ar + 8);
                            bl[i] = *(const h8_t*)(br + 8);
                        }
                    }
#pragma unroll
                    for (int i = 0; i < 2; ++i)
#pragma unroll
                        for (int j = 0; j < 2; ++j) {
                            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[i], bh[j], acc[i][j], 0, 0, 0);
                            if (!ONE) {
                                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[i], bl[j], acc[i][j], 0, 0, 0);
                                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al[i], bh[j], acc[i][j], 0, 0, 0);
                            }
                        }
                }
            };
            load_chunk(0, ra0, rb0);
            if (nk > 1) load_chunk(1, ra1, rb1);
            for (int kc = 0; kc < nk; kc += 2) {
                chunk(kc, ra0, rb0);
                if (kc + 1 < nk) chunk(kc + 1, ra1, rb1);
            }
            __syncthreads();                                // every wave is done reading As/Bs: S may overwrite them
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int e = 0; e < 16; ++e)            // accumulator (e, lane): row (e/4)*8 + lh*4 + e%4, column l31
                        S[(i * 32 + (e >> 2) * 8 + lh * 4 + (e & 3)) * CSP + wv * 64 + j * 32 + l31] =
                            acc[i][j][e] * (EXACT ? inv_sqrt_c : inv_sqrt_c / (PP_A_SCALE * PP_A_SCALE));
            __syncthreads();
            corr_blend<CRW>(ts, d, S, CSP, 0, CM, ox, oy, l, r);
            corr_pass_retire(ts, fit, ox, oy);
        }
        __syncthreads();
    }
}

// ---- the operand-input lookup again: a region per pyramid level, chunks staged by LDS-DMA into a ring ------------------------------
// The skeleton and the arithmetic of corr_lookup_mfma_kernel<true> (an entry of S is accumulated over the channels in ascending order,
// per 16 channels hi.hi, hi.lo, lo.hi; it does not depend on the region or the pass that produced it: the same bits), but
//   * every level has its own compile-time region: 16 x 16 at level 0 as before; the footprint of an 8 x 8 tile shrinks to 4 + 6 positions
//     at the once-pooled level and 2 + 6 at the twice-pooled one, and both take 11 x 11 (slack for flow divergence inside the tile: 2 and
//     12 source pixels, against 3 at level 0; one pass per tile on the benchmark's flows down to 10 x 10, profiles/r13) — 128 columns of S
//     instead of 256, half the rows fetched and multiplied;
//   * a K step is 16 channels, one 64-byte segment per row, moved global -> LDS by LDS-DMA (pp_gemm_u_kernel.h): no staging registers,
//     no ds_write.  A wave instruction fills 16 rows; the 16-byte chunk c of row r sits at position c ^ (r >> 2 & 3) — conflict-free
//     ds_read_b128 for the 32x32x16 fragment pattern (lane l: row l & 31, chunk 2 (l >> 5) + term) — applied to the per-lane SOURCE
//     address.  Ring of two stages, one wait and one barrier per step;
//   * S holds one half of the tile's pixels at a time (32 rows: 33 KB), so ring and S fit in 40 KB and THREE workgroups share a CU: the
//     kernel is bound by its serial phases (setup, barriers, the blend), not by the matrix cores or the staging — with one workgroup per CU
//     and a deep ring it took 2.2 ms where two take 1.27 and three 1.04 (profiles/r13/corr_lookup.md);
//   * region rows outside the image, rows past the level's region and steps past the K loop are out-of-range buffer offsets: the DMA
//     writes zeros, no traffic, no branch, no lane mask held across a load.
constexpr int RK = 16, RROW = 2 * RK;      // channels per K step; halfs per staged row
constexpr int RP = 512 / RROW, LPR = 64 / RP;   // rows per DMA piece (1 KB per wave instruction); lanes per row
constexpr int RST = 2;                     // ring stages
// region edge and staged region rows (whole DMA pieces for each of the 4 waves: a multiple of 64) per pyramid level
constexpr int RG0_W = 16, RG0_N = 256, RG1_W = 11, RG1_N = 128, RG2_W = 11, RG2_N = 128;
constexpr int corr_ring_nb(int rw) { return (rw * rw + 31) / 32; }      // 32-column blocks of S that hold region positions
constexpr size_t corr_ring_bytes(int rw, int nrp) {
    const size_t ring = (size_t)RST * (CM + nrp) * RROW * 2, s = (size_t)(CM / 2) * (corr_ring_nb(rw) * 32 + 4) * 4;
    return ring > s ? ring : s;
}
constexpr size_t CORR_RING_LDS = corr_ring_bytes(RG0_W, RG0_N);
static_assert(corr_ring_bytes(RG1_W, RG1_N) <= CORR_RING_LDS && corr_ring_bytes(RG2_W, RG2_N) <= CORR_RING_LDS, "level 0 sizes the LDS");
static_assert(corr_ring_nb(RG0_W) * 32 <= RG0_N && corr_ring_nb(RG1_W) * 32 <= RG1_N && corr_ring_nb(RG2_W) * 32 <= RG2_N, "S columns are staged rows");
static_assert(RG0_N % (4 * RP) == 0 && RG1_N % (4 * RP) == 0 && RG2_N % (4 * RP) == 0 && CM % (4 * RP) == 0, "whole DMA pieces per wave");

#if defined(__HIP_DEVICE_COMPILE__)   // (the host pass only needs the launch stub: it cannot instantiate the LDS-DMA builtin)
typedef __attribute__((address_space(3))) void* corr_lds_ptr_t;

// one pyramid level of one tile.  f1b: image b of the render operand; f2v: the level's query operand (images of H >> l x W >> l).
// Every global store of a wave (pad and outside-image zeros, the previous pass's results) drains at the vmcnt(0) before a pass's first
// CORR_RING_ISSUE; from there to the vmcnt(0) after the K loop only the DMA touches global memory: the counted waits count its pieces alone.
template <int RW, int NRP>
__device__ __forceinline__ void corr_ring_level(float* sm, corr_tile_t& ts, const corr_dst_t& d, int l, const _Float16* f1b, int ld_f1,
                                                int f1_bytes, const void* f2v, int f2_batch, int H, int W, int C, float gx, float gy, int r,
                                                float inv_sqrt_c) {
    const int Hl = H >> l, Wl = W >> l;
    const _Float16* f2b = (const _Float16*)f2v + (size_t)(d.b % f2_batch) * Hl * Wl * C * 2;
    constexpr int NB = corr_ring_nb(RW), NT = (2 * NB + 3) / 4;   // column blocks of S; 32 x 32 tiles of S per wave (tile t = wave + 4 i)
    constexpr int PA = CM / RP / 4, PB = NRP / RP / 4, NP = PA + PB;   // DMA pieces per wave and step: tile rows, region rows
    constexpr int STG = (CM + NRP) * RROW;                        // halfs per stage: [64 tile rows | NRP region rows]
    constexpr int SP = NB * 32 + 4;                               // row pitch of S
    _Float16* ring = (_Float16*)sm;
    float* S = sm;                                                // [32][SP]: aliases the ring once the K loop is over
    const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6), l31 = lane & 31, lh = lane >> 5;
    const int fit = RW - (2 * r + 2);
    corr_level_begin(ts, d, l, Hl, Wl, gx, gy, r);
    // DMA slot of this lane: a piece fills 16 rows, lane -> row lane >> 2, chunk position lane & 3, which holds source chunk sc (the key
    // reads bits 2, 3 of the row = of lane >> 2: the same for every piece)
    const int lr = lane / LPR, sc = (lane % LPR) ^ ((lr >> 2) & 3);
    const __amdgpu_buffer_rsrc_t Ar = __builtin_amdgcn_make_buffer_rsrc((void*)f1b, 0, f1_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t Br = __builtin_amdgcn_make_buffer_rsrc((void*)f2b, 0, Hl * Wl * C * 4, 0x00020000);
    unsigned abyte[PA];                                       // tile pixels of this lane's pieces of the render operand
#pragma unroll
    for (int j = 0; j < PA; ++j) {
        const int ma = (j * 4 + wv) * RP + lr;
        abyte[j] = (unsigned)(((d.y0 + (ma >> 3)) * d.W + d.x0 + (ma & 7)) * ld_f1) * 4u + (unsigned)sc * 16u;
    }
    const int ns = C / RK;
    // fragment reads: lane (l31, lh) feeds row / column l31 with channels 8 lh .. + 7 of the step: chunk 2 lh (hi terms), 2 lh + 1 (lo)
    const int ph = ((2 * lh) ^ ((l31 >> 2) & 3)) * 8, pl = ph ^ 8;
    while (ts.todo > 0) {                                   // (uniform: read after a barrier, written before the next)
        const int2 org = corr_pass_origin(ts, fit);
        const int ox = org.x, oy = org.y;
        unsigned bbyte[PB];                                 // region rows of this lane's pieces: byte offset of channel 0 (+ its chunk)
#pragma unroll
        for (int j = 0; j < PB; ++j) {
            const int n = (j * 4 + wv) * RP + lr, ry = n / RW, qy = oy + ry, qx = ox + n - ry * RW;
            const bool in = n < RW * RW && qx >= 0 && qx < Wl && qy >= 0 && qy < Hl;
            bbyte[j] = in ? (unsigned)((qy * Wl + qx) * C) * 4u + (unsigned)sc * 16u : 0xFFFFFFFFu;
        }
        // the pieces of K step STEP into stage STAGE (a macro, not a lambda: pp_gemm_u_kernel.h).  A step past the K loop is all
        // out-of-range offsets, so every wave issues NP pieces per step and the counted wait below holds to the end.
#define CORR_RING_ISSUE(STEP, STAGE)                                                                                                \
        {                                                                                                                               \
            const unsigned dead_ = (STEP) < ns ? 0u : 0xFFFFFFFFu;                                                                      \
            const int so_ = (STEP) * (RK * 4);                                                                                          \
            _Float16* st_ = ring + (STAGE) * STG;                                                                                       \
            _Pragma("unroll") for (int j = 0; j < PA; ++j)                                                                              \
                __builtin_amdgcn_raw_ptr_buffer_load_lds(Ar, (corr_lds_ptr_t)(st_ + (j * 4 + wv) * RP * RROW), 16, abyte[j] | dead_,    \
                                                         so_, 0, 0);                                                                    \
            _Pragma("unroll") for (int j = 0; j < PB; ++j)                                                                              \
                __builtin_amdgcn_raw_ptr_buffer_load_lds(Br, (corr_lds_ptr_t)(st_ + (CM + (j * 4 + wv) * RP) * RROW), 16,               \
                                                         bbyte[j] | dead_, so_, 0, 0);                                                  \
        }
        // ---- S = F1_tile . F2_region^T
        f32x16_t acc[NT];
#pragma unroll
        for (int i = 0; i < NT; ++i)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][e] = 0.f;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");    // this wave's result stores have left: the counted waits count DMA pieces alone
#pragma unroll
        for (int s = 0; s < RST - 1; ++s) CORR_RING_ISSUE(s, s)
        int cur = 0;
        for (int s = 0; s < ns; ++s) {
            asm volatile("s_waitcnt vmcnt(%0)" ::"n"((RST - 2) * NP) : "memory");   // this wave's pieces of step s have landed
            __builtin_amdgcn_s_barrier();                   // ... and everybody's; every wave is done reading the stage of step s - 1
            const int nxt = cur == 0 ? RST - 1 : cur - 1;
            CORR_RING_ISSUE(s + RST - 1, nxt)
            const _Float16* sa = ring + cur * STG;
            const _Float16* sb = sa + CM * RROW;
#pragma unroll
            for (int i = 0; i < NT; ++i) {
                const int t = wv + 4 * i;
                if ((2 * NB) % 4 == 0 || t < 2 * NB) {      // (wave-uniform)
                    const int m = t / NB, n = t - m * NB;
                    const _Float16* ar = sa + (m * 32 + l31) * RROW;
                    const _Float16* br = sb + (n * 32 + l31) * RROW;
                    const h8_t ah = *(const h8_t*)(ar + ph), al = *(const h8_t*)(ar + pl);
                    const h8_t bh = *(const h8_t*)(br + ph), bl = *(const h8_t*)(br + pl);
                    acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bh, acc[i], 0, 0, 0);
                    acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bl, acc[i], 0, 0, 0);
                    acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, bh, acc[i], 0, 0, 0);
                }
            }
            cur = cur == RST - 1 ? 0 : cur + 1;
        }
#undef CORR_RING_ISSUE
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");    // the zero pieces past the loop have landed too: S overwrites the ring
        __syncthreads();                                    // every wave is done reading the ring
        // S holds one half of the tile's pixels (a 32-row block of the accumulators) at a time
        for (int half = 0; half < 2; ++half) {
            if (half) __syncthreads();                      // the first half's samples have been read
#pragma unroll
            for (int i = 0; i < NT; ++i) {
                const int t = wv + 4 * i;
                if (((2 * NB) % 4 == 0 || t < 2 * NB) && t / NB == half) {
                    const int n = t - half * NB;
#pragma unroll
                    for (int e = 0; e < 16; ++e)            // accumulator (e, lane): row (e/4)*8 + lh*4 + e%4 of the half, column l31
                        S[((e >> 2) * 8 + lh * 4 + (e & 3)) * SP + n * 32 + l31] =
                            acc[i][e] * (inv_sqrt_c / (PP_A_SCALE * PP_A_SCALE));
                }
            }
            __syncthreads();
            corr_blend<RW>(ts, d, S, SP, 32 * half, CM / 2, ox, oy, l, r);
        }
        corr_pass_retire(ts, fit, ox, oy);
    }
    __syncthreads();
}
#endif

__global__ __launch_bounds__(256, 3) void corr_lookup_ring_kernel(const void* __restrict__ f1v, int ld_f1, int f2_batch,
                                                                  const void* __restrict__ f2l0, const void* __restrict__ f2l1,
                                                                  const void* __restrict__ f2l2, const float* __restrict__ flow, int B,
                                                                  int H, int W, int C, int L, int r, int ld_flow, float inv_sqrt_c,
                                                                  float* __restrict__ out, int ld_out, _Float16* __restrict__ out_hl) {
#if defined(__HIP_DEVICE_COMPILE__)
    extern __shared__ __attribute__((aligned(16))) float sm[];
    __shared__ corr_tile_t ts;
    float gx, gy;
    const corr_dst_t d = corr_tile_begin(B, H, W, flow, ld_flow, out, out_hl, ld_out, L, r, gx, gy);
    const _Float16* f1b = (const _Float16*)f1v + d.row0 * ld_f1 * 2;
    const int f1_bytes = ((H * W - 1) * ld_f1 + C) * 4;
    corr_ring_level<RG0_W, RG0_N>(sm, ts, d, 0, f1b, ld_f1, f1_bytes, f2l0, f2_batch, H, W, C, gx, gy, r, inv_sqrt_c);
    if (L > 1) corr_ring_level<RG1_W, RG1_N>(sm, ts, d, 1, f1b, ld_f1, f1_bytes, f2l1, f2_batch, H, W, C, gx, gy, r, inv_sqrt_c);
    if (L > 2) corr_ring_level<RG2_W, RG2_N>(sm, ts, d, 2, f1b, ld_f1, f1_bytes, f2l2, f2_batch, H, W, C, gx, gy, r, inv_sqrt_c);
#endif
}

}  // namespace

PP_SAT_SETTER(pp_sat_set_corr)

// one workgroup per 8 x 8 pixel tile: the variants of the register-staged kernel and the ring kernel take the same arguments
static int corr_tiled_launch(bool hl, const void* f1, int ld_f1, const void* f2_l0, const void* f2_l1, const void* f2_l2, int f2_batch,
                             const float* flow, int B, int H, int W, int C, int levels, int radius, int ld_flow, float* out, int ld_out,
                             void* stream, bool exact = false, bool one = false, void* out_hl = nullptr) {
    constexpr size_t lds = (size_t)(CM * CSP > (CM + CN) * CKP ? CM * CSP : (CM + CN) * CKP) * sizeof(float);
    enum { FP32, EXACT, ONE, HL, RING };   // the order of the table
    static const struct { decltype(&corr_lookup_ring_kernel) kernel; size_t bytes; } variants[] = {
        {corr_lookup_mfma_kernel<false>, lds}, {corr_lookup_mfma_kernel<false, true>, lds}, {corr_lookup_mfma_kernel<false, false, true>, lds},
        {corr_lookup_mfma_kernel<true>, lds}, {corr_lookup_ring_kernel, CORR_RING_LDS}};
    static signed char attr[PP_MAX_DEVICES];
    signed char& ok = attr[pp_cur_device()];
    if (ok == 0) {
        ok = 1;
        for (const auto& v : variants)
            if (hipFuncSetAttribute((const void*)v.kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)v.bytes) != hipSuccess) ok = -1;
    }
    if (ok < 0) return PP_ELAUNCH;
    // operand input: the ring-staged kernel (PP_CORR_RING=0, read per call, keeps the register-staged one: the tests run both in one process).
    // Its DMA offsets are 32-bit and signed on the way: an image of either operand beyond 2 GiB stays with the register-staged kernel.
    const char* re = getenv("PP_CORR_RING");
    const bool ring = hl && !(re && re[0] == '0') && (long long)H * W * ld_f1 * 4 < 0x7FFFFFFFLL && (long long)H * W * C * 4 < 0x7FFFFFFFLL;
    const auto& v = variants[ring ? RING : exact ? EXACT : one ? ONE : hl ? HL : FP32];
    hipLaunchKernelGGL(v.kernel, dim3((unsigned)((H / CT) * (W / CT) * B)), dim3(256), v.bytes, (hipStream_t)stream, f1, ld_f1, f2_batch, f2_l0,
                       f2_l1, f2_l2, flow, B, H, W, C, levels, radius, ld_flow, 1.0f / sqrtf((float)C), out, ld_out, (_Float16*)out_hl);
    return pp_last_launch();
}

extern "C" {

int pp_corr_lookup_nhwc_ex(const float* f1, int ld_f1, const float* f2_l0, const float* f2_l1, const float* f2_l2,
                           int f2_batch, const float* flow, int B, int H, int W, int C, int levels, int radius,
                           int ld_flow, int prec, float* out, int ld_out, void* stream) {
    if (prec != PP_PREC_F32 && prec != PP_PREC_F16X3 && prec != PP_PREC_F16) return PP_EINVAL;
    if (!f1 || !f2_l0 || !flow || !out || B <= 0 || H <= 0 || W <= 0 || C <= 0 || C % 4 != 0) return PP_EINVAL;
    if (ld_f1 < C || ld_f1 % 4 != 0 || ((uintptr_t)f1 % 16) != 0 || f2_batch <= 0) return PP_EINVAL;
    if (levels < 1 || levels > MAXL || radius < 1 || radius > MAXR) return PP_EINVAL;
    if ((levels > 1 && !f2_l1) || (levels > 2 && !f2_l2)) return PP_EINVAL;
    if ((H >> (levels - 1)) < 1 || (W >> (levels - 1)) < 1 || ld_flow < 2) return PP_EINVAL;
    const int win = 2 * radius + 1;
    if (ld_out < levels * win * win) return PP_EINVAL;
    const char* te = getenv("PP_CORR_TILED");   // read per call: the tests run both kernels in one process
    const bool tiled = !(te && te[0] == '0');   // (PP_PREC_F32: the tiled kernel on exact fp32 MFMAs — every product and sum fp32)
    // every pyramid level the tiled kernel reads goes through 16-byte vector loads: a misaligned one falls back (as the hl entry
    // point below rejects it) instead of faulting
    const bool aligned = (((uintptr_t)f2_l0 | (levels > 1 ? (uintptr_t)f2_l1 : 0) | (levels > 2 ? (uintptr_t)f2_l2 : 0)) % 16) == 0;
    // (H, W % 8 == 0 and at most three levels: a tiled kernel never sees a pooled axis shorter than 2, the case corr_lookup_kernel treats apart)
    if (tiled && H % CT == 0 && W % CT == 0 && C % CK == 0 && aligned)   // (PP_CORR_TILED=0 keeps the lane-per-position kernel)
        return corr_tiled_launch(false, f1, ld_f1, f2_l0, f2_l1, f2_l2, f2_batch, flow, B, H, W, C, levels, radius, ld_flow, out, ld_out, stream,
                                 prec == PP_PREC_F32, prec == PP_PREC_F16);
    // (PP_PREC_F16 on the lane-per-position kernel below: fp32 products — finer than the mode asks for)
    const size_t smem = (size_t)4 * (C + MAXL * TW * TW) * sizeof(float);
    hipLaunchKernelGGL(corr_lookup_kernel, dim3((H * W + 3) / 4, B), dim3(256), smem, (hipStream_t)stream, f1, ld_f1, f2_batch, f2_l0, f2_l1,
                       f2_l2, flow, H, W, C, levels, radius, ld_flow, 1.0f / sqrtf((float)C), out, ld_out);
    return pp_last_launch();
}

int pp_corr_lookup_nhwc_hl_op(const void* f1_hl, int ld_f1, const void* f2_hl_l0, const void* f2_hl_l1, const void* f2_hl_l2,
                              int f2_batch, const float* flow, int B, int H, int W, int C, int levels, int radius, int ld_flow,
                              float* out, int ld_out, void* out_hl, int ld_out_h, void* stream) {
    if (!f1_hl || !f2_hl_l0 || !flow || (out != nullptr) == (out_hl != nullptr) || B <= 0 || H <= 0 || W <= 0 || C <= 0 || f2_batch <= 0)
        return PP_EINVAL;
    if (H % CT != 0 || W % CT != 0 || C % CK != 0 || ld_f1 < C || ld_f1 % 8 != 0) return PP_EINVAL;   // tiled shapes only
    if (((uintptr_t)f1_hl | (uintptr_t)f2_hl_l0 | (uintptr_t)f2_hl_l1 | (uintptr_t)f2_hl_l2) % 16 != 0) return PP_EINVAL;
    if (levels < 1 || levels > MAXL || radius < 1 || radius > MAXR) return PP_EINVAL;
    if ((levels > 1 && !f2_hl_l1) || (levels > 2 && !f2_hl_l2)) return PP_EINVAL;
    if ((H >> (levels - 1)) < 1 || (W >> (levels - 1)) < 1 || ld_flow < 2) return PP_EINVAL;
    const int win = 2 * radius + 1, ld = out_hl ? ld_out_h : ld_out;
    if (ld < levels * win * win) return PP_EINVAL;
    if (out_hl && (ld_out_h % 8 != 0 || ((uintptr_t)out_hl % 16) != 0)) return PP_EINVAL;   // whole groups of 8 channels
    return corr_tiled_launch(true, f1_hl, ld_f1, f2_hl_l0, f2_hl_l1, f2_hl_l2, f2_batch, flow, B, H, W, C, levels, radius, ld_flow, out, ld,
                             stream, false, false, out_hl);
}

int pp_corr_lookup_nhwc_hl(const void* f1_hl, int ld_f1, const void* f2_hl_l0, const void* f2_hl_l1, const void* f2_hl_l2,
                           int f2_batch, const float* flow, int B, int H, int W, int C, int levels, int radius, int ld_flow,
                           float* out, int ld_out, void* stream) {
    return pp_corr_lookup_nhwc_hl_op(f1_hl, ld_f1, f2_hl_l0, f2_hl_l1, f2_hl_l2, f2_batch, flow, B, H, W, C, levels, radius, ld_flow, out, ld_out,
                                     nullptr, 0, stream);
}

int pp_corr_lookup_nhwc(const float* f1, int ld_f1, const float* f2_l0, const float* f2_l1, const float* f2_l2,
                        int f2_batch, const float* flow, int B, int H, int W, int C, int levels, int radius,
                        int ld_flow, float* out, int ld_out, void* stream) {
    return pp_corr_lookup_nhwc_ex(f1, ld_f1, f2_l0, f2_l1, f2_l2, f2_batch, flow, B, H, W, C, levels, radius, ld_flow,
                                  PP_PREC_F16X3, out, ld_out, stream);
}

}  // extern "C"
