// Sampling kernels of stage 3 (NHWC): bilinear resize (align_corners=True), the feature warp
// (grid_sample, zeros padding) and the on-demand local correlation lookup that replaces the
// reference's materialised correlation pyramid.

#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <stdint.h>
#include "../../include/picopose_hip.h"
#include "pp_common.h"
#include "pp_crop_dev.h"

namespace {

typedef float f4 __attribute__((ext_vector_type(4)));

// One blend for every path of resize_kernel, with the contraction spelled out: left to the compiler, the 4-channel path fused the outer
// sum into an fma and the scalar and 8-channel paths did not, so the same element differed in its last bit between the plain map, the
// dual output's map and a misaligned view (tests/test_kernel_bounds_gpu.py).  This is the form the scalar and operand paths had.
__device__ __forceinline__ float resize_blend(float a, float b, float c, float d, float hx, float lx, float hy, float ly, float mul) {
#pragma clang fp contract(off)
    const float top = fmaf(hx, a, lx * b), bot = fmaf(hx, c, lx * d);
    return (hy * top + ly * bot) * mul;
}

// F.interpolate(mode="bilinear", align_corners=True) — dpt.py:150-152, flow_decoder.py:88-92.
// ATen: src = dst * (in-1)/(out-1); i0 = floor, i1 = min(i0+1, in-1), lambda = src - i0.
__global__ __launch_bounds__(256) void resize_kernel(const float* __restrict__ in, int H, int W, int C,
                                                     int Ho, int Wo, float mul, float* __restrict__ out,
                                                     _Float16* __restrict__ out_hl, int terms) {
    const int b = blockIdx.z, oy = blockIdx.y, tid = threadIdx.x;
    const float sy = Ho > 1 ? (float)(H - 1) / (float)(Ho - 1) : 0.f;
    const float sx = Wo > 1 ? (float)(W - 1) / (float)(Wo - 1) : 0.f;
    const float fy = sy * (float)oy;
    const int y0 = (int)fy, y1 = y0 + (y0 < H - 1 ? 1 : 0);
    const float ly = fy - (float)y0, hy = 1.f - ly;
    const float* ib = in + (size_t)b * H * W * C;
    if (out_hl) {  // the result as the f16x3 operand of the following 1x1 convolution (and, `out` given, as the fp32 map too): 8 channels per thread
        _Float16* oh = out_hl + ((size_t)b * Ho + oy) * Wo * terms * C;   // terms = 2: hl format, 1: h format
        float* of = out ? out + ((size_t)b * Ho + oy) * Wo * C : nullptr;
        const int C8 = C >> 3;
        for (int i = blockIdx.x * 256 + tid; i < Wo * C8; i += gridDim.x * 256) {
            const int ox = i / C8, c = (i - ox * C8) * 8;
            const float fx = sx * (float)ox;
            const int x0 = (int)fx, x1 = x0 + (x0 < W - 1 ? 1 : 0);
            const float lx = fx - (float)x0, hx = 1.f - lx;
            typedef _Float16 h8 __attribute__((ext_vector_type(8)));
            h8 hh, ll;
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const int cc = c + 4 * q;
                const f4 a = *(const f4*)(ib + ((size_t)y0 * W + x0) * C + cc), bq = *(const f4*)(ib + ((size_t)y0 * W + x1) * C + cc);
                const f4 cq = *(const f4*)(ib + ((size_t)y1 * W + x0) * C + cc), dq = *(const f4*)(ib + ((size_t)y1 * W + x1) * C + cc);
                f4 vq;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const float v = resize_blend(a[k], bq[k], cq[k], dq[k], hx, lx, hy, ly, mul);
                    _Float16 h, l;
                    pp_split_f16_chk(v, h, l);
                    hh[4 * q + k] = h;
                    ll[4 * q + k] = l;
                    vq[k] = v;
                }
                if (of) *(f4*)(of + (size_t)ox * C + cc) = vq;
            }
            *(h8*)(oh + ((size_t)ox * C + c) * terms) = hh;
            if (terms == 2) *(h8*)(oh + (size_t)ox * 2 * C + 2 * c + 8) = ll;
        }
        return;
    }
    float* ob = out + ((size_t)b * Ho + oy) * Wo * C;
    if ((C & 3) == 0 && (((uintptr_t)in | (uintptr_t)out) & 15) == 0) {  // 4 channels per thread: same arithmetic per element
        const int C4 = C >> 2;
        for (int i = blockIdx.x * 256 + tid; i < Wo * C4; i += gridDim.x * 256) {
            const int ox = i / C4, c = (i - ox * C4) * 4;
            const float fx = sx * (float)ox;
            const int x0 = (int)fx, x1 = x0 + (x0 < W - 1 ? 1 : 0);
            const float lx = fx - (float)x0, hx = 1.f - lx;
            const f4 a = *(const f4*)(ib + ((size_t)y0 * W + x0) * C + c), bq = *(const f4*)(ib + ((size_t)y0 * W + x1) * C + c);
            const f4 cq = *(const f4*)(ib + ((size_t)y1 * W + x0) * C + c), dq = *(const f4*)(ib + ((size_t)y1 * W + x1) * C + c);
            f4 v;
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = resize_blend(a[k], bq[k], cq[k], dq[k], hx, lx, hy, ly, mul);
            *(f4*)(ob + (size_t)ox * C + c) = v;
        }
        return;
    }
    for (int i = blockIdx.x * 256 + tid; i < Wo * C; i += gridDim.x * 256) {
        const int ox = i / C, c = i - ox * C;
        const float fx = sx * (float)ox;
        const int x0 = (int)fx, x1 = x0 + (x0 < W - 1 ? 1 : 0);
        const float lx = fx - (float)x0, hx = 1.f - lx;
        ob[i] = resize_blend(ib[((size_t)y0 * W + x0) * C + c], ib[((size_t)y0 * W + x1) * C + c], ib[((size_t)y1 * W + x0) * C + c],
                             ib[((size_t)y1 * W + x1) * C + c], hx, lx, hy, ly, mul);
    }
}

// coordinate round trip of the reference: bilinear_sample scales pixel coords to [-1,1]
// (corr_lookup.py:61-63) and grid_sample(align_corners=True) maps them back
__device__ __forceinline__ float roundtrip(float x, int size) {
    const float n = x * 2.f / (float)(size - 1 > 1 ? size - 1 : 1) - 1.f;
    return ((n + 1.f) / 2.f) * (float)(size - 1);
}

// FlowDecoder.feature_sample — flow_decoder.py:49-56: out[p] = bilinear(feat, p + flow[p]), zeros padding.
// One wave per pixel, lanes over channels (float4).
// HL: the result leaves only as columns of an hl operand (rows of ld_out ELEMENTS = 2 ld_out halfs): a lane's 4 channels
// are half of a group of 8 — 4 hi terms and 4 lo terms, 8 bytes each.
template <bool HL>
__global__ __launch_bounds__(256) void warp_kernel(const float* __restrict__ feat, int feat_batch,
                                                   const float* __restrict__ flow, int H, int W, int C, int ld_flow,
                                                   float* __restrict__ out, int ld_out, int terms) {
    const int b = blockIdx.y, p = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (p >= H * W) return;
    const int y = p / W, x = p - y * W;
    const float* fl = flow + ((size_t)b * H * W + p) * ld_flow;
    // (clamped as floats BEFORE the integer conversion: a huge or NaN flow lands two pixels outside the image — every tap
    // invalid, like any other out-of-image sample — instead of in an undefined float -> int conversion; fmaxf drops a NaN)
    const float ix = fminf(fmaxf(roundtrip((float)x + fl[0], W), -2.f), (float)W + 1.f);
    const float iy = fminf(fmaxf(roundtrip((float)y + fl[1], H), -2.f), (float)H + 1.f);
    const float x0f = floorf(ix), y0f = floorf(iy);
    const int x0 = (int)x0f, y0 = (int)y0f;
    const float wx1 = ix - x0f, wx0 = (x0f + 1.f) - ix, wy1 = iy - y0f, wy0 = (y0f + 1.f) - iy;
    const float* fb = feat + (size_t)(b % feat_batch) * H * W * C;  // feat given once for several hypotheses
    float* o = HL ? nullptr : out + ((size_t)b * H * W + p) * ld_out;
    _Float16* oh = HL ? (_Float16*)out + ((size_t)b * H * W + p) * terms * ld_out : nullptr;   // terms = 2: hl, 1: h format
    const bool vx0 = x0 >= 0 && x0 < W, vx1 = x0 + 1 >= 0 && x0 + 1 < W;
    const bool vy0 = y0 >= 0 && y0 < H, vy1 = y0 + 1 >= 0 && y0 + 1 < H;
    // Taps outside the image read a clamped pixel whose VALUE is then masked to zero (bitwise: all-ones / all-zeros mask) —
    // zeros padding exactly like grid_sample, also when the clamped pixel holds Inf / NaN (a zero WEIGHT would turn those
    // into NaN) — instead of being skipped by a lane-masked branch: no per-tap lane masks held in SGPR pairs across the
    // loads.  With two busy PROCESSES on one card bits 48..63 of such masks were seen corrupted (lanes 48-63 of single
    // waves lost taps: tests/stress_pc.py); the branch-free form ran 12 000 iterations under that load clean.
    typedef unsigned u4w __attribute__((ext_vector_type(4)));
    const unsigned m00 = 0u - (unsigned)(vy0 & vx0), m01 = 0u - (unsigned)(vy0 & vx1), m10 = 0u - (unsigned)(vy1 & vx0),
                   m11 = 0u - (unsigned)(vy1 & vx1);
    const int xa = min(max(x0, 0), W - 1), xb = min(max(x0 + 1, 0), W - 1), ya = min(max(y0, 0), H - 1), yb = min(max(y0 + 1, 0), H - 1);
    auto tap = [&](int yy, int xx, int c, unsigned m) __attribute__((always_inline)) -> f4 {
        const u4w raw = *(const u4w*)(fb + ((size_t)yy * W + xx) * C + c) & m;
        return __builtin_bit_cast(f4, raw);
    };
    for (int c = lane * 4; c < C; c += 256) {
        f4 acc = {0.f, 0.f, 0.f, 0.f};
        acc += tap(ya, xa, c, m00) * (wx0 * wy0);
        acc += tap(ya, xb, c, m01) * (wx1 * wy0);
        acc += tap(yb, xa, c, m10) * (wx0 * wy1);
        acc += tap(yb, xb, c, m11) * (wx1 * wy1);
        if (HL) {
            typedef _Float16 h4w __attribute__((ext_vector_type(4)));
            _Float16 h0, h1, h2, h3, l0, l1, l2, l3;
            pp_split_f16_chk(acc.x, h0, l0);
            pp_split_f16_chk(acc.y, h1, l1);
            pp_split_f16_chk(acc.z, h2, l2);
            pp_split_f16_chk(acc.w, h3, l3);
            if (terms == 2) {
                _Float16* q = oh + pp_hl_col(c, 0);
                *(h4w*)q = h4w{h0, h1, h2, h3};
                *(h4w*)(q + 8) = h4w{l0, l1, l2, l3};
            } else {
                *(h4w*)(oh + c) = h4w{h0, h1, h2, h3};
            }
        } else {
            *(f4*)(o + c) = acc;
        }
    }
}

// nn.AvgPool2d(2, 2) on NHWC (the pyramid levels of raft_decoder.py:49-51, applied to the
// feature map instead of the correlation volume: the mean commutes with the dot product)
__global__ __launch_bounds__(256) void avgpool2_kernel(const float* __restrict__ in, int H, int W, int C,
                                                       float* __restrict__ out) {
    const int Ho = H / 2, Wo = W / 2, b = blockIdx.y;
    const size_t n = (size_t)Ho * Wo * C;
    const float* ib = in + (size_t)b * H * W * C;
    float* ob = out + (size_t)b * n;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const int c = (int)(i % C);
        const size_t q = i / C;
        const int ox = (int)(q % Wo), oy = (int)(q / Wo);
        const float* p = ib + ((size_t)(2 * oy) * W + 2 * ox) * C + c;
        ob[i] = ((p[0] + p[C]) + (p[(size_t)W * C] + p[(size_t)W * C + C])) * 0.25f;
    }
}

// The same pool with the pooled map's hl operand written alongside (C % 8 == 0; a thread takes 4 channels: half of a group of 8 — 4 hi and
// 4 lo terms): the sum order and the factor of avgpool2_kernel, the split of pp_split_f16_chk — the bits and the saturation report of
// avgpool2_kernel followed by split_act_kernel.  out may be null (the last pyramid level: only its operand is read).
__global__ __launch_bounds__(256) void avgpool2_hl_kernel(const float* __restrict__ in, int H, int W, int C, float* __restrict__ out,
                                                          _Float16* __restrict__ out_hl) {
    const int Ho = H / 2, Wo = W / 2, b = blockIdx.y, C4 = C >> 2;
    const size_t n4 = (size_t)Ho * Wo * C4;
    const float* ib = in + (size_t)b * H * W * C;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
        const int c = (int)(i % C4) * 4;
        const size_t q = i / C4;
        const int ox = (int)(q % Wo), oy = (int)(q / Wo);
        const float* p = ib + ((size_t)(2 * oy) * W + 2 * ox) * C + c;
        const f4 p0 = *(const f4*)p, p1 = *(const f4*)(p + C), p2 = *(const f4*)(p + (size_t)W * C), p3 = *(const f4*)(p + (size_t)W * C + C);
        f4 v;
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = ((p0[k] + p1[k]) + (p2[k] + p3[k])) * 0.25f;
        const size_t row = (size_t)b * Ho * Wo + q;
        if (out) *(f4*)(out + row * C + c) = v;
        _Float16 h0, h1, h2, h3, l0, l1, l2, l3;
        pp_split_f16_chk(v[0], h0, l0);
        pp_split_f16_chk(v[1], h1, l1);
        pp_split_f16_chk(v[2], h2, l2);
        pp_split_f16_chk(v[3], h3, l3);
        _Float16* o = out_hl + row * 2 * (size_t)C + pp_hl_col(c, 0);
        typedef _Float16 h4w __attribute__((ext_vector_type(4)));
        *(h4w*)o = h4w{h0, h1, h2, h3};
        *(h4w*)(o + 8) = h4w{l0, l1, l2, l3};
    }
}

// CorrelationPyramid + CorrLookup fused — raft_decoder.py:30-53, corr_lookup.py:100-134.
// corr_l[p, q] = <f1[p], pool_l(f2)[q]> / sqrt(C); for every pixel p and level l the (2r+1)^2
// window around (p + flow[p]) / 2^l is bilinearly sampled (zeros padding).  Output channel
// l*(2r+1)^2 + a*(2r+1) + b samples at x offset a-r, y offset b-r (the reference's transposed
// window order).  One wave per pixel: the (2r+2)^2 integer neighbours per level are dotted by
// one lane each (C sequential fmas, f1[p] broadcast from LDS), then lanes blend the 4 corners.
constexpr int MAXR = 2, TW = 2 * MAXR + 2, MAXL = 3;
__global__ __launch_bounds__(256) void corr_lookup_kernel(const float* __restrict__ f1, int ld_f1,
                                                          int f2_batch, const float* __restrict__ f2l0,
                                                          const float* __restrict__ f2l1,
                                                          const float* __restrict__ f2l2,
                                                          const float* __restrict__ flow, int H, int W, int C,
                                                          int L, int r, int ld_flow, float inv_sqrt_c,
                                                          float* __restrict__ out, int ld_out) {
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
            // (clamped as floats before the integer conversion: a huge / NaN flow is an out-of-image sample, all zeros)
            cx[l] = fminf(fmaxf(roundtrip(gx / sc, Wl), -(float)(r + 2)), (float)(Wl + r + 1));
            cy[l] = fminf(fmaxf(roundtrip(gy / sc, Hl), -(float)(r + 2)), (float)(Hl + r + 1));
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
            const float* t = tab + l * tw * tw + bi * tw + ai;  // x offset a-r -> dx = ai, y offset b-r -> dy = bi
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
// neighbourhood does not fit the region are served by further passes with a new region (a pixel with the smallest
// origin is always covered, so the loop ends; smooth flows need one pass), neighbourhoods entirely outside the image
// are zeros without any work.  f2 rows outside the image enter as zero rows (grid_sample's zeros padding).
constexpr int CT = 8, CM = CT * CT;            // source-pixel tile
constexpr int CRW = 16, CN = CRW * CRW;        // region of f2 positions
constexpr int CK = 32, CKP = CK + 4;           // channels per chunk; LDS row = 32 hi + 32 lo halfs + pad = 36 dwords
                                               // (144 B: conflict-free b128 reads)
typedef _Float16 h8_t __attribute__((ext_vector_type(8)));
typedef _Float16 h4_t __attribute__((ext_vector_type(4)));
constexpr int CSP = CN + 4;                    // row pitch of S
typedef float f32x16_t __attribute__((ext_vector_type(16)));

// One result element of the tiled lookups: channel ch of pixel row `row`, into the fp32 map (rows of ld_out floats) or, out_hl given, into
// the hl operand of the 1x1 convolution that reads the map (rows of ld_out channels = 2 ld_out halfs) — the split of pp_split_f16_chk, so
// the bits and the saturation report are those of the fp32 map going through split_act_kernel.
__device__ __forceinline__ void corr_put(float* __restrict__ out, _Float16* __restrict__ out_hl, size_t row, int ld_out, int ch, float v) {
    if (out_hl) {
        _Float16 h, l;
        pp_split_f16_chk(v, h, l);
        _Float16* q = out_hl + row * 2 * (size_t)ld_out + pp_hl_col(ch, 0);
        q[0] = h;
        q[8] = l;
    } else {
        out[row * ld_out + ch] = v;
    }
}

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
    __shared__ float s_cx[CM], s_cy[CM];
    __shared__ int s_bx[CM], s_by[CM], s_state[CM], s_ox, s_oy, s_todo;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, l31 = lane & 31, lh = lane >> 5;
    const int tiles_x = W / CT, tiles = tiles_x * (H / CT), total = tiles * B;
    // workgroups are dealt round-robin to the 8 XCDs: make consecutive tiles (same image, overlapping regions) share an L2
    int g = blockIdx.x;
    if (total % 8 == 0) g = (g % 8) * (total / 8) + g / 8;
    const int b = g / tiles, tile = g - b * tiles;
    const int y0 = (tile / tiles_x) * CT, x0 = (tile % tiles_x) * CT;
    const int tw = 2 * r + 2, win = 2 * r + 1, fit = CRW - tw;
    const int my = tid >> 3, mx = tid & 7;                  // tid < 64: the pixel this thread describes
    float gx = 0.f, gy = 0.f;
    if (tid < CM) {
        const float* fl = flow + ((size_t)b * H * W + (size_t)(y0 + my) * W + x0 + mx) * ld_flow;
        gx = (float)(x0 + mx) + fl[0];
        gy = (float)(y0 + my) + fl[1];
    }
    // the pad channels [L win^2, ld_out) of the tile's 64 rows: zeros (the caller allocates without a fill)
    for (int npad = ld_out - L * win * win, idx = tid; idx < CM * npad; idx += 256) {
        const int m = idx / npad, o = idx - m * npad;
        corr_put(out, out_hl, (size_t)b * H * W + (size_t)(y0 + (m >> 3)) * W + x0 + (m & 7), ld_out, L * win * win + o, 0.f);
    }
    for (int l = 0; l < L; ++l) {
        const int Hl = H >> l, Wl = W >> l;
        const void* f2v = l == 0 ? f2l0 : (l == 1 ? f2l1 : f2l2);
        const float* f2 = (const float*)f2v + (size_t)(b % f2_batch) * Hl * Wl * C;                 // fp32 input
        const _Float16* f2h = (const _Float16*)f2v + (size_t)(b % f2_batch) * Hl * Wl * C * 2;      // hl input
        const float* f1 = (const float*)f1v;
        const _Float16* f1h = (const _Float16*)f1v;
        if (tid == 0) s_todo = 0;
        __syncthreads();
        if (tid < CM) {
            const float sc = (float)(1 << l);
            // centre sample (offset 0): its integer corner anchors the neighbourhood (clamped far outside: no overflow)
            const float cx = fminf(fmaxf(roundtrip(gx / sc, Wl), -1.0e6f), 1.0e6f);
            const float cy = fminf(fmaxf(roundtrip(gy / sc, Hl), -1.0e6f), 1.0e6f);
            const int bx = (int)floorf(cx) - r, by = (int)floorf(cy) - r;
            s_cx[tid] = cx; s_cy[tid] = cy; s_bx[tid] = bx; s_by[tid] = by;
            const bool outside = bx >= Wl || by >= Hl || bx + tw <= 0 || by + tw <= 0;
            s_state[tid] = outside ? 2 : 0;                // 0 = to do, 1 = done, 2 = all zeros
            if (!outside) atomicAdd(&s_todo, 1);
        }
        __syncthreads();
        for (int idx = tid; idx < CM * win * win; idx += 256) {   // neighbourhoods outside the image: zeros
            const int m = idx / (win * win), o = idx - m * (win * win);
            if (s_state[m] == 2)
                corr_put(out, out_hl, (size_t)b * H * W + (size_t)(y0 + (m >> 3)) * W + x0 + (m & 7), ld_out, l * win * win + o, 0.f);
        }
        while (s_todo > 0) {                                // (uniform: read after a barrier, written before the next)
            // ---- region of this pass: origin = smallest bx still to do, then the smallest by among its column band
            if (tid == 0) { s_ox = 0x7fffffff; s_oy = 0x7fffffff; }
            __syncthreads();
            if (tid < CM && s_state[tid] == 0) atomicMin(&s_ox, s_bx[tid]);
            __syncthreads();
            if (tid < CM && s_state[tid] == 0 && s_bx[tid] - s_ox <= fit) atomicMin(&s_oy, s_by[tid]);
            __syncthreads();
            const int ox = s_ox, oy = s_oy;
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
                    const int m = row0 + 32 * i;
                    const size_t px = (size_t)b * H * W + (size_t)(y0 + (m >> 3)) * W + x0 + (m & 7);
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
            // ---- blend the 25 samples of every pixel whose neighbourhood lies in the region
            for (int idx = tid; idx < CM * win * win; idx += 256) {
                const int m = idx / (win * win), o = idx - m * (win * win), ai = o / win, bi = o - ai * win;
                const int dx = s_bx[m] - ox, dy = s_by[m] - oy;
                if (s_state[m] == 0 && dx >= 0 && dx <= fit && dy >= 0 && dy <= fit) {
                    const float cx = s_cx[m], cy = s_cy[m];
                    const float wx1 = cx - floorf(cx), wy1 = cy - floorf(cy), wx0 = 1.f - wx1, wy0 = 1.f - wy1;
                    const float* t = S + m * CSP + (dy + bi) * CRW + dx + ai;   // x offset a-r -> +ai, y offset b-r -> +bi
                    corr_put(out, out_hl, (size_t)b * H * W + (size_t)(y0 + (m >> 3)) * W + x0 + (m & 7), ld_out, l * win * win + o,
                             t[0] * (wx0 * wy0) + t[1] * (wx1 * wy0) + t[CRW] * (wx0 * wy1) + t[CRW + 1] * (wx1 * wy1));
                }
            }
            __syncthreads();
            if (tid < CM && s_state[tid] == 0) {
                const int dx = s_bx[tid] - ox, dy = s_by[tid] - oy;
                if (dx >= 0 && dx <= fit && dy >= 0 && dy <= fit) {
                    s_state[tid] = 1;
                    atomicSub(&s_todo, 1);
                }
            }
            __syncthreads();
        }
        __syncthreads();
    }
}

// ---- the operand-input lookup again: a region per pyramid level, chunks staged by LDS-DMA into a ring ------------------------------
// Same tiles, same pass loop and same arithmetic as corr_lookup_mfma_kernel<true> (an entry of S is accumulated over the channels in
// ascending order, per 16 channels hi.hi, hi.lo, lo.hi; it does not depend on the region or the pass that produced it: the same bits),
// but
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

// one pyramid level of one tile.  f1b: image b of the render operand; f2b: image b % f2_batch of the level's query operand (Hl x Wl);
// s_org = {region origin x, y, pixels still to do}
template <int RW, int NRP>
__device__ __forceinline__ void corr_ring_level(float* sm, float* s_cx, float* s_cy, int* s_bx, int* s_by, int* s_state, int* s_org, int l,
                                                const _Float16* f1b, int ld_f1, int f1_bytes, const _Float16* f2b, int Hl, int Wl, int C,
                                                float gx, float gy, int r, float inv_sqrt_c, size_t row0, int y0, int x0, int W,
                                                float* __restrict__ out, _Float16* __restrict__ out_hl, int ld_out) {
    constexpr int NB = corr_ring_nb(RW), NT = (2 * NB + 3) / 4;   // column blocks of S; 32 x 32 tiles of S per wave (tile t = wave + 4 i)
    constexpr int PA = CM / RP / 4, PB = NRP / RP / 4, NP = PA + PB;   // DMA pieces per wave and step: tile rows, region rows
    constexpr int STG = (CM + NRP) * RROW;                        // halfs per stage: [64 tile rows | NRP region rows]
    constexpr int SP = NB * 32 + 4;                               // row pitch of S
    _Float16* ring = (_Float16*)sm;
    float* S = sm;                                                // [32][SP]: aliases the ring once the K loop is over
    const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6), l31 = lane & 31, lh = lane >> 5;
    const int tw = 2 * r + 2, win = 2 * r + 1, fit = RW - tw;
    if (tid == 0) s_org[2] = 0;
    __syncthreads();
    if (tid < CM) {
        const float sc = (float)(1 << l);
        // centre sample (offset 0): its integer corner anchors the neighbourhood (clamped far outside: no overflow)
        const float cx = fminf(fmaxf(roundtrip(gx / sc, Wl), -1.0e6f), 1.0e6f);
        const float cy = fminf(fmaxf(roundtrip(gy / sc, Hl), -1.0e6f), 1.0e6f);
        const int bx = (int)floorf(cx) - r, by = (int)floorf(cy) - r;
        s_cx[tid] = cx; s_cy[tid] = cy; s_bx[tid] = bx; s_by[tid] = by;
        const bool outside = bx >= Wl || by >= Hl || bx + tw <= 0 || by + tw <= 0;
        s_state[tid] = outside ? 2 : 0;                // 0 = to do, 1 = done, 2 = all zeros
        if (!outside) atomicAdd(&s_org[2], 1);
    }
    __syncthreads();
    for (int idx = tid; idx < CM * win * win; idx += 256) {   // neighbourhoods outside the image: zeros
        const int m = idx / (win * win), o = idx - m * (win * win);
        if (s_state[m] == 2) corr_put(out, out_hl, row0 + (size_t)(y0 + (m >> 3)) * W + x0 + (m & 7), ld_out, l * win * win + o, 0.f);
    }
    // DMA slot of this lane: a piece fills 16 rows, lane -> row lane >> 2, chunk position lane & 3, which holds source chunk sc (the key
    // reads bits 2, 3 of the row = of lane >> 2: the same for every piece)
    const int lr = lane / LPR, sc = (lane % LPR) ^ ((lr >> 2) & 3);
    const __amdgpu_buffer_rsrc_t Ar = __builtin_amdgcn_make_buffer_rsrc((void*)f1b, 0, f1_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t Br = __builtin_amdgcn_make_buffer_rsrc((void*)f2b, 0, Hl * Wl * C * 4, 0x00020000);
    unsigned abyte[PA];                                       // tile pixels of this lane's pieces of the render operand
#pragma unroll
    for (int j = 0; j < PA; ++j) {
        const int ma = (j * 4 + wv) * RP + lr;
        abyte[j] = (unsigned)(((y0 + (ma >> 3)) * W + x0 + (ma & 7)) * ld_f1) * 4u + (unsigned)sc * 16u;
    }
    const int ns = C / RK;
    // fragment reads: lane (l31, lh) feeds row / column l31 with channels 8 lh .. + 7 of the step: chunk 2 lh (hi terms), 2 lh + 1 (lo)
    const int ph = ((2 * lh) ^ ((l31 >> 2) & 3)) * 8, pl = ph ^ 8;
    while (s_org[2] > 0) {                                  // (uniform: read after a barrier, written before the next)
        // ---- region of this pass: origin = smallest bx still to do, then the smallest by among its column band
        if (tid == 0) { s_org[0] = 0x7fffffff; s_org[1] = 0x7fffffff; }
        __syncthreads();
        if (tid < CM && s_state[tid] == 0) atomicMin(&s_org[0], s_bx[tid]);
        __syncthreads();
        if (tid < CM && s_state[tid] == 0 && s_bx[tid] - s_org[0] <= fit) atomicMin(&s_org[1], s_by[tid]);
        __syncthreads();
        const int ox = s_org[0], oy = s_org[1];
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
            // ---- blend the 25 samples of every pixel whose neighbourhood lies in the region
            for (int idx = tid; idx < CM / 2 * win * win; idx += 256) {
                const int ms = idx / (win * win), o = idx - ms * (win * win), ai = o / win, bi = o - ai * win, m = ms + 32 * half;
                const int dx = s_bx[m] - ox, dy = s_by[m] - oy;
                if (s_state[m] == 0 && dx >= 0 && dx <= fit && dy >= 0 && dy <= fit) {
                    const float cx = s_cx[m], cy = s_cy[m];
                    const float wx1 = cx - floorf(cx), wy1 = cy - floorf(cy), wx0 = 1.f - wx1, wy0 = 1.f - wy1;
                    const float* t = S + ms * SP + (dy + bi) * RW + dx + ai;   // x offset a-r -> +ai, y offset b-r -> +bi
                    corr_put(out, out_hl, row0 + (size_t)(y0 + (m >> 3)) * W + x0 + (m & 7), ld_out, l * win * win + o,
                             t[0] * (wx0 * wy0) + t[1] * (wx1 * wy0) + t[RW] * (wx0 * wy1) + t[RW + 1] * (wx1 * wy1));
                }
            }
        }
        __syncthreads();
        if (tid < CM && s_state[tid] == 0) {
            const int dx = s_bx[tid] - ox, dy = s_by[tid] - oy;
            if (dx >= 0 && dx <= fit && dy >= 0 && dy <= fit) {
                s_state[tid] = 1;
                atomicSub(&s_org[2], 1);
            }
        }
        __syncthreads();
    }
    __syncthreads();
}
#endif

__global__ __launch_bounds__(256, 3) void corr_lookup_ring_kernel(const _Float16* __restrict__ f1h, int ld_f1, int f2_batch,
                                                                  const _Float16* __restrict__ f2l0, const _Float16* __restrict__ f2l1,
                                                                  const _Float16* __restrict__ f2l2, const float* __restrict__ flow, int B,
                                                                  int H, int W, int C, int L, int r, int ld_flow, float inv_sqrt_c,
                                                                  float* __restrict__ out, int ld_out, _Float16* __restrict__ out_hl) {
#if defined(__HIP_DEVICE_COMPILE__)
    extern __shared__ __attribute__((aligned(16))) float sm[];
    __shared__ float s_cx[CM], s_cy[CM];
    __shared__ int s_bx[CM], s_by[CM], s_state[CM], s_org[3];
    const int tid = threadIdx.x;
    const int tiles_x = W / CT, tiles = tiles_x * (H / CT), total = tiles * B;
    // workgroups are dealt round-robin to the 8 XCDs: make consecutive tiles (same image, overlapping regions) share an L2
    int g = blockIdx.x;
    if (total % 8 == 0) g = (g % 8) * (total / 8) + g / 8;
    const int b = g / tiles, tile = g - b * tiles;
    const int y0 = (tile / tiles_x) * CT, x0 = (tile % tiles_x) * CT;
    const int win = 2 * r + 1;
    const int my = tid >> 3, mx = tid & 7;                  // tid < 64: the pixel this thread describes
    const size_t row0 = (size_t)b * H * W;
    float gx = 0.f, gy = 0.f;
    if (tid < CM) {
        const float* fl = flow + (row0 + (size_t)(y0 + my) * W + x0 + mx) * ld_flow;
        gx = (float)(x0 + mx) + fl[0];
        gy = (float)(y0 + my) + fl[1];
    }
    // the pad channels [L win^2, ld_out) of the tile's 64 rows: zeros (the caller allocates without a fill)
    for (int npad = ld_out - L * win * win, idx = tid; idx < CM * npad; idx += 256) {
        const int m = idx / npad, o = idx - m * npad;
        corr_put(out, out_hl, row0 + (size_t)(y0 + (m >> 3)) * W + x0 + (m & 7), ld_out, L * win * win + o, 0.f);
    }
    const _Float16* f1b = f1h + row0 * ld_f1 * 2;
    const int f1_bytes = ((H * W - 1) * ld_f1 + C) * 4;
    const size_t q = (size_t)(b % f2_batch);
    corr_ring_level<RG0_W, RG0_N>(sm, s_cx, s_cy, s_bx, s_by, s_state, s_org, 0, f1b, ld_f1, f1_bytes, f2l0 + q * H * W * C * 2, H, W, C, gx, gy,
                                  r, inv_sqrt_c, row0, y0, x0, W, out, out_hl, ld_out);
    if (L > 1)
        corr_ring_level<RG1_W, RG1_N>(sm, s_cx, s_cy, s_bx, s_by, s_state, s_org, 1, f1b, ld_f1, f1_bytes, f2l1 + q * (H >> 1) * (W >> 1) * C * 2,
                                      H >> 1, W >> 1, C, gx, gy, r, inv_sqrt_c, row0, y0, x0, W, out, out_hl, ld_out);
    if (L > 2)
        corr_ring_level<RG2_W, RG2_N>(sm, s_cx, s_cy, s_bx, s_by, s_state, s_org, 2, f1b, ld_f1, f1_bytes, f2l2 + q * (H >> 2) * (W >> 2) * C * 2,
                                      H >> 2, W >> 2, C, gx, gy, r, inv_sqrt_c, row0, y0, x0, W, out, out_hl, ld_out);
#endif
}

// Row gather: dst[i] = src[index[i]] for rows of `row` floats (row % 4 == 0, 16-byte aligned): the selection of the
// top-k templates' data (model/picopose.py:55-62 — torch.gather with an expanded index over (B,N,3,224,224) etc.)
__global__ __launch_bounds__(256) void gather_rows_kernel(const float* __restrict__ src, const long long* __restrict__ index,
                                                          long long row, long long nsrc, float* __restrict__ dst) {
    const long long r = index[blockIdx.y];
    if (r < 0 || r >= nsrc) return;  // (validated on the host side of the mirrors; never expected)
    const f4* s4 = (const f4*)(src + r * row);
    f4* d4 = (f4*)(dst + (long long)blockIdx.y * row);
    const long long n4 = row >> 2;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) d4[i] = s4[i];
}

// Bank rows to token rows: tokens[(j T + skip + p) ld + c] = bank[(index[j] C + c) P + p] — the gather above fused with the
// (C, P) -> (P, C) transpose of transpose_kernel (32x33 LDS tile; p runs along the lanes on the load, c on the store), so the last-level
// patch tokens of the selected templates come out of the feature bank (run_test.py:130-134, 161-162) as rows of the level buffer.
// The `skip` leading rows of every image (the cls row, which nothing reads) are zeroed by the blocks of the first tile row.
__global__ __launch_bounds__(256) void bank_rows_to_tokens_kernel(const float* __restrict__ bank, const long long* __restrict__ index,
                                                                  long long nsrc, int C, int P, float* __restrict__ tokens, int ld, int T,
                                                                  int skip) {
    __shared__ float t[32][33];
    const long long r = index[blockIdx.z];
    if (r < 0 || r >= nsrc) return;  // (as gather_rows_kernel; uniform over the block, before the barrier)
    const int c0 = blockIdx.x * 32, p0 = blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
    const float* src = bank + (size_t)r * C * P;
    float* dst = tokens + (size_t)blockIdx.z * T * ld;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c = c0 + ty + 8 * i, p = p0 + tx;
        if (c < C && p < P) t[ty + 8 * i][tx] = src[(size_t)c * P + p];
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int p = p0 + ty + 8 * i, c = c0 + tx;
        if (p < P && c < C) dst[(size_t)(skip + p) * ld + c] = t[tx][ty + 8 * i];
    }
    if (blockIdx.y == 0 && c0 + tx < C)
        for (int s = ty; s < skip; s += 8) dst[(size_t)s * ld + c0 + tx] = 0.f;
}

// Stream-ordered snapshot of the sticky saturation word (pp_saturation_take): one lane moves the word into the caller's slot and clears it,
// so the slot covers exactly the producers enqueued on this stream since the previous take.
__global__ __launch_bounds__(64) void saturation_take_kernel(unsigned* __restrict__ word, unsigned* __restrict__ slot) {
    if (threadIdx.x == 0) *slot = atomicExch(word, 0u);
}

// Crop + resize + normalise of one detection (provider/bop_test_dataset.py:162-177 with utils/data_utils.py:231-250):
// out_rgb[c] = (resize_linear(image[y1:y2, x1:x2, 2-c] / 255 [* (mask > 0)]) - mean[c]) / std[c], out_mask =
// resize_nearest(mask[y1:y2, x1:x2]).  cv2.resize semantics on a float image (pixel centres, edge clamp), in double
// like OpenCV's CV_64F path and torchvision's Normalize on the float64 tensor.  One thread per output pixel.
__global__ __launch_bounds__(256) void crop_resize_kernel(const unsigned char* __restrict__ img, int W,
                                                          const unsigned char* __restrict__ mask, int y1, int y2, int x1,
                                                          int x2, int S, int mask_rgb, double m0, double m1, double m2,
                                                          double s0, double s1, double s2, float* __restrict__ out_rgb,
                                                          float* __restrict__ out_mask) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= S * S) return;
    const int oy = i / S, ox = i - oy * S, h = y2 - y1, w = x2 - x1;
    int ya, yb, xa, xb;
    double fy, fx;
    pp_crop_taps(oy, h, S, ya, yb, fy);
    pp_crop_taps(ox, w, S, xa, xb, fx);
    const double mean[3] = {m0, m1, m2}, stdv[3] = {s0, s1, s2};
    auto px = [&](int yy, int xx, int c) -> double {  // channel c of the flipped ([..., ::-1]) crop, / 255, optionally masked
        const size_t p = (size_t)(y1 + yy) * W + (x1 + xx);
        double v = (double)img[p * 3 + (2 - c)] / 255.0;
        if (mask_rgb && mask && mask[p] == 0) v = 0.0;
        return v;
    };
#pragma unroll
    for (int c = 0; c < 3; ++c) out_rgb[(size_t)c * S * S + i] = pp_crop_blend(px, c, ya, yb, xa, xb, fx, fy, mean[c], stdv[c]);
    if (out_mask) {
        const int yi = pp_crop_nearest(oy, h, S), xi = pp_crop_nearest(ox, w, S);
        out_mask[i] = mask ? (float)mask[(size_t)(y1 + yi) * W + (x1 + xi)] : 1.f;
    }
}

// Template lookup points (provider/bop_test_dataset.py:233-235 with utils/data_utils.py:97-115): the back-projected depth
// crop, INTER_NEAREST-resized to P x P: out[i, j] = ((x - cx) z / fx, (y - cy) z / fy, z) at the sampled crop pixel.
__global__ __launch_bounds__(256) void depth_points_kernel(const float* __restrict__ depth, int W, int y1, int y2, int x1,
                                                           int x2, int P, float fx, float fy, float cx, float cy,
                                                           float* __restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= P * P) return;
    const int oy = i / P, ox = i - oy * P, h = y2 - y1, w = x2 - x1;
    const int y = y1 + pp_crop_nearest(oy, h, P), x = x1 + pp_crop_nearest(ox, w, P);
    pp_depth_point(depth[(size_t)y * W + x], x, y, fx, fy, cx, cy, out + 3 * i);
}


// ---- convolutions with one or two output channels (the flow / certainty predict layers, raft_decoder.py:287-289) -----
// On the GEMM engine such a layer pads its 2 (or 1) filters to a 64-wide tile and re-reads every pixel per tap from L2
// (0.6 ms for the 3x3 at 64 x 64 x 160, 10 TFLOP/s).  Here a workgroup takes a band of 256 / W full image rows (one output
// pixel per thread), stages the band plus a one-pixel halo per 32-channel slice in LDS (the input is the hl operand its
// producer wrote: 128 bytes per pixel and slice; x = hi + lo, the exact fp32 value x 4, is formed once per staged element) and
// every thread walks the taps of its pixel: the weights are the layer's fp32 filters (scalar loads: the index is uniform), fp32 fma.
constexpr int NRW_PITCH = 144;   // bytes per staged pixel: 128 + 16 (conflict-free 16-byte reads along a row of pixels)

// F32IN (round 5, ops.PRECISION = "f32"): the input is the fp32 NHWC map itself (ldx floats per pixel; a 32-channel slice of a pixel is
// the same 128 bytes), every product and sum fp32 — the exact-mode form of the same layers (they ran as GEMMs padded from 2 columns to 64).
template <int KS, int NOUT, bool F32IN = false>
__global__ __launch_bounds__(256) void conv_narrow_kernel(const _Float16* __restrict__ x, int ldx, int H, int W, int C,
                                                          const float* __restrict__ w, const float* __restrict__ bias,
                                                          const float* __restrict__ residual, float* __restrict__ out) {
    constexpr int R = KS / 2;
    extern __shared__ __attribute__((aligned(16))) unsigned char nsm[];
    const int TH = 256 / W, bands = H / TH;
    const int b = blockIdx.x / bands, y0 = (blockIdx.x % bands) * TH;
    const int tid = threadIdx.x, ty = tid / W, tx = tid % W;
    const int PW = W + 2 * R, PH = TH + 2 * R;       // staged pixels per row / rows
    float acc[NOUT];
#pragma unroll
    for (int n = 0; n < NOUT; ++n) acc[n] = 0.f;
    const int K = KS * KS * C;
    // staged items of this thread, fetched one slice ahead.  fp32 input: 16-byte pieces (at most 13 for the 6 x 66 band of a 64-wide
    // image).  hl input: 32-byte items — the hi and the lo terms of 8 channels — at most 7; they are summed to the fp32 value ONCE as
    // they are staged (round 6: every tap of every neighbour used to redo the two conversions and the add — 3 of the 5 vector
    // instructions per product), so LDS holds 32 floats per pixel and slice either way and the tap loop is pure fma.
    constexpr int MAXP = F32IN ? 13 : 7, PPX = F32IN ? 8 : 4;      // items per thread; items per pixel
    const int npiece = PH * PW * PPX;
    float4 pre[F32IN ? MAXP : 2 * MAXP];
    auto fetch = [&](int c0) __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < MAXP; ++j) {
            // halo pixels outside the image and slots past the band: the load runs on a clamped pixel and its value is masked
            // to zero bit-wise (zero padding) — no per-lane guarded load, no lane masks held across it
            const int i = min(tid + 256 * j, npiece - 1);
            const int piece = i % PPX, px = i / PPX, sy = px / PW, sx = px - sy * PW;
            const int iy = y0 + sy - R, ix = sx - R;
            const unsigned m = 0u - (unsigned)((tid + 256 * j < npiece) & (iy >= 0) & (iy < H) & (ix >= 0) & (ix < W));
            const int iyc = min(max(iy, 0), H - 1), ixc = min(max(ix, 0), W - 1);
            typedef unsigned u4n __attribute__((ext_vector_type(4)));
            if constexpr (F32IN) {
                const u4n raw = *(const u4n*)((const float*)x + (((size_t)b * H + iyc) * W + ixc) * (size_t)ldx + c0 + 4 * piece) & m;
                pre[j] = __builtin_bit_cast(float4, raw);
            } else {
                const u4n* src = (const u4n*)(x + (((size_t)b * H + iyc) * W + ixc) * (size_t)(2 * ldx) + 2 * c0 + 16 * piece);
                pre[2 * j] = __builtin_bit_cast(float4, src[0] & m);       // 8 hi terms
                pre[2 * j + 1] = __builtin_bit_cast(float4, src[1] & m);   // 8 lo terms
            }
        }
    };
    fetch(0);
    for (int c0 = 0; c0 < C; c0 += 32) {
        __syncthreads();                             // the previous slice has been read
#pragma unroll
        for (int j = 0; j < MAXP; ++j) {
            const int i = tid + 256 * j;
            if (i >= npiece) continue;
            if constexpr (F32IN) {
                *(float4*)(nsm + (size_t)(i >> 3) * NRW_PITCH + 16 * (i & 7)) = pre[j];
            } else {
                typedef _Float16 h8v __attribute__((ext_vector_type(8)));
                const h8v hi = __builtin_bit_cast(h8v, pre[2 * j]), lo = __builtin_bit_cast(h8v, pre[2 * j + 1]);
                float4 a, c;
                a.x = (float)hi[0] + (float)lo[0]; a.y = (float)hi[1] + (float)lo[1]; a.z = (float)hi[2] + (float)lo[2]; a.w = (float)hi[3] + (float)lo[3];
                c.x = (float)hi[4] + (float)lo[4]; c.y = (float)hi[5] + (float)lo[5]; c.z = (float)hi[6] + (float)lo[6]; c.w = (float)hi[7] + (float)lo[7];
                unsigned char* d = nsm + (size_t)(i >> 2) * NRW_PITCH + 32 * (i & 3);
                *(float4*)d = a;
                *(float4*)(d + 16) = c;
            }
        }
        __syncthreads();
        if (c0 + 32 < C) fetch(c0 + 32);             // in flight under this slice's arithmetic
#pragma unroll
        for (int dy = 0; dy < KS; ++dy)
#pragma unroll
            for (int dx = 0; dx < KS; ++dx) {
                const unsigned char* p = nsm + (size_t)((ty + dy) * PW + tx + dx) * NRW_PITCH;
                const float* wt = w + (dy * KS + dx) * C + c0;
#pragma unroll
                for (int g = 0; g < 8; ++g) {        // (channels in ascending order, as before the staging change: same bits)
                    const f4 xv = *(const f4*)(p + 16 * g);
#pragma unroll
                    for (int e = 0; e < 4; ++e)
#pragma unroll
                        for (int n = 0; n < NOUT; ++n) acc[n] = fmaf(xv[e], wt[n * K + 4 * g + e], acc[n]);
                }
            }
    }
    const size_t o = (((size_t)b * H + y0 + ty) * W + tx) * NOUT;
#pragma unroll
    for (int n = 0; n < NOUT; ++n) {
        float v = (F32IN ? acc[n] : acc[n] * (1.0f / PP_A_SCALE)) + (bias ? bias[n] : 0.f);
        if (residual) v += residual[o + n];
        out[o + n] = v;
    }
}

// The flow of a decoder level as the operand of flow_net[0] (raft_decoder.py:141-147): row p of `op8` <- 8 channels, 0 and 1 = the flow,
// 2..7 zero.  One thread per pixel; the split of pp_split_f16_chk, so the bits and the saturation report are those of a zero-padded
// fp32 map going through split_act_kernel.
__global__ __launch_bounds__(256) void flow_operand_kernel(const float* __restrict__ flow, int ld_flow, long long rows, _Float16* __restrict__ op8,
                                                           int terms) {
    const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
    if (p >= rows) return;
    const float* f = flow + p * ld_flow;
    _Float16 h0, l0, h1, l1;
    pp_split_f16_chk(f[0], h0, l0);
    pp_split_f16_chk(f[1], h1, l1);
    const _Float16 z = (_Float16)0.f;
    const h8_t hi = {h0, h1, z, z, z, z, z, z}, lo = {l0, l1, z, z, z, z, z, z};
    h8_t* o = (h8_t*)(op8 + p * 8 * terms);
    o[0] = hi;
    if (terms == 2) o[1] = lo;
}

// Patch-embed operand straight from the image bank: image j < n_front is front[j], image n_front + i is bank[index[i]] ((3, HW) fp32
// planes); row (j HW + p) of `out` <- the 8-channel operand of pixel p (channels 0..2 = the planes' values, 3..7 zero) — what the row
// gather, the concatenation, the NCHW -> NHWC-8 transpose and split_act_kernel leave, in one pass.  A workgroup stages PO_TILE pixels of
// the three planes in LDS (16-byte loads along the plane where HW % 4 == 0) and writes the operand rows as consecutive 16-byte pieces
// (terms = 2: piece 2 q = the hi terms of pixel q, 2 q + 1 its lo terms; terms = 1: piece q).  A bank row outside [0, n_rows) leaves its
// image's rows unwritten, as gather_rows_kernel does.
constexpr int PO_TILE = 1024;
__global__ __launch_bounds__(256) void patch_operand_kernel(const float* __restrict__ bank, const long long* __restrict__ index, long long n_rows,
                                                            const float* __restrict__ front, int n_front, int HW, _Float16* __restrict__ out,
                                                            int terms) {
    __shared__ __attribute__((aligned(16))) float t[3][PO_TILE];
    const int j = blockIdx.y, tid = threadIdx.x;
    const float* src;
    if (j < n_front) {
        src = front + (size_t)j * 3 * HW;
    } else {
        const long long r = index[j - n_front];
        if (r < 0 || r >= n_rows) return;   // (uniform over the block, before the barrier)
        src = bank + (size_t)r * 3 * HW;
    }
    const int p0 = blockIdx.x * PO_TILE, np = min(PO_TILE, HW - p0);
    if ((HW & 3) == 0) {      // planes and tiles start on 16 bytes, np % 4 == 0
        for (int i = tid; i < 3 * (np >> 2); i += 256) {
            const int c = i / (np >> 2), q = i - c * (np >> 2);
            *(f4*)&t[c][4 * q] = *(const f4*)(src + (size_t)c * HW + p0 + 4 * q);
        }
    } else {
        for (int i = tid; i < 3 * np; i += 256) {
            const int c = i / np, q = i - c * np;
            t[c][q] = src[(size_t)c * HW + p0 + q];
        }
    }
    __syncthreads();
    h8_t* o = (h8_t*)(out + ((size_t)j * HW + p0) * 8 * terms);
    const _Float16 z = (_Float16)0.f;
    for (int i = tid; i < np * terms; i += 256) {
        const int q = terms == 2 ? i >> 1 : i;
        _Float16 h0, l0, h1, l1, h2, l2;
        if (terms == 1 || (i & 1) == 0) {   // (one report per pixel)
            pp_split_f16_chk(t[0][q], h0, l0);
            pp_split_f16_chk(t[1][q], h1, l1);
            pp_split_f16_chk(t[2][q], h2, l2);
            o[i] = h8_t{h0, h1, h2, z, z, z, z, z};
        } else {
            pp_split_f16(t[0][q], h0, l0);
            pp_split_f16(t[1][q], h1, l1);
            pp_split_f16(t[2][q], h2, l2);
            o[i] = h8_t{l0, l1, l2, z, z, z, z, z};
        }
    }
}

}  // namespace

PP_SAT_SETTER(pp_sat_set_sample)

extern "C" {

int pp_resize_bilinear_nhwc(const float* in, int B, int H, int W, int C, int Ho, int Wo, float mul, float* out,
                            void* stream) {
    if (!in || !out || B <= 0 || H <= 0 || W <= 0 || C <= 0 || Ho <= 0 || Wo <= 0) return PP_EINVAL;
    const bool vec = (C & 3) == 0 && (((uintptr_t)in | (uintptr_t)out) & 15) == 0;  // (the kernel makes the same test)
    const int work = vec ? Wo * (C / 4) : Wo * C;
    const int gx = (work + 1023) / 1024;  // four items per thread: one workgroup per output row for 64 x 256 channels
    hipLaunchKernelGGL(resize_kernel, dim3(gx < 64 ? gx : 64, Ho, B), dim3(256), 0, (hipStream_t)stream, in, H, W,
                       C, Ho, Wo, mul, out, (_Float16*)nullptr, 2);
    return pp_last_launch();
}

int pp_resize_bilinear_nhwc_t(const float* in, int B, int H, int W, int C, int Ho, int Wo, float mul, void* out_hl,
                              int terms, void* stream) {
    if (!in || !out_hl || B <= 0 || H <= 0 || W <= 0 || C <= 0 || C % 8 != 0 || Ho <= 0 || Wo <= 0 ||
        (((uintptr_t)in | (uintptr_t)out_hl) & 15) != 0 || (terms != 1 && terms != 2))
        return PP_EINVAL;
    const int gx = (Wo * (C / 8) + 1023) / 1024;
    hipLaunchKernelGGL(resize_kernel, dim3(gx < 64 ? gx : 64, Ho, B), dim3(256), 0, (hipStream_t)stream, in, H, W,
                       C, Ho, Wo, mul, (float*)nullptr, (_Float16*)out_hl, terms);
    return pp_last_launch();
}

int pp_resize_bilinear_nhwc_dual(const float* in, int B, int H, int W, int C, int Ho, int Wo, float mul, float* out, void* out_hl,
                                 int terms, void* stream) {
    if (!in || !out || !out_hl || B <= 0 || H <= 0 || W <= 0 || C <= 0 || C % 8 != 0 || Ho <= 0 || Wo <= 0 ||
        (((uintptr_t)in | (uintptr_t)out | (uintptr_t)out_hl) & 15) != 0 || (terms != 1 && terms != 2))
        return PP_EINVAL;
    const int gx = (Wo * (C / 8) + 1023) / 1024;
    hipLaunchKernelGGL(resize_kernel, dim3(gx < 64 ? gx : 64, Ho, B), dim3(256), 0, (hipStream_t)stream, in, H, W,
                       C, Ho, Wo, mul, out, (_Float16*)out_hl, terms);
    return pp_last_launch();
}

int pp_resize_bilinear_nhwc_hl(const float* in, int B, int H, int W, int C, int Ho, int Wo, float mul, void* out_hl,
                               void* stream) {
    return pp_resize_bilinear_nhwc_t(in, B, H, W, C, Ho, Wo, mul, out_hl, 2, stream);
}

int pp_warp_nhwc(const float* feat, int feat_batch, const float* flow, int B, int H, int W, int C, int ld_flow,
                 float* out, int ld_out, void* stream) {
    if (!feat || !flow || !out || B <= 0 || H <= 0 || W <= 0 || C <= 0 || C % 4 != 0 || ld_flow < 2 || feat_batch <= 0 ||
        ld_out < C || ld_out % 4 != 0 || ((uintptr_t)out % 16) != 0)
        return PP_EINVAL;
    hipLaunchKernelGGL(warp_kernel<false>, dim3((H * W + 3) / 4, B), dim3(256), 0, (hipStream_t)stream, feat, feat_batch, flow,
                       H, W, C, ld_flow, out, ld_out, 2);
    return pp_last_launch();
}

int pp_warp_nhwc_t(const float* feat, int feat_batch, const float* flow, int B, int H, int W, int C, int ld_flow,
                   void* out_hl, int ld_h, int terms, void* stream) {
    if (!feat || !flow || !out_hl || B <= 0 || H <= 0 || W <= 0 || C <= 0 || C % 8 != 0 || ld_flow < 2 || feat_batch <= 0 ||
        ld_h < C || ld_h % 8 != 0 || ((uintptr_t)out_hl % 16) != 0 || (terms != 1 && terms != 2))
        return PP_EINVAL;
    hipLaunchKernelGGL(warp_kernel<true>, dim3((H * W + 3) / 4, B), dim3(256), 0, (hipStream_t)stream, feat, feat_batch, flow,
                       H, W, C, ld_flow, (float*)out_hl, ld_h, terms);
    return pp_last_launch();
}

int pp_warp_nhwc_hl(const float* feat, int feat_batch, const float* flow, int B, int H, int W, int C, int ld_flow,
                    void* out_hl, int ld_h, void* stream) {
    return pp_warp_nhwc_t(feat, feat_batch, flow, B, H, W, C, ld_flow, out_hl, ld_h, 2, stream);
}

int pp_avgpool2_nhwc(const float* in, int B, int H, int W, int C, float* out, void* stream) {
    if (!in || !out || B <= 0 || H < 2 || W < 2 || C <= 0 || H % 2 != 0 || W % 2 != 0) return PP_EINVAL;
    const size_t n = (size_t)(H / 2) * (W / 2) * C;
    const int gx = (int)((n + 255) / 256 < 1024 ? (n + 255) / 256 : 1024);
    hipLaunchKernelGGL(avgpool2_kernel, dim3(gx, B), dim3(256), 0, (hipStream_t)stream, in, H, W, C, out);
    return pp_last_launch();
}

int pp_avgpool2_hl(const float* in, int B, int H, int W, int C, float* out, void* out_hl, void* stream) {
    if (!in || !out_hl || B <= 0 || H < 2 || W < 2 || C <= 0 || H % 2 != 0 || W % 2 != 0 || C % 8 != 0) return PP_EINVAL;
    if (((uintptr_t)in | (uintptr_t)out | (uintptr_t)out_hl) % 16 != 0) return PP_EINVAL;
    const size_t n = (size_t)(H / 2) * (W / 2) * (C / 4);
    const int gx = (int)((n + 255) / 256 < 1024 ? (n + 255) / 256 : 1024);
    hipLaunchKernelGGL(avgpool2_hl_kernel, dim3(gx, B), dim3(256), 0, (hipStream_t)stream, in, H, W, C, out, (_Float16*)out_hl);
    return pp_last_launch();
}

static int corr_tiled_launch(bool hl, const void* f1, int ld_f1, const void* f2_l0, const void* f2_l1, const void* f2_l2, int f2_batch,
                             const float* flow, int B, int H, int W, int C, int levels, int radius, int ld_flow, float* out, int ld_out,
                             void* stream, bool exact = false, bool one = false, void* out_hl = nullptr) {
    // matrix-core version: one workgroup per 8 x 8 pixel tile
    const size_t lds = (size_t)(CM * CSP > (CM + CN) * CKP ? CM * CSP : (CM + CN) * CKP) * sizeof(float);
    static signed char attr[PP_MAX_DEVICES];
    signed char& ok = attr[pp_cur_device()];
    if (ok == 0)
        ok = hipFuncSetAttribute((const void*)corr_lookup_mfma_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) == hipSuccess &&
                     hipFuncSetAttribute((const void*)corr_lookup_mfma_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) == hipSuccess &&
                     hipFuncSetAttribute((const void*)corr_lookup_mfma_kernel<false, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) == hipSuccess &&
                     hipFuncSetAttribute((const void*)corr_lookup_mfma_kernel<false, false, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) == hipSuccess &&
                     hipFuncSetAttribute((const void*)corr_lookup_ring_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)CORR_RING_LDS) == hipSuccess
                 ? 1 : -1;
    if (ok < 0) return PP_ELAUNCH;
    const dim3 grid((unsigned)((H / CT) * (W / CT) * B));
    _Float16* oh = (_Float16*)out_hl;
    // operand input: the ring-staged kernel (PP_CORR_RING=0, read per call, keeps the register-staged one: the tests run both in one process).
    // Its DMA offsets are 32-bit and signed on the way: an image of either operand beyond 2 GiB stays with the register-staged kernel.
    const char* re = getenv("PP_CORR_RING");
    const bool ring = hl && !(re && re[0] == '0') && (long long)H * W * ld_f1 * 4 < 0x7FFFFFFFLL && (long long)H * W * C * 4 < 0x7FFFFFFFLL;
    if (ring)
        hipLaunchKernelGGL(corr_lookup_ring_kernel, grid, dim3(256), CORR_RING_LDS, (hipStream_t)stream, (const _Float16*)f1, ld_f1, f2_batch,
                           (const _Float16*)f2_l0, (const _Float16*)f2_l1, (const _Float16*)f2_l2, flow, B, H, W, C, levels, radius, ld_flow,
                           1.0f / sqrtf((float)C), out, ld_out, oh);
    else if (exact)
        hipLaunchKernelGGL((corr_lookup_mfma_kernel<false, true>), grid, dim3(256), lds, (hipStream_t)stream, f1, ld_f1, f2_batch, f2_l0, f2_l1, f2_l2,
                           flow, B, H, W, C, levels, radius, ld_flow, 1.0f / sqrtf((float)C), out, ld_out, oh);
    else if (one)
        hipLaunchKernelGGL((corr_lookup_mfma_kernel<false, false, true>), grid, dim3(256), lds, (hipStream_t)stream, f1, ld_f1, f2_batch, f2_l0, f2_l1,
                           f2_l2, flow, B, H, W, C, levels, radius, ld_flow, 1.0f / sqrtf((float)C), out, ld_out, oh);
    else if (hl)
        hipLaunchKernelGGL(corr_lookup_mfma_kernel<true>, grid, dim3(256), lds, (hipStream_t)stream, f1, ld_f1, f2_batch, f2_l0, f2_l1, f2_l2,
                           flow, B, H, W, C, levels, radius, ld_flow, 1.0f / sqrtf((float)C), out, ld_out, oh);
    else
        hipLaunchKernelGGL(corr_lookup_mfma_kernel<false>, grid, dim3(256), lds, (hipStream_t)stream, f1, ld_f1, f2_batch, f2_l0, f2_l1, f2_l2,
                           flow, B, H, W, C, levels, radius, ld_flow, 1.0f / sqrtf((float)C), out, ld_out, oh);
    return pp_last_launch();
}

int pp_conv_narrow_f32(const float* x, int ld_x, int B, int H, int W, int C, const float* weight, const float* bias, int ksize,
                       int n_out, const float* residual, float* out, void* stream) {
    if (!x || !weight || !out || B <= 0 || H <= 0 || C <= 0 || C % 32 != 0 || ld_x < C || ld_x % 4 != 0) return PP_EINVAL;
    if ((W != 16 && W != 32 && W != 64) || H % (256 / W) != 0 || (ksize != 1 && ksize != 3) || (n_out != 1 && n_out != 2)) return PP_EINVAL;
    if (((uintptr_t)x % 16) != 0) return PP_EINVAL;
    const int TH = 256 / W, R = ksize / 2;
    const size_t lds = (size_t)(TH + 2 * R) * (W + 2 * R) * NRW_PITCH;
    const dim3 grid((unsigned)(B * (H / TH)));
    hipStream_t st = (hipStream_t)stream;
#define NRW_LAUNCH(KS_, N_)                                                                                                                  \
    hipLaunchKernelGGL((conv_narrow_kernel<KS_, N_, true>), grid, dim3(256), lds, st, (const _Float16*)x, ld_x, H, W, C, weight, bias, residual, out)
    if (ksize == 3 && n_out == 2) NRW_LAUNCH(3, 2);
    else if (ksize == 3) NRW_LAUNCH(3, 1);
    else if (n_out == 2) NRW_LAUNCH(1, 2);
    else NRW_LAUNCH(1, 1);
#undef NRW_LAUNCH
    return pp_last_launch();
}

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
    if (tiled && H % CT == 0 && W % CT == 0 && C % CK == 0 && aligned)   // (PP_CORR_TILED=0 keeps the lane-per-position kernel)
        return corr_tiled_launch(false, f1, ld_f1, f2_l0, f2_l1, f2_l2, f2_batch, flow, B, H, W, C, levels, radius, ld_flow, out, ld_out, stream,
                                 prec == PP_PREC_F32, prec == PP_PREC_F16);
    // (PP_PREC_F16 on the lane-per-position kernel below: fp32 products — finer than the mode asks for)
    const size_t smem = (size_t)4 * (C + MAXL * TW * TW) * sizeof(float);
    hipLaunchKernelGGL(corr_lookup_kernel, dim3((H * W + 3) / 4, B), dim3(256), smem, (hipStream_t)stream, f1, ld_f1,
                       f2_batch, f2_l0, f2_l1, f2_l2, flow, H, W, C, levels, radius, ld_flow, 1.0f / sqrtf((float)C), out,
                       ld_out);
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

int pp_gather_rows(const float* src, const long long* index, long long n_src_rows, long long row_floats, int n, float* dst,
                   void* stream) {
    if (!src || !index || !dst || n <= 0 || n_src_rows <= 0 || row_floats <= 0 || row_floats % 4 != 0 ||
        ((uintptr_t)src % 16) != 0 || ((uintptr_t)dst % 16) != 0)
        return PP_EINVAL;
    const long long n4 = row_floats / 4;
    const int gx = (int)((n4 + 255) / 256 < 64 ? (n4 + 255) / 256 : 64);
    hipLaunchKernelGGL(gather_rows_kernel, dim3(gx, n), dim3(256), 0, (hipStream_t)stream, src, index, row_floats, n_src_rows,
                       dst);
    return pp_last_launch();
}

int pp_bank_rows_to_tokens(const float* bank, long long n_bank_rows, int C, int P, const long long* index, int n, float* tokens, int ld,
                           int T, int skip, void* stream) {
    if (!bank || !index || !tokens || n_bank_rows <= 0 || C <= 0 || P <= 0 || n <= 0 || ld < C || skip < 0 || T <= 0 ||
        (long long)skip + P > T)
        return PP_EINVAL;
    if (n > 65535 || (P + 31) / 32 > 65535) return PP_EINVAL;   // grid.z / grid.y
    hipLaunchKernelGGL(bank_rows_to_tokens_kernel, dim3((C + 31) / 32, (P + 31) / 32, n), dim3(256), 0, (hipStream_t)stream, bank, index,
                       n_bank_rows, C, P, tokens, ld, T, skip);
    return pp_last_launch();
}

int pp_patch_operand(const float* bank, long long n_bank_rows, const long long* index, int n, const float* front, int n_front, int H, int W,
                     void* out, int terms, void* stream) {
    if (!out || n < 0 || n_front < 0 || n + n_front <= 0 || H <= 0 || W <= 0 || (terms != 1 && terms != 2)) return PP_EINVAL;
    if ((n > 0 && (!bank || !index || n_bank_rows <= 0)) || (n_front > 0 && !front)) return PP_EINVAL;
    if (((uintptr_t)out | (n > 0 ? (uintptr_t)bank : 0) | (n_front > 0 ? (uintptr_t)front : 0)) % 16 != 0) return PP_EINVAL;
    const long long hw = (long long)H * W, tiles = (hw + PO_TILE - 1) / PO_TILE;
    if (n + n_front > 65535 || hw > 0x7fffffff || tiles > 0x7fffffff) return PP_EINVAL;   // grid.y; 32-bit pixel indices
    hipLaunchKernelGGL(patch_operand_kernel, dim3((unsigned)tiles, n + n_front), dim3(256), 0, (hipStream_t)stream, bank, index, n_bank_rows,
                       front, n_front, (int)hw, (_Float16*)out, terms);
    return pp_last_launch();
}

int pp_flow_operand(const float* flow, int ld_flow, long long rows, void* out8, int terms, void* stream) {
    if (!flow || !out8 || rows <= 0 || ld_flow < 2 || ((uintptr_t)out8 % 16) != 0 || (terms != 1 && terms != 2)) return PP_EINVAL;
    if ((rows + 255) / 256 > 0x7fffffff) return PP_EINVAL;
    hipLaunchKernelGGL(flow_operand_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, (hipStream_t)stream, flow, ld_flow, rows,
                       (_Float16*)out8, terms);
    return pp_last_launch();
}

int pp_saturation_take(unsigned int* word, unsigned int* slot, void* stream) {
    if (!word || !slot) return PP_EINVAL;
    hipLaunchKernelGGL(saturation_take_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, word, slot);
    return pp_last_launch();
}

int pp_crop_resize_normalize(const unsigned char* image, int H, int W, const unsigned char* mask, int y1, int y2, int x1,
                             int x2, int S, int rgb_mask_flag, const double* mean3, const double* std3, float* out_rgb,
                             float* out_mask, void* stream) {
    if (!image || !out_rgb || !mean3 || !std3 || H <= 0 || W <= 0 || S <= 0 || y1 < 0 || x1 < 0 || y2 > H || x2 > W ||
        y2 <= y1 || x2 <= x1)
        return PP_EINVAL;
    hipLaunchKernelGGL(crop_resize_kernel, dim3((S * S + 255) / 256), dim3(256), 0, (hipStream_t)stream, image, W, mask, y1, y2,
                       x1, x2, S, rgb_mask_flag, mean3[0], mean3[1], mean3[2], std3[0], std3[1], std3[2], out_rgb, out_mask);
    return pp_last_launch();
}

int pp_depth_points_nearest(const float* depth_m, int H, int W, int y1, int y2, int x1, int x2, int P, float fx, float fy,
                            float cx, float cy, float* out_pts, void* stream) {
    if (!depth_m || !out_pts || H <= 0 || W <= 0 || P <= 0 || y1 < 0 || x1 < 0 || y2 > H || x2 > W || y2 <= y1 || x2 <= x1 ||
        fx == 0.f || fy == 0.f)
        return PP_EINVAL;
    hipLaunchKernelGGL(depth_points_kernel, dim3((P * P + 255) / 256), dim3(256), 0, (hipStream_t)stream, depth_m, W, y1, y2, x1,
                       x2, P, fx, fy, cx, cy, out_pts);
    return pp_last_launch();
}

int pp_conv_narrow_hl(const void* x_hl, int ld_x, int B, int H, int W, int C, const float* weight, const float* bias, int ksize,
                      int n_out, const float* residual, float* out, void* stream) {
    if (!x_hl || !weight || !out || B <= 0 || H <= 0 || C <= 0 || C % 32 != 0 || ld_x < C || ld_x % 8 != 0) return PP_EINVAL;
    if ((W != 16 && W != 32 && W != 64) || H % (256 / W) != 0 || (ksize != 1 && ksize != 3) || (n_out != 1 && n_out != 2)) return PP_EINVAL;
    if (((uintptr_t)x_hl % 16) != 0) return PP_EINVAL;
    const int TH = 256 / W, R = ksize / 2;
    const size_t lds = (size_t)(TH + 2 * R) * (W + 2 * R) * NRW_PITCH;
    const dim3 grid((unsigned)(B * (H / TH)));
    hipStream_t st = (hipStream_t)stream;
#define NRW_LAUNCH(KS_, N_)                                                                                                        \
    hipLaunchKernelGGL((conv_narrow_kernel<KS_, N_>), grid, dim3(256), lds, st, (const _Float16*)x_hl, ld_x, H, W, C, weight, bias, \
                       residual, out)
    if (ksize == 3 && n_out == 2) NRW_LAUNCH(3, 2);
    else if (ksize == 3) NRW_LAUNCH(3, 1);
    else if (n_out == 2) NRW_LAUNCH(1, 2);
    else NRW_LAUNCH(1, 1);
#undef NRW_LAUNCH
    return pp_last_launch();
}

}  // extern "C"
