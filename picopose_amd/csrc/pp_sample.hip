// Sampling kernels of stage 3 (NHWC): bilinear resize (align_corners=True), the feature warp
// (grid_sample, zeros padding), the pools of the correlation pyramid (its lookup: pp_corr.hip), gathers, crops, narrow convolutions, operand builders.

#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/picopose_hip.h"
#include "pp_common.h"
#include "pp_corr_dev.h"
#include "pp_crop_dev.h"

namespace {

typedef float f4 __attribute__((ext_vector_type(4)));
typedef _Float16 h8_t __attribute__((ext_vector_type(8)));

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
    const float ix = fminf(fmaxf(pp_roundtrip((float)x + fl[0], W), -2.f), (float)W + 1.f);
    const float iy = fminf(fmaxf(pp_roundtrip((float)y + fl[1], H), -2.f), (float)H + 1.f);
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
