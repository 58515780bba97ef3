// Training-pair assembly (provider/training_dataset.py:173-316): the gdrnpp colour augmentation executed from per-image
// programs, the 8-bit INTER_LINEAR resize + CLIP normalisation, and the full-frame depth conversions.
//
// The crop buffers hold 4-byte pixels (uchar4): the three colour bytes and the mask (real view) or alpha (template view)
// byte, so every access after the crop is one 4-byte vector.  Template frames arrive as RGBA (uchar4 too); real frames
// arrive as decoded, 3-byte RGB plus a mask frame, and only the pixels inside the box are read.  The host samples the programs and plans the passes (picopose_amd/provider/training_batch.py); the kernels
// only execute them.  Every op is integer, LUT-free fixed point or float32 with contraction off, so
// tests/train_batch_oracle.py restates each one bit for bit.
#include "pp_common.h"
#include "pp_reduce_dev.h"
#include "pp_hash_dev.h"             // aug_mix, aug_hash: the counter-based hash, shared with pp_synth.hip

#pragma clang fp contract(off)

namespace {

constexpr int OP_WORDS = PP_AUG_OP_WORDS, IMG_WORDS = PP_AUG_IMG_WORDS;
enum : int {
    OP_DROPOUT = 1, OP_BLUR = 2, OP_SHARPNESS = 3, OP_CONTRAST = 4, OP_BRIGHTNESS = 5, OP_COLOR = 6, OP_ADD = 7, OP_INVERT = 8,
    OP_MULTIPLY_PC = 9, OP_MULTIPLY = 10, OP_NOISE = 11, OP_LINEAR_CONTRAST = 12, OP_GRAYSCALE = 13
};

__device__ __forceinline__ int clamp255(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }
// PIL Image.blend on uint8 (and the LinearContrast LUT): clip(trunc(d + f (v - d))) in float32, one rounding per operation
__device__ __forceinline__ int blend_trunc(int d, int v, float f) {
    const float t = __fadd_rn((float)d, __fmul_rn(f, (float)(v - d)));
    return t <= 0.f ? 0 : (t >= 255.f ? 255 : (int)t);
}
__device__ __forceinline__ int pil_l(int c0, int c1, int c2) { return (c0 * 19595 + c1 * 38470 + c2 * 7471 + 0x8000) >> 16; }
__device__ __forceinline__ float rec_f(const int* r, int k) { return __int_as_float(r[k]); }

// BORDER_REFLECT_101 index (OpenCV borderInterpolate)
__device__ __forceinline__ int reflect101(int p, int n) {
    if (n == 1) return 0;
    while ((unsigned)p >= (unsigned)n) p = p < 0 ? -p : 2 * n - 2 - p;
    return p;
}

// one pointwise op on the three colour bytes of crop pixel (y, x)
__device__ __forceinline__ void pointwise(const int* r, int v[3], unsigned seed, int y, int x, int h, int w) {
    switch (r[0]) {
    case OP_DROPOUT: {
        const int gh = max(h * 5 / 100, 3), gw = max(w * 5 / 100, 3);
        const unsigned cell = (unsigned)((y * gh / h) * gw + x * gw / w);
        if (aug_hash(seed, cell, 0xd0u) < PP_AUG_DROP_THRESHOLD) v[0] = v[1] = v[2] = 0;
        break;
    }
    case OP_BRIGHTNESS:
        for (int c = 0; c < 3; ++c) v[c] = blend_trunc(0, v[c], rec_f(r, 1));
        break;
    case OP_COLOR: {
        const int l = pil_l(v[0], v[1], v[2]);
        for (int c = 0; c < 3; ++c) v[c] = blend_trunc(l, v[c], rec_f(r, 1));
        break;
    }
    case OP_ADD:
        for (int c = 0; c < 3; ++c) v[c] = clamp255(v[c] + r[1 + c]);
        break;
    case OP_INVERT:
        for (int c = 0; c < 3; ++c) v[c] = r[1 + c] ? 255 - v[c] : v[c];
        break;
    case OP_MULTIPLY_PC:
    case OP_MULTIPLY:
        for (int c = 0; c < 3; ++c) v[c] = clamp255((int)rintf(__fmul_rn((float)v[c], rec_f(r, 1 + c))));
        break;
    case OP_NOISE: {
        const unsigned p = (unsigned)(y * w + x);
        for (int c = 0; c < 3; ++c) {
            int s = 0;
            for (unsigned k = 0; k < 3; ++k) {
                const unsigned hh = aug_hash(seed, 3u * p + (unsigned)c, k);
                s += (int)(hh & 255u) + (int)((hh >> 8) & 255u) + (int)((hh >> 16) & 255u) + (int)(hh >> 24);
            }
            v[c] = clamp255(v[c] + (((2 * s - 12 * 255) * 10 + 256) >> 9));
        }
        break;
    }
    case OP_LINEAR_CONTRAST:
        for (int c = 0; c < 3; ++c) v[c] = blend_trunc(127, v[c], rec_f(r, 1 + c));
        break;
    case OP_GRAYSCALE: {
        const float a = rec_f(r, 1), b = __fsub_rn(1.f, a);
        const float g = (float)((v[0] * 4899 + v[1] * 9617 + v[2] * 1868 + 8192) >> 14);
        for (int c = 0; c < 3; ++c) v[c] = clamp255((int)rintf(__fadd_rn(__fmul_rn(a, g), __fmul_rn(b, (float)v[c]))));
        break;
    }
    default:
        break;  // neighbourhood / global ops only start a pass (the host plans it so)
    }
}

// One pass of the executor.  Block = one 16 x 16 tile of one image (the host's tile list of this pass).  Pass 0 crops the
// frame (channel flip fused) and runs the program's leading pointwise ops; pass p > 0 starts with the op that needed the
// whole previous image (blur, sharpness: neighbours of the stored pixels; contrast: the L sum of the stored image) and runs
// the pointwise ops up to the next such op.  A pass whose output feeds a Contrast adds the image's PIL-L values into lsum.
__global__ __launch_bounds__(256) void aug_pass_kernel(const unsigned char* __restrict__ rgb0, const unsigned char* __restrict__ mask0,
                                                       long long n_frame0, const uchar4* __restrict__ rgba1, long long n_frame1,
                                                       const int* __restrict__ images, int n_images,
                                                       const int* __restrict__ ops, int n_ops, const int4* __restrict__ tiles,
                                                       int pass, const uchar4* __restrict__ src, uchar4* __restrict__ dst,
                                                       long long n_buf, unsigned* __restrict__ lsum) {
    const int4 t = tiles[blockIdx.x];
    if (t.x < 0 || t.x >= n_images) return;
    const int* d = images + (size_t)t.x * IMG_WORDS;
    const int h = d[5], w = d[6], buf_off = d[7], op_off = d[9], nseg = d[10];
    const unsigned seed = (unsigned)d[8];
    if (pass >= nseg || nseg > PP_AUG_MAX_PASSES || h <= 0 || w <= 0 || buf_off < 0 || (long long)buf_off + (long long)h * w > n_buf)
        return;
    const int k0 = d[11 + pass], k1 = d[12 + pass];
    if (k0 < 0 || k1 < k0 || op_off < 0 || op_off + k1 > n_ops) return;
    const int* rec = ops + (size_t)op_off * OP_WORDS;
    const bool sums = pass + 1 < nseg && op_off + k1 < n_ops && rec[(size_t)k1 * OP_WORDS] == OP_CONTRAST;

    if (pass == 0) {
        const long long hi = (long long)d[1] + (long long)(d[3] + h - 1) * d[2] + d[4] + w;
        if (d[1] < 0 || d[3] < 0 || d[4] < 0 || d[4] + w > d[2] || hi > (d[0] ? n_frame1 : n_frame0)) return;
    }
    const int y = t.y + (int)(threadIdx.x >> 4), x = t.z + (int)(threadIdx.x & 15);
    const bool inside = y < h && x < w;
    int lval = 0;
    if (inside) {
        int v[3], m, k = k0;
        if (pass == 0) {
            const int fsel = d[0], foff = d[1], fw = d[2], y1 = d[3], x1 = d[4];
            const size_t px = (size_t)foff + (size_t)(y1 + y) * fw + (x1 + x);
            if (fsel) {
                const uchar4 q = rgba1[px];
                v[0] = q.z, v[1] = q.y, v[2] = q.x, m = q.w;  // image[..., ::-1]: the crop is BGR-ordered
            } else {  // 3-byte frames as decoded (read once, only inside the box) and the mask frame
                const unsigned char* q = rgb0 + 3 * px;
                v[0] = q[2], v[1] = q[1], v[2] = q[0], m = mask0[px];
            }
        } else {
            const uchar4* s = src + buf_off;
            const uchar4 q = s[(size_t)y * w + x];
            v[0] = q.x, v[1] = q.y, v[2] = q.z, m = q.w;
            const int* r = rec + (size_t)k * OP_WORDS;
            if (r[0] == OP_BLUR && r[1] > 0) {
                // OpenCV-style 8-bit Gaussian: quantised separable taps (sum 256 per axis), exact integer accumulation,
                // one rounding of the 16 fractional bits
                const int rad = min(r[1], 4);
                int acc[3] = {0, 0, 0};
                for (int i = -rad; i <= rad; ++i) {
                    const uchar4* row = s + (size_t)reflect101(y + i, h) * w;
                    int racc[3] = {0, 0, 0};
                    for (int j = -rad; j <= rad; ++j) {
                        const uchar4 p = row[reflect101(x + j, w)];
                        const int q2 = r[2 + abs(j)];
                        racc[0] += q2 * p.x, racc[1] += q2 * p.y, racc[2] += q2 * p.z;
                    }
                    const int q1 = r[2 + abs(i)];
                    for (int c = 0; c < 3; ++c) acc[c] += q1 * racc[c];
                }
                for (int c = 0; c < 3; ++c) v[c] = (acc[c] + 32768) >> 16;
            } else if (r[0] == OP_SHARPNESS) {
                // PIL ImageFilter.SMOOTH ([[1,1,1],[1,5,1],[1,1,1]] / 13, rounded) on the interior, border pixels copied
                int dg[3] = {v[0], v[1], v[2]};
                if (y > 0 && x > 0 && y < h - 1 && x < w - 1) {
                    int acc[3] = {4 * v[0], 4 * v[1], 4 * v[2]};
                    for (int i = -1; i <= 1; ++i)
                        for (int j = -1; j <= 1; ++j) {
                            const uchar4 p = s[(size_t)(y + i) * w + (x + j)];
                            acc[0] += p.x, acc[1] += p.y, acc[2] += p.z;
                        }
                    for (int c = 0; c < 3; ++c) dg[c] = (acc[c] + 6) / 13;
                }
                for (int c = 0; c < 3; ++c) v[c] = blend_trunc(dg[c], v[c], rec_f(r, 1));
            } else if (r[0] == OP_CONTRAST) {
                // PIL ImageEnhance.Contrast: degenerate = int(mean(L) + 0.5) of the whole image
                const int dg = (int)(__dadd_rn(__ddiv_rn((double)lsum[t.x], (double)h * (double)w), 0.5));
                for (int c = 0; c < 3; ++c) v[c] = blend_trunc(dg, v[c], rec_f(r, 1));
            }
            ++k;
        }
        for (; k < k1; ++k) pointwise(rec + (size_t)k * OP_WORDS, v, seed, y, x, h, w);
        dst[(size_t)buf_off + (size_t)y * w + x] = make_uchar4((unsigned char)v[0], (unsigned char)v[1], (unsigned char)v[2],
                                                               (unsigned char)m);
        lval = pil_l(v[0], v[1], v[2]);
    }
    if (sums) {  // uniform per block: integer sum, so exact and independent of the order of the adds
        const unsigned s = wave_sum((unsigned)lval);
        if ((threadIdx.x & 63) == 0 && s) atomicAdd(lsum + t.x, s);
    }
}

__device__ __forceinline__ int round_short(float v) { return (int)fminf(fmaxf(rintf(v), -32768.f), 32767.f); }

// cv::resize INTER_LINEAR of a uint8 crop (the fixed-point path: 11-bit coefficients, int horizontal pass, (v + 2^21) >> 22
// vertical), INTER_AREA for an exact 2x downscale, then / 255 and Normalize in double; INTER_NEAREST of the mask byte.
__global__ __launch_bounds__(256) void aug_resize_kernel(const uchar4* __restrict__ buf0, const uchar4* __restrict__ buf1,
                                                         long long n_buf, const int* __restrict__ images, int S, int mask_rgb,
                                                         double m0, double m1, double m2, double s0, double s1, double s2,
                                                         float* __restrict__ out_rgb, float* __restrict__ out_mask) {
    const int i = blockIdx.x * 256 + threadIdx.x, img = blockIdx.y;
    if (i >= S * S) return;
    const int* d = images + (size_t)img * IMG_WORDS;
    const int h = d[5], w = d[6], buf_off = d[7], nseg = d[10], alpha = d[16];
    if (h <= 0 || w <= 0 || buf_off < 0 || nseg < 1 || (long long)buf_off + (long long)h * w > n_buf) return;
    const uchar4* s = ((nseg - 1) & 1 ? buf1 : buf0) + buf_off;
    const int oy = i / S, ox = i - oy * S;
    auto px = [&](int yy, int xx, int c) -> int {
        const uchar4 q = s[(size_t)yy * w + xx];
        if (mask_rgb && q.w == 0) return 0;
        return c == 0 ? q.x : (c == 1 ? q.y : q.z);
    };
    int val[3];
    if (w == 2 * S && h == 2 * S) {
        for (int c = 0; c < 3; ++c)
            val[c] = (px(2 * oy, 2 * ox, c) + px(2 * oy, 2 * ox + 1, c) + px(2 * oy + 1, 2 * ox, c) + px(2 * oy + 1, 2 * ox + 1, c) + 2) >> 2;
    } else {
        float fx = (float)__dsub_rn(__dmul_rn((double)ox + 0.5, 1.0 / ((double)S / (double)w)), 0.5);
        int sx = (int)floorf(fx);
        fx = __fsub_rn(fx, (float)sx);
        if (sx < 0) fx = 0.f, sx = 0;
        if (sx >= w - 1) fx = 0.f, sx = w - 1;
        const int sx1 = min(sx + 1, w - 1);
        const int a0 = round_short(__fmul_rn(__fsub_rn(1.f, fx), 2048.f)), a1 = round_short(__fmul_rn(fx, 2048.f));
        float fy = (float)__dsub_rn(__dmul_rn((double)oy + 0.5, 1.0 / ((double)S / (double)h)), 0.5);
        const int sy = (int)floorf(fy);
        fy = __fsub_rn(fy, (float)sy);
        const int b0 = round_short(__fmul_rn(__fsub_rn(1.f, fy), 2048.f)), b1 = round_short(__fmul_rn(fy, 2048.f));
        const int r0 = min(max(sy, 0), h - 1), r1 = min(max(sy + 1, 0), h - 1);
        for (int c = 0; c < 3; ++c) {
            const int h0 = px(r0, sx, c) * a0 + px(r0, sx1, c) * a1, h1 = px(r1, sx, c) * a0 + px(r1, sx1, c) * a1;
            val[c] = clamp255((b0 * h0 + b1 * h1 + (1 << 21)) >> 22);
        }
    }
    const double mean[3] = {m0, m1, m2}, stdv[3] = {s0, s1, s2};
    float* o = out_rgb + (size_t)img * 3 * S * S + i;
    for (int c = 0; c < 3; ++c) o[(size_t)c * S * S] = (float)__ddiv_rn(__dsub_rn((double)val[c] / 255.0, mean[c]), stdv[c]);
    const int ny = min((int)floor(__dmul_rn((double)oy, 1.0 / ((double)S / (double)h))), h - 1);
    const int nx = min((int)floor(__dmul_rn((double)ox, 1.0 / ((double)S / (double)w))), w - 1);
    const int m = s[(size_t)ny * w + nx].w;
    out_mask[(size_t)img * S * S + i] = alpha ? (m == 255 ? 1.f : 0.f) : (float)m;
}

// real depth: f32(d) * f32(depth_scale) / 1000 in float32; four pixels (8 bytes in, 16 out) per lane
__global__ __launch_bounds__(256) void depth_scaled_kernel(const unsigned short* __restrict__ dep, long long n_per, int n_frames,
                                                           const float* __restrict__ scale, float* __restrict__ out) {
    const long long i = ((long long)blockIdx.x * 256 + threadIdx.x) * 4, n = n_per * n_frames;
    if (i >= n) return;
    if ((n_per & 3) == 0) {
        const ushort4 q = *(const ushort4*)(dep + i);
        const float sc = scale[i / n_per];
        *(float4*)(out + i) = make_float4(__fdiv_rn(__fmul_rn((float)q.x, sc), 1000.f), __fdiv_rn(__fmul_rn((float)q.y, sc), 1000.f),
                                          __fdiv_rn(__fmul_rn((float)q.z, sc), 1000.f), __fdiv_rn(__fmul_rn((float)q.w, sc), 1000.f));
    } else {
        for (long long j = i; j < i + 4 && j < n; ++j) out[j] = __fdiv_rn(__fmul_rn((float)dep[j], scale[j / n_per]), 1000.f);
    }
}

// template depth: (float)(d * 0.1 / 1000.0) in double
__global__ __launch_bounds__(256) void depth_template_kernel(const unsigned short* __restrict__ dep, long long n,
                                                             float* __restrict__ out) {
    const long long i = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i >= n) return;
    auto cv = [](unsigned short v) { return (float)__ddiv_rn(__dmul_rn((double)v, 0.1), 1000.0); };
    if (i + 4 <= n) {
        const ushort4 q = *(const ushort4*)(dep + i);
        *(float4*)(out + i) = make_float4(cv(q.x), cv(q.y), cv(q.z), cv(q.w));
    } else {
        for (long long j = i; j < n; ++j) out[j] = cv(dep[j]);
    }
}

}  // namespace

extern "C" {

int pp_augment_execute(const unsigned char* rgb0, const unsigned char* mask0, long long n_frame0_px, const unsigned char* rgba1,
                       long long n_frame1_px,
                       const int* images, int n_images, const int* ops, int n_ops, const int* tiles, const int* pass_tiles,
                       int n_passes, unsigned char* buf0, unsigned char* buf1, long long n_buf_px, unsigned int* lsum,
                       void* stream) {
    if (!rgb0 || !mask0 || !rgba1 || !images || !ops || !tiles || !pass_tiles || !buf0 || !buf1 || !lsum || n_images <= 0 ||
        n_ops <= 0 || n_passes < 1 || n_passes > PP_AUG_MAX_PASSES || n_frame0_px <= 0 || n_frame1_px <= 0 || n_buf_px <= 0)
        return PP_EINVAL;
    if (((uintptr_t)rgba1 | (uintptr_t)buf0 | (uintptr_t)buf1) % 4 != 0) return PP_EINVAL;
    if (pass_tiles[0] != 0 || pass_tiles[1] <= 0) return PP_EINVAL;
    for (int p = 0; p < n_passes; ++p)
        if (pass_tiles[p + 1] < pass_tiles[p]) return PP_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    PP_CHECK_HIP(hipMemsetAsync(lsum, 0, sizeof(unsigned) * (size_t)n_images, st));
    for (int p = 0; p < n_passes; ++p) {
        const int nt = pass_tiles[p + 1] - pass_tiles[p];
        if (nt == 0) continue;
        const uchar4* src = (const uchar4*)(p & 1 ? buf0 : buf1);
        uchar4* dst = (uchar4*)(p & 1 ? buf1 : buf0);
        hipLaunchKernelGGL(aug_pass_kernel, dim3(nt), dim3(256), 0, st, rgb0, mask0, n_frame0_px, (const uchar4*)rgba1, n_frame1_px, images, n_images, ops, n_ops,
                           (const int4*)tiles + pass_tiles[p], p, src, dst, n_buf_px, lsum);
        const int rc = pp_last_launch();
        if (rc != PP_OK) return rc;
    }
    return PP_OK;
}

int pp_augment_resize(const unsigned char* buf0, const unsigned char* buf1, long long n_buf_px, const int* images, int n_images,
                      int S, int rgb_mask_flag, const double* mean3, const double* std3, float* out_rgb, float* out_mask,
                      void* stream) {
    if (!buf0 || !buf1 || !images || !mean3 || !std3 || !out_rgb || !out_mask || n_images <= 0 || n_images > 65535 || S <= 0 ||
        S > 4096 || n_buf_px <= 0)
        return PP_EINVAL;
    hipLaunchKernelGGL(aug_resize_kernel, dim3((S * S + 255) / 256, n_images), dim3(256), 0, (hipStream_t)stream,
                       (const uchar4*)buf0, (const uchar4*)buf1, n_buf_px, images, S, rgb_mask_flag, mean3[0], mean3[1], mean3[2],
                       std3[0], std3[1], std3[2], out_rgb, out_mask);
    return pp_last_launch();
}

int pp_depth_u16_scaled(const unsigned short* depth, long long n_per_frame, int n_frames, const float* scale, float* out,
                        void* stream) {
    if (!depth || !scale || !out || n_per_frame <= 0 || n_frames <= 0) return PP_EINVAL;
    if (((uintptr_t)depth % 8) != 0 || ((uintptr_t)out % 16) != 0) return PP_EINVAL;
    const long long n4 = (n_per_frame * n_frames + 3) / 4;
    hipLaunchKernelGGL(depth_scaled_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, depth,
                       n_per_frame, n_frames, scale, out);
    return pp_last_launch();
}

int pp_depth_u16_template(const unsigned short* depth, long long n, float* out, void* stream) {
    if (!depth || !out || n <= 0) return PP_EINVAL;
    if (((uintptr_t)depth % 8) != 0 || ((uintptr_t)out % 16) != 0) return PP_EINVAL;
    const long long n4 = (n + 3) / 4;
    hipLaunchKernelGGL(depth_template_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, depth, n, out);
    return pp_last_launch();
}

}  // extern "C"
