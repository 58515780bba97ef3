// The scene composite ("THE SCENE COMPOSITE" of include/picopose_hip.h; picopose_amd/provider/synth_scenes.py plans every call and
// tests/synth_oracle.py restates the contract in numpy): rendered object layers over a background -> the colour frame, the 16-bit
// depth, the instance map and, per layer, the covered and won pixel counts, the box of the won pixels and the visible mask.
//
//   scene_composite_kernel<VEC>  one workgroup per PP_SYNTH_TILE consecutive pixels of one image, four pixels per lane (VEC: four
//                            neighbours, 16-byte loads and stores; otherwise pixels 256 apart, one per access).  Pass 1 walks the
//                            image's layers — the range is uniform over the workgroup — keeping per pixel the winner (bits of Z, l);
//                            pass 2 writes the pixel's outputs, then walks the layers again for the masks and the won pixels.  Counts
//                            come from ballots, extrema from xor-shuffles; lane 0 of every wave puts them into LDS and, per 32 layers,
//                            the workgroup writes one record of six integers per layer into the workspace.
//   scene_finish_kernel      one wave per layer: the layer's records in a fixed order -> counts and boxes ({0, 0, -1, -1} when empty)
//   depth_quantize_kernel    pp_depth_quantize_u16
//
// A streaming pass: 4 B per layer sample (the depth), 4 B per won pixel (the winner's colour, gathered after pass 1 instead of reading
// every layer's), 9 B per pixel written, plus the masks.  No atomics, no scratch, no floating-point reduction.
#include <stdint.h>
#include <limits.h>
#include <math.h>
#include "pp_common.h"
#include "pp_reduce_dev.h"
#include "pp_hash_dev.h"

#pragma clang fp contract(off)

namespace {

constexpr int BLOCK = 256;
constexpr int WAVES = BLOCK / 64;
constexpr int PX = 4;                          // pixels per lane
constexpr int TILE = PP_SYNTH_TILE;            // pixels per workgroup
constexpr int LCH = 32;                        // layers per LDS flush
constexpr int REC = 6;                         // px_all, px_visib, x_min, y_min, x_max, y_max
static_assert(TILE == BLOCK * PX, "a workgroup's tile is four pixels per lane");

struct Composite {
    const unsigned char* rgba;                 // (L, H, W, 4)
    const float* z;                            // (L, H, W)
    const int* layer_off;                      // (n_images + 1)
    const int* background;                     // (n_images, 4)
    const unsigned char* bg_images;            // (n_images, H, W, 3) or null
    const float* depth_scale;                  // (n_images)
    int* records;                              // (L, chunks, REC)
    unsigned char* rgb;                        // (n_images, H, W, 3)
    unsigned short* depth;                     // (n_images, H, W)
    int* instance;                             // (n_images, H, W)
    unsigned char* mask;                       // (L, H, W) or null
    int H, W, chunks;
};

// channel c of the lattice background at (x, y): integer bilinear blend of the four hashed node colours
__device__ __forceinline__ unsigned lattice_rgb(unsigned seed, int s, int x, int y) {
    const int S = 1 << s, fx = x & (S - 1), fy = y & (S - 1);
    const unsigned gx = (unsigned)(x >> s), gy = (unsigned)(y >> s);
    const unsigned n00 = aug_hash(seed, gx, gy), n10 = aug_hash(seed, gx + 1, gy), n01 = aug_hash(seed, gx, gy + 1),
                   n11 = aug_hash(seed, gx + 1, gy + 1);
    const int w00 = (S - fx) * (S - fy), w10 = fx * (S - fy), w01 = (S - fx) * fy, w11 = fx * fy, half = 1 << (2 * s - 1);
    unsigned out = 0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int v = (int)((n00 >> (8 * c)) & 255u) * w00 + (int)((n10 >> (8 * c)) & 255u) * w10 + (int)((n01 >> (8 * c)) & 255u) * w01 +
                      (int)((n11 >> (8 * c)) & 255u) * w11;
        out |= (unsigned)((v + half) >> (2 * s)) << (8 * c);
    }
    return out;
}

__device__ __forceinline__ unsigned short quantize(float z, float scale) {
    const float q = rintf(__fdiv_rn(__fmul_rn(1000.0f, z), scale));
    return (unsigned short)(int)fminf(65535.f, q);
}

template <bool VEC>
__global__ __launch_bounds__(BLOCK) void scene_composite_kernel(Composite a) {
    __shared__ int sm_all[WAVES][LCH];
    __shared__ int sm_vis[WAVES][LCH][REC - 1];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int img = blockIdx.x / a.chunks, chunk = blockIdx.x - img * a.chunks;
    const int hw = a.H * a.W;                                      // (< 2^31, checked by the entry)
    const int l0 = a.layer_off[img], l1 = a.layer_off[img + 1];    // uniform: every lane walks the same layers
    unsigned p[PX];                                                // (unsigned: the last tile may reach past 2^31 - 1)
    bool in[PX];
#pragma unroll
    for (int j = 0; j < PX; ++j) {
        p[j] = (unsigned)chunk * TILE + (unsigned)(VEC ? PX * tid + j : BLOCK * j + tid);
        in[j] = p[j] < (unsigned)hw;
    }

    // ---- pass 1: the winner of every pixel; px_all of every layer
    unsigned zbest[PX];
    int lbest[PX];
#pragma unroll
    for (int j = 0; j < PX; ++j) zbest[j] = 0xFFFFFFFFu, lbest[j] = -1;
    for (int c0 = l0; c0 < l1; c0 += LCH) {
        const int c1 = c0 + LCH < l1 ? c0 + LCH : l1;
        for (int l = c0; l < c1; ++l) {
            const float* zl = a.z + (size_t)l * hw;
            float z[PX];
            if (VEC) {
                const float4 v = in[0] ? *reinterpret_cast<const float4*>(zl + p[0]) : make_float4(0.f, 0.f, 0.f, 0.f);
                z[0] = v.x, z[1] = v.y, z[2] = v.z, z[3] = v.w;
            } else {
#pragma unroll
                for (int j = 0; j < PX; ++j) z[j] = in[j] ? zl[p[j]] : 0.f;
            }
            int n = 0;
#pragma unroll
            for (int j = 0; j < PX; ++j) {
                const bool cover = z[j] > 0.f;                     // false for NaN, negatives and +-0
                const unsigned bits = __float_as_uint(z[j]);
                if (cover && bits < zbest[j]) zbest[j] = bits, lbest[j] = l;      // l ascends: on equal depth the lower l stays
                n += __popcll(__ballot(cover));
            }
            if (lane == 0) sm_all[wave][l - c0] = n;
        }
        __syncthreads();
        if (tid < c1 - c0) {
            int n = 0;
#pragma unroll
            for (int q = 0; q < WAVES; ++q) n += sm_all[q][tid];
            a.records[((size_t)(c0 + tid) * a.chunks + chunk) * REC] = n;
        }
        __syncthreads();                                           // sm_all is reused by the next 32 layers
    }

    // ---- the pixel's outputs
    int x[PX], y[PX];
    if (VEC) {
        const int yy = (int)(p[0] / (unsigned)a.W), xx = (int)(p[0] - (unsigned)yy * a.W);    // W % 4 == 0: the four share the row
#pragma unroll
        for (int j = 0; j < PX; ++j) x[j] = xx + j, y[j] = yy;
    } else {
#pragma unroll
        for (int j = 0; j < PX; ++j) y[j] = (int)(p[j] / (unsigned)a.W), x[j] = (int)(p[j] - (unsigned)y[j] * a.W);
    }
    const int* bgd = a.background + PP_SYNTH_BG_WORDS * (size_t)img;
    const int3 bg = make_int3(bgd[0], bgd[1], bgd[2]);             // {mode, a, b}
    const float scale = a.depth_scale[img];
    const size_t base = (size_t)img * hw;
    unsigned col[PX] = {0u, 0u, 0u, 0u};
    unsigned short dq[PX];
    if (VEC && lbest[0] >= 0 && lbest[0] == lbest[1] && lbest[0] == lbest[2] && lbest[0] == lbest[3]) {
        const uint4 v = *reinterpret_cast<const uint4*>(a.rgba + ((size_t)lbest[0] * hw + p[0]) * 4);
        col[0] = v.x, col[1] = v.y, col[2] = v.z, col[3] = v.w;
    } else {
#pragma unroll
        for (int j = 0; j < PX; ++j)
            if (lbest[j] >= 0) {
                const unsigned char* c = a.rgba + ((size_t)lbest[j] * hw + p[j]) * 4;
                col[j] = VEC ? *reinterpret_cast<const unsigned*>(c) : ((unsigned)c[0] | (unsigned)c[1] << 8 | (unsigned)c[2] << 16);
            }
    }
#pragma unroll
    for (int j = 0; j < PX; ++j) {
        dq[j] = 0;
        if (lbest[j] >= 0) {
            dq[j] = quantize(__uint_as_float(zbest[j]), scale);
        } else if (in[j]) {
            if (bg.x == 0) {
                col[j] = (unsigned)bg.y;
            } else if (bg.x == 1) {
                const unsigned char* b = a.bg_images + (base + p[j]) * 3;
                col[j] = (unsigned)b[0] | (unsigned)b[1] << 8 | (unsigned)b[2] << 16;
            } else {
                col[j] = lattice_rgb((unsigned)bg.y, bg.z, x[j], y[j]);
            }
        }
    }
    if (VEC) {
        if (in[0]) {
            // twelve colour bytes of four pixels = three 32-bit words
            const unsigned c0 = col[0] & 0xFFFFFFu, c1 = col[1] & 0xFFFFFFu, c2 = col[2] & 0xFFFFFFu, c3 = col[3] & 0xFFFFFFu;
            unsigned* o = reinterpret_cast<unsigned*>(a.rgb + (base + p[0]) * 3);
            o[0] = c0 | c1 << 24, o[1] = c1 >> 8 | c2 << 16, o[2] = c2 >> 16 | c3 << 8;
            *reinterpret_cast<uint2*>(a.depth + base + p[0]) = make_uint2((unsigned)dq[0] | (unsigned)dq[1] << 16,
                                                                            (unsigned)dq[2] | (unsigned)dq[3] << 16);
            *reinterpret_cast<int4*>(a.instance + base + p[0]) = make_int4(lbest[0], lbest[1], lbest[2], lbest[3]);
        }
    } else {
#pragma unroll
        for (int j = 0; j < PX; ++j)
            if (in[j]) {
                unsigned char* o = a.rgb + (base + p[j]) * 3;
                o[0] = (unsigned char)col[j], o[1] = (unsigned char)(col[j] >> 8), o[2] = (unsigned char)(col[j] >> 16);
                a.depth[base + p[j]] = dq[j];
                a.instance[base + p[j]] = lbest[j];
            }
    }

    // ---- pass 2: per layer the mask, px_visib and the box of the won pixels
    for (int c0 = l0; c0 < l1; c0 += LCH) {
        const int c1 = c0 + LCH < l1 ? c0 + LCH : l1;
        for (int l = c0; l < c1; ++l) {
            bool won[PX];
            int n = 0;
#pragma unroll
            for (int j = 0; j < PX; ++j) {
                won[j] = lbest[j] == l;
                n += __popcll(__ballot(won[j]));
            }
            if (a.mask) {
                unsigned char* m = a.mask + (size_t)l * hw;
                if (VEC) {
                    if (in[0])
                        *reinterpret_cast<unsigned*>(m + p[0]) =
                            (won[0] ? 0xFFu : 0u) | (won[1] ? 0xFF00u : 0u) | (won[2] ? 0xFF0000u : 0u) | (won[3] ? 0xFF000000u : 0u);
                } else {
#pragma unroll
                    for (int j = 0; j < PX; ++j)
                        if (in[j]) m[p[j]] = won[j] ? 255 : 0;
                }
            }
            int e[4] = {INT_MAX, INT_MAX, INT_MIN, INT_MIN};
            if (n > 0) {                                           // uniform over the wave: n comes from ballots
#pragma unroll
                for (int j = 0; j < PX; ++j)
                    if (won[j]) e[0] = min(e[0], x[j]), e[1] = min(e[1], y[j]), e[2] = max(e[2], x[j]), e[3] = max(e[3], y[j]);
                wave_reduce_each(e, [](int c, int p, int q) { return c < 2 ? min(p, q) : max(p, q); });
            }
            if (lane == 0) {
                int* r = sm_vis[wave][l - c0];
                r[0] = n, r[1] = e[0], r[2] = e[1], r[3] = e[2], r[4] = e[3];
            }
        }
        __syncthreads();
        if (tid < (c1 - c0) * (REC - 1)) {
            const int k = tid / (REC - 1), c = tid - k * (REC - 1);
            int v = sm_vis[0][k][c];
#pragma unroll
            for (int q = 1; q < WAVES; ++q) {
                const int w = sm_vis[q][k][c];
                v = c == 0 ? v + w : (c < 3 ? min(v, w) : max(v, w));
            }
            a.records[((size_t)(c0 + k) * a.chunks + chunk) * REC + 1 + c] = v;
        }
        __syncthreads();                                           // sm_vis is reused by the next 32 layers
    }
}

// one wave per layer: lane q folds records q, q + 64, ... in that order, then xor-shuffles; sums and extrema of integers
__global__ __launch_bounds__(64) void scene_finish_kernel(const int* __restrict__ records, int chunks, int* __restrict__ counts,
                                                          int* __restrict__ boxes) {
    const int l = blockIdx.x, lane = threadIdx.x;
    int v[REC] = {0, 0, INT_MAX, INT_MAX, INT_MIN, INT_MIN};
    for (int k = lane; k < chunks; k += 64) {
        const int* r = records + ((size_t)l * chunks + k) * REC;
        v[0] += r[0], v[1] += r[1];
        v[2] = min(v[2], r[2]), v[3] = min(v[3], r[3]), v[4] = max(v[4], r[4]), v[5] = max(v[5], r[5]);
    }
    wave_reduce_each(v, [](int c, int p, int q) { return c < 2 ? p + q : (c < 4 ? min(p, q) : max(p, q)); });
    if (lane == 0) {
        counts[2 * (size_t)l] = v[0], counts[2 * (size_t)l + 1] = v[1];
        const bool empty = v[1] == 0;
        int* b = boxes + 4 * (size_t)l;
        b[0] = empty ? 0 : v[2], b[1] = empty ? 0 : v[3], b[2] = empty ? -1 : v[4], b[3] = empty ? -1 : v[5];
    }
}

__global__ __launch_bounds__(BLOCK) void depth_quantize_kernel(const float* __restrict__ z, long long n, float units, int vec,
                                                              unsigned short* __restrict__ out) {
    const long long stride = (long long)gridDim.x * BLOCK, t = (long long)blockIdx.x * BLOCK + threadIdx.x;
    const long long groups = vec ? n / 4 : 0;
    for (long long g = t; g < groups; g += stride) {
        const float4 v = reinterpret_cast<const float4*>(z)[g];
        const float q[4] = {v.x, v.y, v.z, v.w};
        unsigned u[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) u[j] = q[j] > 0.f ? (unsigned)(int)fminf(65535.f, rintf(__fmul_rn(units, q[j]))) : 0u;
        reinterpret_cast<uint2*>(out)[g] = make_uint2(u[0] | u[1] << 16, u[2] | u[3] << 16);
    }
    for (long long i = groups * 4 + t; i < n; i += stride)        // the tail, or everything when a buffer is not aligned
        out[i] = z[i] > 0.f ? (unsigned short)(int)fminf(65535.f, rintf(__fmul_rn(units, z[i]))) : (unsigned short)0;
}

inline int tile_chunks(int H, int W) { return (int)(((long long)H * W + TILE - 1) / TILE); }

}  // namespace

extern "C" {

int pp_scene_composite_workspace_bytes(int n_layers, int H, int W, size_t* bytes) {
    if (!bytes || n_layers < 0 || H <= 0 || W <= 0 || (long long)H * W >= (1ll << 31) ||
        (long long)n_layers * H * W >= (1ll << 31))
        return PP_EINVAL;
    *bytes = align256((size_t)n_layers * tile_chunks(H, W) * REC * sizeof(int));
    return PP_OK;
}

int pp_scene_composite(const unsigned char* layers_rgba, const float* layers_depth, const int* layer_off, const int* layer_off_host,
                       int n_layers, int n_images, int H, int W, const int* background, const int* background_host,
                       const unsigned char* bg_images, const float* depth_scale, const float* depth_scale_host, void* workspace,
                       size_t workspace_bytes, unsigned char* rgb, unsigned short* depth, int* instance, int* counts, int* boxes,
                       unsigned char* mask_visib, void* stream) {
    if (!layer_off || !layer_off_host || !background || !background_host || !depth_scale || !depth_scale_host || !rgb || !depth ||
        !instance)
        return PP_EINVAL;
    if (n_images <= 0 || H <= 0 || W <= 0 || n_layers < 0) return PP_EINVAL;
    if (n_layers > 0 && (!layers_rgba || !layers_depth || !counts || !boxes)) return PP_EINVAL;
    if ((long long)n_layers * H * W >= (1ll << 31) || (long long)n_images * H * W >= (1ll << 31)) return PP_EINVAL;
    if (layer_off_host[0] != 0 || layer_off_host[n_images] != n_layers) return PP_EINVAL;
    for (int i = 0; i < n_images; ++i) {
        if (layer_off_host[i + 1] < layer_off_host[i]) return PP_EINVAL;
        if (!positive_finite(depth_scale_host[i])) return PP_EINVAL;
        const int* d = background_host + PP_SYNTH_BG_WORDS * (size_t)i;
        if (d[0] < 0 || d[0] > 2) return PP_EINVAL;
        if (d[0] == 1 && !bg_images) return PP_EINVAL;
        if (d[0] == 2 && (d[2] < 2 || d[2] > 7)) return PP_EINVAL;
    }
    size_t need = 0;
    if (pp_scene_composite_workspace_bytes(n_layers, H, W, &need) != PP_OK) return PP_EINVAL;
    if (need > 0 && (!workspace || ((uintptr_t)workspace % 256) != 0 || workspace_bytes < need)) return PP_EWORKSPACE;

    hipStream_t st = (hipStream_t)stream;
    const int chunks = tile_chunks(H, W);
    const Composite a{layers_rgba, layers_depth, layer_off, background, bg_images, depth_scale, (int*)workspace, rgb, depth, instance,
                      mask_visib, H, W, chunks};
    const uintptr_t bits = (uintptr_t)layers_rgba | (uintptr_t)layers_depth | (uintptr_t)rgb | (uintptr_t)depth | (uintptr_t)instance |
                           (uintptr_t)mask_visib;
    const bool vec = W % 4 == 0 && bits % 16 == 0;
    const dim3 grid((unsigned)((long long)n_images * chunks));     // n_images H W < 2^31: at most 2^21 workgroups
    if (vec)
        hipLaunchKernelGGL(scene_composite_kernel<true>, grid, dim3(BLOCK), 0, st, a);
    else
        hipLaunchKernelGGL(scene_composite_kernel<false>, grid, dim3(BLOCK), 0, st, a);
    if (n_layers > 0)
        hipLaunchKernelGGL(scene_finish_kernel, dim3((unsigned)n_layers), dim3(64), 0, st, (const int*)workspace, chunks, counts, boxes);
    return pp_last_launch();
}

int pp_depth_quantize_u16(const float* depth_m, long long n, float units_per_metre, unsigned short* out, void* stream) {
    if (!depth_m || !out || n < 0 || !positive_finite(units_per_metre)) return PP_EINVAL;
    if (n == 0) return PP_OK;
    const int vec = (uintptr_t)depth_m % 16 == 0 && (uintptr_t)out % 8 == 0;
    const long long per = (n + BLOCK * 4 - 1) / (BLOCK * 4);
    hipLaunchKernelGGL(depth_quantize_kernel, dim3((unsigned)(per < 4096 ? per : 4096)), dim3(BLOCK), 0, (hipStream_t)stream, depth_m, n,
                       units_per_metre, vec, out);
    return pp_last_launch();
}

}  // extern "C"
