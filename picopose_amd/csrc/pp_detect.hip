// Detection batch of one test image (provider/bop_test_dataset.py:112-207): every kept detection's crop, resize and CLIP
// normalisation in one launch, with the mask read from its COCO run lengths — no frame-sized mask exists anywhere.
//
// The frame is uploaded once; a detection is its crop window and a slice of `run_ends`, the cumulative ends of its runs over
// the column-major (h, w) mask.  Source pixel (y, x) lies in the mask when an odd number of ends are <= x * H + y.
// The pixel arithmetic is crop_resize_kernel's (pp_sample.hip), operation for operation: the outputs are bit-equal to
// pp_crop_resize_normalize on the decoded mask (tests/test_test_batch_gpu.py).
#include <stdint.h>
#include <limits.h>
#include "pp_common.h"
#include "pp_runs_dev.h"

namespace {

constexpr int TILE = 16;           // output tile of TILE x TILE pixels, one thread each
constexpr int SLICE = 2048;        // run ends a workgroup stages in LDS (8 KB); longer slices are searched in global memory

// Wave-wide search: the number of ends[a..b) that are < key (upper = false) or <= key (upper = true), plus a.  Each round
// 64 lanes probe evenly spaced elements, a ballot counts the prefix that passes, and the range shrinks 64-fold: two rounds
// for 4096 runs where a one-lane bisection takes twelve dependent loads.  Call with all 64 lanes active.
__device__ __forceinline__ int wave_bound(const int* __restrict__ ends, int a, int b, int key, bool upper, int lane) {
    while (a < b) {
        const int step = (b - a + 63) >> 6;
        const long long q = (long long)a + (long long)(lane + 1) * step - 1;
        bool pass = false;
        if (q < b) {
            const int v = ends[q];
            pass = upper ? v <= key : v < key;
        }
        const int cnt = __popcll(__ballot(pass));
        const long long na = (long long)a + (long long)cnt * step, nb = na + step - 1;
        a = (int)na;
        b = nb < b ? (int)nb : b;
    }
    return a;
}

__global__ __launch_bounds__(TILE * TILE) void detections_crop_kernel(
    const unsigned char* __restrict__ img, int H, int W, const int* __restrict__ run_ends, int n_runs,
    const int* __restrict__ run_offset, const int* __restrict__ window, int S, int mask_rgb, double m0, double m1, double m2,
    double s0, double s1, double s2, float* __restrict__ out_rgb, float* __restrict__ out_mask) {
    __shared__ int slice[SLICE];
    __shared__ int bounds[2];
    const int det = blockIdx.y, tid = threadIdx.x, lane = tid & 63;
    const int ntx = (S + TILE - 1) / TILE;
    const int tx0 = (blockIdx.x % ntx) * TILE, ty0 = (blockIdx.x / ntx) * TILE;
    const int y1 = window[det * 4], y2 = window[det * 4 + 1], x1 = window[det * 4 + 2], x2 = window[det * 4 + 3];
    int r0, r1;
    // the host entry validated its copies of both tables; a device copy that disagrees must not lead outside the buffers
    if (!pp_run_slice(run_offset, det, n_runs, r0, r1) || y1 < 0 || x1 < 0 || y2 > H || x2 > W || y2 <= y1 || x2 <= x1) return;
    const int h = y2 - y1, w = x2 - x1;
    auto taps = [](int o, int n, int S_, int& i0, int& i1, double& fr) {
        const double f = ((double)o + 0.5) * ((double)n / (double)S_) - 0.5;
        i0 = (int)floor(f);
        fr = f - (double)i0;
        if (i0 < 0) {
            i0 = 0;
            fr = 0.0;
        }
        if (i0 >= n - 1) {
            i0 = n - 1;
            fr = 0.0;
        }
        i1 = i0 + 1 < n ? i0 + 1 : n - 1;
    };
    auto nearest = [](int o, int n, int S_) {
        const int i = (int)floor((double)o * ((double)n / (double)S_));
        return i < n - 1 ? i : n - 1;
    };

    // ---- the tile's source columns -> the runs that touch them: [lo, hi) of this detection's ends
    const int txl = min(tx0 + TILE, S) - 1;
    int c_lo = nearest(tx0, w, S), c_hi = nearest(txl, w, S);
    if (mask_rgb) {
        int a, b;
        double f;
        taps(tx0, w, S, a, b, f);
        c_lo = min(c_lo, a);
        taps(txl, w, S, a, b, f);
        c_hi = max(c_hi, b);
    }
    const int p_lo = (x1 + c_lo) * H, p_hi = (x1 + c_hi) * H + (H - 1);     // < H * W <= INT_MAX (checked by the entry)
    if (tid < 128) {                                                          // waves 0 and 1, one search each
        const int v = tid < 64 ? wave_bound(run_ends, r0, r1, p_lo, false, lane) : wave_bound(run_ends, r0, r1, p_hi, true, lane);
        if (lane == 0) bounds[tid >> 6] = v;
    }
    __syncthreads();
    const int lo = bounds[0], hi = bounds[1], m = hi - lo;
    const bool staged = m <= SLICE;                                           // uniform over the workgroup
    if (staged)
        for (int k = tid; k < m; k += TILE * TILE) slice[k] = run_ends[lo + k];
    __syncthreads();
    const int* ends = staged ? slice : run_ends + lo;
    const int par0 = (lo - r0) & 1;                                           // runs wholly before the tile's columns
    auto inside = [&](int yy, int xx) -> bool { return ((par0 + pp_count_le(ends, m, (x1 + xx) * H + (y1 + yy))) & 1) != 0; };

    const int oy = ty0 + tid / TILE, ox = tx0 + tid % TILE;
    if (oy >= S || ox >= S) return;
    const int i = oy * S + ox;
    int ya, yb, xa, xb;
    double fy, fx;
    taps(oy, h, S, ya, yb, fy);
    taps(ox, w, S, xa, xb, fx);
    bool in_aa = true, in_ab = true, in_ba = true, in_bb = true;
    if (mask_rgb) {
        in_aa = inside(ya, xa);
        in_ab = inside(ya, xb);
        in_ba = inside(yb, xa);
        in_bb = inside(yb, xb);
    }
    const double mean[3] = {m0, m1, m2}, stdv[3] = {s0, s1, s2};
    auto px = [&](int yy, int xx, int c, bool in) -> double {   // channel c of the flipped ([..., ::-1]) crop, / 255, optionally masked
        const size_t p = (size_t)(y1 + yy) * W + (x1 + xx);
        double v = (double)img[p * 3 + (2 - c)] / 255.0;
        if (!in) v = 0.0;
        return v;
    };
    const size_t plane = (size_t)S * S;
    float* rgb = out_rgb + (size_t)det * 3 * plane;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double top = px(ya, xa, c, in_aa) * (1.0 - fx) + px(ya, xb, c, in_ab) * fx;
        const double bot = px(yb, xa, c, in_ba) * (1.0 - fx) + px(yb, xb, c, in_bb) * fx;
        rgb[(size_t)c * plane + i] = (float)(((top * (1.0 - fy) + bot * fy) - mean[c]) / stdv[c]);
    }
    out_mask[(size_t)det * plane + i] = inside(nearest(oy, h, S), nearest(ox, w, S)) ? 1.f : 0.f;
}

}  // namespace

extern "C" {

int pp_detections_crop(const unsigned char* image, int H, int W, const int* run_ends, int n_runs, const int* run_offset,
                       const int* window, const int* run_offset_host, const int* window_host, int n, int S, int rgb_mask_flag,
                       const double* mean3, const double* std3, float* out_rgb, float* out_mask, void* stream) {
    if (!image || !run_ends || !run_offset || !window || !run_offset_host || !window_host || !mean3 || !std3 || !out_rgb ||
        !out_mask || H <= 0 || W <= 0 || (long long)H * W > INT_MAX || n_runs <= 0 || n <= 0 || n > 65535 || S <= 0 || S > 4096)
        return PP_EINVAL;
    if (!pp_run_offsets_ok(run_offset_host, n, n_runs)) return PP_EINVAL;
    for (int d = 0; d < n; ++d) {
        const int* wd = window_host + 4 * d;
        if (wd[0] < 0 || wd[2] < 0 || wd[1] > H || wd[3] > W || wd[1] <= wd[0] || wd[3] <= wd[2]) return PP_EINVAL;
    }
    const int nt = (S + TILE - 1) / TILE;
    hipLaunchKernelGGL(detections_crop_kernel, dim3(nt * nt, n), dim3(TILE * TILE), 0, (hipStream_t)stream, image, H, W, run_ends,
                       n_runs, run_offset, window, S, rgb_mask_flag, mean3[0], mean3[1], mean3[2], std3[0], std3[1], std3[2],
                       out_rgb, out_mask);
    return pp_last_launch();
}

}  // extern "C"
