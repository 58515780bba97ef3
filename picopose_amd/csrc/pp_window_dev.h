// What READS the ragged z-buffer of pp_vsd_raster_dev.h, shared by pp_vsd.hip, pp_verify.hip, pp_scene_gt.hip and pp_depth_refine.hip
// (internal linkage: every translation unit gets its own copy).  Include it AFTER `#pragma clang fp contract(off)`, like the raster.
//
//   word_depth          a z word -> Z, 0 for an uncovered sample
//   Window, load_window view v's window as a reader takes it; false: the window is empty
//   for_each_window     the views of a workgroup, grid (chunk, view): the blockIdx.y view stride, the empty-window skip and the skip of a
//                       chunk that lies beyond the window.  Every skip is uniform over the workgroup: the body may hold barriers
//   walk_window         the grid-stride loop of chunk blockIdx.x over the window's samples: (x, y, key) per sample, x and y in the
//                       raster's frame.  Callers subtract their own offsets and keep their own early-outs
//   ray_scale, visible  BOP's distance along the ray, r with d = Z r, and its visibility rule.  Three float operations in a fixed order
//                       and one predicate: every entry that states visibility computes the same bits
//   (the workgroup's totals of the readers' int[N] records go through block_reduce_to<WINDOW_WAVES> of pp_reduce_dev.h)
//   window_grid (host)  the (chunk, view) grid of a launch whose kernel goes through for_each_window
#ifndef PP_WINDOW_DEV_H
#define PP_WINDOW_DEV_H
#include "pp_reduce_dev.h"
#include "pp_vsd_raster_dev.h"

namespace {

constexpr int WINDOW_BLOCK = 256;
constexpr int WINDOW_WAVES = WINDOW_BLOCK / 64;

__device__ __forceinline__ float word_depth(unsigned long long key) {
    return key == ~0ull ? 0.f : __uint_as_float((unsigned)(key >> 32));
}

struct Window {
    int x0, y0, ww;                    // origin and width in the raster's frame
    long long n;                       // samples; at most INT_MAX (THE SCENE CHECKS)
    const unsigned long long* z;       // its z words, row-major
};

__device__ __forceinline__ bool load_window(const Scene& s, const unsigned long long* __restrict__ zbuf, int v, Window& out) {
    const int* w = s.windows + 4 * (size_t)v;
    const int ww = w[2] - w[0], wh = w[3] - w[1];
    if (ww <= 0 || wh <= 0) return false;
    out = Window{w[0], w[1], ww, (long long)ww * wh, zbuf + s.view_zoff[v]};
    return true;
}

// body(v, window) for view blockIdx.y, blockIdx.y + gridDim.y, ... when chunk blockIdx.x holds a sample of its window
template <class Body>
__device__ __forceinline__ void for_each_window(const Scene& s, const unsigned long long* __restrict__ zbuf, Body body) {
    for (int v = blockIdx.y; v < s.n_views; v += gridDim.y) {
        Window win;
        if (!load_window(s, zbuf, v, win)) continue;
        if ((long long)blockIdx.x * WINDOW_BLOCK >= win.n) continue;
        body(v, win);
    }
}

// visit(x, y, key) for sample blockIdx.x * 256 + lane, + gridDim.x * 256, ...  The index is 64-bit, so the stride cannot wrap it; the
// sample itself fits 32 bits (Window::n), so its row is a 32-bit division.
template <class Visit>
__device__ __forceinline__ void walk_window(const Window& win, Visit visit) {
    for (long long base = (long long)blockIdx.x * WINDOW_BLOCK; base < win.n; base += (long long)gridDim.x * WINDOW_BLOCK) {
        const long long i = base + threadIdx.x;                   // (base is uniform: the loop's state stays in scalar registers)
        if (i >= win.n) break;                                    // (the window's last chunk)
        const unsigned yy = (unsigned)i / (unsigned)win.ww;
        visit(win.x0 + (int)((unsigned)i - yy * (unsigned)win.ww), win.y0 + (int)yy, win.z[i]);
    }
}

// r = |(xr, yr, 1)| of the ray through pixel (x, y): the distance of a sample at depth Z is d = Z r
__device__ __forceinline__ float ray_scale(int x, int y, float fx, float fy, float cx, float cy) {
    const float xr = ((float)x - cx) / fx, yr = ((float)y - cy) / fy;
    return sqrtf((xr * xr + yr * yr) + 1.f);
}

// a model sample at distance d against the test distance d_test (missing: the test image holds none there)
__device__ __forceinline__ bool visible(float d, float d_test, bool missing, float delta) {
    return d > 0.f && (missing || d - d_test <= delta);
}

inline dim3 window_grid(int n_views, long long max_window) {
    constexpr int CHUNK_SAMPLES = WINDOW_BLOCK * 16;
    constexpr int MAX_CHUNKS = 128;                               // workgroups over one view's window
    const unsigned gv = (unsigned)(n_views < 65535 ? n_views : 65535);                          // (for_each_window's view stride)
    long long chunks = (max_window + CHUNK_SAMPLES - 1) / CHUNK_SAMPLES;
    const long long cap = 8192 / gv > 1 ? 8192 / gv : 1;                                        // bound the grid of a call with many views
    chunks = chunks < 1 ? 1 : (chunks > MAX_CHUNKS ? MAX_CHUNKS : chunks);
    chunks = chunks > cap ? cap : chunks;
    return dim3((unsigned)chunks, gv);
}

}  // namespace
#endif
