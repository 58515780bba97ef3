// The mixed-object windowed depth raster ("THE DEPTH RASTER" of include/picopose_hip.h): the tables of a call, the view loader and the
// two raster kernels, shared by pp_vsd.hip (pp_vsd_errors) and pp_depth_refine.hip (pp_depth_refine).  Each translation unit that
// includes this header gets its own copy of the kernels (internal linkage, no relocatable device code in this build).
//
//   vsd_raster_small_kernel  one lane per (view, triangle of the view's object): tri_setup under the view's camera and window; a box
//                            of at most SMALL_BOX samples is walked by the lane, a larger one goes to the queue
//   vsd_raster_large_kernel  queue entries -> 16 x 16 tiles, one workgroup step per tile (the template renderer's scheme)
//
// The z-buffer is ragged: 8 bytes per WINDOW sample, view v at words [view_zoff[v], view_zoff[v + 1]).  Depth is a 64-bit unsigned
// atomic minimum over (bits of Z) << 32 | face.  Include it AFTER `#pragma clang fp contract(off)`, like pp_raster_dev.h.
#ifndef PP_VSD_RASTER_DEV_H
#define PP_VSD_RASTER_DEV_H
#include "pp_raster_dev.h"

namespace {

constexpr int RASTER_BLOCK = 256;

// the tables of a call (device pointers)
struct Scene {
    const float* verts;
    const int* vert_off;
    const int* faces;
    const int* face_off;
    const float* cams;         // (n_images, 4) fx, fy, cx, cy
    const int* view_obj;
    const int* view_img;
    const float* poses;        // (n_views, 16)
    const int* windows;        // (n_views, 4) x0, y0, x1, y1 (exclusive upper corner)
    const long long* view_zoff;
    int n_views, H, W;
    float near;
    const int* active = nullptr;   // (n_views) or null: a view with active[v] == 0 renders nothing; null: every view is active
};

struct View {
    const float* verts;
    const int* faces;
    const float* pose;
    int Nv, Nf, x0, y0, ww;
    Cam cam;
};

// false: the view's window is empty or the view is not active, nothing is rendered
__device__ __forceinline__ bool load_view(const Scene& s, int v, View& out) {
    if (s.active && s.active[v] == 0) return false;
    const int* w = s.windows + 4 * (size_t)v;
    const int x0 = w[0], y0 = w[1], x1 = w[2], y1 = w[3];
    if (x1 <= x0 || y1 <= y0) return false;
    const int o = s.view_obj[v];
    const float* k = s.cams + 4 * (size_t)s.view_img[v];
    const int v0 = s.vert_off[o], f0 = s.face_off[o];
    out.verts = s.verts + 3 * (size_t)v0;
    out.Nv = s.vert_off[o + 1] - v0;
    out.faces = s.faces + 3 * (size_t)f0;
    out.Nf = s.face_off[o + 1] - f0;
    out.pose = s.poses + 16 * (size_t)v;
    out.x0 = x0;
    out.y0 = y0;
    out.ww = x1 - x0;
    out.cam = Cam{k[0], k[1], k[2], k[3], s.near, s.H, s.W, x0, y0, x1, y1};
    return true;
}

__device__ __forceinline__ unsigned long long* slot_of(unsigned long long* zv, const View& vw, int px, int py) {
    return zv + (size_t)(py - vw.y0) * vw.ww + (px - vw.x0);
}

// view blockIdx.y, blockIdx.y + gridDim.y, ...; faces blockIdx.x * 256 + lane of that view's object
__global__ __launch_bounds__(RASTER_BLOCK) void vsd_raster_small_kernel(Scene s, unsigned long long* __restrict__ zbuf,
                                                                        uint2* __restrict__ queue, unsigned* __restrict__ qcount,
                                                                        unsigned* __restrict__ near_count) {
    const int f = blockIdx.x * RASTER_BLOCK + threadIdx.x;
    for (int v = blockIdx.y; v < s.n_views; v += gridDim.y) {
        View vw;
        if (!load_view(s, v, vw) || f >= vw.Nf) continue;
        Tri t;
        const int st = tri_setup(vw.verts, vw.faces, vw.Nv, vw.pose, vw.cam, f, t);
        if (st == TRI_NEAR) atomicAdd(near_count + v, 1u);
        if (st != TRI_OK) continue;
        if ((t.bx1 - t.bx0 + 1) * (long long)(t.by1 - t.by0 + 1) > SMALL_BOX) {
            queue[atomicAdd(qcount, 1u)] = make_uint2((unsigned)v, (unsigned)f);
            continue;
        }
        unsigned long long* zv = zbuf + s.view_zoff[v];
        for (int py = t.by0; py <= t.by1; ++py)
            for (int px = t.bx0; px <= t.bx1; ++px) depth_test(t, px, py, f, slot_of(zv, vw, px, py));
    }
}

// queue entry blockIdx.y, blockIdx.y + gridDim.y, ...; its tiles blockIdx.x, blockIdx.x + gridDim.x, ...
__global__ __launch_bounds__(TILE * TILE) void vsd_raster_large_kernel(Scene s, unsigned long long* __restrict__ zbuf,
                                                                       const uint2* __restrict__ queue,
                                                                       const unsigned* __restrict__ qcount) {
    const unsigned n = *qcount;
    const int ty = threadIdx.x / TILE, tx = threadIdx.x % TILE;
    for (unsigned e = blockIdx.y; e < n; e += gridDim.y) {
        const uint2 q = queue[e];
        if (q.x >= (unsigned)s.n_views) continue;
        View vw;
        if (!load_view(s, (int)q.x, vw) || q.y >= (unsigned)vw.Nf) continue;
        Tri t;
        if (tri_setup(vw.verts, vw.faces, vw.Nv, vw.pose, vw.cam, (int)q.y, t) != TRI_OK) continue;
        unsigned long long* zv = zbuf + s.view_zoff[q.x];
        const int ntx = (t.bx1 - t.bx0) / TILE + 1, nty = (t.by1 - t.by0) / TILE + 1;
        for (int tile = blockIdx.x; tile < ntx * nty; tile += gridDim.x) {
            const int x0 = t.bx0 + (tile % ntx) * TILE, y0 = t.by0 + (tile / ntx) * TILE;
            const int x1 = min(x0 + TILE - 1, t.bx1), y1 = min(y0 + TILE - 1, t.by1);
            if (tile_outside(t, x0, y0, x1, y1)) continue;
            const int px = x0 + tx, py = y0 + ty;
            if (px <= x1 && py <= y1) depth_test(t, px, py, (int)q.y, slot_of(zv, vw, px, py));
        }
    }
}

// the raster of every view of `s` into the (cleared) z-buffer: the two launches of a call or of one refinement iteration
inline void launch_raster(const Scene& s, int max_faces, long long total_faces, unsigned long long* zbuf, uint2* queue, unsigned* qcount,
                          unsigned* near_count, hipStream_t st) {
    const unsigned gv = (unsigned)(s.n_views < 65535 ? s.n_views : 65535);
    hipLaunchKernelGGL(vsd_raster_small_kernel, dim3((unsigned)((max_faces + RASTER_BLOCK - 1) / RASTER_BLOCK), gv), dim3(RASTER_BLOCK), 0,
                       st, s, zbuf, queue, qcount, near_count);
    const unsigned gy = (unsigned)(total_faces < 4096 ? total_faces : 4096);
    hipLaunchKernelGGL(vsd_raster_large_kernel, dim3(8, gy), dim3(TILE * TILE), 0, st, s, zbuf, queue, qcount);
}

}  // namespace
#endif
