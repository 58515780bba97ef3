// The mixed-object windowed depth raster ("THE DEPTH RASTER" of include/picopose_hip.h), shared by pp_vsd.hip (pp_vsd_errors),
// pp_depth_refine.hip (pp_depth_refine) and pp_scene_gt.hip (pp_scene_gt).  Each translation unit that includes this header gets its
// own copy of the kernels (internal linkage, no relocatable device code in this build).
//
//   vsd_raster_small_kernel  one lane per (view, triangle of the view's object): cover_small under the view's camera and window
//   vsd_raster_large_kernel  one workgroup row per queue entry: cover_large
//   check_scene, device_scene, carve, raster_views (host)  the one validation of a PpScene (null checks included), its tables as the
//                            kernels take them, the one layout of header | z-buffer | queue, and the clears and launches of a call
//                            or of one refinement iteration
//
// The kernels are an index mapping and load_view(); the traversal is pp_raster_dev.h's, the template renderer's.  The z-buffer is
// ragged: 8 bytes per WINDOW sample, view v at words [view_zoff[v], view_zoff[v + 1]).  Include it AFTER `#pragma clang fp
// contract(off)`, like pp_raster_dev.h.
#ifndef PP_VSD_RASTER_DEV_H
#define PP_VSD_RASTER_DEV_H
#include "pp_common.h"
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

// false: the view's window is empty or the view is not active, nothing is rendered
__device__ __forceinline__ bool load_view(const Scene& s, int v, View& out) {
    if (s.active && s.active[v] == 0) return false;
    const int* w = s.windows + 4 * (size_t)v;
    const int x0 = w[0], y0 = w[1], x1 = w[2], y1 = w[3];
    if (x1 <= x0 || y1 <= y0) return false;
    const int o = s.view_obj[v];
    const float* k = s.cams + 4 * (size_t)s.view_img[v];
    const int v0 = s.vert_off[o], f0 = s.face_off[o];
    out = View{s.verts + 3 * (size_t)v0, s.faces + 3 * (size_t)f0, s.poses + 16 * (size_t)v, s.vert_off[o + 1] - v0, s.face_off[o + 1] - f0,
               x0, y0, x1 - x0, Cam{k[0], k[1], k[2], k[3], s.near, s.H, s.W, x0, y0, x1, y1}};
    return true;
}

// view blockIdx.y, blockIdx.y + gridDim.y, ...; faces blockIdx.x * 256 + lane of that view's object
__global__ __launch_bounds__(RASTER_BLOCK) void vsd_raster_small_kernel(Scene s, unsigned long long* __restrict__ zbuf,
                                                                        uint2* __restrict__ queue, unsigned* __restrict__ qcount,
                                                                        unsigned* __restrict__ near_count) {
    const int f = blockIdx.x * RASTER_BLOCK + threadIdx.x;
    for (int v = blockIdx.y; v < s.n_views; v += gridDim.y) {
        View vw;
        if (load_view(s, v, vw) && f < vw.Nf) cover_small(vw, v, f, zbuf + s.view_zoff[v], queue, qcount, near_count + v);
    }
}

// queue entry blockIdx.y, blockIdx.y + gridDim.y, ...; its tiles blockIdx.x, blockIdx.x + gridDim.x, ...
__global__ __launch_bounds__(TILE * TILE) void vsd_raster_large_kernel(Scene s, unsigned long long* __restrict__ zbuf,
                                                                       const uint2* __restrict__ queue,
                                                                       const unsigned* __restrict__ qcount) {
    const unsigned n = *qcount;
    for (unsigned e = blockIdx.y; e < n; e += gridDim.y) {
        const uint2 q = queue[e];
        View vw;
        if (q.x < (unsigned)s.n_views && load_view(s, (int)q.x, vw)) cover_large(vw, q.y, zbuf + s.view_zoff[q.x]);
    }
}

struct SceneSize {
    long long total_faces;     // over the views: the queue's capacity
    int max_faces;             // of one view
    long long samples;         // z-buffer words
    long long max_window;      // samples of the largest window
};

// The one null check of the scene's tables.  device_diameters: whether the entry reads the device table `diameters`.
inline bool scene_tables(const PpScene* h, bool device_diameters) {
    return h && h->vertices && h->vert_off && h->faces && h->face_off && (h->diameters || !device_diameters) && h->cams && h->view_obj &&
           h->view_img && h->poses && h->windows && h->view_zoff && h->vert_off_host && h->faces_host && h->face_off_host &&
           h->diameters_host && h->cams_host && h->view_obj_host && h->view_img_host && h->windows_host && h->view_zoff_host;
}

// THE SCENE CHECKS of include/picopose_hip.h: the pointers (scene_tables), the counts, near, and every host table of `h`: offsets,
// face indices, diameters, cameras, the views' objects and images, windows inside the frame and the z-buffer offsets that follow
// from them.  PP_OK or PP_EINVAL; nothing touches the device.
inline int check_scene(const PpScene* h, bool device_diameters, SceneSize& out) {
    if (!scene_tables(h, device_diameters)) return PP_EINVAL;
    if (h->n_objects <= 0 || h->n_images <= 0 || h->n_views <= 0 || h->H <= 0 || h->W <= 0 || (long long)h->H * h->W > INT_MAX) return PP_EINVAL;
    if (!positive_finite(h->near)) return PP_EINVAL;
    const int* vert_off = h->vert_off_host;
    const int* face_off = h->face_off_host;
    if (vert_off[0] != 0 || face_off[0] != 0) return PP_EINVAL;
    for (int o = 0; o < h->n_objects; ++o) {
        if (vert_off[o + 1] <= vert_off[o] || face_off[o + 1] < face_off[o]) return PP_EINVAL;
        if (!positive_finite(h->diameters_host[o])) return PP_EINVAL;
        const unsigned nv = (unsigned)(vert_off[o + 1] - vert_off[o]);
        for (size_t k = 3 * (size_t)face_off[o]; k < 3 * (size_t)face_off[o + 1]; ++k)
            if ((unsigned)h->faces_host[k] >= nv) return PP_EINVAL;
    }
    for (int i = 0; i < h->n_images; ++i) {
        const float* k = h->cams_host + 4 * (size_t)i;
        if (k[0] == 0.f || k[1] == 0.f || !finite32(k[0]) || !finite32(k[1]) || !finite32(k[2]) || !finite32(k[3])) return PP_EINVAL;
    }
    const long long* view_zoff = h->view_zoff_host;
    if (view_zoff[0] != 0) return PP_EINVAL;
    out = SceneSize{0, 0, 0, 0};
    for (int v = 0; v < h->n_views; ++v) {
        const int o = h->view_obj_host[v];
        if ((unsigned)o >= (unsigned)h->n_objects || (unsigned)h->view_img_host[v] >= (unsigned)h->n_images) return PP_EINVAL;
        const int nf = face_off[o + 1] - face_off[o];
        if (nf <= 0) return PP_EINVAL;                            // an object of the call without faces
        const int* w = h->windows_host + 4 * (size_t)v;
        if (w[0] < 0 || w[1] < 0 || w[2] < w[0] || w[3] < w[1] || w[2] > h->W || w[3] > h->H) return PP_EINVAL;
        const long long window = (long long)(w[2] - w[0]) * (w[3] - w[1]);
        if (view_zoff[v + 1] - view_zoff[v] != window) return PP_EINVAL;
        out.total_faces += nf;
        out.max_faces = nf > out.max_faces ? nf : out.max_faces;
        out.max_window = window > out.max_window ? window : out.max_window;
    }
    if (out.total_faces > (long long)UINT_MAX) return PP_EINVAL;
    out.samples = view_zoff[h->n_views];
    return PP_OK;
}

// the tables of a checked scene as the kernels take them
inline Scene device_scene(const PpScene& h) {
    return Scene{h.vertices, h.vert_off, h.faces, h.face_off, h.cams, h.view_obj, h.view_img, h.poses, h.windows, h.view_zoff, h.n_views, h.H, h.W,
                 h.near};
}

// the front of a workspace: header (the queue counter) | z-buffer, padded to 256 bytes | queue, one slot per (view, triangle)
struct RasterWs {
    unsigned* qcount;
    unsigned long long* zbuf;
    uint2* queue;
};

inline RasterWs carve(void* workspace, const SceneSize& n) {
    char* zbuf = (char*)workspace + WS_HEADER;
    return RasterWs{(unsigned*)workspace, (unsigned long long*)zbuf, (uint2*)(zbuf + align256((size_t)n.samples * 8))};
}

// the raster of every view of `s`: queue and z-buffer clears and the two launches of a call or of one refinement iteration
inline int raster_views(const Scene& s, const SceneSize& n, const RasterWs& ws, unsigned* near_count, hipStream_t st) {
    PP_CHECK_HIP(hipMemsetAsync(ws.qcount, 0, sizeof(unsigned), st));
    if (n.samples == 0) return PP_OK;
    PP_CHECK_HIP(hipMemsetAsync(ws.zbuf, 0xFF, (size_t)n.samples * 8, st));
    const unsigned gv = (unsigned)(s.n_views < 65535 ? s.n_views : 65535);
    hipLaunchKernelGGL(vsd_raster_small_kernel, dim3((unsigned)((n.max_faces + RASTER_BLOCK - 1) / RASTER_BLOCK), gv), dim3(RASTER_BLOCK),
                       0, st, s, ws.zbuf, ws.queue, ws.qcount, near_count);
    const unsigned gy = (unsigned)(n.total_faces < 4096 ? n.total_faces : 4096);
    hipLaunchKernelGGL(vsd_raster_large_kernel, dim3(8, gy), dim3(TILE * TILE), 0, st, s, ws.zbuf, ws.queue, ws.qcount);
    return PP_OK;
}

}  // namespace
#endif
