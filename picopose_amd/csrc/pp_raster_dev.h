// Device functions of the z-buffer rasterisers: items 1-6 of the raster contract (include/picopose_hip.h) for one (view, triangle) and
// the coverage pass built from them.  One statement of the arithmetic AND of the traversal for the template renderer (pp_render.hip)
// and the windowed depth raster (pp_vsd_raster_dev.h): every float operation is a single float32 operation, coverage is exact integer
// arithmetic, and nothing is stored per triangle — tri_setup() gives the same bits wherever it is evaluated.  A raster kernel is its
// index mapping and its View; cover_small() and cover_large() are the rest.  Include it AFTER `#pragma clang fp contract(off)` (it
// repeats the pragma for the translation unit) and after any header that must be compiled in the build's default mode (pp_crop_dev.h).
#ifndef PP_RASTER_DEV_H
#define PP_RASTER_DEV_H
#include <hip/hip_runtime.h>
#include <limits.h>

#pragma clang fp contract(off)

namespace {

constexpr int SUB = 256;                 // sub-pixel units per pixel
constexpr float SNAP_LIMIT = 268435456.f;   // 2^28 sub-pixel units: the edge functions stay below 2^60
constexpr int SMALL_BOX = 64;            // samples a single lane walks
constexpr int TILE = 16;
constexpr size_t WS_HEADER = 256;        // bytes of a workspace in front of the z-buffer: the queue counter, padded to the alignment

enum : int { TRI_OK = 0, TRI_NEAR = 1, TRI_SKIP = 2 };

// samples are taken for clip_x0 <= x < min(clip_x1, W) and clip_y0 <= y < min(clip_y1, H): the clip rectangle defaults to the frame.
// Pixel (x, y) is sampled at the sub-pixel position (256 x + sub_x, 256 y + sub_y): (0, 0) is the pixel centre of item 2, the
// sample planes of THE MULTISAMPLE CONTRACT (M1) set their offset here
struct Cam {
    float fx, fy, cx, cy, near;
    int H, W;
    int clip_x0 = 0, clip_y0 = 0, clip_x1 = INT_MAX, clip_y1 = INT_MAX;
    int sub_x = 0, sub_y = 0;
};

struct Tri {
    int x[3], y[3];      // snapped screen coordinates less the camera's sample offset, ordered so that area2 > 0
    int id[3];           // vertex indices in that order
    int swapped;         // 1 when corners 1 and 2 were exchanged for that: per-corner attributes follow (no arithmetic reads it)
    float iz[3];         // 1 / Zc
    long long area2;
    int bx0, bx1, by0, by1;   // inclusive sample box, clipped to the clip rectangle
};

__device__ __forceinline__ int snap(float u) {
    const float s = fminf(fmaxf(u * (float)SUB, -SNAP_LIMIT), SNAP_LIMIT);
    return (int)rintf(s);
}

__device__ __forceinline__ int tri_setup(const float* __restrict__ verts, const int* __restrict__ faces, int Nv,
                                         const float* __restrict__ P, const Cam& c, int f, Tri& t) {
    bool near_hit = false;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int id = faces[3 * (size_t)f + k];
        if ((unsigned)id >= (unsigned)Nv) return TRI_SKIP;   // (the entry validated the host copy; never a fault)
        const float X = verts[3 * (size_t)id], Y = verts[3 * (size_t)id + 1], Z = verts[3 * (size_t)id + 2];
        const float xc = ((P[0] * X + P[1] * Y) + P[2] * Z) + P[3];
        const float yc = ((P[4] * X + P[5] * Y) + P[6] * Z) + P[7];
        const float zc = ((P[8] * X + P[9] * Y) + P[10] * Z) + P[11];
        t.id[k] = id;
        if (!(zc > c.near)) {
            near_hit = true;
            t.x[k] = t.y[k] = 0;
            t.iz[k] = 0.f;
        } else {
            // M2: the edge functions see differences only, so moving the sample point by the offset is moving the snapped corners back
            t.x[k] = snap((c.fx * xc) / zc + c.cx) - c.sub_x;
            t.y[k] = snap((c.fy * yc) / zc + c.cy) - c.sub_y;
            t.iz[k] = 1.f / zc;
        }
    }
    if (near_hit) return TRI_NEAR;
    long long area2 = (long long)(t.x[1] - t.x[0]) * (t.y[2] - t.y[0]) - (long long)(t.y[1] - t.y[0]) * (t.x[2] - t.x[0]);
    if (area2 == 0) return TRI_SKIP;
    t.swapped = area2 < 0;
    if (area2 < 0) {
        area2 = -area2;
        int s = t.x[1]; t.x[1] = t.x[2]; t.x[2] = s;
        s = t.y[1]; t.y[1] = t.y[2]; t.y[2] = s;
        s = t.id[1]; t.id[1] = t.id[2]; t.id[2] = s;
        const float z = t.iz[1]; t.iz[1] = t.iz[2]; t.iz[2] = z;
    }
    t.area2 = area2;
    const int xmin = min(t.x[0], min(t.x[1], t.x[2])), xmax = max(t.x[0], max(t.x[1], t.x[2]));
    const int ymin = min(t.y[0], min(t.y[1], t.y[2])), ymax = max(t.y[0], max(t.y[1], t.y[2]));
    t.bx0 = max((xmin + SUB - 1) >> 8, c.clip_x0);       // ceil / floor of the sub-pixel extent (arithmetic shifts)
    t.bx1 = min(xmax >> 8, min(c.clip_x1, c.W) - 1);
    t.by0 = max((ymin + SUB - 1) >> 8, c.clip_y0);
    t.by1 = min(ymax >> 8, min(c.clip_y1, c.H) - 1);
    if (t.bx0 > t.bx1 || t.by0 > t.by1) return TRI_SKIP;
    return TRI_OK;
}

// edge function of a -> b at the sample (px, py) (pixels): > 0 inside for area2 > 0
__device__ __forceinline__ long long edge_fn(int ax, int ay, int bx, int by, int px, int py) {
    return (long long)(bx - ax) * ((long long)py * SUB - ay) - (long long)(by - ay) * ((long long)px * SUB - ax);
}
// top-left rule: a sample exactly on the edge a -> b belongs to the triangle when the edge is a left edge (dy < 0) or a top edge
// (dy == 0, dx > 0) of the positively ordered triangle
__device__ __forceinline__ bool edge_owns(int ax, int ay, int bx, int by) { return by < ay || (by == ay && bx > ax); }

__device__ __forceinline__ bool covers(const Tri& t, int px, int py, long long w[3]) {
    w[0] = edge_fn(t.x[1], t.y[1], t.x[2], t.y[2], px, py);
    w[1] = edge_fn(t.x[2], t.y[2], t.x[0], t.y[0], px, py);
    w[2] = edge_fn(t.x[0], t.y[0], t.x[1], t.y[1], px, py);
    if (w[0] < 0 || w[1] < 0 || w[2] < 0) return false;
    if (w[0] == 0 && !edge_owns(t.x[1], t.y[1], t.x[2], t.y[2])) return false;
    if (w[1] == 0 && !edge_owns(t.x[2], t.y[2], t.x[0], t.y[0])) return false;
    if (w[2] == 0 && !edge_owns(t.x[0], t.y[0], t.x[1], t.y[1])) return false;
    return true;
}

// perspective weights p_k = (w_k / area2) / Z_k and their sum q = 1 / Z
__device__ __forceinline__ float weights(const Tri& t, const long long w[3], float p[3]) {
    const float a = (float)t.area2;
#pragma unroll
    for (int k = 0; k < 3; ++k) p[k] = ((float)w[k] / a) * t.iz[k];
    return (p[0] + p[1]) + p[2];
}

// a 16 x 16 tile [x0, x1] x [y0, y1] with all four corners outside one edge holds no covered sample
__device__ __forceinline__ bool tile_outside(const Tri& t, int x0, int y0, int x1, int y1) {
    bool out = false;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int a = (k + 1) % 3, b = (k + 2) % 3;
        out |= edge_fn(t.x[a], t.y[a], t.x[b], t.y[b], x0, y0) < 0 && edge_fn(t.x[a], t.y[a], t.x[b], t.y[b], x1, y0) < 0 &&
               edge_fn(t.x[a], t.y[a], t.x[b], t.y[b], x0, y1) < 0 && edge_fn(t.x[a], t.y[a], t.x[b], t.y[b], x1, y1) < 0;
    }
    return out;
}

// the depth test of one sample: (bits of Z) << 32 | face, 64-bit unsigned minimum (Z > 0, so the bits order like the value)
__device__ __forceinline__ void depth_test(const Tri& t, int px, int py, int face, unsigned long long* __restrict__ slot) {
    long long w[3];
    if (!covers(t, px, py, w)) return;
    float p[3];
    const float z = 1.f / weights(t, w, p);
    const unsigned long long key = ((unsigned long long)__float_as_uint(z) << 32) | (unsigned)face;
    // the slot only ever decreases: a (possibly stale) value at or below the key already rules this fragment out
    if (__hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > key) atomicMin(slot, key);
}

// one view of a coverage launch: its mesh, pose and camera, and where its z-buffer words lie — sample (px, py) is word
// (py - y0) * ww + (px - x0) of the view (a whole frame: origin (0, 0), row stride W)
struct View {
    const float* verts;
    const int* faces;
    const float* pose;
    int Nv, Nf, x0, y0, ww;
    Cam cam;
};

__device__ __forceinline__ unsigned long long* slot_of(unsigned long long* zv, const View& vw, int px, int py) {
    return zv + (size_t)(py - vw.y0) * vw.ww + (px - vw.x0);
}

// the calling lane's triangle f of view v (z-buffer words at zv): a triangle in front of the near plane is counted (in near_slot,
// unless that is null: a further sample plane of a view that plane 0 counts), a box of at most SMALL_BOX samples is walked here, a
// larger one goes to the queue
__device__ __forceinline__ void cover_small(const View& vw, int v, int f, unsigned long long* zv, uint2* __restrict__ queue,
                                            unsigned* __restrict__ qcount, unsigned* __restrict__ near_slot) {
    Tri t;
    const int st = tri_setup(vw.verts, vw.faces, vw.Nv, vw.pose, vw.cam, f, t);
    if (st == TRI_NEAR && near_slot) atomicAdd(near_slot, 1u);
    if (st != TRI_OK) return;
    if ((t.bx1 - t.bx0 + 1) * (long long)(t.by1 - t.by0 + 1) > SMALL_BOX) {
        queue[atomicAdd(qcount, 1u)] = make_uint2((unsigned)v, (unsigned)f);
        return;
    }
    for (int py = t.by0; py <= t.by1; ++py)
        for (int px = t.bx0; px <= t.bx1; ++px) depth_test(t, px, py, f, slot_of(zv, vw, px, py));
}

// the queued triangle f of a view for the calling workgroup of TILE * TILE lanes: the tiles blockIdx.x, blockIdx.x + gridDim.x, ...
// of its box, a lane per sample, after the tile is tested against the three edges
__device__ __forceinline__ void cover_large(const View& vw, unsigned f, unsigned long long* zv) {
    Tri t;
    if (f >= (unsigned)vw.Nf || tri_setup(vw.verts, vw.faces, vw.Nv, vw.pose, vw.cam, (int)f, t) != TRI_OK) return;
    const int ty = threadIdx.x / TILE, tx = threadIdx.x % TILE;
    const int ntx = (t.bx1 - t.bx0) / TILE + 1, nty = (t.by1 - t.by0) / TILE + 1;
    for (int tile = blockIdx.x; tile < ntx * nty; tile += gridDim.x) {
        const int x0 = t.bx0 + (tile % ntx) * TILE, y0 = t.by0 + (tile / ntx) * TILE;
        const int x1 = min(x0 + TILE - 1, t.bx1), y1 = min(y0 + TILE - 1, t.by1);
        if (tile_outside(t, x0, y0, x1, y1)) continue;
        const int px = x0 + tx, py = y0 + ty;
        if (px <= x1 && py <= y1) depth_test(t, px, py, (int)f, slot_of(zv, vw, px, py));
    }
}

}  // namespace
#endif
