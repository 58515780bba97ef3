// Scene ground truth ("SCENE GROUND TRUTH" of include/picopose_hip.h; picopose_amd/scene_gt.py plans every call and
// tests/scene_gt_oracle.py restates the contract in numpy): per ground-truth view the pixel counts, the visible fraction's terms, the
// two boxes and the dense masks of BOP's scene_gt_info.json / mask.json / mask_visib.json, and per image the composite of its views.
//
//   vsd_raster_small_kernel, vsd_raster_large_kernel  the windowed depth raster of pp_vsd_raster_dev.h on the padded CANVAS (shared
//                            with pp_vsd.hip and pp_depth_refine.hip, as are the validation of the tables and the workspace's front)
//   scene_gt_composite_kernel  every in-frame covered window sample: 64-bit atomic minimum of (bits of Z) << 32 | v into the image's
//                            word image (all ones = background)
//   scene_gt_resolve_kernel  the word image -> scene_depth (fp32) and instance_map (int32, through view_label)
//   scene_gt_init_kernel     counts = 0, boxes = {INT_MAX, INT_MAX, INT_MIN, INT_MIN} twice
//   scene_gt_reduce_kernel   workgroups (chunk, view): walks its share of the view's window, reads Z from the z-buffer words and, in-frame,
//                            the test depth or the composite; three INTEGER counters and eight integer extrema per lane, reduced by
//                            xor-shuffles and through LDS, then one integer atomicAdd / atomicMin / atomicMax per value and workgroup;
//                            writes the dense masks on the way
//   scene_gt_finish_kernel   a box that is still {MAX, MAX, MIN, MIN} becomes the empty box {0, 0, -1, -1}
//
// Counts are integer sums, boxes integer extrema and the composite an integer minimum: no output depends on launch order, stream,
// view order, the window or on how the caller groups the views (the map: up to the stated tie rule).  No floating-point atomics.
#include <stdint.h>
#include <limits.h>
#include <math.h>
#include "pp_common.h"

#pragma clang fp contract(off)
#include "pp_window_dev.h"

namespace {

constexpr int BLOCK = WINDOW_BLOCK;
constexpr int WAVES = WINDOW_WAVES;
constexpr int NV = 11;             // all, valid, visib | obj x_min, y_min, x_max, y_max | visib x_min, y_min, x_max, y_max

// the frame inside the canvas and the tables the raster does not know
struct Frame {
    const float* cams;             // (n_images, 4) the FRAME cameras
    int H, W, pad_x, pad_y;
};

__global__ __launch_bounds__(BLOCK) void scene_gt_composite_kernel(Scene s, Frame f, const unsigned long long* __restrict__ zbuf,
                                                                   unsigned long long* __restrict__ comp) {
    for_each_window(s, zbuf, [&](int v, const Window& win) {
        unsigned long long* out = comp + (size_t)s.view_img[v] * f.H * f.W;
        walk_window(win, [&](int xc, int yc, unsigned long long key) {
            const int x = xc - f.pad_x, y = yc - f.pad_y;
            if (x < 0 || x >= f.W || y < 0 || y >= f.H) return;
            if (key == ~0ull) return;
            atomicMin(out + (size_t)y * f.W + x, (key & 0xFFFFFFFF00000000ull) | (unsigned)v);
        });
    });
}

__global__ __launch_bounds__(BLOCK) void scene_gt_resolve_kernel(const unsigned long long* __restrict__ comp, long long n,
                                                                 const int* __restrict__ view_label, float* __restrict__ scene_depth,
                                                                 int* __restrict__ instance_map) {
    for (long long i = (long long)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (long long)gridDim.x * BLOCK) {
        const unsigned long long key = comp[i];
        if (scene_depth) scene_depth[i] = word_depth(key);
        if (instance_map) {
            const int v = (int)(unsigned)key;
            instance_map[i] = key == ~0ull ? -1 : (view_label ? view_label[v] : v);
        }
    }
}

__global__ __launch_bounds__(BLOCK) void scene_gt_init_kernel(int n_views, int* __restrict__ counts, int* __restrict__ boxes) {
    const int v = blockIdx.x * BLOCK + threadIdx.x;
    if (v >= n_views) return;
    for (int c = 0; c < 3; ++c) counts[3 * (size_t)v + c] = 0;
    for (int c = 0; c < 8; ++c) boxes[8 * (size_t)v + c] = (c & 2) ? INT_MIN : INT_MAX;
}

__global__ __launch_bounds__(BLOCK) void scene_gt_finish_kernel(int n_views, int* __restrict__ boxes) {
    const int b = blockIdx.x * BLOCK + threadIdx.x;                // one lane per box
    if (b >= 2 * n_views) return;
    int* box = boxes + 4 * (size_t)b;
    if (box[0] > box[2]) box[0] = 0, box[1] = 0, box[2] = -1, box[3] = -1;
}

// value c of the record: 0..2 are sums, then per box two minima and two maxima
__device__ __forceinline__ int combine(int c, int a, int b) { return c < 3 ? a + b : (((c - 3) & 2) ? max(a, b) : min(a, b)); }

__global__ __launch_bounds__(BLOCK) void scene_gt_reduce_kernel(Scene s, Frame f, const unsigned long long* __restrict__ zbuf,
                                                                const float* __restrict__ depth,
                                                                const unsigned long long* __restrict__ comp, float delta,
                                                                int* __restrict__ counts, int* __restrict__ boxes,
                                                                unsigned char* __restrict__ mask_all,
                                                                unsigned char* __restrict__ mask_visib) {
    __shared__ int sm[WAVES][NV];
    for_each_window(s, zbuf, [&](int v, const Window& win) {
        const int img = s.view_img[v];
        const float* k = f.cams + 4 * (size_t)img;
        const float fx = k[0], fy = k[1], cx = k[2], cy = k[3];
        const size_t frame = (size_t)f.H * f.W;
        int val[NV];
#pragma unroll
        for (int c = 0; c < NV; ++c) val[c] = c < 3 ? 0 : (((c - 3) & 2) ? INT_MIN : INT_MAX);
        walk_window(win, [&](int xc, int yc, unsigned long long key) {
            const float z = word_depth(key);
            if (!(z > 0.f)) return;
            const int x = xc - f.pad_x, y = yc - f.pad_y;
            val[0] += 1;
            val[3] = min(val[3], x), val[4] = min(val[4], y), val[5] = max(val[5], x), val[6] = max(val[6], y);
            if (x < 0 || x >= f.W || y < 0 || y >= f.H) return;
            const size_t pix = (size_t)y * f.W + x;
            if (mask_all) mask_all[(size_t)v * frame + pix] = 255;
            const float z_test = depth ? depth[(size_t)img * frame + pix] : word_depth(comp[(size_t)img * frame + pix]);
            const bool missing = !(z_test > 0.f);
            const float r = ray_scale(x, y, fx, fy, cx, cy);
            val[1] += missing ? 0 : 1;
            if (visible(z * r, z_test * r, missing, delta)) {
                val[2] += 1;
                val[7] = min(val[7], x), val[8] = min(val[8], y), val[9] = max(val[9], x), val[10] = max(val[10], y);
                if (mask_visib) mask_visib[(size_t)v * frame + pix] = 255;
            }
        });
        const int a = block_reduce_to<WAVES>(val, sm, combine);
        if (threadIdx.x < NV) {
            const int c = threadIdx.x;
            if (c < 3) {
                if (a != 0) atomicAdd(counts + 3 * (size_t)v + c, a);
            } else if ((c - 3) & 2) {
                if (a != INT_MIN) atomicMax(boxes + 8 * (size_t)v + (c - 3), a);
            } else {
                if (a != INT_MAX) atomicMin(boxes + 8 * (size_t)v + (c - 3), a);
            }
        }
        __syncthreads();                                          // sm is reused by the workgroup's next view
    });
}

inline bool canvas_dims(int H, int W, int pad_x, int pad_y, int& Hc, int& Wc) {
    if (H <= 0 || W <= 0 || pad_x < 0 || pad_y < 0) return false;
    const long long hc = (long long)H + 2ll * pad_y, wc = (long long)W + 2ll * pad_x;
    if (hc > INT_MAX || wc > INT_MAX || hc * wc > (long long)INT_MAX) return false;
    Hc = (int)hc, Wc = (int)wc;
    return true;
}

}  // namespace

extern "C" {

int pp_scene_gt_workspace_bytes(long long window_samples, long long view_faces, long long composite_pixels, size_t* bytes) {
    size_t front = 0;
    if (!bytes || composite_pixels < 0 || composite_pixels > (LLONG_MAX >> 5) ||
        pp_vsd_workspace_bytes(window_samples, view_faces, &front) != PP_OK)
        return PP_EINVAL;
    *bytes = composite_pixels > 0 ? align256(front) + (size_t)composite_pixels * 8 : front;
    return PP_OK;
}

int pp_scene_gt(const PpScene* scene, const float* canvas_cams, const float* canvas_cams_host, int pad_x, int pad_y, const float* depth,
                float delta, const int* view_label, int use_view_label, void* workspace, size_t workspace_bytes, int* counts, int* boxes,
                unsigned int* near_count, unsigned char* mask_all, unsigned char* mask_visib, float* scene_depth, int* instance_map,
                void* stream) {
    if (!scene_tables(scene, false) || !canvas_cams || !canvas_cams_host || !workspace || !counts || !boxes || !near_count) return PP_EINVAL;
    if (use_view_label && !view_label) return PP_EINVAL;
    if (!(delta >= 0.f) || !finite32(delta)) return PP_EINVAL;
    // the scene as the raster sees it: the canvas cameras and the canvas size in the place of the frame's
    PpScene canvas = *scene;
    canvas.cams = canvas_cams, canvas.cams_host = canvas_cams_host;
    const int n_images = scene->n_images, n_views = scene->n_views, H = scene->H, W = scene->W;
    if (!canvas_dims(H, W, pad_x, pad_y, canvas.H, canvas.W) || n_images <= 0) return PP_EINVAL;
    for (int i = 0; i < n_images; ++i) {
        const float* k = scene->cams_host + 4 * (size_t)i;
        const float* c = canvas_cams_host + 4 * (size_t)i;
        const float sx = k[2] + (float)pad_x, sy = k[3] + (float)pad_y;
        if (!(c[0] == k[0] && c[1] == k[1] && c[2] == sx && c[3] == sy)) return PP_EINVAL;      // (a NaN entry fails here too)
    }
    SceneSize n;
    if (check_scene(&canvas, false, n) != PP_OK) return PP_EINVAL;
    const bool composite = scene_depth || instance_map || !depth;
    const long long comp_pixels = composite ? (long long)n_images * H * W : 0;
    size_t need = 0, front = 0;
    if (pp_vsd_workspace_bytes(n.samples, n.total_faces, &front) != PP_OK ||
        pp_scene_gt_workspace_bytes(n.samples, n.total_faces, comp_pixels, &need) != PP_OK)
        return PP_EINVAL;
    if (((uintptr_t)workspace % 256) != 0 || workspace_bytes < need) return PP_EWORKSPACE;

    hipStream_t st = (hipStream_t)stream;
    const RasterWs ws = carve(workspace, n);
    unsigned long long* comp = composite ? (unsigned long long*)((char*)workspace + align256(front)) : nullptr;
    const Scene s = device_scene(canvas);
    const Frame f{scene->cams, H, W, pad_x, pad_y};
    PP_CHECK_HIP(hipMemsetAsync(near_count, 0, sizeof(unsigned) * (size_t)n_views, st));
    const int rc = raster_views(s, n, ws, near_count, st);
    if (rc != PP_OK) return rc;
    if (mask_all) PP_CHECK_HIP(hipMemsetAsync(mask_all, 0, (size_t)n_views * H * W, st));
    if (mask_visib) PP_CHECK_HIP(hipMemsetAsync(mask_visib, 0, (size_t)n_views * H * W, st));
    const dim3 grid = window_grid(n_views, n.max_window);
    if (composite) {
        PP_CHECK_HIP(hipMemsetAsync(comp, 0xFF, (size_t)comp_pixels * 8, st));
        if (n.samples > 0) hipLaunchKernelGGL(scene_gt_composite_kernel, grid, dim3(BLOCK), 0, st, s, f, ws.zbuf, comp);
        if (scene_depth || instance_map) {
            const long long per = (comp_pixels + BLOCK - 1) / BLOCK;
            hipLaunchKernelGGL(scene_gt_resolve_kernel, dim3((unsigned)(per < 2048 ? per : 2048)), dim3(BLOCK), 0, st, comp, comp_pixels,
                               use_view_label ? view_label : nullptr, scene_depth, instance_map);
        }
    }
    hipLaunchKernelGGL(scene_gt_init_kernel, dim3((unsigned)((n_views + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, st, n_views, counts, boxes);
    if (n.samples > 0)
        hipLaunchKernelGGL(scene_gt_reduce_kernel, grid, dim3(BLOCK), 0, st, s, f, ws.zbuf, depth,
                           depth ? nullptr : comp, delta, counts, boxes, mask_all, mask_visib);
    hipLaunchKernelGGL(scene_gt_finish_kernel, dim3((unsigned)((2 * n_views + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, st, n_views, boxes);
    return pp_last_launch();
}

}  // extern "C"
