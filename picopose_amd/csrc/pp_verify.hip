// Pose verification ("POSE VERIFICATION" of include/picopose_hip.h; picopose_amd/verify.py plans every call and tests/verify_oracle.py
// restates the contract in numpy): per pose hypothesis eight integer counts of its depth render held against the detection's
// bit-packed mask and, when there is one, the test depth image.
//
//   vsd_raster_small_kernel, vsd_raster_large_kernel  the windowed depth raster of pp_vsd_raster_dev.h (shared with pp_vsd.hip,
//                            pp_depth_refine.hip and pp_scene_gt.hip, as are the validation of the tables and the workspace's layout)
//   pose_verify_reduce_kernel  workgroups (chunk, view): walks its share of the view's window, reads Z from the z-buffer words, the
//                            sample's bit of the view's mask and the test depth; eight INTEGER counters per lane, reduced by
//                            xor-shuffles and through LDS, then one integer atomicAdd per counter and workgroup
//
// The z-buffer is row-major within the window and the mask's bits are column-major over the frame.  A wave takes 64 consecutive
// samples of the window: one 512-byte z segment, and a gather of 64 mask words H / 32 words apart, which stay in cache (a mask is
// 38 KB at 640 x 480).  A wave tile of 8 x by 8 y — eight 64-byte z segments, eight mask words — was built and measured slower on
// the MI355X in every case (profiles/r15/pose_verify.md, which states the tile's index mapping), and was removed.
//
// Counts are integer sums: no output depends on launch order, stream, view order, the window or on how the caller groups the views.
// No floating-point atomics.
#include <stdint.h>
#include <limits.h>
#include <math.h>
#include "pp_common.h"

#pragma clang fp contract(off)
#include "pp_window_dev.h"

namespace {

constexpr int BLOCK = WINDOW_BLOCK;
constexpr int WAVES = WINDOW_WAVES;
constexpr int NC = PP_VERIFY_COUNTS;   // render, inter, valid, agree, front, behind, vis, vis_inter

struct Evidence {
    const unsigned* mask_bits;         // (n_masks, words)
    const int* view_mask;              // (n_views)
    const float* depth;                // (n_images, H, W) or null
    int words;
    float delta;
};

__global__ __launch_bounds__(BLOCK) void pose_verify_reduce_kernel(Scene s, Evidence ev, const unsigned long long* __restrict__ zbuf,
                                                                   int* __restrict__ counts) {
    __shared__ int sm[WAVES][NC];
    for_each_window(s, zbuf, [&](int v, const Window& win) {
        const int img = s.view_img[v];
        const float* k = s.cams + 4 * (size_t)img;
        const float fx = k[0], fy = k[1], cx = k[2], cy = k[3];
        const unsigned* mask = ev.mask_bits + (size_t)ev.view_mask[v] * ev.words;
        const float* depth = ev.depth ? ev.depth + (size_t)img * s.H * s.W : nullptr;
        int val[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c) val[c] = 0;
        walk_window(win, [&](int x, int y, unsigned long long key) {                           // in the frame: THE SCENE CHECKS
            const float z = word_depth(key);
            if (!(z > 0.f)) return;
            const unsigned bit = (unsigned)x * (unsigned)s.H + (unsigned)y;
            const int in_mask = (int)((mask[bit >> 5] >> (bit & 31u)) & 1u);
            int valid = 0, front = 0, behind = 0;
            if (depth) {
                const float z_test = depth[(size_t)y * s.W + x];
                if (z_test > 0.f) {                                // (a NaN is missing)
                    const float r = ray_scale(x, y, fx, fy, cx, cy);
                    const float d = z * r, d_test = z_test * r;
                    const float e = d - d_test;
                    valid = 1, front = e > ev.delta ? 1 : 0, behind = -e > ev.delta ? 1 : 0;
                }
            }
            const int vis = 1 - front;
            val[0] += 1, val[1] += in_mask, val[2] += valid, val[3] += valid & ~(front | behind), val[4] += front, val[5] += behind;
            val[6] += vis, val[7] += vis & in_mask;
        });
        const int a = block_reduce_to<WAVES>(val, sm, op_sum{});
        if (threadIdx.x < NC && a != 0) atomicAdd(counts + NC * (size_t)v + threadIdx.x, a);
        __syncthreads();                                          // sm is reused by the workgroup's next view
    });
}

}  // namespace

extern "C" {

int pp_pose_verify(const PpScene* scene, const unsigned* mask_bits, int n_masks, int words, const int* view_mask, const int* view_mask_host,
                   const float* depth, float delta, void* workspace, size_t workspace_bytes, int* counts, unsigned int* near_count,
                   void* stream) {
    SceneSize n;
    if (check_scene(scene, false, n) != PP_OK) return PP_EINVAL;
    if (!mask_bits || !view_mask || !view_mask_host || !workspace || !counts || !near_count) return PP_EINVAL;
    if (n_masks <= 0 || (long long)words != ((long long)scene->H * scene->W + 31) / 32) return PP_EINVAL;
    if (!(delta >= 0.f) || !finite32(delta)) return PP_EINVAL;
    const int n_views = scene->n_views;
    for (int v = 0; v < n_views; ++v)
        if ((unsigned)view_mask_host[v] >= (unsigned)n_masks) return PP_EINVAL;
    size_t need = 0;
    if (pp_vsd_workspace_bytes(n.samples, n.total_faces, &need) != PP_OK) return PP_EINVAL;
    if (((uintptr_t)workspace % 256) != 0 || workspace_bytes < need) return PP_EWORKSPACE;

    hipStream_t st = (hipStream_t)stream;
    const RasterWs ws = carve(workspace, n);
    const Scene s = device_scene(*scene);
    const Evidence ev{mask_bits, view_mask, depth, words, delta};
    PP_CHECK_HIP(hipMemsetAsync(near_count, 0, sizeof(unsigned) * (size_t)n_views, st));
    PP_CHECK_HIP(hipMemsetAsync(counts, 0, sizeof(int) * NC * (size_t)n_views, st));
    const int rc = raster_views(s, n, ws, near_count, st);
    if (rc != PP_OK) return rc;
    if (n.samples > 0) {
        hipLaunchKernelGGL(pose_verify_reduce_kernel, window_grid(n_views, n.max_window), dim3(BLOCK), 0, st, s, ev, ws.zbuf, counts);
    }
    return pp_last_launch();
}

}  // extern "C"
