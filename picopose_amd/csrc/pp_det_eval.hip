// Detection scoring (include/picopose_hip.h, DETECTION SCORING; picopose_amd/detection_eval.py plans every call; tests/detection_eval_oracle.py
// restates the protocol in numpy loops): the overlaps of detections and ground truths inside each (image, category) group, and the
// greedy COCO matching per (group, area range, threshold).  Integers are counted, every IoU is ONE float64 division, nothing is
// accumulated in floating point and there is no atomic: every output is the same bits for any stream, chunking and launch shape.
#include <stdint.h>
#include <limits.h>
#include <math.h>
#include "pp_common.h"
#include "pp_bitrows_dev.h"
#include "pp_det_group.h"
#include "pp_reduce_dev.h"

namespace {

constexpr int WAVE = 64;
constexpr int MATCH_WAVES = 4;               // pp_det_match: independent waves of one workgroup, one (group, area range, threshold) each
                                             // (Group, load_group, groups_ok: pp_det_group.h; PAIR, a workgroup's tile of ONE group: pp_bitrows_dev.h)

// segm: inter = popcount(det row & gt row) over the words, iou = inter / (area_d + area_g - inter), for a crowd inter / area_d.  The
// detections are the bit rows [0, n_det), the ground truths the rows [n_det, n_det + n_gt): bitrow_tile_kernel (pp_bitrows_dev.h)
// with the group's detections on one side and its ground truths on the other.  Nothing of another group is read or written.
struct DetTile {
    const int *__restrict__ area, *__restrict__ groups, *__restrict__ tiles;
    const unsigned char* __restrict__ gt_flags;
    int words, n_det, n_gt, n_groups, n_pairs;
    int* __restrict__ inter;
    double* __restrict__ iou;
    __device__ long long sides(int& ri, int& i0, int& ni, int& rj, int& j0, int& nj) const {
        const int* tile = tiles + (size_t)blockIdx.x * 3;
        Group G = load_group(groups, n_groups, tile[0], n_det, n_gt, n_pairs);
        i0 = tile[1], j0 = tile[2];
        if (i0 < 0 || j0 < 0) G.nd = G.ng = i0 = j0 = 0;                      // (workgroup-uniform: every thread still meets the barriers)
        ri = G.d0 + i0, ni = G.nd, rj = n_det + G.g0 + j0, nj = G.ng;
        return G.off;
    }
    __device__ void store(int d, int g, size_t at, int count) const {         // (g: the ground truth's bit row, n_det + its index)
        const long long ad = area[d], ag = area[g];
        const long long den = (gt_flags[g - n_det] & PP_DET_GT_CROWD) ? ad : ad + ag - count;
        inter[at] = count;
        iou[at] = den > 0 ? (double)count / (double)den : 0.0;                // one IEEE division
    }
};

// bbox: one thread per pair of the tile, float64, never contracted (the header has the expression).
__global__ __launch_bounds__(PAIR * PAIR) void det_overlaps_bbox_kernel(const double* __restrict__ boxes, int n_det, int n_gt,
                                                                        const int* __restrict__ groups, int n_groups,
                                                                        const int* __restrict__ tiles,
                                                                        const unsigned char* __restrict__ gt_flags, int n_pairs,
                                                                        double* __restrict__ iou) {
#pragma clang fp contract(off)
    const int* tile = tiles + (size_t)blockIdx.x * 3;
    const Group G = load_group(groups, n_groups, tile[0], n_det, n_gt, n_pairs);
    const int i = tile[1] + (int)threadIdx.x / PAIR, j = tile[2] + (int)threadIdx.x % PAIR;
    if (tile[1] < 0 || tile[2] < 0 || i >= G.nd || j >= G.ng) return;
    const double* bd = boxes + (size_t)(G.d0 + i) * 4;
    const double* bg = boxes + (size_t)(n_det + G.g0 + j) * 4;
    const double xd = bd[0], yd = bd[1], wd = bd[2], hd = bd[3], xg = bg[0], yg = bg[1], wg = bg[2], hg = bg[3];
    const double iw = fmax(0.0, fmin(xd + wd, xg + wg) - fmax(xd, xg));
    const double ih = fmax(0.0, fmin(yd + hd, yg + hg) - fmax(yd, yg));
    const double num = iw * ih, ad = wd * hd;
    const double den = (gt_flags[G.g0 + j] & PP_DET_GT_CROWD) ? ad : (ad + wg * hg) - num;
    iou[(size_t)G.off + (size_t)i * G.ng + j] = den > 0.0 ? num / den : 0.0;
}

// One wave per (group, area range, threshold); the waves of a workgroup share nothing.  Lane l owns the ground truths j = l + 64 k of
// the group, k < 64 (G_g <= PP_DET_MAX_GT): their ignore, crowd and matched flags are three 64-bit registers of the lane.  The
// group order of the protocol (non-ignored first, stably) is never materialised: inside each class it is the input order, so THE
// CLOSED FORM reads "largest IoU, then highest index" per class, the non-ignored class first.  An IoU is not negative, so its bit
// pattern orders as the value does; a candidate has IoU >= best0 > 0, so the pattern 0 means "no candidate".
__global__ __launch_bounds__(MATCH_WAVES* WAVE) void det_match_kernel(const double* __restrict__ iou, int n_pairs,
                                                                      const int* __restrict__ groups, int n_groups, int n_det, int n_gt,
                                                                      const double* __restrict__ det_area, const double* __restrict__ gt_area,
                                                                      const unsigned char* __restrict__ gt_flags,
                                                                      const double* __restrict__ area_ranges, int A,
                                                                      const double* __restrict__ iou_thrs, int T, int* __restrict__ dt_match,
                                                                      unsigned char* __restrict__ dt_ignore, int* __restrict__ gt_match,
                                                                      unsigned char* __restrict__ gt_ignore) {
    const int lane = threadIdx.x & (WAVE - 1);
    const long long item = (long long)blockIdx.x * MATCH_WAVES + (threadIdx.x >> 6);
    if (item >= (long long)n_groups * A * T) return;                          // wave-uniform, and the kernel has no barrier
    const int t = (int)(item % T), ar = (int)((item / T) % A);
    const Group G = load_group(groups, n_groups, (int)(item / ((long long)T * A)), n_det, n_gt, n_pairs);
    if (G.ng > PP_DET_MAX_GT) return;
    const double lo = area_ranges[2 * ar], hi = area_ranges[2 * ar + 1];
    const double best0 = fmin(iou_thrs[t], 1.0 - 1e-10);
    const size_t drow = ((size_t)ar * T + t) * n_det + G.d0, grow = ((size_t)ar * T + t) * n_gt + G.g0;
    const int nk = (G.ng + WAVE - 1) / WAVE;
    unsigned long long ign = 0, crowd = 0, matched = 0;
    for (int k = 0; k < nk; ++k) {
        const int j = lane + WAVE * k;
        if (j < G.ng) {
            const unsigned f = gt_flags[G.g0 + j];
            const double ga = gt_area[G.g0 + j];
            const bool ig = (f & PP_DET_GT_IGNORE) != 0 || ga < lo || ga > hi;
            ign |= (unsigned long long)ig << k;
            crowd |= (unsigned long long)((f & PP_DET_GT_CROWD) != 0) << k;
            gt_match[grow + j] = -1;
            if (t == 0) gt_ignore[(size_t)ar * n_gt + G.g0 + j] = ig;
        }
    }
    for (int d = 0; d < G.nd; ++d) {
        const double* row = iou + (size_t)G.off + (size_t)d * G.ng;
        unsigned long long bn = 0, bi = 0;                                    // the lane's best candidate per class: IoU bits and index
        int jn = -1, ji = -1;
        for (int k = 0; k < nk; ++k) {
            const int j = lane + WAVE * k;
            if (j >= G.ng) break;
            if (((matched >> k) & 1) && !((crowd >> k) & 1)) continue;
            const double v = row[j];
            if (!(v >= best0)) continue;
            const unsigned long long vb = (unsigned long long)__double_as_longlong(v);
            if ((ign >> k) & 1) {
                if (vb >= bi) bi = vb, ji = j;                                // j ascends: >= keeps the highest index among equals
            } else {
                if (vb >= bn) bn = vb, jn = j;
            }
        }
        int m = -1;
        bool mig = false;
        const unsigned long long wn = wave_max(bn);
        if (wn != 0) {
            m = wave_max(bn == wn ? jn : -1);
        } else {
            const unsigned long long wi = wave_max(bi);
            if (wi != 0) m = wave_max(bi == wi ? ji : -1), mig = true;
        }
        if (m >= 0 && (m & (WAVE - 1)) == lane) {
            matched |= 1ull << (m >> 6);
            gt_match[grow + m] = G.d0 + d;
        }
        if (lane == 0) {
            const double da = det_area[G.d0 + d];
            dt_match[drow + d] = m >= 0 ? G.g0 + m : -1;
            dt_ignore[drow + d] = m >= 0 ? mig : (da < lo || da > hi);
        }
    }
}

}  // namespace

extern "C" {

int pp_det_overlaps(const unsigned* bits, const int* area, int words, const double* boxes, int n_det, int n_gt, const int* groups,
                    const int* groups_host, int n_groups, const int* tiles, const int* tiles_host, int n_tiles,
                    const unsigned char* gt_flags, int n_pairs, int* inter, double* iou, void* stream) {
    if (!groups || !groups_host || !gt_flags || !iou || n_det < 0 || n_gt < 0 || n_groups <= 0 || n_tiles < 0 || n_pairs < 0) return PP_EINVAL;
    if ((bits != nullptr) == (boxes != nullptr)) return PP_EINVAL;           // segm or bbox
    if (bits && (!area || !inter || words <= 0)) return PP_EINVAL;
    if (n_tiles > 0 && (!tiles || !tiles_host)) return PP_EINVAL;
    if (!groups_ok(groups_host, n_groups, n_det, n_gt, n_pairs, INT_MAX)) return PP_EINVAL;
    for (int k = 0; k < n_tiles; ++k) {
        const int* tl = tiles_host + (size_t)k * 3;
        if (tl[0] < 0 || tl[0] >= n_groups || tl[1] < 0 || tl[2] < 0 || tl[1] % PAIR != 0 || tl[2] % PAIR != 0) return PP_EINVAL;
        const int* p = groups_host + (size_t)tl[0] * GF;
        if (tl[1] >= p[1] || tl[2] >= p[3]) return PP_EINVAL;
    }
    if (n_tiles == 0) return PP_OK;                                           // every group has an empty side: no pair, no launch
    if (bits)
        hipLaunchKernelGGL(bitrow_tile_kernel<DetTile>, dim3(n_tiles), dim3(PAIR_THREADS), 0, (hipStream_t)stream, bits,
                           DetTile{area, groups, tiles, gt_flags, words, n_det, n_gt, n_groups, n_pairs, inter, iou});
    else
        hipLaunchKernelGGL(det_overlaps_bbox_kernel, dim3(n_tiles), dim3(PAIR * PAIR), 0, (hipStream_t)stream, boxes, n_det, n_gt, groups,
                           n_groups, tiles, gt_flags, n_pairs, iou);
    return pp_last_launch();
}

int pp_det_match(const double* iou, int n_pairs, const int* groups, const int* groups_host, int n_groups, int n_det, int n_gt,
                 const double* det_area, const double* gt_area, const unsigned char* gt_flags, const double* area_ranges,
                 const double* area_ranges_host, int A, const double* iou_thrs, const double* iou_thrs_host, int T, int* dt_match,
                 unsigned char* dt_ignore, int* gt_match, unsigned char* gt_ignore, void* stream) {
    if (!iou || !groups || !groups_host || !det_area || !gt_area || !gt_flags || !area_ranges || !area_ranges_host || !iou_thrs ||
        !iou_thrs_host || !dt_match || !dt_ignore || !gt_match || !gt_ignore)
        return PP_EINVAL;
    if (n_pairs < 0 || n_groups <= 0 || n_det < 0 || n_gt < 0 || A <= 0 || T <= 0) return PP_EINVAL;
    for (int t = 0; t < T; ++t)
        if (!(iou_thrs_host[t] > 0.0 && iou_thrs_host[t] <= 1.0)) return PP_EINVAL;
    for (int a = 0; a < A; ++a)
        if (!(area_ranges_host[2 * a] <= area_ranges_host[2 * a + 1])) return PP_EINVAL;   // (a NaN fails too)
    if (!groups_ok(groups_host, n_groups, n_det, n_gt, n_pairs, PP_DET_MAX_GT)) return PP_EINVAL;
    const long long items = (long long)n_groups * A * T, blocks = (items + MATCH_WAVES - 1) / MATCH_WAVES;
    if (blocks > 0x7fffffffLL) return PP_EINVAL;
    hipLaunchKernelGGL(det_match_kernel, dim3((unsigned)blocks), dim3(MATCH_WAVES * WAVE), 0, (hipStream_t)stream, iou, n_pairs, groups,
                       n_groups, n_det, n_gt, det_area, gt_area, gt_flags, area_ranges, A, iou_thrs, T, dt_match, dt_ignore, gt_match,
                       gt_ignore);
    return pp_last_launch();
}

}  // extern "C"
