// 6D detection scoring (include/picopose_hip.h, 6D DETECTION SCORING; picopose_amd/pose_detection_eval.py plans every call;
// tests/pose_detection_oracle.py restates the protocol in numpy loops): the greedy matching of pose estimates to ground truths per
// (group, metric, threshold), and the walk that suppresses duplicate poses.  The errors and distances are inputs (pp_pose_errors
// writes them); here they are only compared: no atomic, no floating-point accumulation, no LDS, no barrier — every output is the
// same bits for any stream and launch shape.
#include <stdint.h>
#include <limits.h>
#include <math.h>
#include "pp_common.h"
#include "pp_det_group.h"
#include "pp_reduce_dev.h"

namespace {

constexpr int WAVE = 64;
constexpr int POSE_WAVES = 4;                // independent waves of one workgroup, one problem each
constexpr unsigned NONE = 0xffffffffu;       // "no candidate": the pattern of a NaN, which never qualifies

// One wave per (group, metric, threshold); the waves of a workgroup share nothing.  Lane l owns the ground truths j = l + 64 k of
// the group, k < 64 (G_g <= PP_POSE_MAX_GROUP): their ignore and matched flags are two 64-bit registers of the lane.  A qualifying
// error has its sign bit clear, so its bit pattern orders as the value does.
__global__ __launch_bounds__(POSE_WAVES* WAVE) void pose_match_kernel(const float* __restrict__ err, int M, int n_pairs,
                                                                      const int* __restrict__ groups, int n_groups, int n_est, int n_gt,
                                                                      const unsigned char* __restrict__ gt_ignore,
                                                                      const double* __restrict__ limits, int T, int* __restrict__ est_match,
                                                                      unsigned char* __restrict__ est_ignore, int* __restrict__ gt_match) {
    const int lane = threadIdx.x & (WAVE - 1);
    const long long item = (long long)blockIdx.x * POSE_WAVES + (threadIdx.x >> 6);
    if (item >= (long long)n_groups * M * T) return;                          // wave-uniform, and the kernel has no barrier
    const int t = (int)(item % T), m = (int)((item / T) % M), g = (int)(item / ((long long)T * M));
    const Group G = load_group(groups, n_groups, g, n_est, n_gt, n_pairs);
    if (G.ng > PP_POSE_MAX_GROUP) return;
    const double limit = limits[((size_t)g * M + m) * T + t];
    const size_t erow = ((size_t)m * T + t) * n_est + G.d0, grow = ((size_t)m * T + t) * n_gt + G.g0;
    const float* block = err + (size_t)m * n_pairs + G.off;
    const int nk = (G.ng + WAVE - 1) / WAVE;
    unsigned long long ign = 0, matched = 0;
    for (int k = 0; k < nk; ++k) {
        const int j = lane + WAVE * k;
        if (j < G.ng) {
            ign |= (unsigned long long)(gt_ignore[G.g0 + j] != 0) << k;
            gt_match[grow + j] = -1;
        }
    }
    for (int e = 0; e < G.nd; ++e) {
        const float* row = block + (size_t)e * G.ng;
        unsigned bn = NONE, bi = NONE;                                        // the lane's best candidate per class: error bits and index
        int jn = INT_MAX, ji = INT_MAX;
        for (int k = 0; k < nk; ++k) {
            const int j = lane + WAVE * k;
            if (j >= G.ng) break;
            if ((matched >> k) & 1) continue;
            const float v = row[j];
            const unsigned vb = __float_as_uint(v);
            if ((vb >> 31) || !((double)v < limit)) continue;                 // (a NaN and +inf fail the comparison)
            if ((ign >> k) & 1) {
                if (vb < bi) bi = vb, ji = j;                                 // j ascends: < keeps the lowest index among equals
            } else {
                if (vb < bn) bn = vb, jn = j;
            }
        }
        int w = -1;
        bool wig = false;
        const unsigned wn = wave_min(bn);
        if (wn != NONE) {
            w = wave_min(bn == wn ? jn : INT_MAX);
        } else {
            const unsigned wi = wave_min(bi);
            if (wi != NONE) w = wave_min(bi == wi ? ji : INT_MAX), wig = true;
        }
        if (w >= 0 && (w & (WAVE - 1)) == lane) {
            matched |= 1ull << (w >> 6);
            gt_match[grow + w] = G.d0 + e;
        }
        if (lane == 0) {
            est_match[erow + e] = w >= 0 ? G.g0 + w : -1;
            est_ignore[erow + e] = wig;
        }
    }
}

// One wave per group (its row: pp_det_group.h).  Lane l owns the positions p = l + 64 k of the group's order; bit k of `kept` says that
// p was kept.  Candidate j reads its j earlier partners, contiguous in the triangle, 64 at a time; one ballot per 64 says whether a kept one is near.
__global__ __launch_bounds__(POSE_WAVES* WAVE) void pose_nms_kernel(const float* __restrict__ dist, int n_tri, const int* __restrict__ groups,
                                                                    int n_groups, int n_est, const double* __restrict__ limit,
                                                                    unsigned char* __restrict__ keep) {
    const int lane = threadIdx.x & (WAVE - 1);
    const int g = blockIdx.x * POSE_WAVES + (threadIdx.x >> 6);
    if (g >= n_groups) return;                                                // wave-uniform, and the kernel has no barrier
    const NmsGroup G = load_nms_group(groups, g, n_est, n_tri);
    const double lim = limit[g];
    unsigned long long kept = 0;
    for (int j = 0; j < G.ne; ++j) {
        const float* row = dist + G.off + (long long)j * (j - 1) / 2;
        bool near = false;
        for (int k = 0; WAVE * k < j && !near; ++k) {                         // (near comes from a ballot: uniform over the wave)
            const int i = lane + WAVE * k;
            const bool hit = i < j && ((kept >> k) & 1) && (double)row[i] < lim;
            near = __ballot(hit) != 0ull;
        }
        if (!near && (j & (WAVE - 1)) == lane) kept |= 1ull << (j >> 6);
        if (lane == 0) keep[G.e0 + j] = !near;
    }
}

}  // namespace

extern "C" {

int pp_pose_match(const float* err, int M, int n_pairs, const int* groups, const int* groups_host, int n_groups, int n_est, int n_gt,
                  const unsigned char* gt_ignore, const double* limits, const double* limits_host, int T, int* est_match,
                  unsigned char* est_ignore, int* gt_match, void* stream) {
    if (!err || !groups || !groups_host || !gt_ignore || !limits || !limits_host || !est_match || !est_ignore || !gt_match) return PP_EINVAL;
    if (n_pairs < 0 || n_est < 0 || n_gt < 0 || n_groups <= 0 || M <= 0 || M > PP_POSE_MAX_METRICS || T <= 0) return PP_EINVAL;
    if (!groups_ok(groups_host, n_groups, n_est, n_gt, n_pairs, PP_POSE_MAX_GROUP)) return PP_EINVAL;
    const long long items = (long long)n_groups * M * T, blocks = (items + POSE_WAVES - 1) / POSE_WAVES;
    if (blocks > 0x7fffffffLL) return PP_EINVAL;
    for (long long k = 0; k < items; ++k)
        if (limits_host[k] != limits_host[k]) return PP_EINVAL;
    hipLaunchKernelGGL(pose_match_kernel, dim3((unsigned)blocks), dim3(POSE_WAVES * WAVE), 0, (hipStream_t)stream, err, M, n_pairs, groups,
                       n_groups, n_est, n_gt, gt_ignore, limits, T, est_match, est_ignore, gt_match);
    return pp_last_launch();
}

int pp_pose_nms(const float* dist, int n_tri, const int* groups, const int* groups_host, int n_groups, int n_est, const double* limit,
                const double* limit_host, unsigned char* keep, void* stream) {
    if (!dist || !groups || !groups_host || !limit || !limit_host || !keep) return PP_EINVAL;
    if (n_tri < 0 || n_est < 0 || n_groups <= 0) return PP_EINVAL;
    for (int g = 0; g < n_groups; ++g) {
        const int* p = groups_host + (size_t)g * PP_POSE_NMS_FIELDS;
        if (!nms_row_ok(p[0], p[1], p[2], n_est, n_tri) || !(limit_host[g] >= 0.0)) return PP_EINVAL;      // (a NaN limit fails too)
    }
    hipLaunchKernelGGL(pose_nms_kernel, dim3((unsigned)((n_groups + POSE_WAVES - 1) / POSE_WAVES)), dim3(POSE_WAVES * WAVE), 0,
                       (hipStream_t)stream, dist, n_tri, groups, n_groups, n_est, limit, keep);
    return pp_last_launch();
}

}  // extern "C"
