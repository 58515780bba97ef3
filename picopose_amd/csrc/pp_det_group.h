// The group table of the scoring entries (include/picopose_hip.h, DETECTION SCORING and 6D DETECTION SCORING): a row is
// {first record of the scored side, its count, first ground truth, its count, offset of the group's row-major block}.
#ifndef PP_DET_GROUP_H
#define PP_DET_GROUP_H
#include "pp_common.h"

namespace {

constexpr int GF = PP_DET_GROUP_FIELDS;

struct Group {
    int d0, nd, g0, ng, off;
};

// Row g of the device group table.  The entry validated the host copy; a device copy that disagrees must not lead outside the
// buffers: then the group is empty on both sides.
__device__ __forceinline__ Group load_group(const int* __restrict__ groups, int n_groups, int g, int n_det, int n_gt, int n_pairs) {
    Group r = {0, 0, 0, 0, 0};
    if (g < 0 || g >= n_groups) return r;
    const int* p = groups + (size_t)g * GF;
    const int d0 = p[0], nd = p[1], g0 = p[2], ng = p[3], off = p[4];
    if (d0 < 0 || nd < 0 || g0 < 0 || ng < 0 || off < 0 || nd > n_det - d0 || ng > n_gt - g0 ||
        (long long)off + (long long)nd * ng > (long long)n_pairs)
        return r;
    r.d0 = d0, r.nd = nd, r.g0 = g0, r.ng = ng, r.off = off;
    return r;
}

// The host copy of the group table: ranges inside the call's detections and ground truths, blocks inside the ragged arrays.
inline bool groups_ok(const int* gh, int n_groups, int n_det, int n_gt, int n_pairs, int max_gt) {
    for (int g = 0; g < n_groups; ++g) {
        const int* p = gh + (size_t)g * GF;
        if (p[0] < 0 || p[1] < 0 || p[2] < 0 || p[3] < 0 || p[4] < 0 || p[1] > n_det - p[0] || p[3] > n_gt - p[2] || p[3] > max_gt) return false;
        if ((long long)p[4] + (long long)p[1] * p[3] > (long long)n_pairs) return false;
    }
    return true;
}

// The row of pp_pose_nms, {first estimate, E_g, offset of the group's triangle of E_g (E_g - 1) / 2 pairs}, and THE CHECKS of a row, the
// host copy's and the device copy's alike (as load_group: a device row that disagrees with the validated host copy gives an empty group).
struct NmsGroup {
    int e0, ne;
    long long off;
};

__host__ __device__ __forceinline__ bool nms_row_ok(int e0, int ne, int off, int n_est, int n_tri) {
    return !(e0 < 0 || ne < 0 || off < 0 || ne > n_est - e0 || ne > PP_POSE_MAX_GROUP ||
             (long long)off + (long long)ne * (ne - 1) / 2 > (long long)n_tri);
}

__device__ __forceinline__ NmsGroup load_nms_group(const int* __restrict__ groups, int g, int n_est, int n_tri) {
    const int* p = groups + (size_t)g * PP_POSE_NMS_FIELDS;
    const int e0 = p[0], ne = p[1], off = p[2];
    return nms_row_ok(e0, ne, off, n_est, n_tri) ? NmsGroup{e0, ne, off} : NmsGroup{0, 0, 0};
}

}  // namespace
#endif
