// The run tables of COCO-RLE masks ("run_ends, run_offset, run_offset_host" of pp_detections_crop in include/picopose_hip.h;
// picopose_amd/masks.py builds them): the cumulative run ends of a call's masks in one int32 array, mask d owning the slice
// run_offset[d] .. run_offset[d + 1], an odd run index a run of ones.  What every reader of the tables needs, stated once for
// pp_detections_crop (pp_detect.hip), pp_rle_pack_bits (pp_proposals.hip) and pp_components_rle (pp_depth_proposals.hip): the host
// check of the offsets, the device clamp of a slice, and the search over the ends.
#ifndef PP_RUNS_DEV_H
#define PP_RUNS_DEV_H
#include <hip/hip_runtime.h>

// The host copy of the n + 1 offsets: not negative at the start, not decreasing, not past n_runs.
static inline bool pp_run_offsets_ok(const int* run_offset_host, int n, int n_runs) {
    if (run_offset_host[0] < 0 || run_offset_host[n] > n_runs) return false;
    for (int d = 0; d < n; ++d)
        if (run_offset_host[d + 1] < run_offset_host[d]) return false;
    return true;
}

// Mask d's slice [r0, r1) of run_ends from the device table.  The entry validated the host copy; a device copy that disagrees must
// not lead outside the buffer: then false, and the slice is empty.
__device__ __forceinline__ bool pp_run_slice(const int* __restrict__ run_offset, int d, int n_runs, int& r0, int& r1) {
    r0 = run_offset[d];
    r1 = run_offset[d + 1];
    if (r0 >= 0 && r1 >= r0 && r1 <= n_runs) return true;
    r0 = r1 = 0;
    return false;
}

// ends[0..m) sorted: how many are <= key.  Position p lies in the mask when that count (plus the runs before ends[0]) is odd.
__device__ __forceinline__ int pp_count_le(const int* ends, int m, int key) {
    int lo = 0, hi = m;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (ends[mid] <= key) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

#endif
