// The counter-based hash of include/picopose_hip.h ("Training-pair assembly": h(seed, a, b)), stated once for every kernel that draws
// from it: the augmenter's dropout cells and noise (pp_augment.hip) and the lattice background of the scene composite (pp_synth.hip).
// Keyed by (seed, two counters), never by thread.  The RANSAC sampler of the pose solvers (pp_ransac_dev.h) draws from aug_mix alone.
#ifndef PP_HASH_DEV_H
#define PP_HASH_DEV_H
#include <hip/hip_runtime.h>

__device__ __forceinline__ unsigned aug_mix(unsigned x) {
    x ^= x >> 16;
    x *= 0x7feb352du;
    x ^= x >> 15;
    x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}
__device__ __forceinline__ unsigned aug_hash(unsigned seed, unsigned a, unsigned b) {
    return aug_mix(seed ^ aug_mix(a ^ aug_mix(b + 0x9e3779b9u)));
}

#endif
