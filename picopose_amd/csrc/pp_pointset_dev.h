// The all-pairs core of the point-set kernels: pp_eval.hip (ADD-S) and pp_model_info.hip (diameter, directed Hausdorff distance).
// Internal linkage: every translation unit gets its own copy.  Include it AFTER `#pragma clang fp contract(off)`.
//
//   apply               the rigid 12-float map, one rounding per operation in the stated order (the numpy restatements do the same)
//   Points, Mapped      loaders: point c of a packed (n, 3) array as it is, or under a map
//   load_lane_points    the register side: a workgroup owns P * 256 consecutive points of a set, P per lane
//   stream_pairs        the other side, a range [j0, j1) of a set, through a 256-entry float4 LDS tile (broadcast reads):
//                       visit(k, j, d2) per (register point k of the lane, streamed point j), j ascending, with
//                       d2 = (dx dx + dy dy) + dz dz in difference form, rounded per operation
//   RunningMin          the visitor of a nearest-neighbour search
//
// The core knows neither which side is transformed nor what becomes of d2: both are the caller's callables, and so is its reduction.
// A lane's point past the set's last one repeats the last one with valid[k] = false; the caller leaves it out of its reduction.
#ifndef PP_POINTSET_DEV_H
#define PP_POINTSET_DEV_H
#include "pp_common.h"

namespace {

constexpr int POINT_BLOCK = 256;       // lanes of a workgroup, and streamed points per LDS tile

// X = ((T0 x + T1 y) + T2 z) + T9, ... : one rounding per operation, in this order
__device__ __forceinline__ void apply(const float* __restrict__ T, float x, float y, float z, float& X, float& Y, float& Z) {
    X = ((T[0] * x + T[1] * y) + T[2] * z) + T[9];
    Y = ((T[3] * x + T[4] * y) + T[5] * z) + T[10];
    Z = ((T[6] * x + T[7] * y) + T[8] * z) + T[11];
}

struct Points {
    const float* p;
    __device__ __forceinline__ void operator()(size_t c, float& X, float& Y, float& Z) const { X = p[3 * c], Y = p[3 * c + 1], Z = p[3 * c + 2]; }
};

struct Mapped {
    const float* p;
    const float* T;                    // 12 floats, in the caller's registers
    __device__ __forceinline__ void operator()(size_t c, float& X, float& Y, float& Z) const { apply(T, p[3 * c], p[3 * c + 1], p[3 * c + 2], X, Y, Z); }
};

template <int P>
struct LanePoints {
    float x[P], y[P], z[P];
    bool valid[P];
};

// point k of the lane: index i0 + k * 256 + lane of a set of n points, clamped to the last one
template <int P, class Load>
__device__ __forceinline__ void load_lane_points(int i0, int n, Load load, LanePoints<P>& out) {
#pragma unroll
    for (int k = 0; k < P; ++k) {
        const int i = i0 + k * POINT_BLOCK + (int)threadIdx.x;
        out.valid[k] = i < n;
        load((size_t)(out.valid[k] ? i : n - 1), out.x[k], out.y[k], out.z[k]);
    }
}

// sh: the caller's __shared__ float4[POINT_BLOCK].  Every lane of the workgroup must call it with the same range (barriers).
template <int P, class Load, class Visit>
__device__ __forceinline__ void stream_pairs(const LanePoints<P>& a, int j0, int j1, float4* sh, Load load, Visit&& visit) {
    for (int g0 = j0; g0 < j1; g0 += POINT_BLOCK) {
        const int cnt = j1 - g0 < POINT_BLOCK ? j1 - g0 : POINT_BLOCK;
        __syncthreads();
        if ((int)threadIdx.x < cnt) {
            float X, Y, Z;
            load((size_t)(g0 + (int)threadIdx.x), X, Y, Z);
            sh[threadIdx.x] = make_float4(X, Y, Z, 0.f);
        }
        __syncthreads();
        for (int q = 0; q < cnt; ++q) {
            const float4 g = sh[q];
#pragma unroll
            for (int k = 0; k < P; ++k) {
                const float dx = a.x[k] - g.x, dy = a.y[k] - g.y, dz = a.z[k] - g.z;
                visit(k, g0 + q, (dx * dx + dy * dy) + dz * dz);
            }
        }
    }
}

// per register point the smallest d2 seen: exact, whatever the order
template <int P>
struct RunningMin {
    float d2[P];
    __device__ __forceinline__ RunningMin() {
#pragma unroll
        for (int k = 0; k < P; ++k) d2[k] = INFINITY;
    }
    __device__ __forceinline__ void operator()(int k, int, float v) { d2[k] = fminf(d2[k], v); }
};

}  // namespace
#endif
