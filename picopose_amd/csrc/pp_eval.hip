// BOP pose errors of (estimate, ground truth) pairs: MSSD, MSPD, ADD, ADD-S (picopose_amd/evaluation.py plans every call;
// the contract is stated in include/picopose_hip.h and restated in numpy by tests/pose_error_oracle.py).
//
//   compose_kernel   (pair, symmetry) -> one float32 affine map  R_gt R_S, R_gt t_S + t_gt  (float64 arithmetic, rounded once)
//   sym_max_kernel   one workgroup per (pair, tile of TS symmetries): walks the object's vertices, the estimate's point in registers
//                    across the tile, running maximum of the SQUARED distance per symmetry; wave reduction by shuffles, waves through
//                    LDS, one square root per (pair, symmetry)
//   add_kernel       one workgroup per pair: per-lane float64 partial sums of the distances, fixed reduction tree
//   adds_kernel      all-pairs nearest neighbour on pp_pointset_dev.h's core: a workgroup owns ADDS_TILE estimate-side points (ADDS_EPT
//                    per lane, in registers), streams the ground-truth-side points through LDS, running minimum of the squared distance
//   finalize_kernel  one wave per pair: minimum over the symmetries with its index (lowest index on a tie), ADD-S tile sums in order
//
// Maximum and minimum are exact and order-independent and every sum has a fixed tree: the results do not depend on launch order,
// stream, pair order or the chunking of the pairs.  No atomics.
#include <stdint.h>
#include <limits.h>
#include <math.h>
#include "pp_common.h"

#pragma clang fp contract(off)
#include "pp_pointset_dev.h"
#include "pp_reduce_dev.h"

namespace {

constexpr int BLOCK = POINT_BLOCK;
constexpr int WAVES = BLOCK / 64;
constexpr int TS = 4;                              // symmetries per workgroup of sym_max_kernel
constexpr int ADDS_EPT = PP_EVAL_ADDS_TILE / BLOCK;  // estimate-side points per lane of adds_kernel
static_assert(PP_EVAL_ADDS_TILE % BLOCK == 0, "ADD-S tile");

__global__ __launch_bounds__(BLOCK) void compose_kernel(const int* __restrict__ pair_obj, const float* __restrict__ R_gt,
                                                        const float* __restrict__ t_gt, const float* __restrict__ sym_R,
                                                        const float* __restrict__ sym_t, const int* __restrict__ sym_off, int P,
                                                        int S_max, float* __restrict__ xf) {
    const long long i = (long long)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= (long long)P * S_max) return;
    const int p = (int)(i / S_max), s = (int)(i % S_max);
    const int o = pair_obj[p];
    const int s0 = sym_off[o], ns = sym_off[o + 1] - s0;
    if (s >= ns) return;
    const float* A = R_gt + 9 * (size_t)p;
    const float* B = sym_R + 9 * (size_t)(s0 + s);
    const float* b = sym_t + 3 * (size_t)(s0 + s);
    float* out = xf + 12 * (size_t)i;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const double a0 = A[3 * r], a1 = A[3 * r + 1], a2 = A[3 * r + 2];
#pragma unroll
        for (int c = 0; c < 3; ++c) out[3 * r + c] = (float)((a0 * (double)B[c] + a1 * (double)B[3 + c]) + a2 * (double)B[6 + c]);
        out[9 + r] = (float)(((a0 * (double)b[0] + a1 * (double)b[1]) + a2 * (double)b[2]) + (double)t_gt[3 * (size_t)p + r]);
    }
}

// KIND 0: MSSD (squared distance in millimetres), KIND 1: MSPD (squared distance in pixels; u = (fx X) (1 / Z), the principal point
// cancels in the difference and is never added).  err[p * S_max + s] = sqrt(max over the vertices).
template <int KIND>
__global__ __launch_bounds__(BLOCK) void sym_max_kernel(const float* __restrict__ verts, const int* __restrict__ vert_off,
                                                        const int* __restrict__ sym_off, const int* __restrict__ pair_obj,
                                                        const float* __restrict__ R_est, const float* __restrict__ t_est,
                                                        const float* __restrict__ focal, const float* __restrict__ xf, int S_max,
                                                        float* __restrict__ err) {
    const int p = blockIdx.x, s_base = blockIdx.y * TS;
    const int o = pair_obj[p];
    const int ns = sym_off[o + 1] - sym_off[o];
    if (s_base >= ns) return;                                    // (uniform: before any barrier)
    const int v0 = vert_off[o], nv = vert_off[o + 1] - v0;
    float E[12];
#pragma unroll
    for (int k = 0; k < 9; ++k) E[k] = R_est[9 * (size_t)p + k];
#pragma unroll
    for (int k = 0; k < 3; ++k) E[9 + k] = t_est[3 * (size_t)p + k];
    float fx = 0.f, fy = 0.f;
    if (KIND == 1) {
        fx = focal[2 * (size_t)p];
        fy = focal[2 * (size_t)p + 1];
    }
    // a tile's symmetries past the object's last one repeat the last one (their result is not written)
    const float* T[TS];
#pragma unroll
    for (int j = 0; j < TS; ++j) T[j] = xf + 12 * ((size_t)p * S_max + (s_base + j < ns ? s_base + j : ns - 1));
    float m[TS];
#pragma unroll
    for (int j = 0; j < TS; ++j) m[j] = 0.f;
    const float* vp = verts + 3 * (size_t)v0;
    for (int i = threadIdx.x; i < nv; i += BLOCK) {
        const float x = vp[3 * (size_t)i], y = vp[3 * (size_t)i + 1], z = vp[3 * (size_t)i + 2];
        float Xe, Ye, Ze, ue = 0.f, ve = 0.f, pen_e = 0.f;
        apply(E, x, y, z, Xe, Ye, Ze);
        if (KIND == 1) {
            const float rz = 1.f / Ze;
            ue = (fx * Xe) * rz;
            ve = (fy * Ye) * rz;
            pen_e = Ze > 0.f ? 0.f : INFINITY;                   // a point at or behind the camera plane: +inf
        }
#pragma unroll
        for (int j = 0; j < TS; ++j) {
            float Xg, Yg, Zg;
            apply(T[j], x, y, z, Xg, Yg, Zg);
            if (KIND == 0) {
                const float dx = Xe - Xg, dy = Ye - Yg, dz = Ze - Zg;
                const float d2 = (dx * dx + dy * dy) + dz * dz;
                m[j] = fmaxf(m[j], d2 == d2 ? d2 : INFINITY);    // a NaN (a non-finite pose) must not be dropped by fmaxf: +inf
            } else {                                             // (selects, no branch: every lane does the same work)
                const float rz = 1.f / Zg;
                const float du = ue - (fx * Xg) * rz, dv = ve - (fy * Yg) * rz;
                float d2 = du * du + dv * dv;
                d2 = d2 == d2 ? d2 : INFINITY;
                const float pen = Zg > 0.f ? pen_e : INFINITY;
                m[j] = fmaxf(m[j], fmaxf(d2, pen));
            }
        }
    }
    __shared__ float sm[WAVES][TS];
    const float v = block_reduce_to<WAVES>(m, sm, op_max{});
    if (threadIdx.x < TS && s_base + (int)threadIdx.x < ns) err[(size_t)p * S_max + s_base + threadIdx.x] = sqrtf(v);
}

__global__ __launch_bounds__(BLOCK) void add_kernel(const float* __restrict__ verts, const int* __restrict__ vert_off,
                                                    const int* __restrict__ pair_obj, const float* __restrict__ R_est,
                                                    const float* __restrict__ t_est, const float* __restrict__ R_gt,
                                                    const float* __restrict__ t_gt, float* __restrict__ out) {
    const int p = blockIdx.x;
    const int o = pair_obj[p];
    const int v0 = vert_off[o], nv = vert_off[o + 1] - v0;
    float E[12], G[12];
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        E[k] = R_est[9 * (size_t)p + k];
        G[k] = R_gt[9 * (size_t)p + k];
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        E[9 + k] = t_est[3 * (size_t)p + k];
        G[9 + k] = t_gt[3 * (size_t)p + k];
    }
    const float* vp = verts + 3 * (size_t)v0;
    double acc = 0.0;
    for (int i = threadIdx.x; i < nv; i += BLOCK) {
        const float x = vp[3 * (size_t)i], y = vp[3 * (size_t)i + 1], z = vp[3 * (size_t)i + 2];
        float Xe, Ye, Ze, Xg, Yg, Zg;
        apply(E, x, y, z, Xe, Ye, Ze);
        apply(G, x, y, z, Xg, Yg, Zg);
        const float dx = Xe - Xg, dy = Ye - Yg, dz = Ze - Zg;
        acc = acc + (double)sqrtf((dx * dx + dy * dy) + dz * dz);
    }
    __shared__ double sm[WAVES];
    const double s = block_reduce_all<WAVES>(acc, sm, op_sum{});   // (float64, in the fixed tree of pp_reduce_dev.h)
    if (threadIdx.x == 0) out[p] = (float)(s / (double)nv);
}

__global__ __launch_bounds__(BLOCK) void adds_kernel(const float* __restrict__ verts, const int* __restrict__ vert_off,
                                                     const int* __restrict__ pair_obj, const float* __restrict__ R_est,
                                                     const float* __restrict__ t_est, const float* __restrict__ R_gt,
                                                     const float* __restrict__ t_gt, int tiles_max, double* __restrict__ part) {
    const int p = blockIdx.x, tile = blockIdx.y;
    const int o = pair_obj[p];
    const int v0 = vert_off[o], nv = vert_off[o + 1] - v0;
    if ((long long)tile * PP_EVAL_ADDS_TILE >= nv) return;       // (uniform: before any barrier)
    float E[12], G[12];
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        E[k] = R_est[9 * (size_t)p + k];
        G[k] = R_gt[9 * (size_t)p + k];
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        E[9 + k] = t_est[3 * (size_t)p + k];
        G[9 + k] = t_gt[3 * (size_t)p + k];
    }
    const float* vp = verts + 3 * (size_t)v0;
    LanePoints<ADDS_EPT> e;
    load_lane_points(tile * PP_EVAL_ADDS_TILE, nv, Mapped{vp, E}, e);
    RunningMin<ADDS_EPT> mn;
    __shared__ float4 sh[POINT_BLOCK];
    stream_pairs(e, 0, nv, sh, Mapped{vp, G}, mn);
    double acc = 0.0;
#pragma unroll
    for (int k = 0; k < ADDS_EPT; ++k)
        if (e.valid[k]) acc = acc + (double)sqrtf(mn.d2[k]);
    __shared__ double sm[WAVES];
    const double s = block_reduce_all<WAVES>(acc, sm, op_sum{});   // (float64, in the fixed tree of pp_reduce_dev.h)
    if (threadIdx.x == 0) part[(size_t)p * tiles_max + tile] = s;
}

// the least of e[0..ns) with NaN read as +inf, the lowest index among equals; one wave, lane 0 writes
struct ErrAt {
    float v;
    int i;
};
__device__ __forceinline__ void least_error(const float* __restrict__ e, int ns, int lane, float* out, int* out_idx) {
    const auto lower = [](ErrAt a, const ErrAt& b) {
        if (b.v < a.v || (b.v == a.v && b.i < a.i)) a = b;
        return a;
    };
    ErrAt best{INFINITY, INT_MAX};
    for (int s = lane; s < ns; s += 64) {
        const float v = e[s];
        best = lower(best, ErrAt{v == v ? v : INFINITY, s});
    }
    best = wave_reduce(best, lower);
    if (lane == 0) {
        *out = best.v;
        *out_idx = best.i;
    }
}

__global__ __launch_bounds__(BLOCK) void finalize_kernel(const int* __restrict__ pair_obj, const int* __restrict__ sym_off,
                                                         const int* __restrict__ adds_off, int P, int S_max, int tiles_max,
                                                         const float* __restrict__ err_mssd, const float* __restrict__ err_mspd,
                                                         const double* __restrict__ part, float* __restrict__ mssd,
                                                         int* __restrict__ mssd_sym, float* __restrict__ mspd,
                                                         int* __restrict__ mspd_sym, float* __restrict__ adds) {
    const int p = blockIdx.x * WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (p >= P) return;
    const int o = pair_obj[p];
    const int ns = sym_off[o + 1] - sym_off[o];
    if (err_mssd) least_error(err_mssd + (size_t)p * S_max, ns, lane, mssd + p, mssd_sym + p);
    if (err_mspd) least_error(err_mspd + (size_t)p * S_max, ns, lane, mspd + p, mspd_sym + p);
    if (part && lane == 0) {
        const int nv = adds_off[o + 1] - adds_off[o];
        const int nt = (nv + PP_EVAL_ADDS_TILE - 1) / PP_EVAL_ADDS_TILE;
        double s = 0.0;
        for (int t = 0; t < nt; ++t) s = s + part[(size_t)p * tiles_max + t];
        adds[p] = (float)(s / (double)nv);
    }
}

struct Layout {
    size_t xf, err0, err1, part, total;
};

inline Layout layout(size_t P, size_t S_max, size_t tiles, int kinds) {
    Layout l;
    const bool sym = kinds & (PP_EVAL_MSSD | PP_EVAL_MSPD);
    size_t at = 0;
    l.xf = at;
    at += align256(sym ? P * S_max * 12 * sizeof(float) : 0);
    l.err0 = at;
    at += align256((kinds & PP_EVAL_MSSD) ? P * S_max * sizeof(float) : 0);
    l.err1 = at;
    at += align256((kinds & PP_EVAL_MSPD) ? P * S_max * sizeof(float) : 0);
    l.part = at;
    at += align256((kinds & PP_EVAL_ADDS) ? P * tiles * sizeof(double) : 0);
    l.total = at > 0 ? at : 256;
    return l;
}

inline bool bad_sizes(int n_pairs, int max_syms, int max_adds_vertices, int kinds) {
    return n_pairs <= 0 || max_syms <= 0 || max_syms > 65535 * TS || max_adds_vertices <= 0 || kinds <= 0 ||
           (kinds & ~(PP_EVAL_MSSD | PP_EVAL_MSPD | PP_EVAL_ADD | PP_EVAL_ADDS)) != 0 ||
           (long long)n_pairs * max_syms > (long long)INT_MAX;
}

}  // namespace

extern "C" {

int pp_pose_errors_workspace_bytes(int n_pairs, int max_syms, int max_adds_vertices, int kinds, size_t* bytes) {
    if (!bytes || bad_sizes(n_pairs, max_syms, max_adds_vertices, kinds)) return PP_EINVAL;
    const size_t tiles = ((size_t)max_adds_vertices + PP_EVAL_ADDS_TILE - 1) / PP_EVAL_ADDS_TILE;
    *bytes = layout((size_t)n_pairs, (size_t)max_syms, tiles, kinds).total;
    return PP_OK;
}

int pp_pose_errors(const float* vertices, const int* vert_off, const float* adds_vertices, const int* adds_off, const float* sym_R,
                   const float* sym_t, const int* sym_off, const int* vert_off_host, const int* adds_off_host,
                   const int* sym_off_host, int n_objects, const int* pair_obj, const int* pair_obj_host, const float* R_est,
                   const float* t_est, const float* R_gt, const float* t_gt, const float* focal, int n_pairs, int kinds,
                   void* workspace, size_t workspace_bytes, float* mssd, int* mssd_sym, float* mspd, int* mspd_sym, float* add,
                   float* adds, void* stream) {
    if (!vertices || !vert_off || !adds_vertices || !adds_off || !sym_R || !sym_t || !sym_off || !vert_off_host || !adds_off_host ||
        !sym_off_host || !pair_obj || !pair_obj_host || !R_est || !t_est || !R_gt || !t_gt || !workspace || n_objects <= 0 ||
        n_pairs <= 0 || kinds <= 0 || (kinds & ~(PP_EVAL_MSSD | PP_EVAL_MSPD | PP_EVAL_ADD | PP_EVAL_ADDS)) != 0)
        return PP_EINVAL;
    if (((kinds & PP_EVAL_MSSD) && (!mssd || !mssd_sym)) || ((kinds & PP_EVAL_MSPD) && (!mspd || !mspd_sym || !focal)) ||
        ((kinds & PP_EVAL_ADD) && !add) || ((kinds & PP_EVAL_ADDS) && !adds))
        return PP_EINVAL;
    if (vert_off_host[0] != 0 || adds_off_host[0] != 0 || sym_off_host[0] != 0) return PP_EINVAL;
    for (int o = 0; o < n_objects; ++o)
        if (vert_off_host[o + 1] <= vert_off_host[o] || adds_off_host[o + 1] <= adds_off_host[o] ||
            sym_off_host[o + 1] <= sym_off_host[o])
            return PP_EINVAL;
    int S_max = 0, nv_adds = 0;
    for (int p = 0; p < n_pairs; ++p) {
        const int o = pair_obj_host[p];
        if ((unsigned)o >= (unsigned)n_objects) return PP_EINVAL;
        const int ns = sym_off_host[o + 1] - sym_off_host[o], na = adds_off_host[o + 1] - adds_off_host[o];
        S_max = ns > S_max ? ns : S_max;
        nv_adds = na > nv_adds ? na : nv_adds;
    }
    if (bad_sizes(n_pairs, S_max, nv_adds, kinds)) return PP_EINVAL;
    const int tiles = (nv_adds + PP_EVAL_ADDS_TILE - 1) / PP_EVAL_ADDS_TILE;
    if (tiles > 65535) return PP_EINVAL;
    const Layout l = layout((size_t)n_pairs, (size_t)S_max, (size_t)tiles, kinds);
    if (((uintptr_t)workspace % 256) != 0 || workspace_bytes < l.total) return PP_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)workspace;
    float* xf = (float*)(ws + l.xf);
    float* err0 = (kinds & PP_EVAL_MSSD) ? (float*)(ws + l.err0) : nullptr;
    float* err1 = (kinds & PP_EVAL_MSPD) ? (float*)(ws + l.err1) : nullptr;
    double* part = (kinds & PP_EVAL_ADDS) ? (double*)(ws + l.part) : nullptr;
    const unsigned sym_tiles = (unsigned)((S_max + TS - 1) / TS);
    if (kinds & (PP_EVAL_MSSD | PP_EVAL_MSPD)) {
        const long long n = (long long)n_pairs * S_max;
        hipLaunchKernelGGL(compose_kernel, dim3((unsigned)((n + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, st, pair_obj, R_gt, t_gt, sym_R,
                           sym_t, sym_off, n_pairs, S_max, xf);
    }
    if (kinds & PP_EVAL_MSSD)
        hipLaunchKernelGGL(sym_max_kernel<0>, dim3(n_pairs, sym_tiles), dim3(BLOCK), 0, st, vertices, vert_off, sym_off, pair_obj,
                           R_est, t_est, focal, xf, S_max, err0);
    if (kinds & PP_EVAL_MSPD)
        hipLaunchKernelGGL(sym_max_kernel<1>, dim3(n_pairs, sym_tiles), dim3(BLOCK), 0, st, vertices, vert_off, sym_off, pair_obj,
                           R_est, t_est, focal, xf, S_max, err1);
    if (kinds & PP_EVAL_ADD)
        hipLaunchKernelGGL(add_kernel, dim3(n_pairs), dim3(BLOCK), 0, st, vertices, vert_off, pair_obj, R_est, t_est, R_gt, t_gt, add);
    if (kinds & PP_EVAL_ADDS)
        hipLaunchKernelGGL(adds_kernel, dim3(n_pairs, tiles), dim3(BLOCK), 0, st, adds_vertices, adds_off, pair_obj, R_est, t_est, R_gt,
                           t_gt, tiles, part);
    if (kinds & (PP_EVAL_MSSD | PP_EVAL_MSPD | PP_EVAL_ADDS))
        hipLaunchKernelGGL(finalize_kernel, dim3((unsigned)((n_pairs + WAVES - 1) / WAVES)), dim3(BLOCK), 0, st, pair_obj, sym_off,
                           adds_off, n_pairs, S_max, tiles, err0, err1, part, mssd, mssd_sym, mspd, mspd_sym, adds);
    return pp_last_launch();
}

}  // extern "C"
