// RGB-D pose recovery on the GPU: the correspondences of pp_pnp_ransac, each lifted to a 3D-3D pair by the test depth image,
// RANSAC over three-point rigid fits, a rigid refit on the consensus set.  One batched launch, one 512-thread workgroup per
// (instance, hypothesis) problem, no per-problem host sync.  The contract is stated in include/picopose_hip.h ("RGB-D POSE
// RECOVERY") and restated in numpy by tests/rgbd_pose_oracle.py.
//
// This is the project's own algorithm: the project it was modelled on recovers poses from RGB alone (EPnP / RANSAC, pp_pnp.hip)
// and has no RGB-D solver to compare with.  The model solver is closed-form (Horn 1987: the rotation is the eigenvector of the
// largest eigenvalue of a 4x4 symmetric matrix built from the centred cross-covariance), so a hypothesis is a few hundred fp64
// operations of one thread — nothing like EPnP's 12x12 system and its 16-lane solver groups.
//
// Layout of a problem in LDS (138 KiB of the 160 KiB): the kept pairs as fp32 (source point in the object frame, camera point
// rounded once from its fp64 value), 256 poses, per-hypothesis counts, the listed index of every kept pair, two byte masks.
// Phase 1: thread h fits hypothesis h.  Phase 2: wave w scores hypotheses w, w + 8, ...; its lanes walk the points, one ballot /
// popcount per 64 points.  No atomics.  Phase 3: the whole workgroup refits on the winner's consensus set, sums reduced in a fixed
// order (xor-butterfly within a wave, then the 8 wave partials in order), every thread solving the same small system.
//
// The rules shared with pp_pnp_ransac — workgroup shape and capacities, the cyclic Jacobi behind horn_fit and eig3_top2, the
// sampling sequence, the failure outputs, the object-frame source point — are the functions of pp_ransac_dev.h, the ones pp_pnp.hip
// calls; the block sum and the winner's tie rule are block_reduce_all and winner of pp_reduce_dev.h.  The kernel keeps 224 VGPRs, no spills and no scratch.

#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/picopose_hip.h"
#include "pp_common.h"
#include "pp_ransac_dev.h"           // NT, NW, MAXP, MAXH and the rules shared with pp_pnp.hip

namespace {

constexpr int SAMPLE = 3;
constexpr int NRED = 16;          // doubles of reduction scratch per wave: block_reduce_all<NW> over CNT values needs CNT <= NRED (15 is the widest)
constexpr double DEGENERATE = 1e-6;

// ------------------------------------------------------------------ small dense helpers (double, everything in registers)

// the two largest eigenvalues of a symmetric 3x3 (cyclic Jacobi)
__device__ inline void eig3_top2(double (&A)[3][3], double& l1, double& l2) {
    double V[3][3];
    jacobi_sym<3>(A, V);
    const double a = A[0][0], b = A[1][1], c = A[2][2];
    l1 = fmax(a, fmax(b, c));
    l2 = fmax(fmin(a, b), fmin(fmax(a, b), c));   // the median
}

// Least-squares rigid fit  q ~ R p + t  from the centred cross-covariance S[i][j] = sum (p - pm)_i (q - qm)_j and the two
// centroids (Horn 1987): the unit quaternion of R is the eigenvector of the largest eigenvalue (lowest index among equals) of
// the 4x4 symmetric matrix below; R is a proper rotation by construction.  Pose: R (9, row-major), t (3).
__device__ inline void horn_fit(const double (&S)[9], const double (&pm)[3], const double (&qm)[3], double (&R)[9], double (&t)[3]) {
    const double Sxx = S[0], Sxy = S[1], Sxz = S[2], Syx = S[3], Syy = S[4], Syz = S[5], Szx = S[6], Szy = S[7], Szz = S[8];
    double A[4][4] = {{Sxx + Syy + Szz, Syz - Szy, Szx - Sxz, Sxy - Syx},
                      {Syz - Szy, Sxx - Syy - Szz, Sxy + Syx, Szx + Sxz},
                      {Szx - Sxz, Sxy + Syx, -Sxx + Syy - Szz, Syz + Szy},
                      {Sxy - Syx, Szx + Sxz, Syz + Szy, -Sxx - Syy + Szz}};
    double V[4][4];
    jacobi_sym<4>(A, V);
    int best = 0;
    double lam = A[0][0];
#pragma unroll
    for (int k = 1; k < 4; ++k)
        if (A[k][k] > lam) { lam = A[k][k]; best = k; }
    double q[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) q[k] = best == 0 ? V[0][k] : best == 1 ? V[1][k] : best == 2 ? V[2][k] : V[3][k];
    const double inv = 1.0 / sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    const double w = q[0] * inv, x = q[1] * inv, y = q[2] * inv, z = q[3] * inv;
    R[0] = 1.0 - 2.0 * (y * y + z * z); R[1] = 2.0 * (x * y - w * z);       R[2] = 2.0 * (x * z + w * y);
    R[3] = 2.0 * (x * y + w * z);       R[4] = 1.0 - 2.0 * (x * x + z * z); R[5] = 2.0 * (y * z - w * x);
    R[6] = 2.0 * (x * z - w * y);       R[7] = 2.0 * (y * z + w * x);       R[8] = 1.0 - 2.0 * (x * x + y * y);
#pragma unroll
    for (int r = 0; r < 3; ++r) t[r] = qm[r] - (R[r * 3] * pm[0] + R[r * 3 + 1] * pm[1] + R[r * 3 + 2] * pm[2]);
}

// |a x b|^2 <= 1e-6 |a|^2 |b|^2 for the two edges of a triangle from its first point (also true for an edge of length 0)
__device__ __forceinline__ bool degenerate_triangle(const double (&p)[3][3]) {
    const double a0 = p[1][0] - p[0][0], a1 = p[1][1] - p[0][1], a2 = p[1][2] - p[0][2];
    const double b0 = p[2][0] - p[0][0], b1 = p[2][1] - p[0][1], b2 = p[2][2] - p[0][2];
    const double c0 = a1 * b2 - a2 * b1, c1 = a2 * b0 - a0 * b2, c2 = a0 * b1 - a1 * b0;
    return c0 * c0 + c1 * c1 + c2 * c2 <= DEGENERATE * (a0 * a0 + a1 * a1 + a2 * a2) * (b0 * b0 + b1 * b1 + b2 * b2);
}

// squared 3-D residual |M p + t - q|^2 of pair i under the pose M (12 doubles).  The multiply-adds are spelled out, so that the
// scoring pass, the consensus pass and the rms pass evaluate a pair with the same operations whatever the compiler would fuse.
__device__ __forceinline__ double residual2(const double* M, const float* ps, const float* pq, int i) {
    const double X = ps[3 * i], Y = ps[3 * i + 1], Z = ps[3 * i + 2];
    const double dx = fma(M[0], X, fma(M[1], Y, fma(M[2], Z, M[9]))) - (double)pq[3 * i];
    const double dy = fma(M[3], X, fma(M[4], Y, fma(M[5], Z, M[10]))) - (double)pq[3 * i + 1];
    const double dz = fma(M[6], X, fma(M[7], Y, fma(M[8], Z, M[11]))) - (double)pq[3 * i + 2];
    return fma(dx, dx, fma(dy, dy, dz * dz));
}

__device__ __forceinline__ bool finite12(const double (&R)[9], const double (&t)[3]) {
    bool f = true;
#pragma unroll
    for (int k = 0; k < 9; ++k) f = f && R[k] - R[k] == 0.0;
#pragma unroll
    for (int k = 0; k < 3; ++k) f = f && t[k] - t[k] == 0.0;
    return f;
}

constexpr size_t SMEM_BYTES = (size_t)2 * MAXP * 3 * sizeof(float) + (size_t)MAXH * 12 * sizeof(double) +
                              (size_t)NW * NRED * sizeof(double) + (size_t)MAXH * sizeof(int) + (size_t)MAXP * sizeof(unsigned short) +
                              2 * (size_t)MAXP;

// One workgroup per problem.
//   tar_pts_2d (P,2,H,W), src_pts_3d (P,3,H,W), K (P,3,3), tem_pose (P,4,4), tar_pts/src_pts (P,N,2) int64, depth (n_images,dH,dW),
//   image_index (P) int32, inlier_dist (P)
//   out: rot (P,9) f64, tvec (P,3) f64, ratio (P) f64, ok, npts, nlisted (P) int32, rms (P) f64, mask (P,N) uint8 or null
__global__ __launch_bounds__(NT) void rgbd_ransac_kernel(const float* __restrict__ tar2d, const float* __restrict__ src3d,
                                                         const float* __restrict__ Kmat, const float* __restrict__ tem_pose,
                                                         const int64_t* __restrict__ tar_pts, const int64_t* __restrict__ src_pts,
                                                         int H, int W, int N, const float* __restrict__ depth, int n_images, int dH,
                                                         int dW, const int32_t* __restrict__ image_index,
                                                         const float* __restrict__ inlier_dist, int iters, double* __restrict__ rot,
                                                         double* __restrict__ tvec, double* __restrict__ ratio,
                                                         int32_t* __restrict__ ok, int32_t* __restrict__ npts,
                                                         int32_t* __restrict__ nlisted, double* __restrict__ rms,
                                                         uint8_t* __restrict__ mask) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* ps = (float*)smem;                                  // [MAXP][3] source points, object frame
    float* pq = ps + 3 * MAXP;                                 // [MAXP][3] camera points
    double* hyp = (double*)(pq + 3 * MAXP);                    // [MAXH][12] R, t of every hypothesis
    double* red = hyp + MAXH * 12;                             // [NW][NRED]
    int* cnt = (int*)(red + NW * NRED);                        // [MAXH] consensus of a hypothesis (-1 until scored: degenerate sample)
    unsigned short* lidx = (unsigned short*)(cnt + MAXH);      // [MAXP] listed index of a kept pair
    unsigned char* use = (unsigned char*)(lidx + MAXP);        // [MAXP] consensus membership, kept order
    unsigned char* lmask = use + MAXP;                         // [MAXP] consensus membership, listed order
    __shared__ int wsl[NW], wsk[NW], base_l, base_k, best_h, best_c;
    const int prob = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int64_t* tp = tar_pts + (size_t)prob * N * 2;
    const int64_t* sp = src_pts + (size_t)prob * N * 2;
    const float* f2 = tar2d + (size_t)prob * 2 * H * W;
    const float* f3 = src3d + (size_t)prob * 3 * H * W;
    const float* P = tem_pose + (size_t)prob * 16;
    const float* Kp = Kmat + (size_t)prob * 9;
    const double fx = Kp[0], fy = Kp[4], cx = Kp[2], cy = Kp[5];
    const int img = image_index[prob];
    const bool img_ok = img >= 0 && img < n_images;            // (out of range: no depth is read, every entry is dropped)
    const float* D = depth + (size_t)(img_ok ? img : 0) * dH * dW;

    // ---- gather: the listed entries (no -1) in list order, as pnp_ransac_kernel walks them; of these, the ones with a depth
    if (tid == 0) { base_l = 0; base_k = 0; }
    __syncthreads();
    for (int n0 = 0; n0 < N; n0 += NT) {
        const int n = n0 + tid;
        int64_t tx = -1, ty = -1, sx = -1, sy = -1;
        if (n < N) { tx = tp[2 * n]; ty = tp[2 * n + 1]; sx = sp[2 * n]; sy = sp[2 * n + 1]; }
        const bool v = tx != -1 && ty != -1 && sx != -1 && sy != -1;
        float u = 0.f, vv = 0.f, z = 0.f;
        bool keep = false;
        if (v) {
            u = f2[ty * W + tx];
            vv = f2[(size_t)H * W + ty * W + tx];
            const float xf = floorf(u + 0.5f), yf = floorf(vv + 0.5f);
            if (img_ok && xf >= 0.f && xf < 2147483648.f && yf >= 0.f && yf < 2147483648.f) {   // (a NaN fails the comparisons)
                const int xi = (int)xf, yi = (int)yf;
                if (xi < dW && yi < dH) {
                    z = D[(size_t)yi * dW + xi];
                    keep = z > 0.f && z < __builtin_inff();
                }
            }
        }
        const unsigned long long bl = __ballot(v), bk = __ballot(keep);
        if (lane == 0) { wsl[wv] = __popcll(bl); wsk[wv] = __popcll(bk); }
        __syncthreads();
        int offl = base_l, offk = base_k, totl = 0, totk = 0;
        for (int i = 0; i < NW; ++i) {
            offl += i < wv ? wsl[i] : 0; totl += wsl[i];
            offk += i < wv ? wsk[i] : 0; totk += wsk[i];
        }
        if (keep) {
            const unsigned long long below = (1ull << lane) - 1ull;
            const int rl = offl + __popcll(bl & below), rk = offk + __popcll(bk & below);
            if (rl < MAXP) {     // (N <= MAXP: always)
                object_frame_point(f3, P, H, W, sx, sy, ps + 3 * rk);
                const double zd = z;
                pq[3 * rk] = (float)(((double)u - cx) * zd / fx);
                pq[3 * rk + 1] = (float)(((double)vv - cy) * zd / fy);
                pq[3 * rk + 2] = z;
                lidx[rk] = (unsigned short)rl;
            }
        }
        __syncthreads();
        if (tid == 0) { base_l += totl; base_k += totk; }
        __syncthreads();
    }
    const int nl = base_l < MAXP ? base_l : MAXP;
    const int np = base_k < MAXP ? base_k : MAXP;
    if (tid == 0) { nlisted[prob] = nl; npts[prob] = np; }
    auto fail = [&]() {
        if (tid == 0) {
            ransac_fail_outputs(prob, rot, tvec, ratio, ok);
            rms[prob] = 0.0;
        }
        if (mask)
            for (int i = tid; i < N; i += NT) mask[(size_t)prob * N + i] = 0;
    };
    const float dist = inlier_dist[prob];
    if (np < SAMPLE || !(dist > 0.f)) { fail(); return; }       // (uniform over the workgroup)
    const double th2 = (double)dist * (double)dist;

    // ---- phase 1: thread h fits hypothesis h on its 3-pair sample
    const int nh = iters < MAXH ? iters : MAXH;
    if (tid < nh) {
        const int h = tid;
        int idx[SAMPLE];
        ransac_sample<SAMPLE>(prob, h, np, idx);
        double a[3][3], b[3][3];
#pragma unroll
        for (int k = 0; k < 3; ++k)
#pragma unroll
            for (int c = 0; c < 3; ++c) { a[k][c] = ps[3 * idx[k] + c]; b[k][c] = pq[3 * idx[k] + c]; }
        const bool deg = degenerate_triangle(a) || degenerate_triangle(b);
        double R[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0}, t[3] = {0.0, 0.0, 0.0};
        if (!deg) {
            double pm[3], qm[3], S[9];
#pragma unroll
            for (int c = 0; c < 3; ++c) { pm[c] = (a[0][c] + a[1][c] + a[2][c]) / 3.0; qm[c] = (b[0][c] + b[1][c] + b[2][c]) / 3.0; }
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int j = 0; j < 3; ++j)
                    S[i * 3 + j] = (a[0][i] - pm[i]) * (b[0][j] - qm[j]) + (a[1][i] - pm[i]) * (b[1][j] - qm[j]) + (a[2][i] - pm[i]) * (b[2][j] - qm[j]);
            horn_fit(S, pm, qm, R, t);
        }
#pragma unroll
        for (int k = 0; k < 9; ++k) hyp[h * 12 + k] = R[k];
#pragma unroll
        for (int k = 0; k < 3; ++k) hyp[h * 12 + 9 + k] = t[k];
        cnt[h] = deg ? -1 : 0;
    }
    __syncthreads();

    // ---- phase 2: wave w scores hypotheses w, w + NW, ...: lanes over the pairs, one ballot / popcount per 64 pairs
    for (int h = wv; h < nh; h += NW) {
        int c = 0;
        if (cnt[h] >= 0) {       // (uniform over the wave; a degenerate sample scores 0)
            const double* M = hyp + h * 12;
            for (int i0 = 0; i0 < np; i0 += 64) {
                const int i = i0 + lane;
                const bool in = i < np && residual2(M, ps, pq, i < np ? i : 0) <= th2;   // NaN (a non-finite fit) is never an inlier
                c += __popcll(__ballot(in));
            }
        }
        if (lane == 0) cnt[h] = c;
    }
    __syncthreads();
    if (tid < 64) {
        const Winner w = winner<1>(cnt, nh, nullptr, 0);
        if (tid == 0) { best_h = w.h; best_c = w.c; }
    }
    for (int i = tid; i < MAXP; i += NT) lmask[i] = 0;
    __syncthreads();
    if (best_c < SAMPLE) { fail(); return; }
    const double* Mw = hyp + best_h * 12;
    for (int i = tid; i < np; i += NT) {
        const unsigned char in = residual2(Mw, ps, pq, i) <= th2 ? 1 : 0;
        use[i] = in;
        lmask[lidx[i]] = in;
    }
    __syncthreads();
    if (mask)
        for (int i = tid; i < N; i += NT) mask[(size_t)prob * N + i] = lmask[i];

    // ---- phase 3: rigid refit on the consensus set (all threads cooperate, identical small algebra in every thread)
    double s7[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int i = tid; i < np; i += NT) {
        if (!use[i]) continue;
#pragma unroll
        for (int c = 0; c < 3; ++c) { s7[c] += ps[3 * i + c]; s7[3 + c] += pq[3 * i + c]; }
        s7[6] += 1.0;
    }
    __syncthreads();   // (the previous use of `red` has been read by everyone)
    block_reduce_all<NW>(s7, red, op_sum{}, 0.0);
    const double n = s7[6];
    double pm[3], qm[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) { pm[c] = s7[c] / n; qm[c] = s7[3 + c] / n; }
    double s15[15];
#pragma unroll
    for (int c = 0; c < 15; ++c) s15[c] = 0.0;
    for (int i = tid; i < np; i += NT) {
        if (!use[i]) continue;
        const double a0 = ps[3 * i] - pm[0], a1 = ps[3 * i + 1] - pm[1], a2 = ps[3 * i + 2] - pm[2];
        const double b0 = pq[3 * i] - qm[0], b1 = pq[3 * i + 1] - qm[1], b2 = pq[3 * i + 2] - qm[2];
        s15[0] += a0 * b0; s15[1] += a0 * b1; s15[2] += a0 * b2;
        s15[3] += a1 * b0; s15[4] += a1 * b1; s15[5] += a1 * b2;
        s15[6] += a2 * b0; s15[7] += a2 * b1; s15[8] += a2 * b2;
        s15[9] += a0 * a0; s15[10] += a0 * a1; s15[11] += a0 * a2; s15[12] += a1 * a1; s15[13] += a1 * a2; s15[14] += a2 * a2;
    }
    __syncthreads();   // (the previous use of `red` has been read by everyone)
    block_reduce_all<NW>(s15, red, op_sum{}, 0.0);
    double M[12];
    {
        double S[9], R[9], t[3];
#pragma unroll
        for (int c = 0; c < 9; ++c) S[c] = s15[c];
        horn_fit(S, pm, qm, R, t);
        double C[3][3] = {{s15[9], s15[10], s15[11]}, {s15[10], s15[12], s15[13]}, {s15[11], s15[13], s15[14]}}, l1, l2;
        eig3_top2(C, l1, l2);
        const bool refit = finite12(R, t) && !(l2 <= DEGENERATE * l1);   // (collinear source points: the winner's pose is returned)
#pragma unroll
        for (int k = 0; k < 9; ++k) M[k] = refit ? R[k] : Mw[k];
#pragma unroll
        for (int k = 0; k < 3; ++k) M[9 + k] = refit ? t[k] : Mw[9 + k];
    }
    double e[1] = {0.0};
    for (int i = tid; i < np; i += NT)
        if (use[i]) e[0] += residual2(M, ps, pq, i);
    __syncthreads();   // (the previous use of `red` has been read by everyone)
    block_reduce_all<NW>(e, red, op_sum{}, 0.0);
    if (tid == 0) {
        for (int k = 0; k < 9; ++k) rot[(size_t)prob * 9 + k] = M[k];
        for (int k = 0; k < 3; ++k) tvec[(size_t)prob * 3 + k] = M[9 + k];
        ratio[prob] = (double)best_c / (double)np;
        ok[prob] = 1;
        rms[prob] = sqrt(e[0] / n);
    }
}

}  // namespace

extern "C" {

int pp_rgbd_ransac(const float* tar_pts_2d, const float* src_pts_3d, const float* K, const float* tem_pose,
                   const int64_t* tar_pts, const int64_t* src_pts, int P, int H, int W, int N,
                   const float* depth, int n_images, int dH, int dW, const int32_t* image_index,
                   const float* inlier_dist, int iterations,
                   double* rot, double* tvec, double* inlier_ratio, int32_t* success,
                   int32_t* num_points, int32_t* num_listed, double* rms, uint8_t* inlier_mask, void* stream) {
    if (!tar_pts_2d || !src_pts_3d || !K || !tem_pose || !tar_pts || !src_pts || !depth || !image_index || !inlier_dist || !rot ||
        !tvec || !inlier_ratio || !success || !num_points || !num_listed || !rms)
        return PP_EINVAL;
    if (P <= 0 || H <= 0 || W <= 0 || N <= 0 || N > MAXP || n_images <= 0 || dH <= 0 || dW <= 0 || iterations <= 0) return PP_EINVAL;
    static bool attr_set[PP_MAX_DEVICES];   // the dynamic-LDS opt-in is per device
    if (!attr_set[pp_cur_device()]) {
        PP_CHECK_HIP(hipFuncSetAttribute((const void*)rgbd_ransac_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)SMEM_BYTES));
        attr_set[pp_cur_device()] = true;
    }
    hipLaunchKernelGGL(rgbd_ransac_kernel, dim3(P), dim3(NT), SMEM_BYTES, (hipStream_t)stream, tar_pts_2d, src_pts_3d, K, tem_pose,
                       tar_pts, src_pts, H, W, N, depth, n_images, dH, dW, image_index, inlier_dist, iterations, rot, tvec,
                       inlier_ratio, success, num_points, num_listed, rms, inlier_mask);
    return pp_last_launch();
}

}  // extern "C"
