// The rules the two batched RANSAC pose solvers share — pp_pnp.hip (EPnP, samples of 5) and pp_rgbd_pose.hip (3D-3D rigid fits,
// samples of 3) — each stated once.  include/picopose_hip.h ("RGB-D POSE RECOVERY") promises that the solvers agree on the gather
// order, the sampling sequence, the tie rule and the failure outputs; the numpy restatements draw from oracle/pnp.py the same way.
// Device-only; both kernels run one NT-thread workgroup per problem.
#ifndef PP_RANSAC_DEV_H
#define PP_RANSAC_DEV_H
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "pp_hash_dev.h"
#include "pp_reduce_dev.h"

constexpr int NT = 512;           // 8 waves, one workgroup per CU (the correspondences of a problem fill most of the LDS)
constexpr int NW = NT / 64;
constexpr int MAXP = 4096;        // correspondences per problem
constexpr int MAXH = 256;         // RANSAC hypotheses kept per problem

// ------------------------------------------------------------------ cyclic Jacobi on a small symmetric matrix (double)
// Everything keeps its operands in registers: every array index is a compile-time constant after unrolling (a per-lane matrix
// with run-time indices lives in scratch memory; pp_pnp.hip tells what that cost).

// one Jacobi rotation of the symmetric A (full storage) annihilating A[P][Q]; the rows of V accumulate the eigenvectors
template <int N, int P, int Q>
__device__ __forceinline__ void jrot(double (&A)[N][N], double (&V)[N][N]) {
    const double apq = A[P][Q];
    if (fabs(apq) >= 1e-300) {
        const double theta = (A[Q][Q] - A[P][P]) / (2.0 * apq);
        const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
        const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
#pragma unroll
        for (int k = 0; k < N; ++k) {
            const double akp = A[k][P], akq = A[k][Q];
            A[k][P] = c * akp - s * akq;
            A[k][Q] = s * akp + c * akq;
        }
#pragma unroll
        for (int k = 0; k < N; ++k) {
            const double apk = A[P][k], aqk = A[Q][k];
            A[P][k] = c * apk - s * aqk;
            A[Q][k] = s * apk + c * aqk;
        }
#pragma unroll
        for (int k = 0; k < N; ++k) {
            const double vpk = V[P][k], vqk = V[Q][k];
            V[P][k] = c * vpk - s * vqk;
            V[Q][k] = s * vpk + c * vqk;
        }
    }
}

template <int N>
__device__ __forceinline__ bool jacobi_converged(const double (&A)[N][N]) {
    double off = 0.0, diag = 0.0;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        diag += A[i][i] * A[i][i];
#pragma unroll
        for (int j = i + 1; j < N; ++j) off += A[i][j] * A[i][j];
    }
    return !(off > 1e-30 * (diag + 1e-300));      // (a NaN ends the sweeps as well)
}

// the rotations of one sweep from pair (P, Q) on: (0,1), (0,2), ..., (N-2,N-1) in row-major order, expanded at compile time
template <int N, int P = 0, int Q = 1>
__device__ __forceinline__ void jacobi_sweep(double (&A)[N][N], double (&V)[N][N]) {
    jrot<N, P, Q>(A, V);
    if constexpr (Q + 1 < N) jacobi_sweep<N, P, Q + 1>(A, V);
    else if constexpr (P + 2 < N) jacobi_sweep<N, P + 1, P + 2>(A, V);
}

// cyclic Jacobi on a symmetric NxN, at most 30 sweeps: eigenvalues on the diagonal of A (unordered), eigenvector k in row k of V
template <int N>
__device__ inline void jacobi_sym(double (&A)[N][N], double (&V)[N][N]) {
#pragma unroll
    for (int i = 0; i < N; ++i)
#pragma unroll
        for (int j = 0; j < N; ++j) V[i][j] = i == j ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 30; ++sweep) {
        if (jacobi_converged(A)) break;
        jacobi_sweep<N>(A, V);
    }
}

// ------------------------------------------------------------------ workgroup rules
// The sums of vals[0..CNT) over the NW waves go through block_reduce_all<NW>(vals, red, op_sum{}, 0.0) of pp_reduce_dev.h: every
// thread ends with the same bits and can run the same small algebra on them without a broadcast.  red: NW * CNT doubles of LDS;
// the caller's barrier before the call guards its previous use.  The winner (arg-max of the consensus, lowest hypothesis index
// among equals, hypothesis 0 and count -1 when there is none) is winner<1>(cnt, nh, nullptr, 0), run by the first wave.

// The SAMPLE distinct indices in [0, np) of hypothesis h of problem `prob`: a counter-based sequence, keyed by the problem and
// the hypothesis and never by the thread, so the two phases of the PnP redraw the same sample.  s = mix(0x9E3779B9 (prob + 1) ^
// (h 7919 + 17)), then per index s = mix(s + 0x6D2B79F5), c = s % np, drawn again while c repeats an earlier index.  np >= SAMPLE.
template <int SAMPLE>
__device__ __forceinline__ void ransac_sample(int prob, int h, int np, int (&idx)[SAMPLE]) {
    unsigned s = aug_mix(0x9E3779B9u * (unsigned)(prob + 1) ^ (unsigned)(h * 7919 + 17));
#pragma unroll
    for (int k = 0; k < SAMPLE; ++k) {
        for (;;) {
            s = aug_mix(s + 0x6D2B79F5u);
            const int c = (int)(s % (unsigned)np);
            bool dup = false;
#pragma unroll
            for (int j = 0; j < SAMPLE; ++j) dup |= j < k && idx[j] == c;
            if (!dup) { idx[k] = c; break; }
        }
    }
}

// The outputs of a failed problem that both solvers share, written by one thread: (I, [0,0,1], ratio 0, ok 0), the reference's
// except branch (utils/pose_recovery.py:99-105).  Each kernel adds its own extras after it.
__device__ __forceinline__ void ransac_fail_outputs(int prob, double* rot, double* tvec, double* ratio, int32_t* ok) {
    for (int k = 0; k < 9; ++k) rot[(size_t)prob * 9 + k] = (k % 4 == 0) ? 1.0 : 0.0;
    tvec[(size_t)prob * 3] = 0.0; tvec[(size_t)prob * 3 + 1] = 0.0; tvec[(size_t)prob * 3 + 2] = 1.0;
    ratio[prob] = 0.0;
    ok[prob] = 0;
}

// The object-frame source point of one listed entry: (src3d[:, sy, sx] - t_tem) @ R_tem (utils/pose_recovery.py:84), in float.
// f3: the problem's (3, H, W) map, P: its template pose (4x4, row-major); component j = sum_i d_i R[i][j].
__device__ __forceinline__ void object_frame_point(const float* f3, const float* P, int H, int W, int64_t sx, int64_t sy, float* out) {
    const float X = f3[sy * W + sx] - P[3], Y = f3[(size_t)H * W + sy * W + sx] - P[7], Z = f3[(size_t)2 * H * W + sy * W + sx] - P[11];
    out[0] = X * P[0] + Y * P[4] + Z * P[8];
    out[1] = X * P[1] + Y * P[5] + Z * P[9];
    out[2] = X * P[2] + Y * P[6] + Z * P[10];
}

#endif
