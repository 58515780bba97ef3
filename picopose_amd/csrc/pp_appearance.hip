// The appearance score of the proposal labelling (include/picopose_hip.h, PROPOSAL LABELLING, THE APPEARANCE SCORE;
// picopose_amd/proposals.py plans every call): which patches of a crop are foreground, and per proposal the masked best cosine of
// every query patch to the valid patches of one template view, with its masked mean.  No atomics; every cosine is one k-ordered
// fma chain (the fp32 MFMA), every sum one fixed tree, so equal rows give equal bits and the lowest-index tie rule is exact.
#include <stdint.h>
#include "pp_common.h"
#include "pp_reduce_dev.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f4 __attribute__((ext_vector_type(4)));

constexpr int WAVE = 64;
constexpr int APP_WAVES = 4;
constexpr int APP_Q = PP_APP_TILE;           // query patches of one workgroup: 2 tiles of 32, shared by the four waves
constexpr int APP_T = 64 * APP_WAVES;        // template patches of one chunk: 2 tiles of 32 per wave
constexpr int APP_K = 16;                    // channels of one LDS stage
// LDS images are [channel][patch]: an operand read is 32 consecutive dwords per lane half (conflict-free); the strides are 4
// mod 32, so the four lanes that stage one patch's 16 channels store to banks 16 apart (2-way: free on ds_write_b32)
constexpr int APP_QS = APP_Q + 4, APP_TS = APP_T + 4;
static_assert(PP_APP_MAX_N % APP_T == 0, "the validity bytes of a view are staged for whole chunks");

__global__ __launch_bounds__(256) void patch_valid_kernel(const float* __restrict__ mask, int S, int p,
                                                          unsigned char* __restrict__ valid, int* __restrict__ n_valid) {
    __shared__ int part[4];
    const int d = blockIdx.x, tid = threadIdx.x;
    const int w0 = S / p, N = w0 * w0, half = p * p;
    const float* m = mask + (size_t)d * S * S;
    int cnt = 0;
    for (int i = tid; i < N; i += 256) {
        const float* cell = m + (size_t)(i / w0) * p * S + (size_t)(i % w0) * p;
        int c = 0;
        for (int y = 0; y < p; ++y)
            for (int x = 0; x < p; ++x) c += cell[(size_t)y * S + x] > 0.5f ? 1 : 0;          // (false for a NaN)
        const int v = 2 * c >= half ? 1 : 0;
        valid[(size_t)d * N + i] = (unsigned char)v;
        cnt += v;
    }
    cnt = block_reduce_to<4>(cnt, part, op_sum{});                                            // integers: any order gives the same sum
    if (tid == 0) n_valid[d] = cnt;
}

// a (value, index) candidate replaces the running best when the best is empty, when it is larger, or equal with a lower index
__device__ __forceinline__ void take_better(float& bv, int& bi, float v, int i) {
    if (i >= 0 && (bi < 0 || v > bv || (v == bv && i < bi))) {
        bv = v;
        bi = i;
    }
}

// One workgroup = (proposal p, APP_Q query patches from i0).  For every chunk of APP_T template patches wave w owns the patches
// j0 + 64 w .. + 63 as the A operand (rows) and all APP_Q query patches as the B operand (columns): acc[a][b] is template tile a
// against query tile b, register e of lane l being template patch 32 a + (e & 3) + 8 (e >> 2) + 4 (l >> 5) and query patch
// 32 b + (l & 31).  The channels pass through LDS APP_K at a time, the next stage's global loads in flight under the products;
// lane half h feeds channel 2 kk + h of step kk, so an accumulator is the chain fma(q[k], t[k], acc), k ascending.  A lane meets
// its template patches in ascending order (e, then a, then the chunk), so a strict > keeps the lowest index among equal cosines.
__global__ __launch_bounds__(APP_WAVES * WAVE) void appearance_match_kernel(
    const float* __restrict__ query, const float* __restrict__ bank, const unsigned char* __restrict__ t_valid,
    const int* __restrict__ pair_row, int R, int N, int C, float* __restrict__ patch_sim, int* __restrict__ patch_arg) {
    __shared__ float Qs[APP_K * APP_QS];
    __shared__ float Ts[APP_K * APP_TS];
    __shared__ unsigned char tv[PP_APP_MAX_N];
    __shared__ float wval[APP_WAVES][APP_Q];
    __shared__ int widx[APP_WAVES][APP_Q];
    const int p = blockIdx.x, i0 = blockIdx.y * APP_Q;
    const int r = pair_row[p];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, l31 = lane & 31, lh = lane >> 5;
    // the entry validated the host copy; a device copy that disagrees must not lead outside the bank: such a proposal is
    // answered like one whose view has no valid patch (uniform over the workgroup, before any barrier)
    if (r < 0 || r >= R) {
        if (tid < APP_Q && i0 + tid < N) {
            patch_sim[(size_t)p * N + i0 + tid] = 0.f;
            patch_arg[(size_t)p * N + i0 + tid] = -1;
        }
        return;
    }
    for (int j = tid; j < PP_APP_MAX_N; j += APP_WAVES * WAVE) tv[j] = j < N ? t_valid[(size_t)r * N + j] : (unsigned char)0;
    const float* qg = query + (size_t)p * N * C;
    const float* tg = bank + (size_t)r * N * C;
    // staging: thread -> patch tid >> 2 (+ 64 s for the template) and the four channels 4 (tid & 3) .. + 3 of the stage
    const int sp = tid >> 2, sq = (tid & 3) * 4;
    const f4 zero = {0.f, 0.f, 0.f, 0.f};
    f4 qn, tn[APP_WAVES];
    auto load_stage = [&](int j0, int kc) {
        const int c = kc * APP_K + sq;
        const bool in = c < C;                                               // (C is a multiple of 4: a quad is whole or absent)
        qn = in && i0 + sp < N ? *reinterpret_cast<const f4*>(qg + (size_t)(i0 + sp) * C + c) : zero;
#pragma unroll
        for (int s = 0; s < APP_WAVES; ++s) {
            const int j = j0 + sp + 64 * s;
            tn[s] = in && j < N ? *reinterpret_cast<const f4*>(tg + (size_t)j * C + c) : zero;
        }
    };
    float best[2] = {0.f, 0.f};
    int barg[2] = {-1, -1};
    const int nk = (C + APP_K - 1) / APP_K;
    for (int j0 = 0; j0 < N; j0 += APP_T) {
        f32x16 acc[2][2];
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b)
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[a][b][e] = 0.f;
        load_stage(j0, 0);
        for (int kc = 0; kc < nk; ++kc) {
            __syncthreads();                                                 // the previous stage has been read (first pass: tv is written)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                Qs[(sq + e) * APP_QS + sp] = qn[e];
#pragma unroll
                for (int s = 0; s < APP_WAVES; ++s) Ts[(sq + e) * APP_TS + sp + 64 * s] = tn[s][e];
            }
            __syncthreads();
            if (kc + 1 < nk) load_stage(j0, kc + 1);
#pragma unroll
            for (int kk = 0; kk < APP_K / 2; ++kk) {
                float ta[2], qb[2];
#pragma unroll
                for (int a = 0; a < 2; ++a) {
                    ta[a] = Ts[(2 * kk + lh) * APP_TS + w * 64 + a * 32 + l31];
                    qb[a] = Qs[(2 * kk + lh) * APP_QS + a * 32 + l31];
                }
#pragma unroll
                for (int a = 0; a < 2; ++a)
#pragma unroll
                    for (int b = 0; b < 2; ++b) acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(ta[a], qb[b], acc[a][b], 0, 0, 0);
            }
        }
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int j = j0 + w * 64 + a * 32 + (e & 3) + 8 * (e >> 2) + 4 * lh;        // < PP_APP_MAX_N: tv holds 0 past N
                if (tv[j]) {
#pragma unroll
                    for (int b = 0; b < 2; ++b)
                        if (barg[b] < 0 || acc[a][b][e] > best[b]) {
                            best[b] = acc[a][b][e];
                            barg[b] = j;
                        }
                }
            }
    }
#pragma unroll
    for (int b = 0; b < 2; ++b) {                                            // the other lane half holds the rows 4 .. 7 of every 8
        const float ov = lane_xor(best[b], 32);
        const int oi = lane_xor(barg[b], 32);
        take_better(best[b], barg[b], ov, oi);
    }
    if (lh == 0) {
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            wval[w][b * 32 + l31] = best[b];
            widx[w][b * 32 + l31] = barg[b];
        }
    }
    __syncthreads();
    if (tid < APP_Q && i0 + tid < N) {
        float bv = wval[0][tid];
        int bi = widx[0][tid];
#pragma unroll
        for (int k = 1; k < APP_WAVES; ++k) take_better(bv, bi, wval[k][tid], widx[k][tid]);
        const size_t at = (size_t)p * N + i0 + tid;
        patch_sim[at] = bi < 0 ? 0.f : bv;
        patch_arg[at] = bi;
    }
}

// One wave per proposal: the masked sum of patch_sim in THE ROW ORDER (lane l adds i = l, l + 64, ... ascending from 0, then the
// butterfly of wave_sum) and one division.
__global__ __launch_bounds__(WAVE) void appearance_mean_kernel(const float* __restrict__ patch_sim, const unsigned char* __restrict__ q_valid,
                                                               int N, int* __restrict__ n_valid, float* __restrict__ app) {
    const int p = blockIdx.x, lane = threadIdx.x;
    const float* ps = patch_sim + (size_t)p * N;
    const unsigned char* qv = q_valid + (size_t)p * N;
    float s = 0.f;
    int n = 0;
    for (int i = lane; i < N; i += WAVE)
        if (qv[i]) {
            s += ps[i];
            ++n;
        }
    s = wave_sum(s);
    n = wave_sum(n);
    if (lane == 0) {
        n_valid[p] = n;
        app[p] = n > 0 ? s / (float)n : 0.f;                                 // (a view without a valid patch: every patch_sim is 0)
    }
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" {

int pp_patch_valid(const float* mask, int n, int S, int p, unsigned char* valid, int* n_valid, void* stream) {
    if (!mask || !valid || !n_valid || n <= 0 || S <= 0 || S > PP_APP_MAX_S || p <= 0 || S % p != 0) return PP_EINVAL;
    hipLaunchKernelGGL(patch_valid_kernel, dim3(n), dim3(256), 0, (hipStream_t)stream, mask, S, p, valid, n_valid);
    return pp_last_launch();
}

int pp_appearance_match(const float* query, const unsigned char* q_valid, int P, const float* bank, const unsigned char* t_valid, int R,
                        const int* pair_row, const int* pair_row_host, int N, int C, float* patch_sim, int* patch_arg, int* n_valid,
                        float* app, void* stream) {
    if (!query || !q_valid || !bank || !t_valid || !pair_row || !pair_row_host || !patch_sim || !patch_arg || !n_valid || !app ||
        P <= 0 || R <= 0 || N <= 0 || C <= 0 || N > PP_APP_MAX_N || (C & 3) != 0 || C > PP_MATCH_MAX_C || !aligned16(query) ||
        !aligned16(bank))
        return PP_EINVAL;
    for (int p = 0; p < P; ++p)
        if (pair_row_host[p] < 0 || pair_row_host[p] >= R) return PP_EINVAL;
    hipLaunchKernelGGL(appearance_match_kernel, dim3(P, (N + APP_Q - 1) / APP_Q), dim3(APP_WAVES * WAVE), 0, (hipStream_t)stream, query,
                       bank, t_valid, pair_row, R, N, C, patch_sim, patch_arg);
    if (hipGetLastError() != hipSuccess) return PP_ELAUNCH;
    hipLaunchKernelGGL(appearance_mean_kernel, dim3(P), dim3(WAVE), 0, (hipStream_t)stream, patch_sim, q_valid, N, n_valid, app);
    return pp_last_launch();
}

}  // extern "C"
