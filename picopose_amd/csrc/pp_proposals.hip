// Proposal labelling (include/picopose_hip.h, PROPOSAL LABELLING; picopose_amd/proposals.py plans every call): unit descriptors,
// the cosine / top-k / arg-max match of mask proposals against the ragged template-descriptor bank, and the bit-packed masks and
// pairwise intersections that the host's mask NMS reads.  No atomics, no floating-point reduction whose order depends on the
// launch shape: every dot product is one fixed tree (below), so equal rows give equal bits and the tie rules are exact.
#include <stdint.h>
#include <limits.h>
#include <math.h>
#include "pp_common.h"
#include "pp_bitrows_dev.h"
#include "pp_reduce_dev.h"
#include "pp_runs_dev.h"

namespace {

constexpr int WAVE = 64;
constexpr int MATCH_P = PP_MATCH_TILE;       // proposals of one workgroup
constexpr int MATCH_WAVES = 4;
constexpr int MATCH_CH = PP_MATCH_MAX_C / 4 / WAVE;   // 16-byte chunks of a row that one lane owns, at most
constexpr int MATCH_K = PP_MATCH_MAX_TOPK;   // entries of a top-k list

// THE DOT-PRODUCT ORDER (the header states it): lane l owns the 16-byte chunks l, l + 64, ... of a row and adds their products
// in ascending element order with one fma each, starting from 0; the 64 lane sums are then folded by a butterfly over the lane
// masks 32, 16, 8, 4, 2, 1.  a + b is commutative, so after the step with mask m lanes l and l ^ m hold the same bits: the
// result is one value in every lane, and a lane that runs only its own branch of the butterfly (fold16 below) gets that value.
// (wave_sum of pp_reduce_dev.h is that butterfly.)

// 16 values per lane -> the full butterfly sum of value p in the lanes with ((l >> 2) & 15) bit-reversed == p: at the steps 32,
// 16, 8, 4 a lane keeps the half of its values that its lane bit selects and hands the other half to its partner (8 + 4 + 2 + 1
// shuffles), the steps 2 and 1 are plain.  Value p of lane l sees the additions of wave_sum at lane l, in the same order.
// (Stays as written: a step adds what the PARTNER hands over to what the lane keeps, a reduce-scatter and not a wave_reduce walk;
// only the shuffle is the header's lane_xor.  One template instance per step: with the step's constants known at compile time
// each exchange is two selects and a shuffle.)
template <int HALF, int M>
__device__ __forceinline__ void fold_step(float (&a)[MATCH_P], int lane) {
    const bool hi = (lane & M) != 0;
#pragma unroll
    for (int i = 0; i < HALF; ++i) {
        const float send = hi ? a[i] : a[i + HALF];
        const float keep = hi ? a[i + HALF] : a[i];
        a[i] = keep + lane_xor(send, M);
    }
}
__device__ __forceinline__ float fold16(float (&a)[MATCH_P], int lane) {
    fold_step<8, 32>(a, lane);
    fold_step<4, 16>(a, lane);
    fold_step<2, 8>(a, lane);
    fold_step<1, 4>(a, lane);
    return wave_reduce_range<2, 1>(a[0], op_sum{});
}
__device__ __forceinline__ int fold16_owner(int lane) {
    return (((lane >> 5) & 1) << 3) | (((lane >> 4) & 1) << 2) | (((lane >> 3) & 1) << 1) | ((lane >> 2) & 1);
}

__global__ __launch_bounds__(256) void descriptor_normalize_kernel(const float* __restrict__ x, int n, int C, float eps,
                                                                   float* __restrict__ y) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= n) return;                                      // (whole waves leave: the shuffles below see 64 lanes)
    const float* xr = x + (size_t)row * C;
    float ss = 0.f;
    for (int c = lane; c < C; c += WAVE) ss = fmaf(xr[c], xr[c], ss);
    const float d = fmaxf(sqrtf(wave_sum(ss)), eps);
    float* yr = y + (size_t)row * C;
    for (int c = lane; c < C; c += WAVE) yr[c] = xr[c] / d;
}

// descending list of the MATCH_K largest (value, index), among equal values the lower index first.  BY_INDEX = false: an equal
// value goes behind the entries already there (the caller offers indices in ascending order); true: the indices are compared.
// From the slot the new entry takes, every old entry moves one slot down and the last one falls out.
template <bool BY_INDEX>
__device__ __forceinline__ void topk_insert(float (&val)[MATCH_K], int (&idx)[MATCH_K], float v, int t) {
    bool first = false;
#pragma unroll
    for (int i = 0; i < MATCH_K; ++i) {
        first = first || v > val[i] || (BY_INDEX && v == val[i] && t < idx[i]);
        const float ov = val[i];
        const int ot = idx[i];
        val[i] = first ? v : ov;
        idx[i] = first ? t : ot;
        v = first ? ov : v;
        t = first ? ot : t;
    }
}

// One workgroup = (tile of MATCH_P proposals, object).  The tile's query rows are staged in LDS; wave w takes the object's
// templates 2w, 2w + 1, 2w + 8, 2w + 9, ...: every lane loads its 16-byte chunks of two template rows and carries 2 x 16 partial
// sums, one per (template, proposal), each query chunk read from LDS once for both.  After fold16 the lanes with (l & 3) == 0
// own one proposal each and keep its top-k list in registers; the four waves' lists meet in LDS (the staging area, reused) and
// threads 0 .. MATCH_P - 1 merge them in wave order.
__global__ __launch_bounds__(MATCH_WAVES * WAVE) void proposal_match_kernel(
    const float* __restrict__ query, const float* __restrict__ bank, const int* __restrict__ offsets, int P, int O, int C, int total,
    int topk, float* __restrict__ score, int* __restrict__ view) {
    extern __shared__ float4 smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int p0 = blockIdx.x * MATCH_P, o = blockIdx.y;
    const int t0 = offsets[o], t1 = offsets[o + 1];
    // the entry validated its host copy; a device copy that disagrees must not lead outside the bank
    if (t0 < 0 || t1 <= t0 || t1 > total) return;
    const int T = t1 - t0, C4 = C >> 2;
    const float4* q4 = reinterpret_cast<const float4*>(query);
    for (int k = tid; k < MATCH_P * C4; k += MATCH_WAVES * WAVE) {
        const int p = p0 + k / C4;
        smem[k] = p < P ? q4[(size_t)p * C4 + k % C4] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    __syncthreads();

    float val[MATCH_K];
    int idx[MATCH_K];
#pragma unroll
    for (int i = 0; i < MATCH_K; ++i) {
        val[i] = -INFINITY;
        idx[i] = INT_MAX;
    }
    const bool owner = (lane & 3) == 0;
    // a lane's chunks of a template pair (at most MATCH_CH each): loaded one pair ahead, so the loads of the next pair are in
    // flight under the products of this one.  nch chunks per lane, uniform; in the last one the lanes past the row's end hold
    // zeros and read chunk 0 of the query: their products add +0 to a sum, which leaves its bits as they are.
    const int nch = (C4 + WAVE - 1) / WAVE;
    auto load_pair = [&](int ta, float4 (&a)[MATCH_CH], float4 (&b)[MATCH_CH]) {
        const float4* da = reinterpret_cast<const float4*>(bank + (size_t)(t0 + ta) * C);
        const float4* db = reinterpret_cast<const float4*>(bank + (size_t)(t0 + (ta + 1 < T ? ta + 1 : ta)) * C);
#pragma unroll
        for (int i = 0; i < MATCH_CH; ++i)
            if (i < nch) {
                const int c = lane + i * WAVE;
                const bool in = c < C4;
                const float4 va = da[in ? c : 0], vb = db[in ? c : 0];
                a[i] = in ? va : make_float4(0.f, 0.f, 0.f, 0.f);
                b[i] = in ? vb : make_float4(0.f, 0.f, 0.f, 0.f);
            }
    };
    float4 a[MATCH_CH] = {}, b[MATCH_CH] = {}, na[MATCH_CH] = {}, nb[MATCH_CH] = {};
    if (2 * wave < T) load_pair(2 * wave, a, b);
    for (int ta = 2 * wave; ta < T; ta += 2 * MATCH_WAVES) {               // uniform over the wave
        if (ta + 2 * MATCH_WAVES < T) load_pair(ta + 2 * MATCH_WAVES, na, nb);
        float sa[MATCH_P], sb[MATCH_P];
#pragma unroll
        for (int p = 0; p < MATCH_P; ++p) sa[p] = sb[p] = 0.f;
#pragma unroll
        for (int i = 0; i < MATCH_CH; ++i)
            if (i < nch) {
                const int c = lane + i * WAVE < C4 ? lane + i * WAVE : 0;
#pragma unroll
                for (int p = 0; p < MATCH_P; ++p) {
                    const float4 q = smem[p * C4 + c];
                    sa[p] = fmaf(q.w, a[i].w, fmaf(q.z, a[i].z, fmaf(q.y, a[i].y, fmaf(q.x, a[i].x, sa[p]))));
                    sb[p] = fmaf(q.w, b[i].w, fmaf(q.z, b[i].z, fmaf(q.y, b[i].y, fmaf(q.x, b[i].x, sb[p]))));
                }
            }
        const float ca = fold16(sa, lane), cb = fold16(sb, lane);
        if (owner) {
            topk_insert<false>(val, idx, ca, ta);
            if (ta + 1 < T) topk_insert<false>(val, idx, cb, ta + 1);
        }
#pragma unroll
        for (int i = 0; i < MATCH_CH; ++i) {
            a[i] = na[i];
            b[i] = nb[i];
        }
    }
    __syncthreads();                                                        // every wave is done with the staged queries
    float* lval = reinterpret_cast<float*>(smem);                           // [wave][proposal][MATCH_K]
    int* lidx = reinterpret_cast<int*>(smem) + MATCH_WAVES * MATCH_P * MATCH_K;
    if (owner) {
        const int base = (wave * MATCH_P + fold16_owner(lane)) * MATCH_K;
#pragma unroll
        for (int i = 0; i < MATCH_K; ++i) {
            lval[base + i] = val[i];
            lidx[base + i] = idx[i];
        }
    }
    __syncthreads();
    if (tid < MATCH_P && p0 + tid < P) {
#pragma unroll
        for (int i = 0; i < MATCH_K; ++i) {
            val[i] = lval[tid * MATCH_K + i];
            idx[i] = lidx[tid * MATCH_K + i];
        }
#pragma unroll 1
        for (int w = 1; w < MATCH_WAVES; ++w) {
            // a wave's list is sorted: behind an entry that finds no place in the merged list none of its followers does
            bool more = true;
#pragma unroll
            for (int i = 0; i < MATCH_K; ++i) {
                const int e = (w * MATCH_P + tid) * MATCH_K + i;
                const float v = lval[e];
                const int t = lidx[e];
                more = more && t != INT_MAX && (v > val[MATCH_K - 1] || (v == val[MATCH_K - 1] && t < idx[MATCH_K - 1]));
                if (more) topk_insert<true>(val, idx, v, t);
            }
        }
        const int k = min(topk, T);
        float s = val[0];
#pragma unroll
        for (int i = 1; i < MATCH_K; ++i)
            if (i < k) s += val[i];
        const size_t at = (size_t)(p0 + tid) * O + o;
        score[at] = s / (float)k;
        view[at] = idx[0];
    }
}

__global__ __launch_bounds__(256) void proposal_label_kernel(const float* __restrict__ score, int P, int O, int* __restrict__ label,
                                                             float* __restrict__ best) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= P) return;
    const float* s = score + (size_t)p * O;
    float b = s[0];
    int l = 0;
    for (int o = 1; o < O; ++o)
        if (s[o] > b) {
            b = s[o];
            l = o;
        }
    label[p] = l;
    best[p] = b;
}

// One thread per 32-pixel word of one mask: the runs that touch the word are walked from the first end beyond its first pixel.
// Workgroup x = 0 of a mask also adds up the mask's 1-runs (integers: any order gives the same sum).
__global__ __launch_bounds__(256) void rle_pack_bits_kernel(const int* __restrict__ run_ends, int n_runs,
                                                            const int* __restrict__ run_offset, int hw, int words,
                                                            unsigned* __restrict__ bits, int* __restrict__ area) {
    __shared__ int part[4];
    const int d = blockIdx.y, tid = threadIdx.x;
    int r0, r1;
    pp_run_slice(run_offset, d, n_runs, r0, r1);                            // (an empty mask for a device table that disagrees with the validated copy)
    const int* ends = run_ends + r0;
    const int m = r1 - r0;
    const int w = blockIdx.x * 256 + tid;
    if (w < words) {
        const long long first = (long long)w * 32;
        const int last = (int)(first + 32 < (long long)hw ? first + 32 : (long long)hw);      // one past the word's last pixel
        const int lo = pp_count_le(ends, m, (int)first);                      // ends[0 .. lo) <= first
        unsigned word = 0;
        int pos = (int)first;
        for (int k = lo; k < m && pos < last; ++k) {                          // run k covers [pos, ends[k]); odd k: a run of ones
            int e = ends[k];
            e = e < last ? e : last;
            if (e > pos) {
                if (k & 1) {
                    const int a = pos - (int)first, len = e - pos;            // 1 <= len <= 32
                    word |= (len == 32 ? 0xffffffffu : ((1u << len) - 1u)) << a;
                }
                pos = e;
            }
        }
        bits[(size_t)d * words + w] = word;
    }
    if (blockIdx.x == 0) {
        int s = 0;
        for (int k = 1 + 2 * tid; k < m; k += 512) {
            const int len = ends[k] - ends[k - 1];
            s += len > 0 ? len : 0;
        }
        s = block_reduce_to<4>(s, part, op_sum{});
        if (tid == 0) area[d] = s;
    }
}

// inter[i][j] = popcount(bits[i] & bits[j]): bitrow_tile_kernel (pp_bitrows_dev.h) with both sides in the one list of n rows.
struct MaskTile {
    int n, words;
    int* __restrict__ inter;
    __device__ long long sides(int& ri, int& i0, int& ni, int& rj, int& j0, int& nj) const {
        ri = i0 = blockIdx.y * PAIR, rj = j0 = blockIdx.x * PAIR, ni = nj = n;
        return 0;
    }
    __device__ void store(int, int, size_t at, int count) const { inter[at] = count; }
};

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" {

int pp_descriptor_normalize(const float* x, int n, int C, float eps, float* y, void* stream) {
    if (!x || !y || n <= 0 || C <= 0 || !(eps > 0.f)) return PP_EINVAL;
    hipLaunchKernelGGL(descriptor_normalize_kernel, dim3((n + 3) / 4), dim3(256), 0, (hipStream_t)stream, x, n, C, eps, y);
    return pp_last_launch();
}

int pp_proposal_match(const float* query, int P, const float* bank, const int* offsets, const int* offsets_host, int O, int C,
                      int topk, float* score, int* view, int* label, float* best, void* stream) {
    if (!query || !bank || !offsets || !offsets_host || !score || !view || !label || !best || P <= 0 || O <= 0 || C <= 0 ||
        (C & 3) != 0 || C > PP_MATCH_MAX_C || topk < 1 || topk > PP_MATCH_MAX_TOPK || O > 65535 || !aligned16(query) || !aligned16(bank))
        return PP_EINVAL;
    if (offsets_host[0] != 0) return PP_EINVAL;
    for (int o = 0; o < O; ++o)
        if (offsets_host[o + 1] <= offsets_host[o]) return PP_EINVAL;
    const size_t lists = (size_t)MATCH_WAVES * MATCH_P * MATCH_K * 8, stage = (size_t)MATCH_P * C * sizeof(float);
    const size_t lds = stage > lists ? stage : lists;                       // <= 64 KB at PP_MATCH_MAX_C
    hipLaunchKernelGGL(proposal_match_kernel, dim3((P + MATCH_P - 1) / MATCH_P, O), dim3(MATCH_WAVES * WAVE), lds, (hipStream_t)stream,
                       query, bank, offsets, P, O, C, offsets_host[O], topk, score, view);
    if (hipGetLastError() != hipSuccess) return PP_ELAUNCH;
    hipLaunchKernelGGL(proposal_label_kernel, dim3((P + 255) / 256), dim3(256), 0, (hipStream_t)stream, score, P, O, label, best);
    return pp_last_launch();
}

int pp_rle_pack_bits(const int* run_ends, int n_runs, const int* run_offset, const int* run_offset_host, int n, int hw, int words,
                     unsigned* bits, int* area, void* stream) {
    if (!run_ends || !run_offset || !run_offset_host || !bits || !area || n_runs <= 0 || n <= 0 || n > PP_MASK_MAX_N || hw <= 0 ||
        words != (int)(((long long)hw + 31) / 32))
        return PP_EINVAL;
    if (!pp_run_offsets_ok(run_offset_host, n, n_runs)) return PP_EINVAL;
    hipLaunchKernelGGL(rle_pack_bits_kernel, dim3((words + 255) / 256, n), dim3(256), 0, (hipStream_t)stream, run_ends, n_runs,
                       run_offset, hw, words, bits, area);
    return pp_last_launch();
}

int pp_mask_intersections(const unsigned* bits, int n, int words, int* inter, void* stream) {
    if (!bits || !inter || n <= 0 || n > PP_MASK_MAX_N || words <= 0) return PP_EINVAL;
    const int t = (n + PAIR - 1) / PAIR;
    hipLaunchKernelGGL(bitrow_tile_kernel<MaskTile>, dim3(t, t), dim3(PAIR_THREADS), 0, (hipStream_t)stream, bits, MaskTile{n, words, inter});
    return pp_last_launch();
}

}  // extern "C"
