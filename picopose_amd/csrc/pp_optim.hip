// Fused multi-tensor Adam / AdamW step (include/picopose_hip.h pp_adam_multi_tensor): the reference's `optim.AdamW` /
// `optim.Adam` step (run_train.py:79-85; torch's `_single_tensor_adam`) over every parameter in two launches.
//   pass 1 (adam_update_kernel): one workgroup per (tensor, chunk of PP_ADAM_CHUNK elements) item, float4 accesses; reads p, g, m, v and
//          writes p, m, v (28 B per element); a tensor that is split in this step also leaves max|p_new| of the chunk in `partials`.
//   pass 2 (adam_split_kernel): one workgroup per chunk of the split tensors; every workgroup folds its tensor's chunk maxima itself and
//          writes the chunk's operand terms — the arithmetic of pp_split_weights_ws (pp_gemm.hip absmax_part_kernel + split_fold_kernel),
//          so the operand is bit for bit the one the next forward would make.  A separate launch orders pass 2 after every chunk of pass 1
//          (no inter-workgroup signalling).

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <vector>
#include "../../include/picopose_hip.h"
#include "pp_common.h"
#include "pp_reduce_dev.h"

namespace {

typedef float f4 __attribute__((ext_vector_type(4)));
typedef _Float16 h8 __attribute__((ext_vector_type(8)));

constexpr int CHUNK = PP_ADAM_CHUNK;
constexpr int EMAX = 30;           // pp_split_weights_ws: exponent clamp of the weight scale

// the device table: one entry per tensor (built from PpAdamTensor when the caller asks for a rebuild)
struct AdamDev {
    float* p;
    float* m;
    float* v;
    _Float16* hl;      // nullptr: not split
    float* scale2;
    long long n;
    int part0;         // first slot of the tensor's chunk maxima in `partials` (split tensors)
    int nchunk;
    int vec;           // p, m, v 16-byte aligned
    int pad;
};

struct Layout {
    int nitems, nsplit;
    size_t off_items, off_split, off_part, table_bytes, total;
};

// one element, in the order of torch.optim.adam._single_tensor_adam (fp32 opmath, scalars rounded to fp32 by the host).  Every torch op
// there is a kernel of its own, so each op's result is rounded to fp32; inside one op the compiler contracts a * b + c into an fma.  The
// same roundings here: contraction off, the fma of each op spelled out.
__device__ __forceinline__ void adam_elem(float& p, float g, float& m, float& v, const PpAdamStep& s) {
#pragma clang fp contract(off)
    if (s.mode == 1) p = p * s.decay;                                   // param.mul_(1 - lr * weight_decay)
    else if (s.mode == 2) g = __builtin_fmaf(s.decay, p, g);             // grad.add(param, alpha=weight_decay)
    const float d = g - m;                                              // exp_avg.lerp_(grad, 1 - beta1) (ATen lerp: two forms)
    m = fabsf(s.lerp_w) < 0.5f ? __builtin_fmaf(s.lerp_w, d, m) : __builtin_fmaf(-d, 1.f - s.lerp_w, g);
    v = v * s.beta2;                                                    // exp_avg_sq.mul_(beta2)
    v = __builtin_fmaf(s.one_minus_beta2, g * g, v);                    //   .addcmul_(grad, grad, value=1 - beta2)
    const float den = sqrtf(v) * s.inv_bc2_sqrt + s.eps;                // (exp_avg_sq.sqrt() / bias_correction2_sqrt).add_(eps): a CPU
                                                                        //   scalar divisor is a product with fp32(1 / b) in ATen
    p = __builtin_fmaf(s.neg_step_size, m / den, p);                    // param.addcdiv_(exp_avg, denom, value=-step_size)
}

// the workgroup's maximum in every thread.  The wave part is pp_reduce_dev.h's walk; the fold over the four waves stays the tree it
// was, not block_reduce_all's ascending fold: the bits would be the same (the operands began at 0.f and met |p| through fmaxf: no
// NaN, no -0), but adam_split_kernel measured above the parent's spread with the ascending fold (profiles/r21/reductions.md)
__device__ __forceinline__ float tree_max4(float m, float* red) {
    PP_WAVE_WALK(o, 32, 1) m = fmaxf(m, lane_xor(m, o));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    return fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

__global__ __launch_bounds__(256) void adam_update_kernel(const AdamDev* __restrict__ table, const int2* __restrict__ items,
                                                          const PpAdamStep* __restrict__ steps, float* __restrict__ partials) {
    __shared__ float red[4];
    const int2 it = items[blockIdx.x];
    const AdamDev d = table[it.x];
    const PpAdamStep s = steps[it.x];
    const long long start = (long long)it.y * CHUNK;
    const long long end = start + CHUNK < d.n ? start + CHUNK : d.n;
    float* __restrict__ P = d.p;
    float* __restrict__ M = d.m;
    float* __restrict__ V = d.v;
    const float* __restrict__ G = s.g;
    float mx = 0.f;
    long long i0 = start;
    if (d.vec && ((uintptr_t)G & 15) == 0) {
        const long long vend = start + ((end - start) & ~3LL);
#pragma unroll 4
        for (long long i = start + 4 * threadIdx.x; i < vend; i += 4 * 256) {
            f4 p = *(const f4*)(P + i), m = *(const f4*)(M + i), v = *(const f4*)(V + i);
            const f4 g = *(const f4*)(G + i);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                float pk = p[k], mk = m[k], vk = v[k];
                adam_elem(pk, g[k], mk, vk, s);
                p[k] = pk;
                m[k] = mk;
                v[k] = vk;
                mx = fmaxf(mx, fabsf(pk));
            }
            *(f4*)(P + i) = p;
            *(f4*)(M + i) = m;
            *(f4*)(V + i) = v;
        }
        i0 = vend;
    }
    for (long long i = i0 + threadIdx.x; i < end; i += 256) {
        float p = P[i], m = M[i], v = V[i];
        adam_elem(p, G[i], m, v, s);
        mx = fmaxf(mx, fabsf(p));
        P[i] = p;
        M[i] = m;
        V[i] = v;
    }
    if (d.hl != nullptr) {                                  // (uniform per workgroup)
        mx = tree_max4(mx, red);
        if (threadIdx.x == 0) partials[d.part0 + it.y] = mx;   // (fmaxf drops a NaN operand, like absmax_part_kernel)
    }
}

__global__ __launch_bounds__(256) void adam_split_kernel(const AdamDev* __restrict__ table, const int2* __restrict__ items,
                                                         const float* __restrict__ partials, int terms) {
    __shared__ float red[4];
    const int2 it = items[blockIdx.x];
    const AdamDev d = table[it.x];
    float m = 0.f;
    for (int i = threadIdx.x; i < d.nchunk; i += 256) m = fmaxf(m, partials[d.part0 + i]);
    m = tree_max4(m, red);
    int e = 0;                                              // the exponent rule of split_fold_kernel: s max|w| in [512, 1024)
    if (m > 0.f && m < INFINITY) {
        (void)frexpf(m, &e);
        e = 10 - e;
    }
    e = e > EMAX ? EMAX : (e < -EMAX ? -EMAX : e);
    const float sc = ldexpf(1.f, e);
    if (it.y == 0 && threadIdx.x == 0) {
        d.scale2[0] = ldexpf(1.f, e);
        d.scale2[1] = ldexpf(1.f, -e);
    }
    const long long start8 = (long long)it.y * (CHUNK / 8);
    const long long end = (long long)it.y * CHUNK + CHUNK < d.n ? (long long)it.y * CHUNK + CHUNK : d.n;
    const long long end8 = end >> 3;                        // (split tensors have n % 8 == 0)
    for (long long j = start8 + threadIdx.x; j < end8; j += 256) {
        const f4 a = ((const f4*)d.p)[2 * j], b = ((const f4*)d.p)[2 * j + 1];
        const float w[8] = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
        h8 hi, lo;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const float x = w[k] * sc;
            const _Float16 h = (_Float16)fminf(fmaxf(x, -65504.f), 65504.f);
            hi[k] = h;
#ifdef PP_STUDY_W_LO_ZERO   // (precision study builds, pp_common.h — as split_fold_kernel)
            lo[k] = (_Float16)0.f;
#else
            lo[k] = (_Float16)(x - (float)h);
#endif
        }
        if (terms == 1) {
            ((h8*)d.hl)[j] = hi;                            // h format: f16(s w)
        } else {
            ((h8*)d.hl)[2 * j] = hi;                        // hl format: per 8 k the hi then the lo terms
            ((h8*)d.hl)[2 * j + 1] = lo;
        }
    }
}

// validates the tensor list and sizes the workspace: [table | items | split items | chunk maxima], each section 256-byte aligned
int adam_layout(const PpAdamTensor* t, int nt, Layout* L) {
    if (!t || nt <= 0) return PP_EINVAL;
    long long nitems = 0, nsplit = 0;
    for (int i = 0; i < nt; ++i) {
        const PpAdamTensor& x = t[i];
        if (!x.p || !x.m || !x.v || x.n <= 0) return PP_EINVAL;
        const long long c = (x.n + CHUNK - 1) / CHUNK;
        nitems += c;
        if (x.hl) {
            if (!x.scale2 || x.n % 8 != 0 || ((uintptr_t)x.p & 15) || ((uintptr_t)x.hl & 15)) return PP_EINVAL;
            nsplit += c;
        }
    }
    if (nitems > (1LL << 30)) return PP_EINVAL;
    L->nitems = (int)nitems;
    L->nsplit = (int)nsplit;
    L->off_items = align256(sizeof(AdamDev) * (size_t)nt);
    L->off_split = L->off_items + align256(sizeof(int2) * (size_t)nitems);
    L->off_part = L->off_split + align256(sizeof(int2) * (size_t)(nsplit > 0 ? nsplit : 1));
    L->table_bytes = L->off_part;
    L->total = L->off_part + align256(sizeof(float) * (size_t)(nsplit > 0 ? nsplit : 1));
    return PP_OK;
}

}  // namespace

extern "C" {

int pp_adam_workspace_bytes(const PpAdamTensor* tensors, int ntensors, size_t* bytes) {
    if (!bytes) return PP_EINVAL;
    Layout L;
    const int rc = adam_layout(tensors, ntensors, &L);
    if (rc != PP_OK) return rc;
    *bytes = L.total;
    return PP_OK;
}

int pp_adam_multi_tensor(const PpAdamTensor* tensors, int ntensors, const PpAdamStep* steps, int terms, int rebuild, void* workspace,
                         size_t workspace_bytes, void* stream) {
    if (!steps || !workspace || (terms != 0 && terms != 1 && terms != 2)) return PP_EINVAL;
    Layout L;
    const int rc = adam_layout(tensors, ntensors, &L);
    if (rc != PP_OK) return rc;
    if (workspace_bytes < L.total || ((uintptr_t)workspace & 255)) return PP_EWORKSPACE;
    const hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)workspace;
    if (rebuild) {   // lay the table out on the host, upload it once (the only wait of this entry point: the host image dies on return)
        std::vector<char> img(L.table_bytes, 0);
        AdamDev* d = (AdamDev*)img.data();
        int2* items = (int2*)(img.data() + L.off_items);
        int2* split = (int2*)(img.data() + L.off_split);
        int k = 0, ks = 0;
        for (int i = 0; i < ntensors; ++i) {
            const PpAdamTensor& x = tensors[i];
            const int c = (int)((x.n + CHUNK - 1) / CHUNK);
            d[i].p = x.p;
            d[i].m = x.m;
            d[i].v = x.v;
            d[i].hl = (_Float16*)x.hl;
            d[i].scale2 = x.hl ? x.scale2 : nullptr;
            d[i].n = x.n;
            d[i].part0 = x.hl ? ks : 0;
            d[i].nchunk = c;
            d[i].vec = (((uintptr_t)x.p | (uintptr_t)x.m | (uintptr_t)x.v) & 15) == 0;
            d[i].pad = 0;
            for (int j = 0; j < c; ++j) {
                items[k++] = make_int2(i, j);
                if (x.hl) split[ks++] = make_int2(i, j);
            }
        }
        PP_CHECK_HIP(hipMemcpyAsync(ws, img.data(), L.table_bytes, hipMemcpyHostToDevice, st));
        PP_CHECK_HIP(hipStreamSynchronize(st));
    }
    const AdamDev* table = (const AdamDev*)ws;
    float* partials = (float*)(ws + L.off_part);
    hipLaunchKernelGGL(adam_update_kernel, dim3(L.nitems), dim3(256), 0, st, table, (const int2*)(ws + L.off_items), steps, partials);
    if (L.nsplit > 0 && terms > 0)
        hipLaunchKernelGGL(adam_split_kernel, dim3(L.nsplit), dim3(256), 0, st, table, (const int2*)(ws + L.off_split),
                           (const float*)partials, terms);
    return pp_last_launch();
}

}  // extern "C"
