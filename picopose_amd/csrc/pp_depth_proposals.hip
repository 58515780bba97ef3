// Mask proposals from the depth image ("DEPTH PROPOSALS" of include/picopose_hip.h; picopose_amd/depth_proposals.py plans every call and
// tests/depth_proposals_oracle.py restates the contract in numpy): the dominant plane of every image by consensus, the pixels that stand
// off it labelled into 4-connected components with a union-find, per-component records, and COCO run lengths of the kept components.
// THE PROJECT'S OWN ALGORITHM, as pp_verify.hip, pp_rgbd_pose.hip and pp_depth_refine.hip are: no parity with any published segmenter.
//
//   plane_score_kernel     workgroups (strip of PP_PLANE_STRIP pixels, image): the image's hypotheses are rebuilt into LDS (three hashed
//                          pixels each), every lane keeps four back-projected pixels in registers, and per hypothesis a wave counts its
//                          inliers by ballot + popcount into an LDS counter; then one integer atomicAdd per hypothesis and workgroup
//   plane_moments_kernel   the same strips: every workgroup finds the winner from the counts (arg-max, lowest h), and sums the ten
//                          float64 moments of its strip's consensus pixels about the winner's first sample point (block_reduce_all's fixed order)
//   plane_finish_kernel    one wave per image adds the strips' partial sums in a fixed order, takes the smallest eigenvector with
//                          jacobi_sym<3> and writes the plane and the info row
//   cc_tile_kernel         one workgroup per 32 x 128 tile: foreground test, labels and depth staged in LDS; every pixel starts at the
//                          head of its horizontal run within its wave's 64 pixels (one ballot), then union-find by atomicMin in LDS over
//                          the links the runs do not hold (an upward link whose square the left neighbour closes is skipped); each
//                          pixel's root is written as a global pixel index
//   cc_border_kernel       the pixel pairs across tile edges: find / atomicMin in global memory
//   cc_flatten_kernel      every label replaced by its root
//   stats_init / stats_accumulate / stats_select   per-root area, box and border flag (lanes of a wave that share a root are reduced
//                          first), the filter and the capped compact list
//   rle_kernel             one workgroup per kept component walks the columns of its box and compacts the toggle positions in order
//
// Only integers meet in atomics, and union by smaller index makes every label the smallest pixel index of its component: no output
// depends on launch order or stream.  Every float32 expression that decides a comparison is written with the rounding intrinsics, in
// the order the header states.
#include <stdint.h>
#include <limits.h>
#include <math.h>
#include "pp_common.h"
#include "pp_runs_dev.h"

#pragma clang fp contract(off)
#include "pp_ransac_dev.h"

namespace {

constexpr int BLOCK = 256;
constexpr int WAVES = BLOCK / 64;
constexpr int STRIP = PP_PLANE_STRIP;
constexpr int PPL = STRIP / BLOCK;                   // pixels per lane of a strip
constexpr int NM = 10;                               // sx sy sz sxx sxy sxz syy syz szz n
constexpr int TW = 128, TH = 32, TPX = TW * TH;      // the component tile
constexpr int REC = 6;                               // area xmin ymin xmax ymax border
constexpr float CROSS_FLOOR = PP_PLANE_MIN_CROSS2;

struct Cam { float fx, fy, cx, cy; };
struct Hyp { float nx, ny, nz, d, px, py, pz; };    // d is NaN for a hypothesis that cannot win
struct Fg { float min_height, max_height, max_range, max_step; };

__device__ __forceinline__ Cam load_cam(const float* cams, int b) {
    const float* k = cams + 4 * (size_t)b;
    return Cam{k[0], k[1], k[2], k[3]};
}
__device__ __forceinline__ bool depth_valid(float z) { return z > 0.f && z < INFINITY; }         // (a NaN is neither)

// THE POINT of the header: X = ((u - cx) z) / fx, Y = ((v - cy) z) / fy, Z = z
__device__ __forceinline__ void back_project(const Cam& k, int u, int v, float z, float& X, float& Y) {
    X = __fdiv_rn(__fmul_rn(__fsub_rn((float)u, k.cx), z), k.fx);
    Y = __fdiv_rn(__fmul_rn(__fsub_rn((float)v, k.cy), z), k.fy);
}
// THE HEIGHT of the header: ((nx X + ny Y) + nz Z) + d
__device__ __forceinline__ float plane_height(float nx, float ny, float nz, float d, float X, float Y, float Z) {
    return __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(nx, X), __fmul_rn(ny, Y)), __fmul_rn(nz, Z)), d);
}

__device__ Hyp make_hypothesis(const float* img, const Cam& k, int W, unsigned hw, unsigned seed, int b, int h) {
    float P[3][3];
    bool ok = true;
#pragma unroll
    for (int s = 0; s < 3; ++s) {
        const unsigned r = aug_hash(seed, (unsigned)b, (unsigned)(3 * h + s));
        const unsigned i = (unsigned)(((unsigned long long)r * hw) >> 32);                         // < hw
        const int v = (int)(i / (unsigned)W), u = (int)(i - (unsigned)v * (unsigned)W);
        const float z = img[i];
        ok = ok && depth_valid(z);
        back_project(k, u, v, z, P[s][0], P[s][1]);
        P[s][2] = z;
    }
    const float ax = __fsub_rn(P[1][0], P[0][0]), ay = __fsub_rn(P[1][1], P[0][1]), az = __fsub_rn(P[1][2], P[0][2]);
    const float bx = __fsub_rn(P[2][0], P[0][0]), by = __fsub_rn(P[2][1], P[0][1]), bz = __fsub_rn(P[2][2], P[0][2]);
    const float cx = __fsub_rn(__fmul_rn(ay, bz), __fmul_rn(az, by));
    const float cy = __fsub_rn(__fmul_rn(az, bx), __fmul_rn(ax, bz));
    const float cz = __fsub_rn(__fmul_rn(ax, by), __fmul_rn(ay, bx));
    const float len2 = __fadd_rn(__fadd_rn(__fmul_rn(cx, cx), __fmul_rn(cy, cy)), __fmul_rn(cz, cz));
    Hyp o{0.f, 0.f, 0.f, NAN, P[0][0], P[0][1], P[0][2]};
    if (ok && len2 > CROSS_FLOOR && len2 < INFINITY) {
        const float inv = __fdiv_rn(1.f, __fsqrt_rn(len2));
        o.nx = __fmul_rn(cx, inv), o.ny = __fmul_rn(cy, inv), o.nz = __fmul_rn(cz, inv);
        o.d = -__fadd_rn(__fadd_rn(__fmul_rn(o.nx, o.px), __fmul_rn(o.ny, o.py)), __fmul_rn(o.nz, o.pz));
    }
    return o;
}

// pixel i of the image as a point; an invalid pixel (or one past the frame) is all NaN and fails every comparison
__device__ __forceinline__ void load_point(const float* img, const Cam& k, int W, unsigned hw, unsigned i, float& X, float& Y, float& Z) {
    X = Y = Z = NAN;
    if (i < hw) {
        const float z = img[i];
        if (depth_valid(z)) {
            const int v = (int)(i / (unsigned)W), u = (int)(i - (unsigned)v * (unsigned)W);
            back_project(k, u, v, z, X, Y);
            Z = z;
        }
    }
}

__global__ __launch_bounds__(BLOCK) void plane_score_kernel(const float* __restrict__ depth, const float* __restrict__ cams, int H, int W,
                                                            int n_hyp, unsigned seed, float tau, int* __restrict__ counts) {
    __shared__ float4 hyp[PP_PLANE_MAX_HYP];
    __shared__ int cnt[PP_PLANE_MAX_HYP];
    const int b = blockIdx.y, lane = threadIdx.x & 63;
    const unsigned hw = (unsigned)H * (unsigned)W;
    const float* img = depth + (size_t)b * hw;
    const Cam k = load_cam(cams, b);
    for (int h = threadIdx.x; h < n_hyp; h += BLOCK) {
        const Hyp q = make_hypothesis(img, k, W, hw, seed, b, h);
        hyp[h] = make_float4(q.nx, q.ny, q.nz, q.d);
        cnt[h] = 0;
    }
    float X[PPL], Y[PPL], Z[PPL];
#pragma unroll
    for (int j = 0; j < PPL; ++j)
        load_point(img, k, W, hw, blockIdx.x * (unsigned)STRIP + (unsigned)(j * BLOCK) + threadIdx.x, X[j], Y[j], Z[j]);
    __syncthreads();
    for (int h = 0; h < n_hyp; ++h) {
        const float4 p = hyp[h];
        if (!(p.w == p.w)) continue;                                 // (uniform: a dead hypothesis scores 0)
        int c = 0;
#pragma unroll
        for (int j = 0; j < PPL; ++j) c += __popcll(__ballot(fabsf(plane_height(p.x, p.y, p.z, p.w, X[j], Y[j], Z[j])) <= tau));
        if (lane == 0 && c) atomicAdd(&cnt[h], c);
    }
    __syncthreads();
    for (int h = threadIdx.x; h < n_hyp; h += BLOCK)
        if (cnt[h]) atomicAdd(counts + (size_t)b * n_hyp + h, cnt[h]);
}

__global__ __launch_bounds__(BLOCK) void plane_moments_kernel(const float* __restrict__ depth, const float* __restrict__ cams, int H, int W,
                                                              int n_hyp, unsigned seed, float tau, int min_inliers,
                                                              const int* __restrict__ counts, double* __restrict__ partial) {
    __shared__ Winner sm[WAVES];
    __shared__ double red[WAVES * NM];
    const int b = blockIdx.y;
    const unsigned hw = (unsigned)H * (unsigned)W;
    const float* img = depth + (size_t)b * hw;
    double* out = partial + ((size_t)b * gridDim.x + blockIdx.x) * NM;
    const Winner win = winner<WAVES>(counts + (size_t)b * n_hyp, n_hyp, sm, INT_MAX);
    const int wh = win.h, wc = win.c;
    if (wc < min_inliers) {                                          // (uniform: no plane)
        if (threadIdx.x < NM) out[threadIdx.x] = 0.0;
        return;
    }
    const Cam k = load_cam(cams, b);
    const Hyp w = make_hypothesis(img, k, W, hw, seed, b, wh);
    double v[NM];
#pragma unroll
    for (int c = 0; c < NM; ++c) v[c] = 0.0;
#pragma unroll
    for (int j = 0; j < PPL; ++j) {
        float X, Y, Z;
        load_point(img, k, W, hw, blockIdx.x * (unsigned)STRIP + (unsigned)(j * BLOCK) + threadIdx.x, X, Y, Z);
        if (fabsf(plane_height(w.nx, w.ny, w.nz, w.d, X, Y, Z)) <= tau) {
            const double qx = (double)X - (double)w.px, qy = (double)Y - (double)w.py, qz = (double)Z - (double)w.pz;
            v[0] += qx, v[1] += qy, v[2] += qz;
            v[3] += qx * qx, v[4] += qx * qy, v[5] += qx * qz, v[6] += qy * qy, v[7] += qy * qz, v[8] += qz * qz;
            v[9] += 1.0;
        }
    }
    __syncthreads();   // (kept: the sum has always had a barrier before its LDS write as well as after it)
    block_reduce_all<WAVES>(v, red, op_sum{}, 0.0);
    if (threadIdx.x < NM) {
#pragma unroll
        for (int c = 0; c < NM; ++c)
            if (threadIdx.x == c) out[c] = v[c];
    }
}

__global__ __launch_bounds__(64) void plane_finish_kernel(const float* __restrict__ depth, const float* __restrict__ cams, int H, int W,
                                                          int n_hyp, unsigned seed, int min_inliers, int n_strips,
                                                          const int* __restrict__ counts, const double* __restrict__ partial,
                                                          float* __restrict__ plane, double* __restrict__ plane64, int* __restrict__ info) {
    const int b = blockIdx.x;
    const unsigned hw = (unsigned)H * (unsigned)W;
    const Winner win = winner<1>(counts + (size_t)b * n_hyp, n_hyp, nullptr, INT_MAX);
    const int wh = win.h, wc = win.c;
    double v[NM];
#pragma unroll
    for (int c = 0; c < NM; ++c) v[c] = 0.0;
    for (int s = threadIdx.x; s < n_strips; s += 64) {               // lane l: strips l, l + 64, ... in ascending order
        const double* p = partial + ((size_t)b * n_strips + s) * NM;
#pragma unroll
        for (int c = 0; c < NM; ++c) v[c] += p[c];
    }
#pragma unroll
    for (int c = 0; c < NM; ++c) v[c] = wave_sum(v[c]);
    if (threadIdx.x != 0) return;
    double n0 = 0.0, n1 = 0.0, n2 = 0.0, d = 0.0;
    const bool has = wc >= min_inliers;
    if (has) {
        const Hyp w = make_hypothesis(depth + (size_t)b * hw, load_cam(cams, b), W, hw, seed, b, wh);
        const double N = v[9], mx = v[0] / N, my = v[1] / N, mz = v[2] / N;
        double A[3][3], V[3][3];
        A[0][0] = v[3] / N - mx * mx, A[0][1] = v[4] / N - mx * my, A[0][2] = v[5] / N - mx * mz;
        A[1][1] = v[6] / N - my * my, A[1][2] = v[7] / N - my * mz, A[2][2] = v[8] / N - mz * mz;
        A[1][0] = A[0][1], A[2][0] = A[0][2], A[2][1] = A[1][2];
        jacobi_sym<3>(A, V);
        const bool k1 = A[1][1] < A[0][0];                           // (selects, not indices: a run-time row index would live in scratch)
        const double e = k1 ? A[1][1] : A[0][0];
        const bool k2 = A[2][2] < e;
        n0 = k2 ? V[2][0] : (k1 ? V[1][0] : V[0][0]);
        n1 = k2 ? V[2][1] : (k1 ? V[1][1] : V[0][1]);
        n2 = k2 ? V[2][2] : (k1 ? V[1][2] : V[0][2]);
        const double len = sqrt(n0 * n0 + n1 * n1 + n2 * n2);
        n0 /= len, n1 /= len, n2 /= len;
        d = -(n0 * ((double)w.px + mx) + n1 * ((double)w.py + my) + n2 * ((double)w.pz + mz));
        if (d < 0.0) { n0 = -n0, n1 = -n1, n2 = -n2, d = -d; }       // the camera is on the positive side
    }
    plane64[4 * (size_t)b] = n0, plane64[4 * (size_t)b + 1] = n1, plane64[4 * (size_t)b + 2] = n2, plane64[4 * (size_t)b + 3] = d;
    plane[4 * (size_t)b] = (float)n0, plane[4 * (size_t)b + 1] = (float)n1, plane[4 * (size_t)b + 2] = (float)n2, plane[4 * (size_t)b + 3] = (float)d;
    info[4 * (size_t)b] = has ? 1 : 0, info[4 * (size_t)b + 1] = wh, info[4 * (size_t)b + 2] = wc, info[4 * (size_t)b + 3] = has ? (int)v[9] : 0;
}

// ------------------------------------------------------------------ components
// Union by smaller index on a parent array whose entries only ever decrease: find follows parents to the entry that is its own,
// unite links the larger root under the smaller with atomicMin and goes on with whatever it displaced.
__device__ __forceinline__ int lds_find(volatile int* lab, int x) {
    for (;;) {
        const int p = lab[x];
        if (p == x) return x;
        x = p;
    }
}
__device__ __forceinline__ void lds_unite(int* lab, int a, int b) {
    for (;;) {
        a = lds_find(lab, a), b = lds_find(lab, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(&lab[a], b);
        if (old == a) return;
        a = old;
    }
}
// the same in global memory; parents are read at agent scope, so a value another XCD has replaced is at worst an older parent
__device__ __forceinline__ int g_find(int* lab, int x) {
    for (;;) {
        const int p = __hip_atomic_load(lab + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (p == x) return x;
        x = p;
    }
}
__device__ __forceinline__ void g_unite(int* lab, int a, int b) {
    for (;;) {
        a = g_find(lab, a), b = g_find(lab, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(lab + a, b);
        if (old == a) return;
        a = old;
    }
}
__device__ __forceinline__ bool stepped(float zp, float zq, float max_step) { return fabsf(__fsub_rn(zp, zq)) <= max_step; }

__global__ __launch_bounds__(BLOCK) void cc_tile_kernel(const float* __restrict__ depth, const float* __restrict__ cams,
                                                        const float* __restrict__ plane, const int* __restrict__ has_plane, int H, int W,
                                                        Fg fg, int* __restrict__ labels) {
    __shared__ int lab[TPX];
    __shared__ float zt[TPX];
    const int b = blockIdx.z, tx0 = blockIdx.x * TW, ty0 = blockIdx.y * TH;
    const size_t hw = (size_t)H * W;
    const float* img = depth + (size_t)b * hw;
    const Cam k = load_cam(cams, b);
    const bool hp = has_plane[b] != 0;
    const float nx = plane[4 * (size_t)b], ny = plane[4 * (size_t)b + 1], nz = plane[4 * (size_t)b + 2], pd = plane[4 * (size_t)b + 3];
    // the depth of a foreground pixel, NaN for every other one: a NaN is connected to nothing (stepped() is false)
    for (int p = threadIdx.x; p < TPX; p += BLOCK) {
        const int x = tx0 + (p & (TW - 1)), y = ty0 + p / TW;
        float zf = NAN;
        if (x < W && y < H) {
            const float z = img[(size_t)y * W + x];
            if (depth_valid(z) && z <= fg.max_range) {
                bool in = true;
                if (hp) {
                    float X, Y;
                    back_project(k, x, y, z, X, Y);
                    const float s = plane_height(nx, ny, nz, pd, X, Y, z);
                    in = s > fg.min_height && s < fg.max_height;
                }
                if (in) zf = z;
            }
        }
        zt[p] = zf;
    }
    __syncthreads();
    // A wave holds 64 consecutive pixels of one tile row (TW and BLOCK are multiples of 64).  Every pixel starts at the first pixel
    // of its horizontal run within those 64: the highest break (a pixel not connected to its left neighbour; lane 0 always) at or
    // below its lane, from one ballot.  A run start is the smallest index of its run, so parents stay below their children.
    const int lane = threadIdx.x & 63;
    for (int p = threadIdx.x; p < TPX; p += BLOCK) {
        const float zp = zt[p];
        const bool left = (p & (TW - 1)) > 0 && stepped(zp, zt[p - 1], fg.max_step);
        const unsigned long long breaks = __ballot(lane == 0 || !left);
        const int start = 63 - __clzll((long long)(breaks & (~0ull >> (63 - lane))));
        lab[p] = zp == zp ? p - (lane - start) : -1;
    }
    __syncthreads();
    // The links the runs do not hold: across the two 64-pixel halves of a row, and upwards.  An upward link is skipped when the
    // left neighbour's closes the same square (p ~ p - 1 ~ p - 1 - TW ~ p - TW): those three links are made elsewhere.
    for (int p = threadIdx.x; p < TPX; p += BLOCK) {
        const float zp = zt[p];
        if (!(zp == zp)) continue;
        const bool left = (p & (TW - 1)) > 0 && stepped(zp, zt[p - 1], fg.max_step);
        if (left && lane == 0) lds_unite(lab, p, p - 1);
        if (p >= TW && stepped(zp, zt[p - TW], fg.max_step)) {
            const bool square = left && stepped(zt[p - 1], zt[p - 1 - TW], fg.max_step) && stepped(zt[p - TW], zt[p - 1 - TW], fg.max_step);
            if (!square) lds_unite(lab, p, p - TW);
        }
    }
    __syncthreads();
    for (int p = threadIdx.x; p < TPX; p += BLOCK) {
        const int x = tx0 + (p & (TW - 1)), y = ty0 + p / TW;
        if (x >= W || y >= H) continue;
        int g = -1;
        if (lab[p] >= 0) {
            const int r = lds_find(lab, p);
            g = (ty0 + r / TW) * W + tx0 + (r & (TW - 1));
        }
        labels[(size_t)b * hw + (size_t)y * W + x] = g;
    }
}

__global__ __launch_bounds__(BLOCK) void cc_border_kernel(const float* __restrict__ depth, int H, int W, int n_rows, int n_items, float max_step,
                                                          int* __restrict__ labels) {
    const int b = blockIdx.y, item = blockIdx.x * BLOCK + threadIdx.x;
    if (item >= n_items) return;
    const size_t hw = (size_t)H * W;
    int p, q;                                                        // the pair: p and its upper or left neighbour q
    if (item < n_rows * W) {
        const int r = item / W;
        p = (r + 1) * TH * W + (item - r * W), q = p - W;
    } else {
        const int j = item - n_rows * W, c = j / H;
        p = (j - c * H) * W + (c + 1) * TW, q = p - 1;
    }
    int* lab = labels + (size_t)b * hw;
    const float* img = depth + (size_t)b * hw;
    if (lab[p] >= 0 && lab[q] >= 0 && stepped(img[p], img[q], max_step)) g_unite(lab, p, q);
}

__global__ __launch_bounds__(BLOCK) void cc_flatten_kernel(int hw, int* __restrict__ labels) {
    int* lab = labels + (size_t)blockIdx.y * hw;
    for (long long i = (long long)blockIdx.x * BLOCK + threadIdx.x; i < hw; i += (long long)gridDim.x * BLOCK) {
        const int l = lab[i];
        if (l < 0) continue;
        const int r = g_find(lab, l);
        if (r != l) lab[i] = r;
    }
}

// ------------------------------------------------------------------ records
__global__ __launch_bounds__(BLOCK) void stats_init_kernel(const int* __restrict__ labels, int hw, int W, int* __restrict__ rec) {
    const int* lab = labels + (size_t)blockIdx.y * hw;
    int* rc = rec + (size_t)blockIdx.y * hw * REC;
    for (long long i = (long long)blockIdx.x * BLOCK + threadIdx.x; i < hw; i += (long long)gridDim.x * BLOCK)
        if (lab[i] == (int)i) {
            int* r = rc + (size_t)i * REC;
            r[0] = 0, r[1] = INT_MAX, r[2] = (int)(i / W), r[3] = -1, r[4] = -1, r[5] = 0;       // (a root is its component's first row)
        }
}

__device__ __forceinline__ void rec_add(int* r, int area, int xmin, int xmax, int ymax, int border) {
    atomicAdd(r, area);
    atomicMin(r + 1, xmin);
    atomicMax(r + 3, xmax);
    atomicMax(r + 4, ymax);
    if (border) atomicOr(r + 5, 1);
}

__global__ __launch_bounds__(BLOCK) void stats_accumulate_kernel(const int* __restrict__ labels, int hw, int H, int W, int* __restrict__ rec) {
    const int* lab = labels + (size_t)blockIdx.y * hw;
    int* rc = rec + (size_t)blockIdx.y * hw * REC;
    const int lane = threadIdx.x & 63;
    for (long long base = (long long)blockIdx.x * BLOCK; base < hw; base += (long long)gridDim.x * BLOCK) {      // (uniform bounds)
        const long long i = base + threadIdx.x;
        int root = i < hw ? lab[i] : -1;
        const int y = (int)(i / W), x = (int)(i - (long long)y * W);
        const bool border = x == 0 || y == 0 || x == W - 1 || y == H - 1;
        for (int it = 0; it < 4; ++it) {                             // the lanes that share a root, one root per turn
            const unsigned long long todo = __ballot(root >= 0);
            if (!todo) break;
            const int leader = __ffsll((long long)todo) - 1;
            const int r = __shfl(root, leader);
            const bool mine = root == r;
            const int area = __popcll(__ballot(mine));
            const int bord = __ballot(mine && border) != 0ull;
            int box[3] = {mine ? x : INT_MAX, mine ? x : -1, mine ? y : -1};                // xmin, xmax, ymax
            wave_reduce_each(box, [](int c, int p, int q) { return c == 0 ? min(p, q) : max(p, q); });
            if (lane == leader) rec_add(rc + (size_t)r * REC, area, box[0], box[1], box[2], bord);
            if (mine) root = -1;
        }
        if (root >= 0) rec_add(rc + (size_t)root * REC, 1, x, x, y, border ? 1 : 0);
    }
}

__global__ __launch_bounds__(BLOCK) void stats_select_kernel(const int* __restrict__ labels, int hw, const int* __restrict__ rec, int min_area,
                                                             int max_area, int drop_border, int cap, int* __restrict__ n_qualified,
                                                             int* __restrict__ comps) {
    const int b = blockIdx.y;
    const int* lab = labels + (size_t)b * hw;
    const int* rc = rec + (size_t)b * hw * REC;
    for (long long i = (long long)blockIdx.x * BLOCK + threadIdx.x; i < hw; i += (long long)gridDim.x * BLOCK) {
        if (lab[i] != (int)i) continue;
        const int* r = rc + (size_t)i * REC;
        if (r[0] < min_area || r[0] > max_area || (drop_border && r[5])) continue;
        const int slot = atomicAdd(n_qualified + b, 1);
        if (slot < cap) {
            int* o = comps + ((size_t)b * cap + slot) * PP_COMPONENT_FIELDS;
            o[0] = (int)i, o[1] = r[0], o[2] = r[1], o[3] = r[2], o[4] = r[3], o[5] = r[4], o[6] = r[5];
        }
    }
}

// ------------------------------------------------------------------ run lengths
// One workgroup per component.  Column-major position f = x H + y toggles when pixel f and pixel f - 1 differ in membership; a set
// pixel lies in the box, so every toggle lies in one of the column walks [x H + ymin, x H + ymax + 1], taken in ascending order.
__global__ __launch_bounds__(BLOCK) void rle_kernel(const int* __restrict__ labels, int H, int W, const int* __restrict__ sel,
                                                    const int* __restrict__ run_offset, int* __restrict__ n_runs, int* __restrict__ ends) {
    __shared__ int wsum[WAVES];
    const int* s = sel + PP_RLE_SEL_FIELDS * (size_t)blockIdx.x;
    const int root = s[1], xmin = s[2], ymin = s[3], xmax = s[4], ymax = s[5];
    const int hw = H * W, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int* img = labels + (size_t)s[0] * hw;
    const bool emit = ends != nullptr;
    const int off = emit ? run_offset[blockIdx.x] : 0, lim = emit ? run_offset[blockIdx.x + 1] : 0;
    const bool full = ymin == 0 && ymax == H - 1;                    // the walks of a full-height box join into one range
    const int L = full ? H : ymax - ymin + 2;
    const long long total = (long long)(xmax - xmin + 1) * L + (full ? 1 : 0);
    auto member = [&](int f) {
        const int x = f / H, y = f - x * H;
        return x >= xmin && x <= xmax && y >= ymin && y <= ymax && img[(size_t)y * W + x] == root;
    };
    int base = img[0] == root ? 1 : 0;                               // the leading 0 when pixel 0 is set
    if (emit && threadIdx.x == 0 && base && off < lim) ends[off] = 0;
    for (long long c0 = 0; c0 < total; c0 += BLOCK) {
        const long long c = c0 + threadIdx.x;
        bool t = false;
        int f = 0;
        if (c < total) {
            const int col = (int)(c / L);
            f = (xmin + col) * H + ymin + (int)(c - (long long)col * L);                           // <= H W
            if (f >= 1 && f < hw) t = member(f) != member(f - 1);
        }
        const unsigned long long m = __ballot(t);
        if (lane == 0) wsum[wave] = __popcll(m);
        __syncthreads();
        int before = 0, all = 0;
#pragma unroll
        for (int w = 0; w < WAVES; ++w) {
            before += w < wave ? wsum[w] : 0;
            all += wsum[w];
        }
        if (t && emit) {
            const int idx = off + base + before + __popcll(m & ((1ull << lane) - 1ull));
            if (idx < lim) ends[idx] = f;
        }
        base += all;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        if (!emit) n_runs[blockIdx.x] = base + 1;
        else if (off + base < lim) ends[off + base] = hw;
    }
}

inline size_t roundup256(size_t n) { return (n + 255) / 256 * 256; }
inline bool frame_ok(int B, int H, int W) { return B > 0 && B <= 65535 && H > 0 && W > 0 && (long long)H * W < (1ll << 31); }
inline unsigned stride_grid(long long n) {
    const long long g = (n + BLOCK - 1) / BLOCK;
    return (unsigned)(g < 1 ? 1 : (g > 2048 ? 2048 : g));
}

}  // namespace

extern "C" {

int pp_depth_plane_workspace_bytes(int B, int H, int W, int n_hyp, size_t* bytes) {
    if (!bytes || !frame_ok(B, H, W) || n_hyp < 1 || n_hyp > PP_PLANE_MAX_HYP) return PP_EINVAL;
    const size_t strips = ((size_t)H * W + STRIP - 1) / STRIP;
    *bytes = roundup256(sizeof(int) * (size_t)B * n_hyp) + roundup256(sizeof(double) * NM * strips * (size_t)B);
    return PP_OK;
}

int pp_depth_plane(const float* depth, const float* cams, int B, int H, int W, int n_hyp, unsigned seed, float tau, int min_inliers,
                   void* workspace, size_t workspace_bytes, float* plane, double* plane64, int* info, void* stream) {
    size_t need = 0;
    if (!depth || !cams || !workspace || !plane || !plane64 || !info) return PP_EINVAL;
    if (pp_depth_plane_workspace_bytes(B, H, W, n_hyp, &need) != PP_OK) return PP_EINVAL;
    if (!(tau >= 0.f) || !(tau < INFINITY) || min_inliers < 3) return PP_EINVAL;
    if (((uintptr_t)workspace % 256) != 0 || workspace_bytes < need) return PP_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const unsigned strips = (unsigned)(((size_t)H * W + STRIP - 1) / STRIP);
    int* counts = (int*)workspace;
    double* partial = (double*)((char*)workspace + roundup256(sizeof(int) * (size_t)B * n_hyp));
    PP_CHECK_HIP(hipMemsetAsync(counts, 0, sizeof(int) * (size_t)B * n_hyp, st));
    hipLaunchKernelGGL(plane_score_kernel, dim3(strips, (unsigned)B), dim3(BLOCK), 0, st, depth, cams, H, W, n_hyp, seed, tau, counts);
    hipLaunchKernelGGL(plane_moments_kernel, dim3(strips, (unsigned)B), dim3(BLOCK), 0, st, depth, cams, H, W, n_hyp, seed, tau, min_inliers,
                       (const int*)counts, partial);
    hipLaunchKernelGGL(plane_finish_kernel, dim3((unsigned)B), dim3(64), 0, st, depth, cams, H, W, n_hyp, seed, min_inliers, (int)strips,
                       (const int*)counts, (const double*)partial, plane, plane64, info);
    return pp_last_launch();
}

int pp_depth_components_workspace_bytes(int B, int H, int W, size_t* bytes) {
    if (!bytes || !frame_ok(B, H, W)) return PP_EINVAL;
    *bytes = 0;                                                      // the labels are the union-find's parent array
    return PP_OK;
}

int pp_depth_components(const float* depth, const float* cams, const float* plane, const int* has_plane, int B, int H, int W,
                        float min_height, float max_height, float max_range, float max_step, void* workspace, size_t workspace_bytes,
                        int* labels, void* stream) {
    (void)workspace, (void)workspace_bytes;
    if (!depth || !cams || !plane || !has_plane || !labels || !frame_ok(B, H, W)) return PP_EINVAL;
    if (min_height != min_height || max_height != max_height || !(max_range > 0.f) || !(max_step >= 0.f) || !(max_step < INFINITY))
        return PP_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const Fg fg{min_height, max_height, max_range, max_step};
    const int gx = (W + TW - 1) / TW, gy = (H + TH - 1) / TH;
    if (gy > 65535) return PP_EINVAL;
    hipLaunchKernelGGL(cc_tile_kernel, dim3((unsigned)gx, (unsigned)gy, (unsigned)B), dim3(BLOCK), 0, st, depth, cams, plane, has_plane, H, W, fg, labels);
    const int n_rows = (H - 1) / TH, n_cols = (W - 1) / TW;
    const long long items = (long long)n_rows * W + (long long)n_cols * H;
    if (items > 0) {
        hipLaunchKernelGGL(cc_border_kernel, dim3((unsigned)((items + BLOCK - 1) / BLOCK), (unsigned)B), dim3(BLOCK), 0, st, depth, H, W, n_rows,
                           (int)items, max_step, labels);
        hipLaunchKernelGGL(cc_flatten_kernel, dim3(stride_grid((long long)H * W), (unsigned)B), dim3(BLOCK), 0, st, H * W, labels);
    }
    return pp_last_launch();
}

int pp_component_stats_workspace_bytes(int B, int H, int W, size_t* bytes) {
    if (!bytes || !frame_ok(B, H, W)) return PP_EINVAL;
    *bytes = roundup256(sizeof(int) * REC * (size_t)B * H * W);
    return PP_OK;
}

int pp_component_stats(const int* labels, int B, int H, int W, int min_area, int max_area, int drop_border, int cap, void* workspace,
                       size_t workspace_bytes, int* n_qualified, int* comps, void* stream) {
    size_t need = 0;
    if (!labels || !workspace || !n_qualified || !comps) return PP_EINVAL;
    if (pp_component_stats_workspace_bytes(B, H, W, &need) != PP_OK || min_area < 1 || max_area < min_area || cap < 1) return PP_EINVAL;
    if (((uintptr_t)workspace % 256) != 0 || workspace_bytes < need) return PP_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const int hw = H * W;
    int* rec = (int*)workspace;
    const dim3 grid(stride_grid(hw), (unsigned)B);
    PP_CHECK_HIP(hipMemsetAsync(n_qualified, 0, sizeof(int) * (size_t)B, st));
    hipLaunchKernelGGL(stats_init_kernel, grid, dim3(BLOCK), 0, st, labels, hw, W, rec);
    hipLaunchKernelGGL(stats_accumulate_kernel, grid, dim3(BLOCK), 0, st, labels, hw, H, W, rec);
    hipLaunchKernelGGL(stats_select_kernel, grid, dim3(BLOCK), 0, st, labels, hw, (const int*)rec, min_area, max_area, drop_border ? 1 : 0, cap,
                       n_qualified, comps);
    return pp_last_launch();
}

int pp_components_rle(const int* labels, int B, int H, int W, const int* sel, const int* sel_host, int n, const int* run_offset,
                      const int* run_offset_host, int n_runs_total, int* n_runs, int* run_ends, void* stream) {
    if (!labels || !sel || !sel_host || !frame_ok(B, H, W) || n <= 0 || n > PP_MASK_MAX_N) return PP_EINVAL;
    const bool emit = run_ends != nullptr;
    if (emit ? (!run_offset || !run_offset_host || n_runs_total <= 0) : !n_runs) return PP_EINVAL;
    for (int k = 0; k < n; ++k) {
        const int* s = sel_host + PP_RLE_SEL_FIELDS * (size_t)k;
        if ((unsigned)s[0] >= (unsigned)B || s[1] < 0 || s[1] >= H * W) return PP_EINVAL;
        if (s[2] < 0 || s[2] > s[4] || s[4] >= W || s[3] < 0 || s[3] > s[5] || s[5] >= H) return PP_EINVAL;
    }
    if (emit) {
        if (!pp_run_offsets_ok(run_offset_host, n, n_runs_total) || run_offset_host[0] != 0 || run_offset_host[n] != n_runs_total)
            return PP_EINVAL;
    }
    hipLaunchKernelGGL(rle_kernel, dim3((unsigned)n), dim3(BLOCK), 0, (hipStream_t)stream, labels, H, W, sel, run_offset, n_runs, run_ends);
    return pp_last_launch();
}

}  // extern "C"
