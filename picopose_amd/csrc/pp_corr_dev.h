// The parts of the correlation lookup that exist once: the coordinate round trip that the sampling kernels and their adjoints share, and
// the tile and pass skeleton of the two matrix-core lookups (pp_corr.hip).  The skeleton defines the result — window order, zeros padding,
// which pixel a pass serves, when the pass loop ends —; a kernel owns only its "S = F1_tile . F2_region^T" step.
#ifndef PP_CORR_DEV_H
#define PP_CORR_DEV_H
#include "pp_common.h"

// coordinate round trip of the reference: bilinear_sample scales pixel coords to [-1,1]
// (corr_lookup.py:61-63) and grid_sample(align_corners=True) maps them back
__device__ __forceinline__ float pp_roundtrip(float x, int size) {
    const float n = x * 2.f / (float)(size - 1 > 1 ? size - 1 : 1) - 1.f;
    return ((n + 1.f) / 2.f) * (float)(size - 1);
}

// For every pixel p and pyramid level l the (2r+1)^2 window around c = roundtrip((p + flow[p]) / 2^l) is bilinearly sampled, zeros
// padding.  WINDOW ORDER: output channel l*(2r+1)^2 + a*(2r+1) + b samples at x offset a-r, y offset b-r (the reference's transposed
// order); the integer corner (bx, by) = floor(c) - r anchors the (2r+2)^2 neighbourhood that the window's four-corner blends read.
// The tiled kernels give a workgroup an 8 x 8 tile of pixels, and per level a pixel is in one of three STATES: 0 = to do (a pass whose
// region holds its whole neighbourhood blends it), 1 = done, 2 = all zeros (the neighbourhood lies outside the map: no work).
constexpr int MAXR = 2, TW = 2 * MAXR + 2, MAXL = 3;   // radius, neighbourhood edge, levels
constexpr int CT = 8, CM = CT * CT;                    // source-pixel tile

// One result element of the tiled lookups: channel ch of pixel row `row`, into the fp32 map (rows of ld_out floats) or, out_hl given, into
// the hl operand of the 1x1 convolution that reads the map (rows of ld_out channels = 2 ld_out halfs) — the split of pp_split_f16_chk, so
// the bits and the saturation report are those of the fp32 map going through split_act_kernel.
__device__ __forceinline__ void corr_put(float* __restrict__ out, _Float16* __restrict__ out_hl, size_t row, int ld_out, int ch, float v) {
    if (out_hl) {
        _Float16 h, l;
        pp_split_f16_chk(v, h, l);
        _Float16* q = out_hl + row * 2 * (size_t)ld_out + pp_hl_col(ch, 0);
        q[0] = h;
        q[8] = l;
    } else {
        out[row * ld_out + ch] = v;
    }
}

// the tile's state in static LDS (1292 bytes)
struct corr_tile_t {
    float cx[CM], cy[CM];               // per pixel and level: the centre sample c ...
    int bx[CM], by[CM], state[CM];      // ... the corner of its neighbourhood, its state
    int ox, oy, todo;                   // region origin of the current pass; pixels still to do
};

// the tile of a workgroup and where its results go (uniform values): image b, whose first pixel row is row0, top-left pixel (y0, x0) of
// a map W wide; corr_row: the pixel row of tile pixel m
struct corr_dst_t {
    float* out;
    _Float16* out_hl;
    int ld_out, b, y0, x0, W;
    size_t row0;
};
__device__ __forceinline__ size_t corr_row(const corr_dst_t& d, int m) { return d.row0 + (size_t)(d.y0 + (m >> 3)) * d.W + d.x0 + (m & 7); }

// tile begin: the tile of this workgroup (workgroups are dealt round-robin to the 8 XCDs: make consecutive tiles — same image, overlapping
// regions — share an L2); thread m < 64 reads the target (gx, gy) = p + flow[p] of tile pixel m; all threads zero the pad channels
// [L win^2, ld_out) of the tile's 64 rows (the caller allocates without a fill)
__device__ __forceinline__ corr_dst_t corr_tile_begin(int B, int H, int W, const float* __restrict__ flow, int ld_flow, float* out,
                                                      _Float16* out_hl, int ld_out, int L, int r, float& gx, float& gy) {
    const int tid = threadIdx.x, win = 2 * r + 1, tiles_x = W / CT, tiles = tiles_x * (H / CT), total = tiles * B;
    int g = blockIdx.x;
    if (total % 8 == 0) g = (g % 8) * (total / 8) + g / 8;
    const int b = g / tiles, tile = g - b * tiles;
    const corr_dst_t d = {out, out_hl, ld_out, b, (tile / tiles_x) * CT, (tile % tiles_x) * CT, W, (size_t)b * H * W};
    gx = gy = 0.f;
    if (tid < CM) {
        const float* fl = flow + corr_row(d, tid) * ld_flow;
        gx = (float)(d.x0 + (tid & 7)) + fl[0];
        gy = (float)(d.y0 + (tid >> 3)) + fl[1];
    }
    for (int npad = d.ld_out - L * win * win, idx = tid; idx < CM * npad; idx += 256) {
        const int m = idx / npad, o = idx - m * npad;
        corr_put(d.out, d.out_hl, corr_row(d, m), d.ld_out, L * win * win + o, 0.f);
    }
    return d;
}

// level begin: anchors, states and the to-do count of level l (Hl x Wl), zero rows for the neighbourhoods outside the map.  ts.todo is
// first read after the second barrier here and next written between the barriers of corr_pass_retire.
__device__ __forceinline__ void corr_level_begin(corr_tile_t& ts, const corr_dst_t& d, int l, int Hl, int Wl, float gx, float gy, int r) {
    const int tid = threadIdx.x, tw = 2 * r + 2, win = 2 * r + 1;
    if (tid == 0) ts.todo = 0;
    __syncthreads();
    if (tid < CM) {
        const float sc = (float)(1 << l);
        // centre sample (offset 0): its integer corner anchors the neighbourhood (clamped far outside: no overflow)
        const float cx = fminf(fmaxf(pp_roundtrip(gx / sc, Wl), -1.0e6f), 1.0e6f);
        const float cy = fminf(fmaxf(pp_roundtrip(gy / sc, Hl), -1.0e6f), 1.0e6f);
        const int bx = (int)floorf(cx) - r, by = (int)floorf(cy) - r;
        ts.cx[tid] = cx; ts.cy[tid] = cy; ts.bx[tid] = bx; ts.by[tid] = by;
        const bool outside = bx >= Wl || by >= Hl || bx + tw <= 0 || by + tw <= 0;
        ts.state[tid] = outside ? 2 : 0;
        if (!outside) atomicAdd(&ts.todo, 1);
    }
    __syncthreads();
    for (int idx = tid; idx < CM * win * win; idx += 256) {   // neighbourhoods outside the image: zeros
        const int m = idx / (win * win), o = idx - m * (win * win);
        if (ts.state[m] == 2) corr_put(d.out, d.out_hl, corr_row(d, m), d.ld_out, l * win * win + o, 0.f);
    }
}

// region origin of a pass: the smallest bx still to do, then the smallest by among its column band (fit = region edge - (2r+2), the
// slack of a neighbourhood inside the region).  A pixel with the smallest origin is always served, so the pass loop ends.  LDS only;
// three unconditional barriers, the origin is read after the last.
__device__ __forceinline__ int2 corr_pass_origin(corr_tile_t& ts, int fit) {
    const int tid = threadIdx.x;
    if (tid == 0) { ts.ox = 0x7fffffff; ts.oy = 0x7fffffff; }
    __syncthreads();
    if (tid < CM && ts.state[tid] == 0) atomicMin(&ts.ox, ts.bx[tid]);
    __syncthreads();
    if (tid < CM && ts.state[tid] == 0 && ts.bx[tid] - ts.ox <= fit) atomicMin(&ts.oy, ts.by[tid]);
    __syncthreads();
    return make_int2(ts.ox, ts.oy);
}

// whether the pass with origin (ox, oy) serves pixel m: still to do, its neighbourhood starting (dx, dy) inside the region's slack
__device__ __forceinline__ bool corr_in_pass(const corr_tile_t& ts, int m, int fit, int ox, int oy, int& dx, int& dy) {
    dx = ts.bx[m] - ox;
    dy = ts.by[m] - oy;
    return ts.state[m] == 0 && dx >= 0 && dx <= fit && dy >= 0 && dy <= fit;
}

// blend the (2r+1)^2 samples of level l for those of the pixels m0 .. m0 + nm - 1 that the pass serves, out of S: row ms (of `pitch`
// floats) holds the correlation of pixel m0 + ms with the RW x RW region, position (y, x) in column y RW + x
template <int RW>
__device__ __forceinline__ void corr_blend(const corr_tile_t& ts, const corr_dst_t& d, const float* S, int pitch, int m0, int nm, int ox,
                                           int oy, int l, int r) {
    const int win = 2 * r + 1, fit = RW - (2 * r + 2);
    for (int idx = threadIdx.x; idx < nm * win * win; idx += 256) {
        const int ms = idx / (win * win), o = idx - ms * (win * win), ai = o / win, bi = o - ai * win, m = m0 + ms;
        int dx, dy;
        if (corr_in_pass(ts, m, fit, ox, oy, dx, dy)) {
            const float cx = ts.cx[m], cy = ts.cy[m];
            const float wx1 = cx - floorf(cx), wy1 = cy - floorf(cy), wx0 = 1.f - wx1, wy0 = 1.f - wy1;
            const float* t = S + ms * pitch + (dy + bi) * RW + dx + ai;   // x offset a-r -> +ai, y offset b-r -> +bi
            corr_put(d.out, d.out_hl, corr_row(d, m), d.ld_out, l * win * win + o,
                     t[0] * (wx0 * wy0) + t[1] * (wx1 * wy0) + t[RW] * (wx0 * wy1) + t[RW + 1] * (wx1 * wy1));
        }
    }
}

// retire the pixels the pass served: after a barrier (every blend has read the states), before a barrier (ts.todo is read next)
__device__ __forceinline__ void corr_pass_retire(corr_tile_t& ts, int fit, int ox, int oy) {
    int dx, dy;
    __syncthreads();
    if (threadIdx.x < CM && corr_in_pass(ts, threadIdx.x, fit, ox, oy, dx, dy)) {
        ts.state[threadIdx.x] = 1;
        atomicSub(&ts.todo, 1);
    }
    __syncthreads();
}

#endif
