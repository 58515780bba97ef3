// The wave and workgroup reductions of every kernel (device code, internal linkage: every translation unit gets its own copy).
//
// THE ORDER, written once: within a wave v = op(v, v of lane ^ o) at o = 32, 16, 8, 4, 2, 1, the lane's own value on the left;
// then the waves w = 0, 1, ... in ascending order, the running value on the left.  Every bit-equality the kernels promise (batch
// item against lone item, deterministic adjoints, the tie rules) rests on all sites walking this one tree.
//
//   lane_xor<WIDTH>          the value of lane ^ o: a scalar (float, double, int, unsigned, unsigned long long) in one shuffle, a
//                            record of two or three 32-bit words word by word
//   wave_reduce_range<HI,LO> offsets HI, HI / 2, ..., LO; the result is in every lane of each aligned group of 2 HI lanes
//   wave_reduce              offsets 32 .. 1: the result is in every lane
//   wave_sum/_max/_min       wave_reduce under op_sum, op_max, op_min
//   wave_reduce_each         wave_reduce of N values side by side, offset by offset
//   block_reduce_all         the walk 32 .. 1, lane 0 of each wave writes red, ONE barrier, the waves folded in order by every thread:
//                            the result is in every thread.  With a seed the fold is op(seed, wave 0), ...: a sum that used to
//                            begin at 0.0 keeps its bits (0.0 + -0.0 is +0.0)
//   block_reduce_to          the same up to the barrier; thread c < N folds value c and returns it, every other thread returns T()
//   winner                   arg-max of cnt[0..n) with the lowest index among equals, over the workgroup, in every thread
//
// red is the caller's LDS, a T[NWAVES][N] or a pointer to NWAVES * N values laid out the same way, and holds the waves' values
// afterwards.  A caller that uses red again puts its own barrier in between: the helpers hold exactly the one between the write and the fold.  Over an array the
// operation may take the position, op(c, a, b); a predicate (a tie rule, a guard) stays at the site and is passed in.
#ifndef PP_REDUCE_DEV_H
#define PP_REDUCE_DEV_H
#include <hip/hip_runtime.h>

#include <type_traits>

namespace {

struct op_sum {
    template <class T>
    __device__ __forceinline__ T operator()(T a, T b) const { return a + b; }
};
struct op_max {
    __device__ __forceinline__ float operator()(float a, float b) const { return fmaxf(a, b); }
    __device__ __forceinline__ double operator()(double a, double b) const { return fmax(a, b); }
    template <class T>
    __device__ __forceinline__ T operator()(T a, T b) const { return b > a ? b : a; }
};
struct op_min {
    __device__ __forceinline__ float operator()(float a, float b) const { return fminf(a, b); }
    __device__ __forceinline__ double operator()(double a, double b) const { return fmin(a, b); }
    template <class T>
    __device__ __forceinline__ T operator()(T a, T b) const { return b < a ? b : a; }
};

template <int WIDTH = 64, class T>
__device__ __forceinline__ T lane_xor(const T& v, int o) {
    if constexpr (std::is_arithmetic_v<T>) {
        return __shfl_xor(v, o, WIDTH);
    } else if constexpr (sizeof(T) == 8) {       // (an aggregate of two or of three 32-bit members: each goes as its own type)
        const auto& [a, b] = v;
        return T{__shfl_xor(a, o, WIDTH), __shfl_xor(b, o, WIDTH)};
    } else {
        const auto& [a, b, c] = v;
        return T{__shfl_xor(a, o, WIDTH), __shfl_xor(b, o, WIDTH), __shfl_xor(c, o, WIDTH)};
    }
}

// THE WALK: o = HI, HI / 2, ..., LO, unrolled.  The one spelling of the order; the three loops below are it.  (The workgroup form
// holds the loop itself and does not call wave_reduce: the compiler simplifies a helper on its own before it inlines it, and a
// loop that was written out inside its kernel then compiles to other registers - profiles/r21/reductions.md.)
#define PP_WAVE_WALK(o, HI, LO) _Pragma("unroll") for (int o = (HI); o >= (LO); o >>= 1)

// op(a, b), or op(c, a, b) where the operation depends on the position in the array
template <class T, class Op>
__device__ __forceinline__ T reduce_apply(Op op, int c, const T& a, const T& b) {
    if constexpr (std::is_invocable_v<Op, int, T, T>) return op(c, a, b);
    else return op(a, b);
}

// (c: the position of v in the caller's array, for an operation that depends on it)
template <int HI, int LO = 1, int WIDTH = 64, class T, class Op>
__device__ __forceinline__ T wave_reduce_range(T v, Op op, int c = 0) {
    static_assert(HI >= LO && LO >= 1 && HI < WIDTH && (HI & (HI - 1)) == 0 && (LO & (LO - 1)) == 0, "powers of two inside the width");
    PP_WAVE_WALK(o, HI, LO) v = reduce_apply(op, c, v, lane_xor<WIDTH>(v, o));
    return v;
}

template <class T, class Op>
__device__ __forceinline__ T wave_reduce(T v, Op op, int c = 0) {
    return wave_reduce_range<32, 1>(v, op, c);
}
// N values side by side, op(c, a, b) or op(a, b): every offset visits the whole array before the next one (the bits are those of
// N calls of wave_reduce; the instructions interleave as the kernels that reduce a box or a record at once were written)
template <int N, class T, class Op>
__device__ __forceinline__ void wave_reduce_each(T (&v)[N], Op op) {
    PP_WAVE_WALK(o, 32, 1) {
#pragma unroll
        for (int c = 0; c < N; ++c) v[c] = reduce_apply(op, c, v[c], lane_xor(v[c], o));
    }
}
template <class T>
__device__ __forceinline__ T wave_sum(T v) { return wave_reduce(v, op_sum{}); }
template <class T>
__device__ __forceinline__ T wave_max(T v) { return wave_reduce(v, op_max{}); }
template <class T>
__device__ __forceinline__ T wave_min(T v) { return wave_reduce(v, op_min{}); }

// value c of wave w in the caller's LDS, which is a T[NWAVES][N] or a flat T*
template <int N, class T>
__device__ __forceinline__ T& red_at(T (*red)[N], int w, int c) { return red[w][c]; }
template <int N, class T>
__device__ __forceinline__ T& red_at(T* red, int w, int c) { return red[w * N + c]; }

// the part both workgroup forms share: each value through the wave form, lane 0 of each wave writes red[wave][c], the barrier
template <int N, class T, class Red, class Op>
__device__ __forceinline__ void block_reduce_stage(const T (&v)[N], Red red, Op op) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int c = 0; c < N; ++c) {
        T a = v[c];
        PP_WAVE_WALK(o, 32, 1) a = reduce_apply(op, c, a, lane_xor(a, o));
        if (lane == 0) red_at<N>(red, wave, c) = a;
    }
    __syncthreads();
}

template <int NWAVES, int N, class T, class Red, class Op>
__device__ __forceinline__ void block_reduce_all(T (&v)[N], Red red, Op op) {
    block_reduce_stage(v, red, op);
#pragma unroll
    for (int c = 0; c < N; ++c) {
        T a = red_at<N>(red, 0, c);
#pragma unroll
        for (int w = 1; w < NWAVES; ++w) a = reduce_apply(op, c, a, red_at<N>(red, w, c));
        v[c] = a;
    }
}

template <int NWAVES, int N, class T, class Red, class Op>
__device__ __forceinline__ void block_reduce_all(T (&v)[N], Red red, Op op, T seed) {
    block_reduce_stage(v, red, op);
#pragma unroll
    for (int c = 0; c < N; ++c) {
        T a = seed;
#pragma unroll
        for (int w = 0; w < NWAVES; ++w) a = reduce_apply(op, c, a, red_at<N>(red, w, c));
        v[c] = a;
    }
}

template <int NWAVES, class T, class Op>
__device__ __forceinline__ T block_reduce_all(T v, T* red, Op op) {
    T a[1] = {v};
    block_reduce_all<NWAVES>(a, red, op);
    return a[0];
}

template <int NWAVES, int N, class T, class Red, class Op>
__device__ __forceinline__ T block_reduce_to(const T (&v)[N], Red red, Op op) {
    block_reduce_stage(v, red, op);
    if ((int)threadIdx.x >= N) return T();
    const int c = threadIdx.x;
    T a = red_at<N>(red, 0, c);
#pragma unroll
    for (int w = 1; w < NWAVES; ++w) a = reduce_apply(op, c, a, red_at<N>(red, w, c));
    return a;
}

template <int NWAVES, class T, class Op>
__device__ __forceinline__ T block_reduce_to(T v, T* red, Op op) {
    const T a[1] = {v};
    return block_reduce_to<NWAVES>(a, red, op);
}

// a consensus count and its hypothesis: the greater count wins, then the lower index (a total order: no two lanes hold one index)
struct Winner {
    int c, h;
};
__device__ __forceinline__ Winner better_winner(Winner a, const Winner& b) {
    if (b.c > a.c || (b.c == a.c && b.h < a.h)) a = b;
    return a;
}

// -> in every thread of the NWAVES-wave workgroup the winner of cnt[0..n); with n == 0 it is (-1, empty_h): the callers differ in
// the index they report for an empty list.  red: NWAVES records of LDS, unused (nullptr) with one wave.
template <int NWAVES>
__device__ __forceinline__ Winner winner(const int* cnt, int n, Winner* red, int empty_h) {
    Winner b{-1, empty_h};
    for (int h = threadIdx.x; h < n; h += NWAVES * 64)
        if (cnt[h] > b.c) b = Winner{cnt[h], h};
    if constexpr (NWAVES > 1) return block_reduce_all<NWAVES>(b, red, better_winner);
    else return wave_reduce(b, better_winner);
}

}  // namespace
#endif
