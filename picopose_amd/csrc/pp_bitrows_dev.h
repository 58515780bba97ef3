// The PAIR x PAIR tile of popcount(row & row) over bit-packed mask rows (pp_rle_pack_bits' layout): pp_mask_intersections and segm pp_det_overlaps.
// THE BANKS: a half-wave reads one row i (four addresses: broadcasts) and eight rows j, PAIR_LD = 68 words apart: word
// 68 j + 4 m + kq lies on bank (4 j + kq) mod 32 for j < 8, kq < 4: 32 different banks.
#ifndef PP_BITROWS_DEV_H
#define PP_BITROWS_DEV_H
#include "pp_common.h"
#include "pp_reduce_dev.h"

namespace {

constexpr int PAIR = 8;                      // a workgroup owns PAIR x PAIR pairs,
constexpr int PAIR_Q = 4;                    // PAIR_Q threads per pair,
constexpr int PAIR_KW = 64;                  // PAIR_KW words of every row staged per step,
constexpr int PAIR_LD = PAIR_KW + 4;         // rows 68 words apart in LDS (THE BANKS)
constexpr int PAIR_THREADS = PAIR * PAIR * PAIR_Q;
static_assert(PAIR == PP_DET_TILE, "pp_det_overlaps' tile list steps by the tile of this walk");

// THE KERNEL of both entries.  tile.sides places the workgroup's tile: it starts at (i0, j0) of a row-major ni x nj block of pairs
// that begins at the returned offset of the output, and tile row r of side i is the bit row ri + r (j alike); tile.store(bit row i,
// bit row j, place in the output, count) is a pair's final store.  Rows past ni or nj and words past the row read as 0.  A step's
// words go to registers, then to LDS, and the next step's loads fly under this step's counting; the PAIR_Q threads of a pair take
// the words k = 4 m + kq and add up at the end (integers: any order).  EVERY thread meets the two barriers of a step: the sides are
// uniform over the workgroup, and one with empty sides still walks the words.
template <class Tile>
__global__ __launch_bounds__(PAIR_THREADS) void bitrow_tile_kernel(const unsigned* __restrict__ bits, const Tile tile) {
    const int words = tile.words;
    __shared__ unsigned a[PAIR * PAIR_LD], b[PAIR * PAIR_LD];
    const int tid = threadIdx.x, kq = tid % PAIR_Q, tj = (tid / PAIR_Q) % PAIR, ti = tid / (PAIR_Q * PAIR);
    int ri, i0, ni, rj, j0, nj, count = 0;
    const long long off = tile.sides(ri, i0, ni, rj, j0, nj);
    constexpr int PER = PAIR * PAIR_KW / PAIR_THREADS;                       // staged words of a and of b per thread and step
    unsigned ra[PER], rb[PER];
    auto fetch = [&](int k0) {
#pragma unroll
        for (int u = 0; u < PER; ++u) {
            const int e = tid + u * PAIR_THREADS, r = e / PAIR_KW, c = e % PAIR_KW;
            const bool in = k0 + c < words;
            ra[u] = in && i0 + r < ni ? bits[(size_t)(ri + r) * words + k0 + c] : 0u;
            rb[u] = in && j0 + r < nj ? bits[(size_t)(rj + r) * words + k0 + c] : 0u;
        }
    };
    fetch(0);
    for (int k0 = 0; k0 < words; k0 += PAIR_KW) {
#pragma unroll
        for (int u = 0; u < PER; ++u) {
            const int e = tid + u * PAIR_THREADS, r = e / PAIR_KW, c = e % PAIR_KW;
            a[r * PAIR_LD + c] = ra[u];
            b[r * PAIR_LD + c] = rb[u];
        }
        __syncthreads();
        if (k0 + PAIR_KW < words) fetch(k0 + PAIR_KW);
#pragma unroll
        for (int k = 0; k < PAIR_KW; k += PAIR_Q) count += __popc(a[ti * PAIR_LD + k + kq] & b[tj * PAIR_LD + k + kq]);
        __syncthreads();
    }
    count = wave_reduce_range<PAIR_Q / 2, 1>(count, op_sum{});
    if (kq == 0 && i0 + ti < ni && j0 + tj < nj) tile.store(ri + ti, rj + tj, (size_t)off + (size_t)(i0 + ti) * nj + j0 + tj, count);
}

}  // namespace
#endif
