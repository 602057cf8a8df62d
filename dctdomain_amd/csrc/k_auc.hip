// dct-sim --auc1: per query the true positives ranked before its first false positive (AUC1, and with it the top-1 rates).  Entry
// (r, c) of an int32 tile is the L1 of proteins i = row0 + r and j = col0 + c of ONE file; an entry COUNTS exactly when
// tri_filter_count_kernel would count it: j > i and key = min(L1, cap) <= bound, cap for a protein flagged empty on either side (a
// negative value counts as cap too).  A counted entry makes j a hit of i and i a hit of j; fam (int32 per protein) names every
// protein's family, and the hits of x are ranked by the word key << 32 | index of the hit -- unsigned 64-bit order = (key, index),
// ties to the lower protein.  Two passes of band_walk (band_walk.hip.h: the walk, the visibility argument and the atomics a tile
// costs) over the tiles of the triangle:
//   tri_first_fp_kernel  -- a counted entry with fam[i] != fam[j] lowers first[i] to key << 32 | j and first[j] to key << 32 | i.
//                           After all tiles first[x] = the best-ranked hit of x from another family, its first false positive;
//                           all ones = none, which the caller fills in before the first tile.
//   tri_tp_before_kernel -- with the finished first.  A counted entry with fam[i] == fam[j] adds 1 to tp[i] when
//                           key << 32 | j < first[i] and, decided on its own, 1 to tp[j] when key << 32 | i < first[j].  After
//                           all tiles tp[x] = the hits of x's own family ranked before its first false positive; the caller
//                           zeroes tp before the first tile.
//
// The arrays.  first in pass 1 sees lower_hit alone (band_walk.hip.h: the load that skips a minimum which would change nothing,
// then __hip_atomic_fetch_min), tp in pass 2 __hip_atomic_fetch_add alone; a count stays below 2^31.  first and tp are a minimum
// and a count over sets the inputs alone fix.  fam and -- in pass 2 -- first are written by earlier launches and only read: plain
// loads.  An entry of the wrong kind for the pass (one family in pass 1, two in pass 2) is not even loaded.
#define DCTFP_TEMPLATES_ONLY
#include "launch.h"
#include "band_walk.hip.h"

namespace {

__device__ inline void add_count(uint32_t* slot, uint32_t part) {
    __hip_atomic_fetch_add(slot, part, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// fam[x] of protein x: a plain load of a word an earlier launch wrote.
__device__ inline int32_t _family(const int32_t* __restrict__ fam, int64_t x) { return fam[x]; }

// first[x] of protein x in pass 2: a plain load of a word pass 1 -- an earlier launch -- left.
__device__ inline unsigned long long _first_of(const unsigned long long* __restrict__ first, int64_t x) { return first[x]; }

// A row's part = its minimum over the step as key << 10 | column within the step, a column's = its minimum over the band as
// key << 6 | row within the band -- both orders are (key, index) restricted to one row / one column.  The host has checked
// cap <= rect_best_max_cap(): no packed word of a hit is all ones.
struct FirstFpPass {
    using Word = uint32_t;
    using Side = int32_t;                             // the family
    static constexpr bool kBounded = true;
    static constexpr Word kIdle = kNone32;
    const int32_t* fam;
    unsigned long long* first;
    __device__ static Word join(Word a, Word b) { return min(a, b); }
    __device__ Side side(int64_t x) const { return _family(fam, x); }
    __device__ static bool wants(Side row_fam, Side col_fam) { return row_fam != col_fam; }   // (one family: nothing to do)
    __device__ static void entry(uint32_t key, int64_t, int64_t, int rl, int cl, Side, Side, Word& row, Word& col) {
        row = min(row, key << 10 | (uint32_t)cl);
        col = min(col, key << 6 | (uint32_t)rl);
    }
    __device__ void row_out(int64_t i, int64_t j_lo, Word part) const { lower_hit(first + i, part >> 10, j_lo + (part & (kBandStep - 1))); }
    __device__ void col_out(int64_t j, int64_t i_lo, Word part) const { lower_hit(first + j, part >> 6, i_lo + (part & (kBandRows - 1))); }
};

// With the finished first beside fam.  A row's and a column's part = its count; the two ends of an entry are decided separately,
// each against its own first.
struct TpBeforePass {
    using Word = uint32_t;
    struct Side {
        int32_t fam;
        unsigned long long first;
    };
    static constexpr bool kBounded = true;
    static constexpr Word kIdle = 0;
    const int32_t* fam;
    const unsigned long long* first;
    uint32_t* tp;
    __device__ static Word join(Word a, Word b) { return a + b; }
    __device__ Side side(int64_t x) const { return {_family(fam, x), _first_of(first, x)}; }
    __device__ static bool wants(const Side& row, const Side& col) { return row.fam == col.fam; }   // (two families: nothing to do)
    __device__ static void entry(uint32_t key, int64_t i, int64_t j, int, int, const Side& row_side, const Side& col_side, Word& row, Word& col) {
        if (hit_word(key, j) < row_side.first) row += 1;
        if (hit_word(key, i) < col_side.first) col += 1;
    }
    __device__ void row_out(int64_t i, int64_t, Word part) const { add_count(tp + i, part); }
    __device__ void col_out(int64_t j, int64_t, Word part) const { add_count(tp + j, part); }
};

__global__ __launch_bounds__(kBandThreads) void tri_first_fp_kernel(const TriTile t, const int32_t* __restrict__ fam, unsigned long long* first,
                                                                     int64_t n_bands, int64_t n_steps) {
    band_walk(t, n_bands, n_steps, FirstFpPass{fam, first});
}

__global__ __launch_bounds__(kBandThreads) void tri_tp_before_kernel(const TriTile t, const int32_t* __restrict__ fam,
                                                                      const unsigned long long* __restrict__ first, uint32_t* tp, int64_t n_bands,
                                                                      int64_t n_steps) {
    band_walk(t, n_bands, n_steps, TpBeforePass{fam, first, tp});
}

}  // namespace

namespace dctfp_host {

void launch_tri_first_fp(const TriTile& t, const int32_t* fam, uint64_t* first, hipStream_t stream) {
    const BandGrid g = band_grid(t);
    hipLaunchKernelGGL(tri_first_fp_kernel, dim3(g.blocks), dim3(kBandThreads), 0, stream, t, fam, reinterpret_cast<unsigned long long*>(first),
                       g.n_bands, g.n_steps);
}

void launch_tri_tp_before(const TriTile& t, const int32_t* fam, const uint64_t* first, uint32_t* tp, hipStream_t stream) {
    const BandGrid g = band_grid(t);
    hipLaunchKernelGGL(tri_tp_before_kernel, dim3(g.blocks), dim3(kBandThreads), 0, stream, t, fam,
                       reinterpret_cast<const unsigned long long*>(first), tp, g.n_bands, g.n_steps);
}

}  // namespace dctfp_host
