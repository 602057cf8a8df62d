// dct-sim --cluster --rep medoid: per protein the sum of its distances to the members of its own cluster.  Entry (r, c) of an int32
// tile is the L1 of proteins i = row0 + r and j = col0 + c of ONE file; key = min(L1, cap), cap for a protein flagged empty on either
// side (a negative value counts as cap too: the rule of the kernels that scan the all-against-all's tiles).
//   label_sums_kernel -- one pass of band_walk (band_walk.hip.h: the walk, the visibility argument and the atomics a tile costs):
//                        every entry with j > i and labels[i] == labels[j] adds its key to sums[i] and to sums[j], whatever the
//                        tile's bound.  The stripes' tiles hold valid entries on both sides of the diagonal; j > i takes each
//                        unordered pair once.  After all tiles of the triangle sums[x] = the sum of key(x, y) over the other
//                        members y of x's cluster; the caller zeroes sums before the first tile and reads it after the last.
//
// The arrays.  sums sees 64-bit __hip_atomic_fetch_add alone: no load.  A sum stays below 2^64 (fewer than 2^31 members times a key
// below 2^22): the result is a sum over a set the inputs alone fix.  labels is written by an earlier launch and only read: plain
// loads, and an entry of two labels is not even loaded.
#define DCTFP_TEMPLATES_ONLY
#include "launch.h"
#include "band_walk.hip.h"

namespace {

__device__ inline void add_sum(unsigned long long* slot, uint32_t part) {
    __hip_atomic_fetch_add(slot, (unsigned long long)part, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// labels[x] of protein x: a plain load of a word an earlier launch wrote.
__device__ inline int32_t _label(const int32_t* __restrict__ labels, int64_t x) { return labels[x]; }

// A row's and a column's part = the sum of its keys in the job.  The host has checked cap <= label_sums_max_cap(): no part leaves
// 32 bits.
struct LabelSumsPass {
    using Word = uint32_t;
    using Side = int32_t;                             // the label
    static constexpr bool kBounded = false;
    static constexpr Word kIdle = 0;
    const int32_t* labels;
    unsigned long long* sums;
    __device__ static Word join(Word a, Word b) { return a + b; }
    __device__ Side side(int64_t x) const { return _label(labels, x); }
    __device__ static bool wants(Side row_label, Side col_label) { return row_label == col_label; }
    __device__ static void entry(uint32_t key, int64_t, int64_t, int, int, Side, Side, Word& row, Word& col) {
        row += key;
        col += key;
    }
    __device__ void row_out(int64_t i, int64_t, Word part) const { add_sum(sums + i, part); }
    __device__ void col_out(int64_t j, int64_t, Word part) const { add_sum(sums + j, part); }
};

__global__ __launch_bounds__(kBandThreads) void label_sums_kernel(const TriTile t, const int32_t* __restrict__ labels, unsigned long long* sums,
                                                                   int64_t n_bands, int64_t n_steps) {
    band_walk(t, n_bands, n_steps, LabelSumsPass{labels, sums});
}

}  // namespace

namespace dctfp_host {

// the largest cap whose partial sums stay in 32 bits: kBandStep keys of a row, kBandRows keys of a column
int label_sums_max_cap() { return (int)min((uint32_t)0x7fffffff, 0xffffffffu / (uint32_t)max(kBandStep, kBandRows)); }

void launch_label_sums(const TriTile& t, const int32_t* labels, uint64_t* sums, hipStream_t stream) {
    const BandGrid g = band_grid(t);
    hipLaunchKernelGGL(label_sums_kernel, dim3(g.blocks), dim3(kBandThreads), 0, stream, t, labels, reinterpret_cast<unsigned long long*>(sums),
                       g.n_bands, g.n_steps);
}

}  // namespace dctfp_host
