// dct-sim --cluster --min-neighbors: density clusters (DBSCAN with the cut-off as its radius).  Entry (r, c) of an int32 tile is the
// L1 of proteins i = row0 + r and j = col0 + c of ONE file; an entry COUNTS exactly when tri_filter_count_kernel would count it:
// j > i and key = min(L1, cap) <= bound, cap for a protein flagged empty on either side (a negative value counts as cap too).  The
// counted entries are the edges of the graph; two passes of band_walk (band_walk.hip.h: the walk, the visibility argument and the
// atomics a tile costs) over the tiles of the triangle:
//   tri_degree_kernel    -- every counted entry adds 1 to deg[i] and to deg[j].  After all tiles deg[x] = the number of edges at x;
//                           the caller zeroes deg before the first tile and derives core[x] = deg[x] >= M behind the last.
//   tri_link_core_kernel -- with core (uint8 per protein, written by an earlier launch: plain loads).  A counted entry with both ends
//                           core is a uf_union(parent, i, j), as in tri_link_kernel; one with exactly one core end lowers
//                           nearest[the other end] to the core's index (int32, 0x7fffffff = none at the start): after all tiles
//                           nearest[x] of a non-core x = its lowest core neighbour, which names the cluster a border joins.  An
//                           entry without a core end does nothing and is not loaded.
//
// The arrays.  deg sees __hip_atomic_fetch_add alone, nearest __hip_atomic_fetch_min alone, parent the loads, compare-and-swaps
// and minima of union_find.hip.h; the link pass costs one union per core-core edge beside the walk's atomics.  For parent a stale
// view only shows a node as a root that no longer is one, and the CAS on it then fails (k_cluster.hip; a failed CAS means another
// wave succeeded).  A degree stays below 2^31; deg and nearest are a count and a minimum over a set the inputs alone fix, and the
// roots of the forest are the smallest members of their components.
#define DCTFP_TEMPLATES_ONLY
#include "launch.h"
#include "band_walk.hip.h"
#include "union_find.hip.h"   // the forest: uf_union

namespace {

constexpr int32_t kNoCore = 0x7fffffff;           // nearest: no core neighbour (yet)

__device__ inline void add_degree(uint32_t* slot, uint32_t part) {
    __hip_atomic_fetch_add(slot, part, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ inline void lower_nearest(int32_t* slot, int32_t core_index) {
    __hip_atomic_fetch_min(slot, core_index, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// core[x] of protein x: a plain load of a byte an earlier launch wrote.
__device__ inline bool _is_core(const uint8_t* __restrict__ core, int64_t x) { return core[x] != 0; }

// A row's and a column's part = its count of counted entries in the job (at most kBandStep, at most kBandRows).
struct DegreePass {
    using Word = uint32_t;
    using Side = NoSide;
    static constexpr bool kBounded = true;
    static constexpr Word kIdle = 0;
    uint32_t* deg;
    __device__ static Word join(Word a, Word b) { return a + b; }
    __device__ static Side side(int64_t) { return {}; }
    __device__ static bool wants(Side, Side) { return true; }
    __device__ static void entry(uint32_t, int64_t, int64_t, int, int, Side, Side, Word& row, Word& col) {
        row += 1;
        col += 1;
    }
    __device__ void row_out(int64_t i, int64_t, Word part) const { add_degree(deg + i, part); }
    __device__ void col_out(int64_t j, int64_t, Word part) const { add_degree(deg + j, part); }
};

// A non-core row's part = the lowest core column met, a non-core column's the lowest core row (rows ascend, minima all the same);
// a core-core entry is hooked where it is met, by the lane that met it, as in tri_link_kernel.  A core row's part stays idle.
struct LinkCorePass {
    using Word = int32_t;
    using Side = bool;                                // core?
    static constexpr bool kBounded = true;
    static constexpr Word kIdle = kNoCore;
    const uint8_t* core;
    int32_t* parent;
    int32_t* nearest;
    __device__ static Word join(Word a, Word b) { return min(a, b); }
    __device__ Side side(int64_t x) const { return _is_core(core, x); }
    __device__ static bool wants(Side row_core, Side col_core) { return row_core || col_core; }   // (no core end: nothing to do)
    __device__ void entry(uint32_t, int64_t i, int64_t j, int, int, Side row_core, Side col_core, Word& row, Word& col) const {
        if (row_core && col_core)
            uf_union(parent, (int32_t)i, (int32_t)j);
        else if (row_core)
            col = min(col, (int32_t)i);
        else
            row = min(row, (int32_t)j);
    }
    __device__ void row_out(int64_t i, int64_t, Word part) const { lower_nearest(nearest + i, part); }
    __device__ void col_out(int64_t j, int64_t, Word part) const { lower_nearest(nearest + j, part); }
};

__global__ __launch_bounds__(kBandThreads) void tri_degree_kernel(const TriTile t, uint32_t* deg, int64_t n_bands, int64_t n_steps) {
    band_walk(t, n_bands, n_steps, DegreePass{deg});
}

__global__ __launch_bounds__(kBandThreads) void tri_link_core_kernel(const TriTile t, const uint8_t* __restrict__ core, int32_t* parent,
                                                                      int32_t* nearest, int64_t n_bands, int64_t n_steps) {
    band_walk(t, n_bands, n_steps, LinkCorePass{core, parent, nearest});
}

}  // namespace

namespace dctfp_host {

void launch_tri_degree(const TriTile& t, uint32_t* deg, hipStream_t stream) {
    const BandGrid g = band_grid(t);
    hipLaunchKernelGGL(tri_degree_kernel, dim3(g.blocks), dim3(kBandThreads), 0, stream, t, deg, g.n_bands, g.n_steps);
}

void launch_tri_link_core(const TriTile& t, const uint8_t* core, int32_t* parent, int32_t* nearest, hipStream_t stream) {
    const BandGrid g = band_grid(t);
    hipLaunchKernelGGL(tri_link_core_kernel, dim3(g.blocks), dim3(kBandThreads), 0, stream, t, core, parent, nearest, g.n_bands, g.n_steps);
}

}  // namespace dctfp_host
