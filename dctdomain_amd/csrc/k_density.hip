// dct-sim --cluster --min-neighbors: density clusters (DBSCAN with the cut-off as its radius).  Entry (r, c) of an int32 tile is the
// L1 of proteins i = row0 + r and j = col0 + c of ONE file; an entry COUNTS exactly when tri_filter_count_kernel would count it:
// j > i and key = min(L1, cap) <= bound, cap for a protein flagged empty on either side (a negative value counts as cap too).  The
// counted entries are the edges of the graph; two passes over the tiles of the triangle:
//   tri_degree_kernel    -- every counted entry adds 1 to deg[i] and to deg[j].  After all tiles deg[x] = the number of edges at x;
//                           the caller zeroes deg before the first tile and derives core[x] = deg[x] >= M behind the last.
//   tri_link_core_kernel -- with core (uint8 per protein, written by an earlier launch: plain loads).  A counted entry with both ends
//                           core is a uf_union(parent, i, j), as in tri_link_kernel; one with exactly one core end lowers
//                           nearest[the other end] to the core's index (int32, 0x7fffffff = none at the start): after all tiles
//                           nearest[x] of a non-core x = its lowest core neighbour, which names the cluster a border joins.  An
//                           entry without a core end does nothing.
//
// Visibility (eight XCDs with private L2s; the header of k_cluster.hip has the argument).  Inside a launch EVERY access to parent,
// deg and nearest is an agent-scope relaxed atomic (__HIP_MEMORY_SCOPE_AGENT): deg sees __hip_atomic_fetch_add alone, nearest
// __hip_atomic_fetch_min alone, parent the loads, compare-and-swaps and minima of union_find.hip.h.  There is no plain load or store
// of any of them and nothing goes through the scalar path.  An add or a minimum is decided at the one copy the atomics of all XCDs
// reach and nobody reads deg or nearest before the launch has ended, so no ordering beyond atomicity is needed; for parent a stale
// view only shows a node as a root that no longer is one, and the CAS on it then fails (k_cluster.hip).  Addition and minimum
// commute and are associative, and a degree stays below 2^31: deg and nearest are a count and a minimum over a set the inputs
// alone fix, and the roots of the forest are the smallest members of their components.  None of them depends on the order in which
// workgroups ran, on how the caller cut the triangle into tiles or on the order of its calls.  The tile, the flags and core are
// written by earlier launches and only read here: plain loads.  No wave waits for another workgroup: no flags, no tickets, no spin
// loops (a failed CAS means another wave succeeded).
//
// Atomics per tile.  label_sums_kernel's walk (k_medoid.hip): a workgroup takes a band of kDenBand rows x kDenStep (1024) columns.
// Thread t reads columns v0 + t + 256 e, e = 0 .. 3, of every row of the band with plain dword loads -- coalesced, and free of any
// alignment rule: any ld, any column view of a wider tensor.  Row side: a row's count (its minimum) is reduced in the wave
// (shuffles), each wave stores its part in a slot of its own in LDS and the four are combined after the band; one global atomic per
// (row, step) at most.  Column side: column v0 + t + 256 e belongs to thread t alone for the whole band, so its count (its minimum)
// over the band's rows stays in a register of that thread; one global atomic per (column, band) at most.  Neither side needs an LDS
// atomic, and a count of zero or a minimum of "none" is not sent.  So a tile of R x C entries costs at most
// R ceil(C / 1024) + C ceil(R / 64) global atomics on deg or nearest -- under 2 % of its entries -- and the link pass one union per
// core-core edge beside them; a job wholly on or left of the diagonal is skipped before it loads anything.
#define DCTFP_TEMPLATES_ONLY
#include "launch.h"
#include "union_find.hip.h"   // the forest: uf_union

namespace {

constexpr int kDenThreads = 256;
constexpr int kDenWaves = kDenThreads / 64;
constexpr int kDenPer = 4;                        // columns of a thread per step
constexpr int kDenStep = kDenThreads * kDenPer;   // columns per step: a row's partial count is at most kDenStep
constexpr int kDenBand = 64;                      // rows of a workgroup's band: a column's partial count is at most kDenBand
constexpr int32_t kNoCore = 0x7fffffff;           // nearest: no core neighbour (yet)

struct DenTile {
    const int32_t* tile;
    int64_t n_rows, n_cols, ld, row0, col0;
    const uint8_t* row_empty;
    const uint8_t* col_empty;
    int32_t cap, bound;
};

__device__ inline void add_degree(uint32_t* slot, uint32_t part) {
    __hip_atomic_fetch_add(slot, part, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ inline void lower_nearest(int32_t* slot, int32_t core_index) {
    __hip_atomic_fetch_min(slot, core_index, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// core[x] of protein x: a plain load of a byte an earlier launch wrote.  Taken once per job for each of its columns and rows --
// the column's flag sits in a register for the whole job, the row's is the same for the whole wave -- never per entry.
__device__ inline bool _is_core(const uint8_t* __restrict__ core, int64_t x) { return core[x] != 0; }

// Does the entry with value x count?  key = min(L1, cap), cap for a flagged row or column and for a negative value; key <= bound.
__device__ inline bool counts(uint32_t x, bool flagged, uint32_t cap, int32_t bound) {
    const uint32_t key = flagged || x >= cap ? cap : x;
    return (int32_t)key <= bound;
}

// One workgroup per (band of kDenBand rows, step of kDenStep columns) at a time.  s_row[rl][w] = the count of wave w over row rl of
// the band, col_deg[e] = the count of this thread's column e over the band.  The host has checked row0 + n_rows <= n_nodes and
// col0 + n_cols <= n_nodes (the length of deg).
__global__ __launch_bounds__(kDenThreads) void tri_degree_kernel(const DenTile t, uint32_t* deg, int64_t n_bands, int64_t n_steps) {
    __shared__ uint32_t s_row[kDenBand][kDenWaves];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int32_t* __restrict__ tile = t.tile;
    const uint8_t* __restrict__ row_empty = t.row_empty;
    const uint8_t* __restrict__ col_empty = t.col_empty;
    const uint32_t cap = (uint32_t)t.cap;
    const int32_t bound = t.bound;
    for (int64_t job = blockIdx.x; job < n_bands * n_steps; job += gridDim.x) {
        const int64_t r_lo = job / n_steps * kDenBand, v0 = job % n_steps * kDenStep;
        const int rows = (int)min((int64_t)kDenBand, t.n_rows - r_lo);
        const int64_t i_lo = t.row0 + r_lo, j_lo = t.col0 + v0;
        if (j_lo + min((int64_t)kDenStep, t.n_cols - v0) - 1 <= i_lo) continue;      // (no entry of the job has j > i)
        bool inside[kDenPer], full[kDenPer];                      // this thread's columns: in the tile, flagged empty
        uint32_t col_deg[kDenPer];
#pragma unroll
        for (int e = 0; e < kDenPer; ++e) {
            const int64_t c = v0 + tid + kDenThreads * e;
            inside[e] = c < t.n_cols;
            full[e] = inside[e] && col_empty && col_empty[c];
            col_deg[e] = 0;
        }
        __syncthreads();                                            // (the previous job's flush has read s_row)
        s_row[tid >> 2][tid & 3] = 0;                               // (kDenBand x kDenWaves = kDenThreads words)
        __syncthreads();
        for (int rl = 0; rl < rows; ++rl) {
            const int64_t i = i_lo + rl;
            const int32_t* __restrict__ row = tile + (r_lo + rl) * t.ld + v0 + tid;
            const bool row_full = row_empty && row_empty[r_lo + rl];
            uint32_t mine = 0;
#pragma unroll
            for (int e = 0; e < kDenPer; ++e) {
                if (!inside[e] || j_lo + tid + kDenThreads * e <= i) continue;
                if (!counts((uint32_t)row[kDenThreads * e], row_full || full[e], cap, bound)) continue;
                mine += 1;
                col_deg[e] += 1;
            }
            if (__ballot(mine != 0) == 0) continue;                 // (the wave adds nothing to this row)
#pragma unroll
            for (int d = 32; d > 0; d >>= 1) mine += (uint32_t)__shfl_xor((int)mine, d);
            if (lane == 0) s_row[rl][wave] = mine;
        }
        __syncthreads();
        if (tid < rows) {
            uint32_t part = 0;
#pragma unroll
            for (int w = 0; w < kDenWaves; ++w) part += s_row[tid][w];
            if (part != 0) add_degree(deg + i_lo + tid, part);
        }
#pragma unroll
        for (int e = 0; e < kDenPer; ++e)
            if (col_deg[e] != 0) add_degree(deg + j_lo + tid + kDenThreads * e, col_deg[e]);
    }
}

// The same walk with core beside the tile.  s_row[rl][w] = the lowest core column wave w met in the non-core row rl of the band,
// col_near[e] = the lowest core row this thread's non-core column e met in the band (rows ascend, minima all the same); a core-core
// entry is hooked where it is met, by the lane that met it, as in tri_link_kernel.  The host has checked row0 + n_rows <= n_nodes
// and col0 + n_cols <= n_nodes (the length of core, parent and nearest).
__global__ __launch_bounds__(kDenThreads) void tri_link_core_kernel(const DenTile t, const uint8_t* __restrict__ core, int32_t* parent,
                                                                     int32_t* nearest, int64_t n_bands, int64_t n_steps) {
    __shared__ int32_t s_row[kDenBand][kDenWaves];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int32_t* __restrict__ tile = t.tile;
    const uint8_t* __restrict__ row_empty = t.row_empty;
    const uint8_t* __restrict__ col_empty = t.col_empty;
    const uint32_t cap = (uint32_t)t.cap;
    const int32_t bound = t.bound;
    for (int64_t job = blockIdx.x; job < n_bands * n_steps; job += gridDim.x) {
        const int64_t r_lo = job / n_steps * kDenBand, v0 = job % n_steps * kDenStep;
        const int rows = (int)min((int64_t)kDenBand, t.n_rows - r_lo);
        const int64_t i_lo = t.row0 + r_lo, j_lo = t.col0 + v0;
        if (j_lo + min((int64_t)kDenStep, t.n_cols - v0) - 1 <= i_lo) continue;      // (no entry of the job has j > i)
        bool inside[kDenPer], full[kDenPer], col_core[kDenPer];   // this thread's columns: in the tile, flagged empty, core
        int32_t col_near[kDenPer];
#pragma unroll
        for (int e = 0; e < kDenPer; ++e) {
            const int64_t c = v0 + tid + kDenThreads * e;
            inside[e] = c < t.n_cols;
            full[e] = inside[e] && col_empty && col_empty[c];
            col_core[e] = inside[e] && _is_core(core, t.col0 + c);
            col_near[e] = kNoCore;
        }
        __syncthreads();                                            // (the previous job's flush has read s_row)
        s_row[tid >> 2][tid & 3] = kNoCore;                         // (kDenBand x kDenWaves = kDenThreads words)
        __syncthreads();
        for (int rl = 0; rl < rows; ++rl) {
            const int64_t i = i_lo + rl;
            const int32_t* __restrict__ row = tile + (r_lo + rl) * t.ld + v0 + tid;
            const bool row_full = row_empty && row_empty[r_lo + rl];
            const bool row_core = _is_core(core, i);                // (the same for the whole workgroup)
            int32_t mine = kNoCore;
#pragma unroll
            for (int e = 0; e < kDenPer; ++e) {
                const int64_t j = j_lo + tid + kDenThreads * e;
                if (!inside[e] || j <= i || (!row_core && !col_core[e])) continue;   // (no core end: nothing to do, nothing to load)
                if (!counts((uint32_t)row[kDenThreads * e], row_full || full[e], cap, bound)) continue;
                if (row_core && col_core[e])
                    uf_union(parent, (int32_t)i, (int32_t)j);
                else if (row_core)
                    col_near[e] = min(col_near[e], (int32_t)i);
                else
                    mine = min(mine, (int32_t)j);
            }
            if (row_core || __ballot(mine != kNoCore) == 0) continue;   // (a core row has no nearest; the wave met no core column)
#pragma unroll
            for (int d = 32; d > 0; d >>= 1) mine = min(mine, __shfl_xor(mine, d));
            if (lane == 0) s_row[rl][wave] = mine;
        }
        __syncthreads();
        if (tid < rows) {
            int32_t part = kNoCore;
#pragma unroll
            for (int w = 0; w < kDenWaves; ++w) part = min(part, s_row[tid][w]);
            if (part != kNoCore) lower_nearest(nearest + i_lo + tid, part);
        }
#pragma unroll
        for (int e = 0; e < kDenPer; ++e)
            if (col_near[e] != kNoCore) lower_nearest(nearest + j_lo + tid + kDenThreads * e, col_near[e]);
    }
}

static_assert(kDenBand * kDenWaves == kDenThreads, "one thread clears one word of s_row");

unsigned density_grid(int64_t n_bands, int64_t n_steps) { return (unsigned)min(n_bands * n_steps, (int64_t)1 << 20); }

}  // namespace

namespace dctfp_host {

void launch_tri_degree(const int32_t* tile, int64_t n_rows, int64_t n_cols, int64_t ld, int64_t row0, int64_t col0, const uint8_t* row_empty,
                       const uint8_t* col_empty, int32_t cap, int32_t bound, uint32_t* deg, hipStream_t stream) {
    const DenTile t{tile, n_rows, n_cols, ld, row0, col0, row_empty, col_empty, cap, bound};
    const int64_t n_bands = (n_rows + kDenBand - 1) / kDenBand, n_steps = (n_cols + kDenStep - 1) / kDenStep;
    hipLaunchKernelGGL(tri_degree_kernel, dim3(density_grid(n_bands, n_steps)), dim3(kDenThreads), 0, stream, t, deg, n_bands, n_steps);
}

void launch_tri_link_core(const int32_t* tile, int64_t n_rows, int64_t n_cols, int64_t ld, int64_t row0, int64_t col0, const uint8_t* row_empty,
                          const uint8_t* col_empty, int32_t cap, int32_t bound, const uint8_t* core, int32_t* parent, int32_t* nearest,
                          hipStream_t stream) {
    const DenTile t{tile, n_rows, n_cols, ld, row0, col0, row_empty, col_empty, cap, bound};
    const int64_t n_bands = (n_rows + kDenBand - 1) / kDenBand, n_steps = (n_cols + kDenStep - 1) / kDenStep;
    hipLaunchKernelGGL(tri_link_core_kernel, dim3(density_grid(n_bands, n_steps)), dim3(kDenThreads), 0, stream, t, core, parent, nearest,
                       n_bands, n_steps);
}

}  // namespace dctfp_host
