// dct-sim --auc1: per query the true positives ranked before its first false positive (AUC1, and with it the top-1 rates).  Entry
// (r, c) of an int32 tile is the L1 of proteins i = row0 + r and j = col0 + c of ONE file; an entry COUNTS exactly when
// tri_filter_count_kernel would count it: j > i and key = min(L1, cap) <= bound, cap for a protein flagged empty on either side (a
// negative value counts as cap too).  A counted entry makes j a hit of i and i a hit of j; fam (int32 per protein) names every
// protein's family, and the hits of x are ranked by the word key << 32 | index of the hit -- unsigned 64-bit order = (key, index),
// ties to the lower protein.  Two passes over the tiles of the triangle:
//   tri_first_fp_kernel  -- a counted entry with fam[i] != fam[j] lowers first[i] to key << 32 | j and first[j] to key << 32 | i.
//                           After all tiles first[x] = the best-ranked hit of x from another family, its first false positive;
//                           all ones = none, which the caller fills in before the first tile.
//   tri_tp_before_kernel -- with the finished first.  A counted entry with fam[i] == fam[j] adds 1 to tp[i] when
//                           key << 32 | j < first[i] and, decided on its own, 1 to tp[j] when key << 32 | i < first[j].  After
//                           all tiles tp[x] = the hits of x's own family ranked before its first false positive; the caller
//                           zeroes tp before the first tile.
//
// Visibility (eight XCDs with private L2s; the header of k_cluster.hip has the argument).  Inside a launch first in pass 1 and tp
// in pass 2 are touched by agent-scope relaxed atomics alone (__HIP_MEMORY_SCOPE_AGENT): first sees the load that skips a minimum
// which would change nothing and then __hip_atomic_fetch_min (lower_hit of k_best.hip: an entry only ever decreases, so a stale
// value read by that load costs one redundant atomic and never a wrong result), tp sees __hip_atomic_fetch_add alone.  There is no
// plain load or store of the array a pass writes and nothing goes through the scalar path.  A minimum or an add is decided at the
// one copy the atomics of all XCDs reach and nobody reads the result before the launch has ended, so no ordering beyond atomicity
// is needed.  Minimum and addition commute and are associative, and a count stays below 2^31: first and tp are a minimum and a
// count over sets the inputs alone fix.  Neither depends on the order in which workgroups ran, on how the caller cut the triangle
// into tiles or on the order of its calls.  The tile, the flags, fam and -- in pass 2 -- first are written by earlier launches and
// only read here: plain loads.  No workgroup waits for another: no flags, no tickets, no spin loops.
//
// Atomics per tile.  tri_degree_kernel's walk (k_density.hip): a workgroup takes a band of kAucBand rows x kAucStep (1024)
// columns.  Thread t reads columns v0 + t + 256 e, e = 0 .. 3, of every row of the band with plain dword loads -- coalesced, and
// free of any alignment rule: any ld, any column view of a wider tensor.  Row side: a row's minimum, packed key << 10 | column
// within the step as in rect_best_kernel (its count in pass 2), is reduced in the wave (shuffles), each wave stores its part in a
// slot of its own in LDS and the four are combined after the band; one global atomic per (row, step) at most.  Column side: column
// v0 + t + 256 e belongs to thread t alone for the whole band, so its minimum over the band's rows, packed key << 6 | row within
// the band (its count), stays in a register of that thread; one global atomic per (column, band) at most.  Neither side needs an
// LDS atomic, and a minimum of "none" or a count of zero is not sent.  So a tile of R x C entries costs at most
// R ceil(C / 1024) + C ceil(R / 64) global atomics -- under 2 % of its entries; a job wholly on or left of the diagonal is skipped
// before it loads anything, and an entry of the wrong kind for the pass (one family in pass 1, two in pass 2) is not even loaded.
#define DCTFP_TEMPLATES_ONLY
#include "launch.h"

namespace {

constexpr int kAucThreads = 256;
constexpr int kAucWaves = kAucThreads / 64;
constexpr int kAucPer = 4;                        // columns of a thread per step
constexpr int kAucStep = kAucThreads * kAucPer;   // columns per step (10 bits of a row's packed minimum; a row's partial count)
constexpr int kAucBand = 64;                      // rows of a workgroup's band (6 bits of a column's packed minimum; a column's partial count)
constexpr uint32_t kNone32 = 0xffffffffu;

struct AucTile {
    const int32_t* tile;
    int64_t n_rows, n_cols, ld, row0, col0;
    const uint8_t* row_empty;
    const uint8_t* col_empty;
    int32_t cap, bound;
};

// key << 32 | index: the rank of a hit among the hits of one protein.
__device__ inline unsigned long long hit_word(uint32_t key, int64_t index) {
    return (unsigned long long)key << 32 | (unsigned long long)index;
}

// *slot = min(*slot, hit): the minimum only when the value seen (possibly stale, never too small) does not rule it out.
__device__ inline void lower_hit(unsigned long long* slot, uint32_t key, int64_t index) {
    const unsigned long long hit = hit_word(key, index);
    if (__hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) <= hit) return;
    __hip_atomic_fetch_min(slot, hit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ inline void add_count(uint32_t* slot, uint32_t part) {
    __hip_atomic_fetch_add(slot, part, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// fam[x] of protein x: a plain load of a word an earlier launch wrote.  Taken once per job for each of its columns and rows -- the
// column's family sits in a register for the whole job, the row's is the same for the whole workgroup -- never per entry.
__device__ inline int32_t _family(const int32_t* __restrict__ fam, int64_t x) { return fam[x]; }

// first[x] of protein x in pass 2: a plain load of a word pass 1 -- an earlier launch -- left.  Once per column and job, once per
// row and job.
__device__ inline unsigned long long _first_of(const unsigned long long* __restrict__ first, int64_t x) { return first[x]; }

// The key of the entry with value x: min(L1, cap), cap for a flagged row or column and for a negative value.  It counts when
// (int32_t)key <= bound: counts() of k_density.hip.
__device__ inline uint32_t key_of(uint32_t x, bool flagged, uint32_t cap) { return flagged || x >= cap ? cap : x; }

// One workgroup per (band of kAucBand rows, step of kAucStep columns) at a time.  s_row[rl][w] = the minimum of wave w over row rl
// of the band as key << 10 | column within the step, col_min[e] = the minimum of this thread's column e over the band as
// key << 6 | row within the band -- both orders are (key, index) restricted to one row / one column.  The host has checked
// cap <= rect_best_max_cap() (no packed word of a hit is all ones), row0 + n_rows <= n_nodes and col0 + n_cols <= n_nodes (the
// length of fam and first).
__global__ __launch_bounds__(kAucThreads) void tri_first_fp_kernel(const AucTile t, const int32_t* __restrict__ fam, unsigned long long* first,
                                                                    int64_t n_bands, int64_t n_steps) {
    __shared__ uint32_t s_row[kAucBand][kAucWaves];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int32_t* __restrict__ tile = t.tile;
    const uint8_t* __restrict__ row_empty = t.row_empty;
    const uint8_t* __restrict__ col_empty = t.col_empty;
    const uint32_t cap = (uint32_t)t.cap;
    const int32_t bound = t.bound;
    for (int64_t job = blockIdx.x; job < n_bands * n_steps; job += gridDim.x) {
        const int64_t r_lo = job / n_steps * kAucBand, v0 = job % n_steps * kAucStep;
        const int rows = (int)min((int64_t)kAucBand, t.n_rows - r_lo);
        const int64_t i_lo = t.row0 + r_lo, j_lo = t.col0 + v0;
        if (j_lo + min((int64_t)kAucStep, t.n_cols - v0) - 1 <= i_lo) continue;      // (no entry of the job has j > i)
        bool inside[kAucPer], full[kAucPer];                      // this thread's columns: in the tile, flagged empty
        int32_t col_fam[kAucPer];
        uint32_t col_min[kAucPer];
#pragma unroll
        for (int e = 0; e < kAucPer; ++e) {
            const int64_t c = v0 + tid + kAucThreads * e;
            inside[e] = c < t.n_cols;
            full[e] = inside[e] && col_empty && col_empty[c];
            col_fam[e] = inside[e] ? _family(fam, t.col0 + c) : 0;
            col_min[e] = kNone32;
        }
        __syncthreads();                                            // (the previous job's flush has read s_row)
        s_row[tid >> 2][tid & 3] = kNone32;                         // (kAucBand x kAucWaves = kAucThreads words)
        __syncthreads();
        for (int rl = 0; rl < rows; ++rl) {
            const int64_t i = i_lo + rl;
            const int32_t* __restrict__ row = tile + (r_lo + rl) * t.ld + v0 + tid;
            const bool row_full = row_empty && row_empty[r_lo + rl];
            const int32_t row_fam = _family(fam, i);                // (the same for the whole workgroup)
            uint32_t mine = kNone32;
#pragma unroll
            for (int e = 0; e < kAucPer; ++e) {
                if (!inside[e] || j_lo + tid + kAucThreads * e <= i || col_fam[e] == row_fam) continue;   // (one family: nothing to do, nothing to load)
                const uint32_t key = key_of((uint32_t)row[kAucThreads * e], row_full || full[e], cap);
                if ((int32_t)key > bound) continue;
                mine = min(mine, key << 10 | (uint32_t)(tid + kAucThreads * e));
                col_min[e] = min(col_min[e], key << 6 | (uint32_t)rl);
            }
            if (__ballot(mine != kNone32) == 0) continue;           // (the wave met no other family within the bound in this row)
#pragma unroll
            for (int d = 32; d > 0; d >>= 1) mine = min(mine, (uint32_t)__shfl_xor((int)mine, d));
            if (lane == 0) s_row[rl][wave] = mine;
        }
        __syncthreads();
        if (tid < rows) {
            uint32_t part = kNone32;
#pragma unroll
            for (int w = 0; w < kAucWaves; ++w) part = min(part, s_row[tid][w]);
            if (part != kNone32) lower_hit(first + i_lo + tid, part >> 10, j_lo + (part & (kAucStep - 1)));
        }
#pragma unroll
        for (int e = 0; e < kAucPer; ++e)
            if (col_min[e] != kNone32) lower_hit(first + j_lo + tid + kAucThreads * e, col_min[e] >> 6, i_lo + (col_min[e] & (kAucBand - 1)));
    }
}

// The same walk with the finished first beside fam.  s_row[rl][w] = the count of wave w over row rl of the band, col_tp[e] = the
// count of this thread's column e over the band; the two ends of an entry are decided separately, each against its own first.  The
// host has checked row0 + n_rows <= n_nodes and col0 + n_cols <= n_nodes (the length of fam, first and tp).
__global__ __launch_bounds__(kAucThreads) void tri_tp_before_kernel(const AucTile t, const int32_t* __restrict__ fam,
                                                                     const unsigned long long* __restrict__ first, uint32_t* tp, int64_t n_bands,
                                                                     int64_t n_steps) {
    __shared__ uint32_t s_row[kAucBand][kAucWaves];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int32_t* __restrict__ tile = t.tile;
    const uint8_t* __restrict__ row_empty = t.row_empty;
    const uint8_t* __restrict__ col_empty = t.col_empty;
    const uint32_t cap = (uint32_t)t.cap;
    const int32_t bound = t.bound;
    for (int64_t job = blockIdx.x; job < n_bands * n_steps; job += gridDim.x) {
        const int64_t r_lo = job / n_steps * kAucBand, v0 = job % n_steps * kAucStep;
        const int rows = (int)min((int64_t)kAucBand, t.n_rows - r_lo);
        const int64_t i_lo = t.row0 + r_lo, j_lo = t.col0 + v0;
        if (j_lo + min((int64_t)kAucStep, t.n_cols - v0) - 1 <= i_lo) continue;      // (no entry of the job has j > i)
        bool inside[kAucPer], full[kAucPer];                      // this thread's columns: in the tile, flagged empty
        int32_t col_fam[kAucPer];
        unsigned long long col_first[kAucPer];
        uint32_t col_tp[kAucPer];
#pragma unroll
        for (int e = 0; e < kAucPer; ++e) {
            const int64_t c = v0 + tid + kAucThreads * e;
            inside[e] = c < t.n_cols;
            full[e] = inside[e] && col_empty && col_empty[c];
            col_fam[e] = inside[e] ? _family(fam, t.col0 + c) : 0;
            col_first[e] = inside[e] ? _first_of(first, t.col0 + c) : 0;
            col_tp[e] = 0;
        }
        __syncthreads();                                            // (the previous job's flush has read s_row)
        s_row[tid >> 2][tid & 3] = 0;                               // (kAucBand x kAucWaves = kAucThreads words)
        __syncthreads();
        for (int rl = 0; rl < rows; ++rl) {
            const int64_t i = i_lo + rl;
            const int32_t* __restrict__ row = tile + (r_lo + rl) * t.ld + v0 + tid;
            const bool row_full = row_empty && row_empty[r_lo + rl];
            const int32_t row_fam = _family(fam, i);                // (the same for the whole workgroup)
            const unsigned long long row_first = _first_of(first, i);
            uint32_t mine = 0;
#pragma unroll
            for (int e = 0; e < kAucPer; ++e) {
                const int64_t j = j_lo + tid + kAucThreads * e;
                if (!inside[e] || j <= i || col_fam[e] != row_fam) continue;   // (two families: nothing to do, nothing to load)
                const uint32_t key = key_of((uint32_t)row[kAucThreads * e], row_full || full[e], cap);
                if ((int32_t)key > bound) continue;
                if (hit_word(key, j) < row_first) mine += 1;
                if (hit_word(key, i) < col_first[e]) col_tp[e] += 1;
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
            for (int w = 0; w < kAucWaves; ++w) part += s_row[tid][w];
            if (part != 0) add_count(tp + i_lo + tid, part);
        }
#pragma unroll
        for (int e = 0; e < kAucPer; ++e)
            if (col_tp[e] != 0) add_count(tp + j_lo + tid + kAucThreads * e, col_tp[e]);
    }
}

static_assert(kAucBand * kAucWaves == kAucThreads, "one thread clears one word of s_row");
static_assert(kAucStep == 1 << 10 && kAucBand == 1 << 6, "the packed minima keep 10 bits of a column and 6 bits of a row");

unsigned auc_grid(int64_t n_bands, int64_t n_steps) { return (unsigned)min(n_bands * n_steps, (int64_t)1 << 20); }

}  // namespace

namespace dctfp_host {

void launch_tri_first_fp(const int32_t* tile, int64_t n_rows, int64_t n_cols, int64_t ld, int64_t row0, int64_t col0, const uint8_t* row_empty,
                         const uint8_t* col_empty, int32_t cap, int32_t bound, const int32_t* fam, uint64_t* first, hipStream_t stream) {
    const AucTile t{tile, n_rows, n_cols, ld, row0, col0, row_empty, col_empty, cap, bound};
    const int64_t n_bands = (n_rows + kAucBand - 1) / kAucBand, n_steps = (n_cols + kAucStep - 1) / kAucStep;
    hipLaunchKernelGGL(tri_first_fp_kernel, dim3(auc_grid(n_bands, n_steps)), dim3(kAucThreads), 0, stream, t, fam,
                       reinterpret_cast<unsigned long long*>(first), n_bands, n_steps);
}

void launch_tri_tp_before(const int32_t* tile, int64_t n_rows, int64_t n_cols, int64_t ld, int64_t row0, int64_t col0, const uint8_t* row_empty,
                          const uint8_t* col_empty, int32_t cap, int32_t bound, const int32_t* fam, const uint64_t* first, uint32_t* tp,
                          hipStream_t stream) {
    const AucTile t{tile, n_rows, n_cols, ld, row0, col0, row_empty, col_empty, cap, bound};
    const int64_t n_bands = (n_rows + kAucBand - 1) / kAucBand, n_steps = (n_cols + kAucStep - 1) / kAucStep;
    hipLaunchKernelGGL(tri_tp_before_kernel, dim3(auc_grid(n_bands, n_steps)), dim3(kAucThreads), 0, stream, t, fam,
                       reinterpret_cast<const unsigned long long*>(first), tp, n_bands, n_steps);
}

}  // namespace dctfp_host
