// The walk over a band of rows of a TriTile (tri_tile.hip.h) of ONE file's triangle -- only entries with j > i count --, once, for the
// kernels that reduce such a tile onto per-protein arrays.
// Users: k_medoid.hip (label_sums), k_density.hip (tri_degree, tri_link_core) and k_auc.hip (tri_first_fp, tri_tp_before): a kernel
// builds a pass object from its own arguments and calls band_walk; the pass says only what differs.  k_best.hip (rect_best) takes
// the constants, the grid, the key rule and lower_hit from here and keeps a loop of its own, for the reason written there.
//
// A pass supplies
//   Word, kIdle, join    -- the partial result of a row or a column, the word that means "nothing yet" and how two parts combine
//                           (0 and +; all ones and unsigned min; 0x7fffffff and signed min)
//   kBounded             -- whether t.bound applies (a sum has no cut-off)
//   Side, side(x)        -- what the pass knows of protein x beside the tile (a label, a family, a flag): loaded once per column
//                           and job and once per row and band, never per entry
//   wants(row, col)      -- on the two side values, BEFORE the entry is loaded: an entry of the wrong kind is not even read
//   entry(...)           -- what a surviving entry does to the thread's word of its row and of its column
//   row_out, col_out     -- the flushes: the only places that touch the output arrays, through the unit's atomic helpers
//
// Visibility (eight XCDs with private L2s; the header of k_cluster.hip has the argument).  Inside a launch EVERY access to an output
// array is an agent-scope relaxed atomic (__HIP_MEMORY_SCOPE_AGENT): there is no plain load or store of any of them and nothing goes
// through the scalar path.  An add or a minimum is decided at the one copy the atomics of all XCDs reach and nobody reads the result
// before the launch has ended, so no ordering beyond atomicity is needed.  Addition and minimum commute and are associative: a
// result is a sum or a minimum over a set the inputs alone fix, and depends neither on the order in which workgroups ran, nor on
// how the caller cut the triangle into tiles, nor on the order of its calls.  The tile, the flags and the side arrays are written
// by earlier launches and only read here: plain loads.  No workgroup waits for another: no flags, no tickets, no spin loops.
//
// Atomics per tile.  A workgroup takes a job of kBandRows (64) rows x kBandStep (1024) columns.  Thread t reads columns
// v0 + t + 256 e, e = 0 .. 3, of every row of the band with plain dword loads -- coalesced, and free of any alignment rule: any ld,
// any column view of a wider tensor.  Row side: a row's part is reduced in the wave (shuffles), each wave stores its part in a slot
// of its own in LDS and the four are joined after the band; one global atomic per (row, step) at most.  Column side: column
// v0 + t + 256 e belongs to thread t alone for the whole band, so its part over the band's rows stays in a register of that
// thread; one global atomic per (column, band) at most.  Neither side needs an LDS atomic, and an idle part is not sent.  So a tile
// of R x C entries costs at most R ceil(C / 1024) + C ceil(R / 64) global atomics -- under 2 % of its entries; a job
// wholly on or left of the diagonal is skipped before it loads anything.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "tri_tile.hip.h"

namespace {

using dctfp::TriTile;

constexpr int kBandThreads = 256;
constexpr int kBandWaves = kBandThreads / 64;
constexpr int kBandPer = 4;                         // columns of a thread per step
constexpr int kBandStep = kBandThreads * kBandPer;  // columns per step (10 bits of a row's packed minimum; at most kBandStep keys in a row's part)
constexpr int kBandRows = 64;                       // rows of a band (6 bits of a column's packed minimum; at most kBandRows keys in a column's part)
constexpr uint32_t kNone32 = 0xffffffffu;           // a packed minimum: no hit

static_assert(kBandRows * kBandWaves == kBandThreads, "one thread clears one word of s_row");
static_assert(kBandStep == 1 << 10 && kBandRows == 1 << 6, "the packed minima keep 10 bits of a column and 6 bits of a row");

// The jobs of a tile and the workgroups that take them; a workgroup beyond the cap's reach takes several jobs, gridDim.x apart.
struct BandGrid {
    int64_t n_bands, n_steps;
    unsigned blocks;
};

inline BandGrid band_grid(const TriTile& t) {
    const int64_t n_bands = (t.n_rows + kBandRows - 1) / kBandRows, n_steps = (t.n_cols + kBandStep - 1) / kBandStep;
    return {n_bands, n_steps, (unsigned)min(n_bands * n_steps, (int64_t)1 << 20)};
}

struct NoSide {};   // the Side of a pass with nothing beside the tile

// The key of the entry with value x: min(L1, cap), cap for a flagged row or column and for a negative value (no L1 is one).
__device__ inline uint32_t key_of(uint32_t x, bool flagged, uint32_t cap) { return flagged || x >= cap ? cap : x; }

// key << 32 | index: the rank of a hit among the hits of one protein.
__device__ inline unsigned long long hit_word(uint32_t key, int64_t index) {
    return (unsigned long long)key << 32 | (unsigned long long)index;
}

// *slot = min(*slot, hit): the minimum only when the value seen (possibly stale, never too small) does not rule it out.  An entry
// only ever decreases, so a stale value read by that load costs one redundant atomic and never a wrong result.
__device__ inline void lower_hit(unsigned long long* slot, uint32_t key, int64_t index) {
    const unsigned long long hit = hit_word(key, index);
    if (__hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) <= hit) return;
    __hip_atomic_fetch_min(slot, hit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// One workgroup per (band of kBandRows rows, step of kBandStep columns) at a time.  s_row[rl][w] = the part of wave w over row rl
// of the band, col[e] = the part of this thread's column e over the band.  The export has checked that every row0 + r and col0 + c
// lies inside the arrays of the pass: bounded on the host, and not on the device.
// (the tile's pointers are __restrict__ locals: struct members cannot carry the qualifier -- profiles/tri_walk/README.md)
template <class Pass>
__device__ inline void band_walk(const TriTile& t, int64_t n_bands, int64_t n_steps, const Pass& pass) {
    using Word = typename Pass::Word;
    using Side = typename Pass::Side;
    __shared__ Word s_row[kBandRows][kBandWaves];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int32_t* __restrict__ tile = t.tile;
    const uint8_t* __restrict__ row_empty = t.row_empty;
    const uint8_t* __restrict__ col_empty = t.col_empty;
    const uint32_t cap = (uint32_t)t.cap;
    const int32_t bound = t.bound;
    for (int64_t job = blockIdx.x; job < n_bands * n_steps; job += gridDim.x) {
        const int64_t r_lo = job / n_steps * kBandRows, v0 = job % n_steps * kBandStep;
        const int rows = (int)min((int64_t)kBandRows, t.n_rows - r_lo);
        const int64_t i_lo = t.row0 + r_lo, j_lo = t.col0 + v0;
        if (j_lo + min((int64_t)kBandStep, t.n_cols - v0) - 1 <= i_lo) continue;                      // (no entry of the job has j > i)
        bool inside[kBandPer], full[kBandPer];                      // this thread's columns: in the tile, flagged empty
        Side col_side[kBandPer];
        Word col[kBandPer];
#pragma unroll
        for (int e = 0; e < kBandPer; ++e) {
            const int64_t c = v0 + tid + kBandThreads * e;
            inside[e] = c < t.n_cols;
            full[e] = inside[e] && col_empty && col_empty[c];
            col_side[e] = inside[e] ? pass.side(t.col0 + c) : Side{};
            col[e] = Pass::kIdle;
        }
        __syncthreads();                                            // (the previous job's flush has read s_row)
        s_row[tid >> 2][tid & 3] = Pass::kIdle;                     // (kBandRows x kBandWaves = kBandThreads words)
        __syncthreads();
        for (int rl = 0; rl < rows; ++rl) {
            const int64_t i = i_lo + rl;
            const int32_t* __restrict__ row = tile + (r_lo + rl) * t.ld + v0 + tid;
            const bool row_full = row_empty && row_empty[r_lo + rl];
            const Side row_side = pass.side(i);                     // (the same for the whole workgroup)
            Word mine = Pass::kIdle;
#pragma unroll
            for (int e = 0; e < kBandPer; ++e) {
                const int cl = tid + kBandThreads * e;              // (the column within the step)
                const int64_t j = j_lo + tid + kBandThreads * e;
                if (!inside[e] || j <= i || !Pass::wants(row_side, col_side[e])) continue;   // (nothing to do, nothing to load)
                const uint32_t key = key_of((uint32_t)row[kBandThreads * e], row_full || full[e], cap);
                if (Pass::kBounded && (int32_t)key > bound) continue;
                pass.entry(key, i, j, rl, cl, row_side, col_side[e], mine, col[e]);
            }
            if (__ballot(mine != Pass::kIdle) == 0) continue;       // (the wave has nothing for this row)
#pragma unroll
            for (int d = 32; d > 0; d >>= 1) mine = Pass::join(mine, (Word)__shfl_xor((int)mine, d));
            if (lane == 0) s_row[rl][wave] = mine;
        }
        __syncthreads();
        if (tid < rows) {
            Word part = Pass::kIdle;
#pragma unroll
            for (int w = 0; w < kBandWaves; ++w) part = Pass::join(part, s_row[tid][w]);
            if (part != Pass::kIdle) pass.row_out(i_lo + tid, j_lo, part);
        }
#pragma unroll
        for (int e = 0; e < kBandPer; ++e)
            if (col[e] != Pass::kIdle) pass.col_out(j_lo + tid + kBandThreads * e, i_lo, col[e]);
    }
}

}  // namespace
