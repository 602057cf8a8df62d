// dct-sim --db --rbh: reciprocal best hits of two files.  Entry (r, c) of an int32 tile is the L1 of protein row0 + r of file A and
// protein col0 + c of file B; key = min(L1, cap), cap for a protein flagged empty on either side (a negative value counts as cap
// too: the rule of the kernels that scan the all-against-all's tiles).  An entry with key <= bound is a hit.
//   rect_best_kernel -- one pass over the full rectangle (no diagonal, no components, no owner): every hit lowers
//                       best_row[row0 + r] to key << 32 | (col0 + c) and best_col[col0 + c] to key << 32 | (row0 + r).
// Unsigned 64-bit order of those words is the order (key, index), so after all tiles best_row[a] names the best hit of a with
// ties to the lower protein of B, and best_col[b] the same the other way round.  All ones = no hit; the caller fills both
// arrays before the first tile and reads them after the last.
//
// The job, the tile, the key rule, the visibility argument and the atomics a tile costs are band_walk.hip.h's.  The arrays: best_row
// and best_col see lower_hit alone (defined there: a load that skips a minimum which would change nothing, then the minimum), so a
// tile costs far fewer atomics than the walk's bound once the arrays have settled.
//
// EXEMPT from band_walk by name: the loop below is the walk's, with one word of LDS per row and an LDS atomicMin by each wave's first
// lane in place of a slot per wave, and without the diagonal.  As a pass of band_walk (a switch for the rectangle, packed minima,
// the wave's index in a scalar register: this loop's 28 vector registers, 1024 bytes of LDS for 256) the kernel, alone on one
// 8192 x 16384 tile, took 0.282 ms where this loop takes 0.187 ms: slower at equal registers, outside the rule of
// profiles/band_walk/README.md, which has the figures.
#define DCTFP_TEMPLATES_ONLY
#include "launch.h"
#include "band_walk.hip.h"

namespace {

// s_row[rl] = row rl's minimum over the step as key << 10 | column within the step, col_min[e] = the minimum of this thread's
// column e over the band as key << 6 | row within the band -- both orders are (key, index) restricted to one row / one column.
// The host has checked cap <= rect_best_max_cap() (no packed word of a hit is all ones), row0 + n_rows <= n_a and
// col0 + n_cols <= n_b (the lengths of best_row and best_col).
__global__ __launch_bounds__(kBandThreads) void rect_best_kernel(const TriTile t, unsigned long long* best_row, unsigned long long* best_col,
                                                                  int64_t n_bands, int64_t n_steps) {
    __shared__ uint32_t s_row[kBandRows];
    const int tid = threadIdx.x, lane = tid & 63;
    const int32_t* __restrict__ tile = t.tile;
    const uint8_t* __restrict__ row_empty = t.row_empty;
    const uint8_t* __restrict__ col_empty = t.col_empty;
    const uint32_t cap = (uint32_t)t.cap;
    for (int64_t job = blockIdx.x; job < n_bands * n_steps; job += gridDim.x) {
        const int64_t r_lo = job / n_steps * kBandRows, v0 = job % n_steps * kBandStep;
        const int rows = (int)min((int64_t)kBandRows, t.n_rows - r_lo);
        bool inside[kBandPer], full[kBandPer];                    // this thread's columns: in the tile, flagged empty
        uint32_t col_min[kBandPer];
#pragma unroll
        for (int e = 0; e < kBandPer; ++e) {
            const int64_t c = v0 + tid + kBandThreads * e;
            inside[e] = c < t.n_cols;
            full[e] = inside[e] && col_empty && col_empty[c];
            col_min[e] = kNone32;
        }
        __syncthreads();                                            // (the previous job's flush has read s_row)
        if (tid < kBandRows) s_row[tid] = kNone32;
        __syncthreads();
        for (int rl = 0; rl < rows; ++rl) {
            const int32_t* __restrict__ row = tile + (r_lo + rl) * t.ld + v0 + tid;
            const bool row_full = row_empty && row_empty[r_lo + rl];
            uint32_t mine = kNone32;
#pragma unroll
            for (int e = 0; e < kBandPer; ++e) {
                if (!inside[e]) continue;
                const uint32_t key = key_of((uint32_t)row[kBandThreads * e], row_full || full[e], cap);
                if ((int32_t)key > t.bound) continue;
                mine = min(mine, key << 10 | (uint32_t)(tid + kBandThreads * e));
                col_min[e] = min(col_min[e], key << 6 | (uint32_t)rl);
            }
            if (__ballot(mine != kNone32) == 0) continue;          // (the wave has no hit in this row)
#pragma unroll
            for (int d = 32; d > 0; d >>= 1) mine = min(mine, (uint32_t)__shfl_xor((int)mine, d));
            if (lane == 0) atomicMin(&s_row[rl], mine);
        }
        __syncthreads();
        if (tid < rows && s_row[tid] != kNone32)
            lower_hit(best_row + t.row0 + r_lo + tid, s_row[tid] >> 10, t.col0 + v0 + (s_row[tid] & (kBandStep - 1)));
#pragma unroll
        for (int e = 0; e < kBandPer; ++e)
            if (col_min[e] != kNone32)
                lower_hit(best_col + t.col0 + v0 + tid + kBandThreads * e, col_min[e] >> 6, t.row0 + r_lo + (col_min[e] & (kBandRows - 1)));
    }
}

}  // namespace

namespace dctfp_host {

int rect_best_max_cap() { return (int)(kNone32 >> 10) - 1; }   // key << 10 | 1023 of a hit is never all ones

void launch_rect_best(const TriTile& t, uint64_t* best_row, uint64_t* best_col, hipStream_t stream) {
    const BandGrid g = band_grid(t);
    hipLaunchKernelGGL(rect_best_kernel, dim3(g.blocks), dim3(kBandThreads), 0, stream, t, reinterpret_cast<unsigned long long*>(best_row),
                       reinterpret_cast<unsigned long long*>(best_col), g.n_bands, g.n_steps);
}

}  // namespace dctfp_host
