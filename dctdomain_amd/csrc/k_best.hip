// dct-sim --db --rbh: reciprocal best hits of two files.  Entry (r, c) of an int32 tile is the L1 of protein row0 + r of file A and
// protein col0 + c of file B; key = min(L1, cap), cap for a protein flagged empty on either side (a negative value counts as cap
// too: the rule of the kernels that scan the all-against-all's tiles).  An entry with key <= bound is a hit.
//   rect_best_kernel -- one pass over the full rectangle (no diagonal, no components, no owner): every hit lowers
//                       best_row[row0 + r] to key << 32 | (col0 + c) and best_col[col0 + c] to key << 32 | (row0 + r).
// Unsigned 64-bit order of those words is the order (key, index), so after all tiles best_row[a] names the best hit of a with
// ties to the lower protein of B, and best_col[b] the same the other way round.  All ones = no hit; the caller fills both
// arrays before the first tile and reads them after the last.
//
// Visibility (eight XCDs with private L2s; the header of k_cluster.hip has the argument).  Inside the launch best_row and best_col
// are touched by agent-scope relaxed atomics alone -- a load that skips a minimum which would change nothing, then the minimum
// (__HIP_MEMORY_SCOPE_AGENT on both).  An entry only ever decreases, so a stale value read by that load costs one redundant
// atomic and never a wrong result; the minimum itself is decided at the one copy the atomics of all XCDs reach.  The result is
// a minimum over a set the inputs alone fix: it does not depend on the order in which workgroups ran, on how the caller cut
// the rectangle into tiles or on the order of its calls.  The tile and the flags are written by earlier launches and only read
// here: plain loads.  No wave waits for another workgroup: no flags, no tickets, no spin loops.
//
// Atomics per tile.  A workgroup takes a band of kBestBand rows x kBestStep (1024) columns.  Thread t reads columns
// v0 + t + 256 e, e = 0 .. 3, of every row of the band with plain dword loads -- coalesced, and free of any alignment rule: any
// ld, any column view of a wider tensor.  Row side: a row's hits are reduced in the wave (shuffles) and across the four waves
// in LDS, packed key << 10 | column within the step; one global minimum per (row, step) at most.  Column side: column
// v0 + t + 256 e belongs to thread t alone for the whole band, so its minimum over the band's rows, packed key << 6 | row
// within the band, stays in a register of that thread; one global minimum per (column, band) at most.  So a tile of R x C entries
// costs at most R ceil(C / 1024) + C ceil(R / 64) global atomics -- under 2 % of its entries, and far fewer once the arrays have
// settled (the load in front).
#define DCTFP_TEMPLATES_ONLY
#include "launch.h"

namespace {

constexpr int kBestThreads = 256;
constexpr int kBestPer = 4;                          // columns of a thread per step
constexpr int kBestStep = kBestThreads * kBestPer;   // columns per step (10 bits of a row's packed minimum)
constexpr int kBestBand = 64;                        // rows of a workgroup's band (6 bits of a column's packed minimum)
constexpr uint32_t kNone32 = 0xffffffffu;

struct RectTile {
    const int32_t* tile;
    int64_t n_rows, n_cols, ld, row0, col0;
    const uint8_t* row_empty;
    const uint8_t* col_empty;
    int32_t cap, bound;
};

// *slot = min(*slot, hit): the minimum only when the value seen (possibly stale, never too small) does not rule it out.
__device__ inline void lower_hit(unsigned long long* slot, uint32_t key, int64_t index) {
    const unsigned long long hit = (unsigned long long)key << 32 | (unsigned long long)index;
    if (__hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) <= hit) return;
    __hip_atomic_fetch_min(slot, hit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// One workgroup per (band of kBestBand rows, step of kBestStep columns) at a time.  s_row = the rows' minimum over the step as
// key << 10 | column within the step, col_min[e] = the minimum of this thread's column e over the band as key << 6 | row within
// the band -- both orders are (key, index) restricted to one row / one column.  The host has checked cap <= rect_best_max_cap() (no
// packed word of a hit is all ones), row0 + n_rows <= n_a and col0 + n_cols <= n_b (the lengths of best_row and best_col).
__global__ __launch_bounds__(kBestThreads) void rect_best_kernel(const RectTile t, unsigned long long* best_row, unsigned long long* best_col,
                                                                  int64_t n_bands, int64_t n_steps) {
    __shared__ uint32_t s_row[kBestBand];
    const int tid = threadIdx.x, lane = tid & 63;
    const int32_t* __restrict__ tile = t.tile;
    const uint8_t* __restrict__ row_empty = t.row_empty;
    const uint8_t* __restrict__ col_empty = t.col_empty;
    const uint32_t cap = (uint32_t)t.cap;
    for (int64_t job = blockIdx.x; job < n_bands * n_steps; job += gridDim.x) {
        const int64_t r_lo = job / n_steps * kBestBand, v0 = job % n_steps * kBestStep;
        const int rows = (int)min((int64_t)kBestBand, t.n_rows - r_lo);
        bool inside[kBestPer], full[kBestPer];                    // this thread's columns: in the tile, flagged empty
        uint32_t col_min[kBestPer];
#pragma unroll
        for (int e = 0; e < kBestPer; ++e) {
            const int64_t c = v0 + tid + kBestThreads * e;
            inside[e] = c < t.n_cols;
            full[e] = inside[e] && col_empty && col_empty[c];
            col_min[e] = kNone32;
        }
        __syncthreads();                                            // (the previous job's flush has read s_row)
        if (tid < kBestBand) s_row[tid] = kNone32;
        __syncthreads();
        for (int rl = 0; rl < rows; ++rl) {
            const int32_t* __restrict__ row = tile + (r_lo + rl) * t.ld + v0 + tid;
            const bool row_full = row_empty && row_empty[r_lo + rl];
            uint32_t mine = kNone32;
#pragma unroll
            for (int e = 0; e < kBestPer; ++e) {
                if (!inside[e]) continue;
                const uint32_t x = (uint32_t)row[kBestThreads * e];
                // (a negative value -- no L1 is -- counts as cap)
                const uint32_t key = row_full || full[e] || x >= cap ? cap : x;
                if ((int32_t)key > t.bound) continue;
                mine = min(mine, key << 10 | (uint32_t)(tid + kBestThreads * e));
                col_min[e] = min(col_min[e], key << 6 | (uint32_t)rl);
            }
            if (__ballot(mine != kNone32) == 0) continue;          // (the wave has no hit in this row)
#pragma unroll
            for (int d = 32; d > 0; d >>= 1) mine = min(mine, (uint32_t)__shfl_xor((int)mine, d));
            if (lane == 0) atomicMin(&s_row[rl], mine);
        }
        __syncthreads();
        if (tid < rows && s_row[tid] != kNone32)
            lower_hit(best_row + t.row0 + r_lo + tid, s_row[tid] >> 10, t.col0 + v0 + (s_row[tid] & (kBestStep - 1)));
#pragma unroll
        for (int e = 0; e < kBestPer; ++e)
            if (col_min[e] != kNone32)
                lower_hit(best_col + t.col0 + v0 + tid + kBestThreads * e, col_min[e] >> 6, t.row0 + r_lo + (col_min[e] & (kBestBand - 1)));
    }
}

}  // namespace

namespace dctfp_host {

int rect_best_max_cap() { return (int)(kNone32 >> 10) - 1; }   // key << 10 | 1023 of a hit is never all ones

void launch_rect_best(const int32_t* tile, int64_t n_rows, int64_t n_cols, int64_t ld, int64_t row0, int64_t col0, const uint8_t* row_empty,
                      const uint8_t* col_empty, int32_t cap, int32_t bound, uint64_t* best_row, uint64_t* best_col, hipStream_t stream) {
    const RectTile t{tile, n_rows, n_cols, ld, row0, col0, row_empty, col_empty, cap, bound};
    const int64_t n_bands = (n_rows + kBestBand - 1) / kBestBand, n_steps = (n_cols + kBestStep - 1) / kBestStep;
    hipLaunchKernelGGL(rect_best_kernel, dim3((unsigned)min(n_bands * n_steps, (int64_t)1 << 20)), dim3(kBestThreads), 0, stream, t,
                       reinterpret_cast<unsigned long long*>(best_row), reinterpret_cast<unsigned long long*>(best_col), n_bands, n_steps);
}

}  // namespace dctfp_host
