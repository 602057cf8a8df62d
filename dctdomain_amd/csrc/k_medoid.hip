// dct-sim --cluster --rep medoid: per protein the sum of its distances to the members of its own cluster.  Entry (r, c) of an int32
// tile is the L1 of proteins i = row0 + r and j = col0 + c of ONE file; key = min(L1, cap), cap for a protein flagged empty on either
// side (a negative value counts as cap too: the rule of the kernels that scan the all-against-all's tiles).
//   label_sums_kernel -- one pass over the tile: every entry with j > i and labels[i] == labels[j] adds its key to sums[i] and to
//                        sums[j].  The stripes' tiles hold valid entries on both sides of the diagonal; j > i takes each unordered
//                        pair once.  After all tiles of the triangle sums[x] = the sum of key(x, y) over the other members y of
//                        x's cluster; the caller zeroes sums before the first tile and reads it after the last.
//
// Visibility (eight XCDs with private L2s; the header of k_cluster.hip has the argument).  Inside the launch sums is touched by
// agent-scope relaxed 64-bit fetch-and-adds alone (__hip_atomic_fetch_add, __HIP_MEMORY_SCOPE_AGENT): no load, no plain store,
// nothing through the scalar path.  An add is decided at the one copy the atomics of all XCDs reach and nobody reads sums before
// the launch has ended, so no ordering beyond atomicity is needed.  Integer addition commutes and is associative, and a sum stays
// below 2^64 (fewer than 2^31 members times a key below 2^22): the result is a sum over a set the inputs alone fix.  It does not
// depend on the order in which workgroups ran, on how the caller cut the triangle into tiles or on the order of its calls.  The
// tile, the flags and the labels are written by earlier launches and only read here: plain loads.  No wave waits for another
// workgroup: no flags, no tickets, no spin loops.
//
// Atomics per tile.  rect_best_kernel's walk (k_best.hip): a workgroup takes a band of kSumBand rows x kSumStep (1024) columns.
// Thread t reads columns v0 + t + 256 e, e = 0 .. 3, of every row of the band with plain dword loads -- coalesced, and free of any
// alignment rule: any ld, any column view of a wider tensor -- and only where the entry counts (the column's label sits in a
// register for the whole job, the row's is the same for the whole wave).  Row side: a row's keys are summed in the wave
// (shuffles), each wave stores its sum in a slot of its own in LDS and the four are added after the band; one global add per
// (row, step) at most.  Column side: column v0 + t + 256 e belongs to thread t alone for the whole band, so its sum over the band's
// rows stays in a register of that thread; one global add per (column, band) at most.  Neither side needs an LDS atomic, and a
// partial sum of zero is not sent.  So a tile of R x C entries costs at most R ceil(C / 1024) + C ceil(R / 64) global atomics --
// under 2 % of its entries; a job wholly left of the diagonal is skipped before it loads anything.
#define DCTFP_TEMPLATES_ONLY
#include "launch.h"

namespace {

constexpr int kSumThreads = 256;
constexpr int kSumWaves = kSumThreads / 64;
constexpr int kSumPer = 4;                        // columns of a thread per step
constexpr int kSumStep = kSumThreads * kSumPer;   // columns per step: a row's partial sum holds at most kSumStep keys
constexpr int kSumBand = 64;                      // rows of a workgroup's band: a column's partial sum holds at most kSumBand keys

struct SumTile {
    const int32_t* tile;
    int64_t n_rows, n_cols, ld, row0, col0;
    const uint8_t* row_empty;
    const uint8_t* col_empty;
    int32_t cap;
};

__device__ inline void add_sum(unsigned long long* slot, uint32_t part) {
    __hip_atomic_fetch_add(slot, (unsigned long long)part, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// One workgroup per (band of kSumBand rows, step of kSumStep columns) at a time.  s_row[rl][w] = the sum of wave w over row rl of
// the band, col_sum[e] = the sum of this thread's column e over the band.  The host has checked cap <= label_sums_max_cap() (no
// partial sum leaves 32 bits), row0 + n_rows <= n_nodes and col0 + n_cols <= n_nodes (the length of labels and of sums).
__global__ __launch_bounds__(kSumThreads) void label_sums_kernel(const SumTile t, const int32_t* __restrict__ labels, unsigned long long* sums,
                                                                  int64_t n_bands, int64_t n_steps) {
    __shared__ uint32_t s_row[kSumBand][kSumWaves];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int32_t* __restrict__ tile = t.tile;
    const uint8_t* __restrict__ row_empty = t.row_empty;
    const uint8_t* __restrict__ col_empty = t.col_empty;
    const uint32_t cap = (uint32_t)t.cap;
    for (int64_t job = blockIdx.x; job < n_bands * n_steps; job += gridDim.x) {
        const int64_t r_lo = job / n_steps * kSumBand, v0 = job % n_steps * kSumStep;
        const int rows = (int)min((int64_t)kSumBand, t.n_rows - r_lo);
        const int64_t i_lo = t.row0 + r_lo, j_lo = t.col0 + v0;
        if (j_lo + min((int64_t)kSumStep, t.n_cols - v0) - 1 <= i_lo) continue;      // (no entry of the job has j > i)
        bool inside[kSumPer], full[kSumPer];                      // this thread's columns: in the tile, flagged empty
        int32_t col_label[kSumPer];
        uint32_t col_sum[kSumPer];
#pragma unroll
        for (int e = 0; e < kSumPer; ++e) {
            const int64_t c = v0 + tid + kSumThreads * e;
            inside[e] = c < t.n_cols;
            full[e] = inside[e] && col_empty && col_empty[c];
            col_label[e] = inside[e] ? labels[t.col0 + c] : 0;
            col_sum[e] = 0;
        }
        __syncthreads();                                            // (the previous job's flush has read s_row)
        s_row[tid >> 2][tid & 3] = 0;                               // (kSumBand x kSumWaves = kSumThreads words)
        __syncthreads();
        for (int rl = 0; rl < rows; ++rl) {
            const int64_t i = i_lo + rl;
            const int32_t* __restrict__ row = tile + (r_lo + rl) * t.ld + v0 + tid;
            const bool row_full = row_empty && row_empty[r_lo + rl];
            const int32_t row_label = labels[i];
            uint32_t mine = 0;
#pragma unroll
            for (int e = 0; e < kSumPer; ++e) {
                if (!inside[e] || j_lo + tid + kSumThreads * e <= i || col_label[e] != row_label) continue;
                const uint32_t x = (uint32_t)row[kSumThreads * e];
                // (a negative value -- no L1 is -- counts as cap)
                const uint32_t key = row_full || full[e] || x >= cap ? cap : x;
                mine += key;
                col_sum[e] += key;
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
            for (int w = 0; w < kSumWaves; ++w) part += s_row[tid][w];
            if (part != 0) add_sum(sums + i_lo + tid, part);
        }
#pragma unroll
        for (int e = 0; e < kSumPer; ++e)
            if (col_sum[e] != 0) add_sum(sums + j_lo + tid + kSumThreads * e, col_sum[e]);
    }
}

static_assert(kSumBand * kSumWaves == kSumThreads, "one thread clears one word of s_row");

}  // namespace

namespace dctfp_host {

// the largest cap whose partial sums stay in 32 bits: kSumStep keys of a row, kSumBand keys of a column
int label_sums_max_cap() { return (int)min((uint32_t)0x7fffffff, 0xffffffffu / (uint32_t)max(kSumStep, kSumBand)); }

void launch_label_sums(const int32_t* tile, int64_t n_rows, int64_t n_cols, int64_t ld, int64_t row0, int64_t col0, const uint8_t* row_empty,
                       const uint8_t* col_empty, int32_t cap, const int32_t* labels, uint64_t* sums, hipStream_t stream) {
    const SumTile t{tile, n_rows, n_cols, ld, row0, col0, row_empty, col_empty, cap};
    const int64_t n_bands = (n_rows + kSumBand - 1) / kSumBand, n_steps = (n_cols + kSumStep - 1) / kSumStep;
    hipLaunchKernelGGL(label_sums_kernel, dim3((unsigned)min(n_bands * n_steps, (int64_t)1 << 20)), dim3(kSumThreads), 0, stream, t, labels,
                       reinterpret_cast<unsigned long long*>(sums), n_bands, n_steps);
}

}  // namespace dctfp_host
