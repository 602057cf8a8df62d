// DCTdomain for every protein x protein pair of two fingerprint sets, straight from the fingerprints (dct-sim --db --rank domain):
//   protein_plan_count_kernel / protein_plan_scan_kernel / protein_plan_write_kernel -- consecutive proteins packed into blocks
//       of at most 128 fingerprint rows and 96 proteins (a protein of more rows: a block of its own), on the device;
//   protein_min_kernel -- one (block of a, block of b) task at a time: sad_tile's 128 x 128 contraction (sad_tile.hip.h), reduced to
//       protein minima in LDS, each task's output entries written once with plain stores (no atomics in global memory, no fill
//       of the tile).
#define DCTFP_TEMPLATES_ONLY
#include "launch.h"
#include "sad_tile.hip.h"

namespace {

using dctfp::kSadLds;
using dctfp::kSadTile;                // fingerprint rows of a sub-tile

constexpr int kPmMaxProt = 96;        // proteins per block: 96 x 96 protein minima fill the two operand tiles' LDS exactly
constexpr int kPlanSeg = 1024;        // proteins per packing segment (one thread each; a block never crosses a segment)
constexpr int kPlanThreads = 256;

static_assert(kPmMaxProt * kPmMaxProt <= 2 * kSadLds, "the protein tile must fit in the operand tiles' LDS");

// Greedy packing of the proteins [s0, s1) of one segment: a block takes proteins while its rows stay within kSadTile and its
// proteins within kPmMaxProt (a protein of more rows than kSadTile alone).  With `starts` == nullptr only counts.
__device__ inline int64_t plan_segment(const int64_t* __restrict__ idx, int64_t s0, int64_t s1, int32_t* __restrict__ starts) {
    int64_t n = 0;
    for (int64_t p = s0; p < s1;) {
        const int64_t r0 = idx[p];
        int64_t q = p + 1;
        while (q < s1 && q - p < kPmMaxProt && idx[q + 1] - r0 <= kSadTile) ++q;
        if (starts) starts[n] = (int32_t)p;
        ++n;
        p = q;
    }
    return n;
}

__global__ __launch_bounds__(kPlanThreads) void protein_plan_count_kernel(const int64_t* __restrict__ idx, int64_t np, int64_t n_seg,
                                                                           int64_t* __restrict__ seg_count) {
    const int64_t s = (int64_t)blockIdx.x * kPlanThreads + threadIdx.x;
    if (s >= n_seg) return;
    seg_count[s] = plan_segment(idx, s * kPlanSeg, min(np, (s + 1) * kPlanSeg), nullptr);
}

// One workgroup: the exclusive prefix sum of the segments' block counts, in place; seg_count[n_seg] = the number of blocks.
__global__ __launch_bounds__(kPlanThreads) void protein_plan_scan_kernel(int64_t* __restrict__ seg_count, int64_t n_seg) {
    __shared__ int64_t part[kPlanThreads];
    int64_t carry = 0;
    for (int64_t c0 = 0; c0 < n_seg; c0 += kPlanThreads) {
        const int64_t s = c0 + threadIdx.x;
        const int64_t v = s < n_seg ? seg_count[s] : 0;
        part[threadIdx.x] = v;
        __syncthreads();
        for (int o = 1; o < kPlanThreads; o <<= 1) {   // (Hillis-Steele; the counts are few: one per 1024 proteins)
            const int64_t t = threadIdx.x >= o ? part[threadIdx.x - o] : 0;
            __syncthreads();
            part[threadIdx.x] += t;
            __syncthreads();
        }
        if (s < n_seg) seg_count[s] = carry + part[threadIdx.x] - v;
        carry += part[kPlanThreads - 1];
        __syncthreads();
    }
    if (threadIdx.x == 0) seg_count[n_seg] = carry;
}

// The blocks' first proteins at the scanned offsets; starts[n_blocks] = np closes the last block.
__global__ __launch_bounds__(kPlanThreads) void protein_plan_write_kernel(const int64_t* __restrict__ idx, int64_t np, int64_t n_seg,
                                                                           const int64_t* __restrict__ seg_off, int32_t* __restrict__ starts) {
    const int64_t s = (int64_t)blockIdx.x * kPlanThreads + threadIdx.x;
    if (s >= n_seg) return;
    plan_segment(idx, s * kPlanSeg, min(np, (s + 1) * kPlanSeg), starts + seg_off[s]);
    if (s == n_seg - 1) starts[seg_off[n_seg]] = (int32_t)np;
}

// Proteins [p0, p0 + n) own the rows [idx[p0], idx[p0 + n]); rows [t0, t0 + rows) of them (a sub-tile) get their protein's
// position within the block in map[].
__device__ inline void protein_map(const int64_t* __restrict__ idx, int64_t p0, int n, int64_t t0, int rows, uint8_t* __restrict__ map) {
    for (int t = threadIdx.x; t < n; t += 256) {
        const int64_t lo = max(idx[p0 + t], t0), hi = min(idx[p0 + t + 1], t0 + rows);
        for (int64_t r = lo; r < hi; ++r) map[r - t0] = (uint8_t)t;
    }
}

// One task = (block ka of a, block kb of b); the grid walks the tasks.  Per pair of 128-row sub-tiles (one unless a block is a
// single protein of more than 128 rows): the 128 x 128 L1 distances from sad_tile<16>, then each thread's 64 values folded along its
// runs of equal column protein and into the block's protein-minimum tile with LDS atomicMin.  That tile lives in the operand
// tiles' LDS when there is one sub-tile (<= 96 x 96 proteins), in a small array of its own when there are several (one side
// is then a single protein: <= 96 entries).  Every entry of the task's output is then stored once; a protein without rows keeps
// 0x7fffffff (block_min_kernel's fill).  Rows start on 16-byte boundaries and lda, ldb < 2^24 (the host checks).
__global__ __launch_bounds__(256, 2) void protein_min_kernel(const int8_t* __restrict__ a, int64_t lda, const int64_t* __restrict__ idx_a,
                                                             const int32_t* __restrict__ start_a, const int64_t* __restrict__ nblk_a,
                                                             const int8_t* __restrict__ b, int64_t ldb, const int64_t* __restrict__ idx_b,
                                                             const int32_t* __restrict__ start_b, const int64_t* __restrict__ nblk_b, int d,
                                                             int32_t* __restrict__ out, int64_t ldo) {
    __shared__ uint32_t lds[2 * kSadLds];
    __shared__ int32_t small_tile[kPmMaxProt];
    __shared__ uint8_t rmap[kSadTile], cmap[kSadTile];
    uint32_t* const sa = lds;
    uint32_t* const sb = lds + kSadLds;
    int32_t* const big_tile = reinterpret_cast<int32_t*>(lds);
    const int ty = threadIdx.x >> 4, tx = threadIdx.x & 15;
    const int64_t n_blk_a = *nblk_a, n_blk_b = *nblk_b, n_tasks = n_blk_a * n_blk_b;
    for (int64_t task = blockIdx.x; task < n_tasks; task += gridDim.x) {
        const int64_t ka = task / n_blk_b, kb = task - ka * n_blk_b;
        const int64_t pa0 = start_a[ka], pb0 = start_b[kb];
        const int na = (int)(start_a[ka + 1] - pa0), nb = (int)(start_b[kb + 1] - pb0);
        const int64_t ra0 = idx_a[pa0], ra1 = idx_a[pa0 + na], rb0 = idx_b[pb0], rb1 = idx_b[pb0 + nb];
        const bool single = ra1 - ra0 <= kSadTile && rb1 - rb0 <= kSadTile;
        int32_t* const tile = single ? big_tile : small_tile;
        const int n_ent = na * nb;
        if (!single || ra1 == ra0 || rb1 == rb0) {
            for (int e = threadIdx.x; e < n_ent; e += 256) tile[e] = 0x7fffffff;
            __syncthreads();
        }
        for (int64_t ta = ra0; ta < ra1; ta += kSadTile)
            for (int64_t tb = rb0; tb < rb1; tb += kSadTile) {
                const int rows_a = (int)min((int64_t)kSadTile, ra1 - ta), rows_b = (int)min((int64_t)kSadTile, rb1 - tb);
                protein_map(idx_a, pa0, na, ta, rows_a, rmap);
                protein_map(idx_b, pb0, nb, tb, rows_b, cmap);
                uint32_t acc[8][8] = {};
                dctfp::sad_tile<16>(a + ta * lda, rows_a, lda, b + tb * ldb, rows_b, ldb, d, sa, sb, acc);
                __syncthreads();                                   // (the operand tiles are read: the protein tile may take them)
                if (single) {
                    for (int e = threadIdx.x; e < n_ent; e += 256) tile[e] = 0x7fffffff;
                    __syncthreads();
                }
                // row ty * 8 + i, column tx * 8 + j (sad_tile)
                const int c0 = tx * 8;
                if (c0 < rows_b) {
                    int cp[8];
#pragma unroll
                    for (int j = 0; j < 8; ++j) cp[j] = c0 + j < rows_b ? cmap[c0 + j] : -1;
#pragma unroll
                    for (int i = 0; i < 8; ++i) {   // (no early exit: acc stays in registers)
                        const int r = ty * 8 + i;
                        const bool live = r < rows_a;
                        int32_t* const trow = tile + (live ? rmap[r] : 0) * nb;
                        int run = cp[0];
                        uint32_t m = acc[i][0];
#pragma unroll
                        for (int j = 1; j < 8; ++j) {
                            if (cp[j] == run) {
                                m = min(m, acc[i][j]);
                            } else {
                                if (live && run >= 0) atomicMin(&trow[run], (int32_t)m);
                                run = cp[j];
                                m = acc[i][j];
                            }
                        }
                        if (live && run >= 0) atomicMin(&trow[run], (int32_t)m);
                    }
                }
                __syncthreads();
            }
        for (int e = threadIdx.x; e < n_ent; e += 256) {
            const int i = e / nb, j = e - i * nb;
            out[(pa0 + i) * ldo + pb0 + j] = tile[e];
        }
        __syncthreads();                                           // (LDS is the next task's)
    }
}

}  // namespace

namespace dctfp_host {

size_t protein_plan_bytes(int64_t np) {
    const int64_t n_seg = (np + kPlanSeg - 1) / kPlanSeg;
    return (size_t)(n_seg + 1) * sizeof(int64_t) + (size_t)((np + 2) / 2 * 2) * sizeof(int32_t);
}

int launch_protein_min(const int8_t* a, int64_t lda, const int64_t* idx_a, int64_t npa, const int8_t* b, int64_t ldb, const int64_t* idx_b,
                       int64_t npb, int d, int32_t* out, int64_t ldo, void* scratch, int n_workgroups, hipStream_t stream) {
    // scratch: per side the segments' block counts (-> offsets, + the total) and the blocks' first proteins (+ the end)
    char* p = (char*)scratch;
    const int64_t* nblk[2];
    const int32_t* start[2];
    const int64_t* idx[2] = {idx_a, idx_b};
    const int64_t np[2] = {npa, npb};
    for (int s = 0; s < 2; ++s) {
        const int64_t n_seg = (np[s] + kPlanSeg - 1) / kPlanSeg;
        int64_t* seg = (int64_t*)p;
        int32_t* st = (int32_t*)(p + (n_seg + 1) * sizeof(int64_t));
        p += protein_plan_bytes(np[s]);
        const unsigned grid = (unsigned)((n_seg + kPlanThreads - 1) / kPlanThreads);
        hipLaunchKernelGGL(protein_plan_count_kernel, dim3(grid), dim3(kPlanThreads), 0, stream, idx[s], np[s], n_seg, seg);
        hipLaunchKernelGGL(protein_plan_scan_kernel, dim3(1), dim3(kPlanThreads), 0, stream, seg, n_seg);
        hipLaunchKernelGGL(protein_plan_write_kernel, dim3(grid), dim3(kPlanThreads), 0, stream, idx[s], np[s], n_seg, (const int64_t*)seg, st);
        nblk[s] = seg + n_seg;
        start[s] = st;
    }
    hipLaunchKernelGGL(protein_min_kernel, dim3((unsigned)n_workgroups), dim3(256), 0, stream, a, lda, idx_a, start[0], nblk[0], b, ldb, idx_b,
                       start[1], nblk[1], d, out, ldo);
    return DCTFP_OK;
}

}  // namespace dctfp_host
