// DCTdomain for every protein x protein pair of two fingerprint sets, straight from the fingerprints (dct-sim --db --rank domain):
//   protein_plan_count_kernel / protein_plan_scan_kernel / protein_plan_write_kernel -- consecutive proteins packed into blocks
//       of at most 128 fingerprint rows and 96 proteins (a protein of more rows: a block of its own), on the device;
//   protein_min_kernel -- one (block of a, block of b) task at a time: sad_tile's 128 x 128 contraction (sad_tile.hip.h), reduced to
//       protein minima in LDS, each task's output entries written once with plain stores (no atomics in global memory, no fill
//       of the tile);
//   protein_cover_kernel -- the same tasks for dct-sim --min-coverage: the same minima, and 0x7fffffff instead where the fingerprint
//       rows within `bound` of the other protein do not carry the weight a protein needs (need_a / need_b).  Which rows are
//       matched by which protein is kept as two bit matrices in LDS (rows of a x proteins of b, rows of b x proteins of a), set
//       from the registers that hold the distances; the weights are summed per entry when it is stored.
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

constexpr int kCovWords = kPmMaxProt / 32;   // words of a row's matched-protein bits
constexpr int kCovAlign = 16;                // sad_tile's fill: rows on 16-byte boundaries, as for protein_min_kernel (the host checks)

// The weight of the rows [r0, r1) whose bit `q` is set in their kCovWords words of `bits`.
__device__ inline int64_t covered_weight(const uint32_t* __restrict__ bits, const int32_t* __restrict__ w, int r0, int r1, int q) {
    int64_t s = 0;
    for (int r = r0; r < r1; ++r)
        if (bits[r * kCovWords + (q >> 5)] >> (q & 31) & 1) s += w[r];
    return s;
}

// protein_min_kernel with a coverage requirement: out[pa, pb] = the protein minimum when the rows of pa matched by pb weigh at
// least need_a[pa] and the rows of pb matched by pa at least need_b[pb], else 0x7fffffff.  Row r of pa is matched by pb when its L1
// to some row of pb is <= bound (signed: a negative bound matches nothing); its weight is w_a[r] (per row of a, as w_b of b); a
// need <= 0 asks nothing of its side, and with none on either side every entry is protein_min_kernel's.  Same tasks, contraction
// and minimum folding as there; in addition every thread turns its 64 distances into a keep mask (sad_keep_mask) and sets, per
// surviving (row, column), the column's protein in bit_a[row] and the row's protein in bit_b[column] with LDS atomicOr.
//   One sub-tile per side (the common task): both bit matrices are complete after the one contraction, and the store pass sums
//   the weights (staged in LDS) over each entry's contiguous rows on both sides -- only for entries within the bound, since a
//   minimum above it means no row matched.
//   Several sub-tiles (a block that is one protein of more than 128 rows; <= 96 entries): the bits of a sub-tile's rows are
//   complete only after it has met every sub-tile of the other side, so there are two passes over the sub-tile pairs -- a's
//   sub-tiles outside (the minima and cov_a), then b's outside (cov_b): twice the contraction, for the rare task.  After the
//   inner loop the rows' weights go to the entries' sums with LDS atomicAdd and the bits are cleared.
// Sums are int64: any int32 weights.
__global__ __launch_bounds__(256, 2) void protein_cover_kernel(const int8_t* __restrict__ a, int64_t lda, const int64_t* __restrict__ idx_a,
                                                               const int32_t* __restrict__ start_a, const int64_t* __restrict__ nblk_a,
                                                               const int32_t* __restrict__ w_a, const int32_t* __restrict__ need_a,
                                                               const int8_t* __restrict__ b, int64_t ldb, const int64_t* __restrict__ idx_b,
                                                               const int32_t* __restrict__ start_b, const int64_t* __restrict__ nblk_b,
                                                               const int32_t* __restrict__ w_b, const int32_t* __restrict__ need_b, int d,
                                                               int32_t bound, int32_t* __restrict__ out, int64_t ldo) {
    __shared__ uint32_t lds[2 * kSadLds];
    __shared__ int32_t small_tile[kPmMaxProt];
    __shared__ unsigned long long cov_a[kPmMaxProt], cov_b[kPmMaxProt];   // several sub-tiles: the entries' covered weights
    __shared__ uint32_t bit_a[kSadTile * kCovWords], bit_b[kSadTile * kCovWords];
    __shared__ int32_t ws_a[kSadTile], ws_b[kSadTile];                     // one sub-tile: the rows' weights
    __shared__ uint8_t first_a[kPmMaxProt + 1], first_b[kPmMaxProt + 1];   // one sub-tile: the proteins' first rows within the block
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
        for (int x = threadIdx.x; x < kSadTile * kCovWords; x += 256) bit_a[x] = bit_b[x] = 0;
        if (single) {
            for (int x = threadIdx.x; x < kSadTile; x += 256) {
                ws_a[x] = ra0 + x < ra1 ? w_a[ra0 + x] : 0;
                ws_b[x] = rb0 + x < rb1 ? w_b[rb0 + x] : 0;
            }
            for (int x = threadIdx.x; x <= na; x += 256) first_a[x] = (uint8_t)(idx_a[pa0 + x] - ra0);
            for (int x = threadIdx.x; x <= nb; x += 256) first_b[x] = (uint8_t)(idx_b[pb0 + x] - rb0);
        } else {
            for (int e = threadIdx.x; e < n_ent; e += 256) cov_a[e] = cov_b[e] = 0;
        }
        if (!single || ra1 == ra0 || rb1 == rb0)
            for (int e = threadIdx.x; e < n_ent; e += 256) tile[e] = 0x7fffffff;
        __syncthreads();
        const int64_t sub_a = (ra1 - ra0 + kSadTile - 1) / kSadTile, sub_b = (rb1 - rb0 + kSadTile - 1) / kSadTile;
        for (int pass = 0; pass < (single ? 1 : 2); ++pass) {      // pass 0: a's sub-tiles outside, pass 1: b's
            const int64_t n_outer = pass == 0 ? sub_a : sub_b, n_inner = pass == 0 ? sub_b : sub_a;
            for (int64_t so = 0; so < n_outer; ++so) {
                for (int64_t si = 0; si < n_inner; ++si) {
                    const int64_t ta = ra0 + (pass == 0 ? so : si) * kSadTile, tb = rb0 + (pass == 0 ? si : so) * kSadTile;
                    const int rows_a = (int)min((int64_t)kSadTile, ra1 - ta), rows_b = (int)min((int64_t)kSadTile, rb1 - tb);
                    protein_map(idx_a, pa0, na, ta, rows_a, rmap);
                    protein_map(idx_b, pb0, nb, tb, rows_b, cmap);
                    uint32_t acc[8][8] = {};
                    dctfp::sad_tile<kCovAlign>(a + ta * lda, rows_a, lda, b + tb * ldb, rows_b, ldb, d, sa, sb, acc);
                    __syncthreads();                               // (the operand tiles are read: the protein tile may take them)
                    if (single) {
                        for (int e = threadIdx.x; e < n_ent; e += 256) tile[e] = 0x7fffffff;
                        __syncthreads();
                    }
                    // row ty * 8 + i, column tx * 8 + j (sad_tile)
                    const int c0 = tx * 8;
                    if (pass == 0 && c0 < rows_b) {                // the minima: protein_min_kernel's folding
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
                    // the matched bits of the side(s) this pass completes; in the common case no lane of a wave has a survivor
                    uint64_t keep = bound < 0 ? 0 : dctfp::sad_keep_mask(acc, 0xffffffffu, (uint32_t)bound, rows_a, rows_b);
                    while (keep) {
                        const int k = __ffsll((unsigned long long)keep) - 1;
                        keep &= keep - 1;
                        const int r = ty * 8 + (k >> 3), c = c0 + (k & 7);
                        const int p = rmap[r], q = cmap[c];
                        if (single || pass == 0) atomicOr(&bit_a[r * kCovWords + (q >> 5)], 1u << (q & 31));
                        if (single || pass == 1) atomicOr(&bit_b[c * kCovWords + (p >> 5)], 1u << (p & 31));
                    }
                    __syncthreads();
                }
                if (!single) {
                    // the outer sub-tile has met every sub-tile of the other side: its rows' weights to their entries, the bits cleared
                    // (rmap / cmap still hold the outer sub-tile's proteins: the inner loop set them if it set any bit)
                    const int64_t t0 = (pass == 0 ? ra0 : rb0) + so * kSadTile;
                    const int rows = (int)min((int64_t)kSadTile, (pass == 0 ? ra1 : rb1) - t0);
                    const int n_other = pass == 0 ? nb : na;
                    uint32_t* const bits = pass == 0 ? bit_a : bit_b;
                    for (int x = threadIdx.x; x < rows * n_other; x += 256) {
                        const int r = x / n_other, q = x - r * n_other;
                        if (bits[r * kCovWords + (q >> 5)] >> (q & 31) & 1) {
                            if (pass == 0) atomicAdd(&cov_a[rmap[r] * nb + q], (unsigned long long)(int64_t)w_a[t0 + r]);
                            else atomicAdd(&cov_b[q * nb + cmap[r]], (unsigned long long)(int64_t)w_b[t0 + r]);
                        }
                    }
                    __syncthreads();
                    for (int x = threadIdx.x; x < kSadTile * kCovWords; x += 256) bits[x] = 0;
                    __syncthreads();
                }
            }
        }
        for (int e = threadIdx.x; e < n_ent; e += 256) {
            const int i = e / nb, j = e - i * nb;
            int32_t v = tile[e];
            const int32_t want_a = need_a[pa0 + i], want_b = need_b[pb0 + j];
            if (want_a > 0 || want_b > 0) {
                if (v > bound) {                                   // (no row of either protein is matched)
                    v = 0x7fffffff;
                } else {
                    const int64_t got_a = want_a <= 0 ? 0 : single ? covered_weight(bit_a, ws_a, first_a[i], first_a[i + 1], j) : (int64_t)cov_a[e];
                    const int64_t got_b = want_b <= 0 ? 0 : single ? covered_weight(bit_b, ws_b, first_b[j], first_b[j + 1], i) : (int64_t)cov_b[e];
                    if (got_a < want_a || got_b < want_b) v = 0x7fffffff;
                }
            }
            out[(pa0 + i) * ldo + pb0 + j] = v;
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

namespace {

// The two block plans, built on the stream in `scratch`: per side the segments' block counts (-> offsets, + the total) and the
// blocks' first proteins (+ the end).
struct BlockPlans {
    const int64_t* nblk[2];
    const int32_t* start[2];
};

BlockPlans plan_blocks(const int64_t* idx_a, int64_t npa, const int64_t* idx_b, int64_t npb, void* scratch, hipStream_t stream) {
    BlockPlans plans;
    char* p = (char*)scratch;
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
        plans.nblk[s] = seg + n_seg;
        plans.start[s] = st;
    }
    return plans;
}

}  // namespace

int launch_protein_min(const int8_t* a, int64_t lda, const int64_t* idx_a, int64_t npa, const int8_t* b, int64_t ldb, const int64_t* idx_b,
                       int64_t npb, int d, int32_t* out, int64_t ldo, void* scratch, int n_workgroups, hipStream_t stream) {
    const BlockPlans plans = plan_blocks(idx_a, npa, idx_b, npb, scratch, stream);
    hipLaunchKernelGGL(protein_min_kernel, dim3((unsigned)n_workgroups), dim3(256), 0, stream, a, lda, idx_a, plans.start[0], plans.nblk[0], b,
                       ldb, idx_b, plans.start[1], plans.nblk[1], d, out, ldo);
    return DCTFP_OK;
}

int launch_protein_cover(const int8_t* a, int64_t lda, const int64_t* idx_a, int64_t npa, const int32_t* w_a, const int32_t* need_a,
                         const int8_t* b, int64_t ldb, const int64_t* idx_b, int64_t npb, const int32_t* w_b, const int32_t* need_b, int d,
                         int32_t bound, int32_t* out, int64_t ldo, void* scratch, int n_workgroups, hipStream_t stream) {
    const BlockPlans plans = plan_blocks(idx_a, npa, idx_b, npb, scratch, stream);
    hipLaunchKernelGGL(protein_cover_kernel, dim3((unsigned)n_workgroups), dim3(256), 0, stream, a, lda, idx_a, plans.start[0], plans.nblk[0],
                       w_a, need_a, b, ldb, idx_b, plans.start[1], plans.nblk[1], w_b, need_b, d, bound, out, ldo);
    return DCTFP_OK;
}

}  // namespace dctfp_host
