// dct-sim --db --zscore: the moments of every protein's background.  Entry (r, c) of an int32 tile is the L1 of protein row0 + r of
// one file and protein col0 + c of another; an entry COUNTS unless its row or its column is flagged empty or its value x has
// (uint32_t)x >= cap -- cap is an EXCLUSION LIMIT here, not a ceiling: a negative value and protein_min's 0x7fffffff are left out,
// and a value below cap counts raw, however far above 17000 it lies.
//   rect_moments_kernel -- one pass over the full rectangle (no diagonal): every counting entry adds (1, x, x * x) to
//                          row_mom[k * n_a + row0 + r] and to col_mom[k * n_b + col0 + c], k = 0, 1, 2: three planes (count, sum,
//                          sum of squares) of exact 64-bit integers.  Either array may be absent (a template switch: the side that
//                          is not asked for costs nothing).  The caller zeroes the arrays; the words add up over tiles, groups and
//                          calls, in any order.
//
// NOT a pass of band_walk, and with a loop of its own over the TriTile: a pass reduces a job onto ONE word per row and one per
// column, a minimum or a count that fits 32 bits; here a row and a column each carry THREE 64-bit words whose parts have different
// widths (a count from ballots, a 32-bit sum, a 64-bit sum of squares), and the rectangle has no diagonal to leave jobs at.  The
// unit takes the tile's description (tri_tile.hip.h) and nothing else of the walks.
//
// The job.  A workgroup of kMomThreads (256) threads takes a job of kMomRows (64) rows x kMomStep (1024) columns at a time,
// gridDim.x apart; thread t owns the columns v0 + t + 256 e, e < kMomPer (4), and reads them row by row with plain dword loads --
// coalesced, and free of any alignment rule: any ld, any column view of a wider tensor.  The flags are loaded once per column and
// job (the thread's own columns) and once per row and job (into LDS, which the row loop reads), never per entry; a flagged row and
// a flagged column are not loaded at all.
//
// The row side.  Per row a thread adds up its four columns: the sum in 32 bits, the squares in 64 bits from the start; the count
// is not carried by the lanes at all -- it is the population of the four ballots, a scalar.  The wave then reduces sum and squares
// with xor shuffles (a 64-bit shuffle is two 32-bit ones) and its first lane stores the wave's part of the row in LDS, a slot per
// (row, wave): plain stores, nothing to zero, nothing to contend for.  Behind the band's last row thread r adds the kMomWaves parts
// of row r in 64 bits and sends them: at most 3 global atomics per (row, step of 1024 columns), consecutive threads on consecutive
// words of each plane.
//
// Why the 32-bit sums cannot overflow.  A wave's sum of one row is at most 64 lanes x kMomPer columns x (cap - 1), a column's sum
// over a band at most kMomRows x (cap - 1); the export refuses a cap above kMomMaxCap = 2^24, for which both stay below 2^32 (the
// static_asserts below).  The 64-bit words: a row meets at most n_b columns and a column at most n_a rows, and the export refuses a
// cap for which n x (cap - 1)^2 does not fit 64 bits.
//
// The column side.  The thread that owns a column keeps its three words in registers over the band (count and sum in 32 bits,
// squares in 64) and sends them at the band's end: at most 3 global atomics per (column, band of 64 rows).  The loop is the unit's
// own, so the band could be taller and the column atomics fewer -- measured, that loses: 128 and 256 rows leave the columns' side
// where it is and slow the rows' side down by 1.6 x and 2.9 x, because a tile then has too few jobs to keep the loads of every CU
// in flight (profiles/zscore/README.md).
//
// An idle part (count 0) is not sent.  Inside a launch row_mom and col_mom are touched by agent-scope relaxed 64-bit
// __hip_atomic_fetch_add alone, through mom_add: no plain load, no plain store, nothing through the scalar path.  An add is decided
// at the one copy the atomics of all eight XCDs reach and nobody reads the result before the launch has ended; integer addition
// commutes and is associative, so the words are sums over a set the inputs alone fix and depend neither on the order in which
// workgroups ran, nor on how the caller cut the rectangle into tiles, nor on the order of its calls.  No workgroup waits for another.
#define DCTFP_TEMPLATES_ONLY
#include "launch.h"
#include "tri_tile.hip.h"

#ifndef DCTFP_MOM_ROWS
#define DCTFP_MOM_ROWS 64           // (an A/B build may try another band height: profiles/zscore/README.md)
#endif

namespace {

using dctfp::TriTile;

constexpr int kMomThreads = 256;
constexpr int kMomWaves = kMomThreads / 64;
constexpr int kMomPer = 4;                              // columns of a thread
constexpr int kMomStep = kMomThreads * kMomPer;         // columns of a job
constexpr int kMomRows = DCTFP_MOM_ROWS;                // rows of a job: the band
constexpr int kMomMaxCap = 1 << 24;                     // the largest exclusion limit
constexpr unsigned kMomMaxBlocks = 256 * 8;             // eight workgroups of four waves fill a CU

static_assert((int64_t)64 * kMomPer * (kMomMaxCap - 1) < ((int64_t)1 << 32), "a wave's 32-bit sum of one row holds its 256 entries");
static_assert((int64_t)kMomRows * (kMomMaxCap - 1) < ((int64_t)1 << 32), "a column's 32-bit sum holds the rows of a band");
static_assert(kMomRows >= 1 && kMomRows <= kMomThreads, "thread r loads the flag of row r of the band and sends its words");

// One wave's part of one row of the band.
struct MomPart {
    uint32_t n, s1;
    unsigned long long s2;
};

// Does the entry with value x count?  (uint32_t: a negative value lies above every cap.)
__device__ inline bool mom_counts(uint32_t x, uint32_t cap) { return x < cap; }

__device__ inline unsigned long long mom_shfl_xor(unsigned long long v, int d) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, d), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), d);
    return (unsigned long long)hi << 32 | lo;
}

// The only place that touches the output arrays.
__device__ inline void mom_add(unsigned long long* slot, unsigned long long value) {
    __hip_atomic_fetch_add(slot, value, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The export has checked cap <= kMomMaxCap, row0 + n_rows <= n_a where row_mom is given and col0 + n_cols <= n_b where col_mom is:
// every index lies inside the tile and the arrays of 3 n_a / 3 n_b words -- bounded on the host, and not on the device.
template <bool kRowSide, bool kColSide>
__global__ __launch_bounds__(kMomThreads) void rect_moments_kernel(const TriTile t, unsigned long long* row_mom, int64_t n_a,
                                                                    unsigned long long* col_mom, int64_t n_b, int64_t n_bands, int64_t n_steps) {
    __shared__ MomPart s_part[kMomRows][kMomWaves];
    __shared__ uint8_t s_flag[kMomRows];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int32_t* __restrict__ tile = t.tile;
    const uint8_t* __restrict__ row_empty = t.row_empty;
    const uint8_t* __restrict__ col_empty = t.col_empty;
    const uint32_t cap = (uint32_t)t.cap;
    for (int64_t job = blockIdx.x; job < n_bands * n_steps; job += gridDim.x) {
        const int64_t r_lo = job / n_steps * kMomRows, v0 = job % n_steps * kMomStep;
        const int rows = (int)min((int64_t)kMomRows, t.n_rows - r_lo);
        bool live[kMomPer];                                         // this thread's columns: in the tile and not flagged empty
        uint32_t col_n[kMomPer], col_s1[kMomPer];
        unsigned long long col_s2[kMomPer];
#pragma unroll
        for (int e = 0; e < kMomPer; ++e) {
            const int64_t c = v0 + tid + kMomThreads * e;
            live[e] = c < t.n_cols && !(col_empty && col_empty[c]);
            col_n[e] = 0, col_s1[e] = 0, col_s2[e] = 0;
        }
        __syncthreads();                                            // (the previous job's flush has read s_part, its rows s_flag)
        if (tid < rows) s_flag[tid] = row_empty ? row_empty[r_lo + tid] : (uint8_t)0;
        __syncthreads();
        for (int rl = 0; rl < rows; ++rl) {
            uint32_t wave_n = 0, s1 = 0;                            // (wave_n: the same in every lane, from ballots)
            unsigned long long s2 = 0;
            if (s_flag[rl] == 0) {                                  // (the same for the whole workgroup: a flagged row is not loaded)
                const int32_t* __restrict__ row = tile + (r_lo + rl) * t.ld + v0 + tid;
#pragma unroll
                for (int e = 0; e < kMomPer; ++e) {
                    const uint32_t x = live[e] ? (uint32_t)row[kMomThreads * e] : cap;
                    const bool counts = mom_counts(x, cap);
                    const uint32_t v = counts ? x : 0u;
                    const unsigned long long sq = (unsigned long long)v * v;
                    if (kRowSide) wave_n += (uint32_t)__popcll(__ballot(counts)), s1 += v, s2 += sq;
                    if (kColSide) col_n[e] += counts ? 1u : 0u, col_s1[e] += v, col_s2[e] += sq;
                }
            }
            if (kRowSide) {
                if (wave_n != 0) {                                  // (a wave without a counting entry in this row has nothing to reduce)
#pragma unroll
                    for (int d = 32; d > 0; d >>= 1) {
                        s1 += (uint32_t)__shfl_xor((int)s1, d);
                        s2 += mom_shfl_xor(s2, d);
                    }
                }
                if (lane == 0) s_part[rl][wave] = MomPart{wave_n, s1, s2};
            }
        }
        if (kRowSide) {
            __syncthreads();
            if (tid < rows) {
                unsigned long long n = 0, s1 = 0, s2 = 0;
#pragma unroll
                for (int w = 0; w < kMomWaves; ++w) n += s_part[tid][w].n, s1 += s_part[tid][w].s1, s2 += s_part[tid][w].s2;
                if (n != 0) {
                    const int64_t i = t.row0 + r_lo + tid;
                    mom_add(row_mom + i, n);
                    mom_add(row_mom + (n_a + i), s1);
                    mom_add(row_mom + (2 * n_a + i), s2);
                }
            }
        }
        if (kColSide) {
#pragma unroll
            for (int e = 0; e < kMomPer; ++e) {
                if (col_n[e] == 0) continue;
                const int64_t j = t.col0 + v0 + tid + kMomThreads * e;
                mom_add(col_mom + j, col_n[e]);
                mom_add(col_mom + (n_b + j), col_s1[e]);
                mom_add(col_mom + (2 * n_b + j), col_s2[e]);
            }
        }
    }
}

}  // namespace

namespace dctfp_host {

int rect_moments_max_cap() { return kMomMaxCap; }

void launch_rect_moments(const TriTile& t, uint64_t* row_out, int64_t n_a, uint64_t* col_out, int64_t n_b, hipStream_t stream) {
    const int64_t n_bands = (t.n_rows + kMomRows - 1) / kMomRows, n_steps = (t.n_cols + kMomStep - 1) / kMomStep;
    const dim3 grid((unsigned)min(n_bands * n_steps, (int64_t)kMomMaxBlocks));
    unsigned long long* const rows = reinterpret_cast<unsigned long long*>(row_out);
    unsigned long long* const cols = reinterpret_cast<unsigned long long*>(col_out);
    if (rows && cols)
        hipLaunchKernelGGL((rect_moments_kernel<true, true>), grid, dim3(kMomThreads), 0, stream, t, rows, n_a, cols, n_b, n_bands, n_steps);
    else if (rows)
        hipLaunchKernelGGL((rect_moments_kernel<true, false>), grid, dim3(kMomThreads), 0, stream, t, rows, n_a, cols, n_b, n_bands, n_steps);
    else
        hipLaunchKernelGGL((rect_moments_kernel<false, true>), grid, dim3(kMomThreads), 0, stream, t, rows, n_a, cols, n_b, n_bands, n_steps);
}

}  // namespace dctfp_host
