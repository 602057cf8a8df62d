// dct-sim --hist: the distribution of one score over all pairs of ONE file, binned on the device.  Entry (r, c) of an int32 tile is the
// L1 of proteins i = row0 + r and j = col0 + c; an entry COUNTS exactly when tri_degree_kernel would count it: j > i and
// key = min(L1, cap) <= bound, cap for a protein flagged empty on either side (a negative value counts as cap too).
//   tri_hist_kernel -- every counted entry adds 1 to hist[cls * (cap + 1) + key]; cls = 0 without fam (one class), else
//                      cls = (fam[i] != fam[j]): row 0 = the pairs of one family, row 1 = the pairs of two.  The caller zeroes hist
//                      before the first tile; the counts add up over tiles and over calls.
//
// NOT a pass of band_walk, and with a loop of its own over the TriTile: a pass reduces a job onto one word per row and one per column
// and sends those to per-protein arrays; here the output is ONE array for the whole grid, indexed by the entry's key, so there is no
// row part and no column part to join -- what a workgroup keeps between jobs is a whole histogram in LDS.  The unit takes the tile's
// description (tri_tile.hip.h) and nothing else of the walks.
//
// The job.  A workgroup of kHistThreads (1024) threads takes a job of kHistRows (64) rows x kHistCols (1024) columns at a time,
// gridDim.x apart; thread t reads column v0 + t of every row with plain dword loads -- coalesced, and free of any alignment rule: any
// ld, any column view of a wider tensor -- kHistDepth (8) rows at a time: the loads carry no branch (a lane off the tile's edge reads
// the edge's entry instead), so all eight of a thread are in flight before the first is waited for.  A job wholly on or left of the
// diagonal is left before it loads anything.  fam and the flags are loaded once per column and job (the thread's own column) and
// once per row and job (lane l of every wave holds row l's, the row loop reads them with a read-lane), never per entry: the row
// loop has no memory access but the tile's.
//
// The counters.  s_bins = classes x (bound + 1) 32-bit counters in LDS -- only the bins 0 .. bound can be hit --, private to the
// workgroup, zeroed at its start, added to with workgroup-scope LDS atomics over ALL its jobs and sent out once, at its end: every
// non-zero bin is one 64-bit __hip_atomic_fetch_add (relaxed, agent scope) on hist, consecutive threads on consecutive words.
// Inside a launch hist is touched by nothing else: no plain load, no plain store, nothing through the scalar path.  An add is decided
// at the one copy the atomics of all eight XCDs reach and nobody reads the result before the launch has ended; integer addition
// commutes and is associative, so the counts are sums over a set the inputs alone fix and depend neither on the order in which
// workgroups ran, nor on how the caller cut the triangle into tiles, nor on the order of its calls.  No workgroup waits for another.
//
// Why a 32-bit counter in LDS cannot overflow.  Between its start and its one flush a workgroup adds at most one per entry of its
// jobs: jobs x kHistRows x kHistCols.  launch_tri_hist gives a launch at most blocks x kHistJobsPerBlock jobs (a taller tile goes out
// as several launches, one range of bands each), the jobs are dealt gridDim.x apart, so a workgroup takes at most kHistJobsPerBlock
// = 2^15 of them: 2^15 x 2^16 = 2^31 entries < 2^32 (the static_assert below).
//
// Occupancy.  Two classes at bound 16999 are 136 KB of LDS: one workgroup per CU, which is why the workgroup is 1024 threads -- 16
// waves per CU, eight loads each in flight; one class is 68 KB and two workgroups fit.  The layout fixes the largest cap: two classes
// of cap + 1 counters within the 160 KiB a single workgroup may declare, kHistMaxCap = 20479.  The grid is one workgroup per CU and
// class row that fits beside it (256 / 512), not one per job: every workgroup flushes up to classes x (bound + 1) words, and more
// workgroups are that many more global atomics for the same tile.
//
// Hot bins.  Scores of unrelated proteins crowd into a narrow range of keys and a tile of one family can be a single key; lanes of a
// wave that add to one LDS counter are served one after the other.  So the wave combines before it adds (wave_count): the lanes
// whose bin equals the first counting lane's are one add of their number by that lane -- a wave of one key costs one LDS atomic, not
// 64 -- and the other lanes add 1 each.  profiles/hist/README.md has what this costs on spread, crowded and equal keys.
#define DCTFP_TEMPLATES_ONLY
#include "launch.h"
#include "tri_tile.hip.h"

namespace {

using dctfp::TriTile;

constexpr int kHistThreads = 1024;
constexpr int kHistCols = kHistThreads;             // columns of a job: one per thread
constexpr int kHistRows = 64;                       // rows of a job
constexpr int kHistDepth = 8;                       // rows whose loads a thread has in flight
constexpr int64_t kHistJobsPerBlock = 1 << 15;      // jobs of one workgroup between its start and its flush, at most
constexpr size_t kHistLdsBytes = 160 * 1024;        // what a single workgroup may declare
constexpr int kHistMaxCap = (int)(kHistLdsBytes / (2 * sizeof(uint32_t))) - 1;   // two classes of cap + 1 counters
constexpr int kHistBlocksPerClassRow = 256;         // one workgroup per CU and class row that fits in its LDS

static_assert(kHistJobsPerBlock * kHistRows * kHistCols < ((int64_t)1 << 32), "a workgroup's 32-bit counters hold its share of the entries");
static_assert(kHistRows % kHistDepth == 0, "the rows of a job are taken kHistDepth at a time");
static_assert(kHistRows == 64, "lane l of a wave holds the flag and the family of row l of the job");

// The key of the entry with value x under the tile's rule: min(L1, cap), cap for a flagged row or column and for a negative value.
__device__ inline uint32_t hist_key(uint32_t x, bool flagged, uint32_t cap) { return flagged || x >= cap ? cap : x; }

// One wave's entries of one row into the workgroup's counters: bin < 0 = the lane's entry does not count.  The lanes that share the
// first counting lane's bin are one add of their number; the others add 1 each.
__device__ inline void wave_count(uint32_t* s_bins, int bin) {
    const unsigned long long live = __ballot(bin >= 0);
    if (live == 0) return;                                          // (the wave has nothing in this row)
    const int lead = __builtin_amdgcn_readlane(bin, __ffsll(live) - 1);
    const unsigned long long same = __ballot(bin == lead);
    if (bin == lead) {
        if ((int)(threadIdx.x & 63) == __ffsll(same) - 1)
            __hip_atomic_fetch_add(s_bins + lead, (uint32_t)__popcll(same), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    } else if (bin >= 0) {
        __hip_atomic_fetch_add(s_bins + bin, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
}

// The only place that touches the output array.
__device__ inline void add_bin(unsigned long long* slot, uint32_t count) {
    __hip_atomic_fetch_add(slot, (unsigned long long)count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The export has checked that every row0 + r and col0 + c lies inside fam, that bound <= cap <= kHistMaxCap and that the launch holds
// at most gridDim.x * kHistJobsPerBlock jobs: bounded on the host, and not on the device.  Dynamic LDS: classes * (bound + 1) words.
__global__ __launch_bounds__(kHistThreads) void tri_hist_kernel(const TriTile t, const int32_t* __restrict__ fam, unsigned long long* bins_out,
                                                                 int64_t n_bands, int64_t n_steps) {
    extern __shared__ uint32_t s_bins[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int32_t* __restrict__ tile = t.tile;
    const uint8_t* __restrict__ row_empty = t.row_empty;
    const uint8_t* __restrict__ col_empty = t.col_empty;
    const uint32_t cap = (uint32_t)t.cap;
    const int32_t bound = t.bound;
    const int width = bound + 1, n_bins = (fam ? 2 : 1) * width;
    for (int b = tid; b < n_bins; b += kHistThreads) s_bins[b] = 0;
    __syncthreads();
    for (int64_t job = blockIdx.x; job < n_bands * n_steps; job += gridDim.x) {
        const int64_t r_lo = job / n_steps * kHistRows, v0 = job % n_steps * kHistCols;
        const int rows = (int)min((int64_t)kHistRows, t.n_rows - r_lo);
        const int64_t i_lo = t.row0 + r_lo, j_lo = t.col0 + v0;
        if (j_lo + min((int64_t)kHistCols, t.n_cols - v0) - 1 <= i_lo) continue;      // (no entry of the job has j > i)
        const int64_t c = v0 + tid, j = j_lo + tid;
        const bool inside = c < t.n_cols;
        const bool col_full = inside && col_empty && col_empty[c];
        const int32_t col_fam = inside && fam ? fam[j] : 0;
        // the rows' side values, once per job: lane l of every wave holds those of row l, the row loop reads them from there
        const bool lane_row = lane < rows;
        const unsigned long long rows_full = __ballot(lane_row && row_empty && row_empty[r_lo + lane]);
        const int32_t lane_fam = lane_row && fam ? fam[i_lo + lane] : 0;
        // (a thread beyond the last column reads the last column, a row beyond the last row of the job its last row: every load
        // is of an entry of the tile, so none needs a branch around it and kHistDepth of them are in flight before the first wait)
        const int32_t* __restrict__ column = tile + r_lo * t.ld + (inside ? c : t.n_cols - 1);
        for (int rl = 0; rl < rows; rl += kHistDepth) {
            uint32_t x[kHistDepth];
#pragma unroll
            for (int u = 0; u < kHistDepth; ++u)                    // (the loads of kHistDepth rows first)
                x[u] = (uint32_t)column[(int64_t)min(rl + u, rows - 1) * t.ld];
#pragma unroll
            for (int u = 0; u < kHistDepth; ++u) {
                if (rl + u >= rows) break;                          // (the same for the whole workgroup)
                const bool row_full = rows_full >> (rl + u) & 1;
                const int32_t row_fam = __builtin_amdgcn_readlane(lane_fam, rl + u);
                const uint32_t key = hist_key(x[u], row_full || col_full, cap);
                const bool counts = inside && j > i_lo + rl + u && (int32_t)key <= bound;
                wave_count(s_bins, counts ? (row_fam != col_fam ? width : 0) + (int)key : -1);
            }
        }
    }
    __syncthreads();
    for (int b = tid; b < n_bins; b += kHistThreads) {
        const uint32_t count = s_bins[b];
        if (count != 0) add_bin(bins_out + (b < width ? b : (int64_t)cap + 1 + (b - width)), count);
    }
}

}  // namespace

namespace dctfp_host {

int tri_hist_max_cap() { return kHistMaxCap; }

int launch_tri_hist(const TriTile& t, const int32_t* fam, uint64_t* hist, hipStream_t stream, LaunchError* err) {
    if (t.bound < 0) return 0;                                      // (no key is within the bound)
    const size_t lds = (size_t)(fam ? 2 : 1) * ((size_t)t.bound + 1) * sizeof(uint32_t);
    static bool raised = false;
    if (!raised) {                                                  // (dynamic LDS above 64 KB has to be asked for, once per kernel)
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&tri_hist_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                                 (int)kHistLdsBytes);
        if (e != hipSuccess) return launch_fail(err, DCTFP_ERR_HIP, "hipFuncSetAttribute(tri_hist_kernel): %s", hipGetErrorString(e));
        raised = true;
    }
    // as many workgroups as fit the CUs beside each other (one class row of 17000 bins: two per CU), never more than jobs
    const int64_t most = (int64_t)kHistBlocksPerClassRow * (lds * 2 <= kHistLdsBytes ? 2 : 1);
    const int64_t n_bands = (t.n_rows + kHistRows - 1) / kHistRows, n_steps = (t.n_cols + kHistCols - 1) / kHistCols;
    // a launch takes a range of bands of at most most * kHistJobsPerBlock jobs (n_steps <= 2^21: at least four bands)
    const int64_t bands_per_launch = max((int64_t)1, most * kHistJobsPerBlock / n_steps);
    for (int64_t b0 = 0; b0 < n_bands; b0 += bands_per_launch) {
        const int64_t bands = min(bands_per_launch, n_bands - b0), r0 = b0 * kHistRows;
        TriTile part = t;
        part.tile = t.tile + r0 * t.ld;
        part.n_rows = min(bands * kHistRows, t.n_rows - r0);
        part.row0 = t.row0 + r0;
        part.row_empty = t.row_empty ? t.row_empty + r0 : nullptr;
        hipLaunchKernelGGL(tri_hist_kernel, dim3((unsigned)min(bands * n_steps, most)), dim3(kHistThreads), lds, stream, part, fam,
                           reinterpret_cast<unsigned long long*>(hist), bands, n_steps);
    }
    return 0;
}

}  // namespace dctfp_host
