// python -m dctdomain_amd.cluster_quality: the sums behind the silhouette of a clustering.  Entry (r, c) of an int32 tile is the L1 of
// proteins i = row0 + r and j = col0 + c of ONE file, the columns being the whole file; beside the tile, cid[j] = the dense id of j's
// cluster if that has two or more members (numbered by first member, with size[] and first[] per id), -1 for a singleton.
//   silhouette_rows_kernel -- per row i: own_sum[i] = Sa, the summed key over the other members of i's cluster; and the neighbour
//                             cluster B of i, the other cluster that minimises S(B) / |B| (S = the summed key over its members), as
//                             near_sum[i] = S(B), near_size[i] = |B|, near_first[i] = its first member (-1: there is no other cluster).
// The key of an entry is the tile scans' (hist_key of k_hist.hip, restated: the unit includes neither walk header): cap for a flagged
// row or column, cap for a negative value or one >= cap, the value otherwise.  i == j never counts, whatever the diagonal holds.
//
// NOT a pass of band_walk, and on the full square, not the triangle: on the triangle pair (i, j) is seen once and has to reach
// S[i][cluster of j] and S[j][cluster of i] -- an n x C accumulator in device memory and a global atomic per entry wherever
// neighbouring columns differ in cluster.  With full rows a row's sums live and die in the LDS of the one workgroup that owns the row.
//
// The row.  One workgroup of kSilThreads (256) threads per row, rows gridDim.x apart beyond the grid.  The cluster ids go in passes of
// K (the launch's pass_clusters, at most kSilMaxPass = 4096): pass p owns the ids [p K, (p + 1) K) and K 64-bit sums in LDS, zeroed at
// its start.  The threads read the row with coalesced dword loads (tid, tid + 256, ..., kSilDepth of them in flight: a lane past
// the row's end reads its last entry instead, so no load sits behind a branch) and cid and the column flag of the same columns.
//   - A column of a multi-member cluster of the pass adds its key to that cluster's sum: a workgroup-scope 64-bit LDS atomic add
//     (64 bits: one cluster of more than 252 645 members at key 17000 leaves 32).  The wave combines first (wave_add): the lanes that
//     share the leading lane's cluster add once, their keys summed with shuffles, when they are a quarter of the wave or more -- a few
//     giant clusters, the common case, would otherwise put 64 adds on one LDS word, one after the other --, the other lanes add
//     their own (profiles/silhouette/README.md has what either costs on one, contiguous, interleaved and paired clusters).
//   - A singleton column (cid < 0) needs no sum: its mean is its key.  It goes into the thread's running minimum of (key, j), in the
//     first pass only; n / 2 singletons cost no LDS slot and no pass.
// Behind the row's last column a barrier, then thread t scans the sums t, t + 256, ... of the pass: the row's own cluster is Sa, every
// other one a candidate (S, size, first) against the best the thread has seen, which it carries across the passes in registers.
// After the last pass the thread's singleton minimum joins as the candidate (key, 1, j), the workgroup reduces the candidates with
// shuffles and one LDS round, and thread 0 writes the row's four words with plain vector stores.
//
// The comparison.  (S1, n1, f1) is before (S2, n2, f2) when S1 n2 < S2 n1, or the products are equal and f1 < f2: the exact
// fractions, ties to the cluster whose first member comes first in the file.  S < 2^22 x 2^31 = 2^53 and n < 2^31, so a product needs up to
// 84 bits: __umul64hi and the low product, compared as a pair.  Two clusters never share a first member, so the order is total and
// the result does not depend on which thread saw which candidate, on the pass length or on the order of the reduction.
//
// Synchronisation.  A workgroup owns its row and the four words it writes: no global atomic, no flag, nothing another workgroup
// waits for or reads in the launch, nothing through the scalar path.  cid, size, first and the flags were written by earlier
// launches (or copies) on the stream and are only read.  Inside the workgroup the LDS sums are ordered by the barriers of the pass:
// zero | add | scan.
#define DCTFP_TEMPLATES_ONLY
#include "launch.h"
#include "tri_tile.hip.h"

#ifndef DCTFP_SIL_SHARED_ADD
#define DCTFP_SIL_SHARED_ADD 1      // (an A/B build may let every lane add its own key: profiles/silhouette/README.md)
#endif

namespace {

using dctfp::TriTile;

constexpr bool kSilSharedAdd = DCTFP_SIL_SHARED_ADD != 0;
constexpr int kSilShareFrom = 16;                       // lanes on one cluster from which the wave adds their keys up first
constexpr int kSilThreads = 256;
constexpr int kSilWaves = kSilThreads / 64;
constexpr int kSilDepth = 4;                            // columns of a thread whose loads are in flight together
constexpr int kSilStep = kSilThreads * kSilDepth;       // columns of one step along the row
constexpr int kSilMaxPass = 4096;                       // 64-bit sums of a pass in LDS: 32 KiB, two workgroups to a CU
constexpr int kSilMaxCap = 1 << 22;                     // the largest key: 2^31 of them stay below 2^53
constexpr unsigned kSilMaxBlocks = 1u << 20;            // rows beyond that many are taken gridDim.x apart

static_assert((int64_t)64 * kSilMaxCap < ((int64_t)1 << 32), "a wave's shared sum of one step of the row fits 32 bits");
static_assert((size_t)kSilMaxPass * sizeof(unsigned long long) <= 32 * 1024, "the sums of a pass are at most 32 KiB of LDS");

// A candidate for the neighbour cluster: the summed key over its members, their number and the first of them; first < 0 = none.
struct SilCand {
    unsigned long long sum;
    uint32_t size;
    int32_t first;
};

// The key of the entry with value x under the tile's rule: min(L1, cap), cap for a flagged row or column and for a negative value.
__device__ inline uint32_t sil_key(uint32_t x, bool flagged, uint32_t cap) { return flagged || x >= cap ? cap : x; }

// Is a before b: a.sum / a.size < b.sum / b.size as exact fractions, ties to the lower first member; none is before nothing.
__device__ inline bool sil_before(const SilCand& a, const SilCand& b) {
    if (a.first < 0) return false;
    if (b.first < 0) return true;
    const unsigned long long l_hi = __umul64hi(a.sum, (unsigned long long)b.size), l_lo = a.sum * b.size;
    const unsigned long long r_hi = __umul64hi(b.sum, (unsigned long long)a.size), r_lo = b.sum * a.size;
    if (l_hi != r_hi) return l_hi < r_hi;
    if (l_lo != r_lo) return l_lo < r_lo;
    return a.first < b.first;
}

__device__ inline SilCand sil_shfl_xor(const SilCand& c, int d) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)c.sum, d), hi = (uint32_t)__shfl_xor((int)(uint32_t)(c.sum >> 32), d);
    return SilCand{(unsigned long long)hi << 32 | lo, (uint32_t)__shfl_xor((int)c.size, d), __shfl_xor(c.first, d)};
}

// One wave's entries of one step into the sums of the pass: slot < 0 = the lane's entry is of no cluster of the pass.  The lanes that
// share the first adding lane's slot are one add of their summed keys, if they are kSilShareFrom or more; the others add their own.
__device__ inline void wave_add(unsigned long long* s_sum, int slot, uint32_t key) {
    const unsigned long long live = __ballot(slot >= 0);
    if (live == 0) return;                                          // (the wave has nothing for this pass in this step)
    const int lead = __builtin_amdgcn_readlane(slot, __ffsll(live) - 1);
    const bool shares = kSilSharedAdd && slot == lead;
    const unsigned long long same = __ballot(shares);
    // (the sum over the sharing lanes costs six shuffles whoever shares: measured, about what a third of a wave's adds on one word
    // cost -- below kSilShareFrom sharing lanes every lane adds its own; `same` is the same in every lane, so the wave does not diverge)
    if (!kSilSharedAdd || __popcll(same) < kSilShareFrom) {
        if (slot >= 0) __hip_atomic_fetch_add(s_sum + slot, (unsigned long long)key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        return;
    }
    uint32_t shared = shares ? key : 0u;
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) shared += (uint32_t)__shfl_xor((int)shared, d);
    if (shares) {
        if ((int)(threadIdx.x & 63) == __ffsll(same) - 1)
            __hip_atomic_fetch_add(s_sum + lead, (unsigned long long)shared, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    } else if (slot >= 0) {
        __hip_atomic_fetch_add(s_sum + slot, (unsigned long long)key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
}

// The export has checked that every row0 + r and col0 + c lies inside the arrays of n_nodes entries, that cap <= kSilMaxCap and that
// 1 <= pass <= kSilMaxPass; the caller vouches for -1 <= cid < n_clusters: bounded on the host, and not on the device.  Dynamic LDS:
// pass 64-bit words.
__global__ __launch_bounds__(kSilThreads) void silhouette_rows_kernel(const TriTile t, const int32_t* __restrict__ cid,
                                                                       const int32_t* __restrict__ size, const int32_t* __restrict__ first,
                                                                       int32_t n_clusters, int32_t pass, unsigned long long* own_sum,
                                                                       unsigned long long* near_sum, int32_t* near_size, int32_t* near_first) {
    extern __shared__ unsigned long long s_sum[];
    __shared__ SilCand s_best[kSilWaves];
    __shared__ unsigned long long s_own;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int32_t* __restrict__ tile = t.tile;
    const uint8_t* __restrict__ row_empty = t.row_empty;
    const uint8_t* __restrict__ col_empty = t.col_empty;
    const uint32_t cap = (uint32_t)t.cap;
    const int n_passes = n_clusters > 0 ? (n_clusters + pass - 1) / pass : 1;       // (a row of singletons alone still is read once)
    for (int64_t r = blockIdx.x; r < t.n_rows; r += gridDim.x) {
        const int64_t i = t.row0 + r;
        const int32_t own = cid[i];
        const bool row_full = row_empty && row_empty[r];
        const int32_t* __restrict__ row = tile + r * t.ld;
        SilCand best{0, 0, -1};                                     // of the multi-member clusters this thread has scanned
        uint32_t lone_key = 0;                                      // the thread's smallest (key, j) over its singleton columns
        int32_t lone = -1;
        if (tid == 0) s_own = 0;                                    // (read by thread 0 alone, behind the barriers of the last pass)
        for (int p = 0; p < n_passes; ++p) {
            const int32_t c_lo = p * pass, c_n = min(pass, n_clusters - c_lo);      // (c_n <= 0: no cluster at all)
            __syncthreads();                                        // (the scan of the pass before has read s_sum)
            for (int k = tid; k < c_n; k += kSilThreads) s_sum[k] = 0;
            __syncthreads();
            for (int64_t v0 = 0; v0 < t.n_cols; v0 += kSilStep) {
                uint32_t x[kSilDepth];
                int32_t cj[kSilDepth];
                bool full[kSilDepth];
#pragma unroll
                for (int e = 0; e < kSilDepth; ++e) {               // (the loads of kSilDepth columns first: none behind a branch)
                    const int64_t c = min(v0 + tid + kSilThreads * e, t.n_cols - 1);
                    x[e] = (uint32_t)row[c];
                    cj[e] = cid[t.col0 + c];
                    full[e] = col_empty && col_empty[c];
                }
#pragma unroll
                for (int e = 0; e < kSilDepth; ++e) {
                    const int64_t c = v0 + tid + kSilThreads * e, j = t.col0 + c;
                    const bool counts = c < t.n_cols && j != i;
                    const uint32_t key = sil_key(x[e], row_full || full[e], cap);
                    if (counts && cj[e] < 0 && p == 0 && (lone < 0 || key < lone_key)) lone_key = key, lone = (int32_t)j;   // (j ascends: ties keep the lower)
                    const int32_t slot = cj[e] - c_lo;
                    wave_add(s_sum, counts && cj[e] >= 0 && slot >= 0 && slot < c_n ? slot : -1, key);
                }
            }
            __syncthreads();
            for (int k = tid; k < c_n; k += kSilThreads) {
                const int32_t g = c_lo + k;
                if (g == own) {
                    s_own = s_sum[k];
                    continue;
                }
                const SilCand cand{s_sum[k], (uint32_t)size[g], first[g]};
                if (sil_before(cand, best)) best = cand;
            }
        }
        if (lone >= 0) {
            const SilCand cand{lone_key, 1u, lone};
            if (sil_before(cand, best)) best = cand;
        }
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) {
            const SilCand other = sil_shfl_xor(best, d);
            if (sil_before(other, best)) best = other;
        }
        if (lane == 0) s_best[wave] = best;
        __syncthreads();
        if (tid == 0) {
#pragma unroll
            for (int w = 1; w < kSilWaves; ++w)
                if (sil_before(s_best[w], best)) best = s_best[w];
            own_sum[i] = s_own;
            near_sum[i] = best.first < 0 ? 0ull : best.sum;
            near_size[i] = best.first < 0 ? 0 : (int32_t)best.size;
            near_first[i] = best.first;
        }
        __syncthreads();                                            // (thread 0 has read s_best and s_own before the next row writes them)
    }
}

}  // namespace

namespace dctfp_host {

int silhouette_max_cap() { return kSilMaxCap; }
int silhouette_max_pass() { return kSilMaxPass; }

void launch_silhouette_rows(const TriTile& t, const int32_t* cid, const int32_t* size, const int32_t* first, int32_t n_clusters,
                            int32_t pass_clusters, uint64_t* own_sum, uint64_t* near_sum, int32_t* near_size, int32_t* near_first,
                            hipStream_t stream) {
    const dim3 grid((unsigned)min(t.n_rows, (int64_t)kSilMaxBlocks));
    // (no more words than the clusters there are: a launch for a dozen clusters declares a dozen sums)
    const size_t lds = (size_t)max(1, min(pass_clusters, n_clusters)) * sizeof(unsigned long long);
    hipLaunchKernelGGL(silhouette_rows_kernel, grid, dim3(kSilThreads), lds, stream, t, cid, size, first, n_clusters, pass_clusters,
                       reinterpret_cast<unsigned long long*>(own_sum), reinterpret_cast<unsigned long long*>(near_sum), near_size, near_first);
}

}  // namespace dctfp_host
