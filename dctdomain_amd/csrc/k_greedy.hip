// dct-sim --cluster --linkage greedy: greedy incremental clusters at a cut-off (CD-HIT's rule in file order).  The representatives
// are the lexicographically first maximal independent set of the graph whose edges are the pairs that pass the cut-offs; every
// other protein gets the lowest representative it has an edge to.  Three int32 per node:
//   assign[x]   the lowest representative seen so far with an edge to x (kGreedyNone: none yet); a representative's own index;
//   state[x]    kUndecided / kMember / kNewRep (decided by the latest decide over x's range) / kDoneRep;
//   blocked[x]  a round number: "an earlier undecided node of the range has an edge to x" as of the mark launch before that round.
// The caller takes the nodes in ranges [i0, i1) in ascending order (the stripes of the tiles, or the row ranges of a pair list):
// when a range starts, every representative below i0 has marked all its columns.  Then rounds, one launch each:
//   greedy_decide_kernel    -- one thread per node of the range.  An undecided node becomes a member if assign is set, a new
//                              representative (assign = own index) if no stamp of this round sits on it, else it stays and is counted;
//   greedy_tri_mark_kernel  -- tri_link_kernel's walk.  A row that is a new representative walks all its columns and lowers
//                              assign[j] to its index at every surviving entry; a row still undecided walks the columns inside the
//                              range and stamps blocked[j] with the next round; any other row costs one read of its state;
//   greedy_pairs_mark_kernel-- the same for a list of pairs, one thread per pair.
// The smallest undecided node of a range never carries a stamp, so every round decides something.
//
// Ordering comes from kernel boundaries only: a launch reads plain only what earlier launches wrote.  Inside a mark launch
// assign is touched by agent-scope relaxed atomic minima and by nothing else, blocked is write-only (every writer stores the
// same value) and state is read-only; the decide launch touches only the words of its own node.  No wave waits for another
// workgroup: no flags, tickets or spin loops.  The result is the minimum over a set of representatives that the graph alone
// fixes, whatever the order in which waves ran.
#define DCTFP_TEMPLATES_ONLY
#include "launch.h"
#include "tri_walk.hip.h"

namespace {

constexpr int kGreedyThreads = 256;
constexpr int32_t kGreedyNone = 0x7fffffff;
enum : int32_t { kUndecided = 0, kMember = 1, kNewRep = 2, kDoneRep = 3 };

__device__ inline void lower(int32_t* assign, int64_t j, int32_t i) {
    __hip_atomic_fetch_min(assign + j, i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// round 0 is the cover pass a range starts with: nothing becomes a representative, a node an earlier range's representative
// has marked becomes a member (so that the first mark launch need not walk its row).  *undecided grows by the nodes left over.
__global__ __launch_bounds__(kGreedyThreads) void greedy_decide_kernel(int32_t* __restrict__ assign, int32_t* __restrict__ state,
                                                                       const int32_t* __restrict__ blocked, int64_t i0, int64_t i1, int32_t round,
                                                                       unsigned long long* undecided) {
    const int64_t x = i0 + (int64_t)blockIdx.x * kGreedyThreads + threadIdx.x;
    bool left = false;
    if (x < i1) {
        const int32_t s = state[x];
        if (s == kNewRep) {
            state[x] = kDoneRep;                              // (it marked in the launch before this one)
        } else if (s == kUndecided) {
            if (assign[x] != kGreedyNone) {
                state[x] = kMember;
            } else if (round != 0 && blocked[x] != round) {
                assign[x] = (int32_t)x;
                state[x] = kNewRep;
            } else {
                left = true;
            }
        }
    }
    const unsigned long long wave = __ballot(left);
    if ((threadIdx.x & 63) == 0 && wave != 0) atomicAdd(undecided, (unsigned long long)__popcll(wave));
}

// Row r is protein i = row0 + r.  `range_end` = i1 of the range the rows belong to: an undecided row looks at columns j < i1
// only (a node beyond the range is decided in a later range, after every representative of this one has marked).  The host
// has checked row0 + n_rows <= n_nodes and col0 + n_cols <= n_nodes.
__global__ __launch_bounds__(kFilterThreads) void greedy_tri_mark_kernel(const TriTile t, int32_t* assign, const int32_t* __restrict__ state,
                                                                         int32_t* blocked, int64_t range_end, int32_t next_round) {
    const int tid = threadIdx.x;
    for (int64_t r = blockIdx.x; r < t.n_rows; r += gridDim.x) {
        const int64_t i = t.row0 + r;
        const int32_t s = state[i];
        if (s != kNewRep && s != kUndecided) continue;
        const bool marks = s == kNewRep;
        const int64_t cols = marks ? t.n_cols : min(t.n_cols, max((int64_t)0, range_end - t.col0));
        const TriRow w = tri_row(t, r);
        for (int64_t v0 = tri_begin(w); v0 < cols + w.shift; v0 += kFilterStep) {
            const int64_t v = v0 + 4 * tid;
            const Quad q = filter_quad(t, w, v, cols);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if (!q.keep[e]) continue;
                const int64_t j = t.col0 + v - w.shift + e;
                if (marks) lower(assign, j, (int32_t)i);
                else blocked[j] = next_round;
            }
        }
    }
}

// Pair n = (pi[n], pj[n]) taken as the edge (lo, hi) of its two ends; a pair with an index outside [0, n_nodes) or with both
// ends equal is skipped, as link_pairs_kernel skips it.  The caller hands in the pairs whose lower end lies in the range.
__global__ __launch_bounds__(kGreedyThreads) void greedy_pairs_mark_kernel(const int32_t* __restrict__ pi, const int32_t* __restrict__ pj, int64_t n_pairs,
                                                                           int32_t* assign, const int32_t* __restrict__ state, int32_t* blocked,
                                                                           int64_t n_nodes, int64_t range_end, int32_t next_round) {
    const int64_t n = (int64_t)blockIdx.x * kGreedyThreads + threadIdx.x;
    if (n >= n_pairs) return;
    const int64_t a = pi[n], b = pj[n];
    if (a < 0 || a >= n_nodes || b < 0 || b >= n_nodes || a == b) return;
    const int64_t lo = min(a, b), hi = max(a, b);
    const int32_t s = state[lo];
    if (s == kNewRep) lower(assign, hi, (int32_t)lo);
    else if (s == kUndecided && hi < range_end) blocked[hi] = next_round;
}

unsigned greedy_grid(int64_t n) { return (unsigned)((n + kGreedyThreads - 1) / kGreedyThreads); }

}  // namespace

namespace dctfp_host {

void launch_greedy_decide(int32_t* assign, int32_t* state, const int32_t* blocked, int64_t i0, int64_t i1, int32_t round,
                          unsigned long long* undecided, hipStream_t stream) {
    hipLaunchKernelGGL(greedy_decide_kernel, dim3(greedy_grid(i1 - i0)), dim3(kGreedyThreads), 0, stream, assign, state, blocked, i0, i1, round,
                       undecided);
}

void launch_greedy_tri_mark(const TriTile& t, int32_t* assign, const int32_t* state, int32_t* blocked, int64_t range_end, int32_t next_round,
                            hipStream_t stream) {
    hipLaunchKernelGGL(greedy_tri_mark_kernel, dim3(filter_grid(t.n_rows)), dim3(kFilterThreads), 0, stream, t, assign, state, blocked, range_end,
                       next_round);
}

void launch_greedy_pairs_mark(const int32_t* pi, const int32_t* pj, int64_t n_pairs, int32_t* assign, const int32_t* state, int32_t* blocked,
                              int64_t n_nodes, int64_t range_end, int32_t next_round, hipStream_t stream) {
    hipLaunchKernelGGL(greedy_pairs_mark_kernel, dim3(greedy_grid(n_pairs)), dim3(kGreedyThreads), 0, stream, pi, pj, n_pairs, assign, state,
                       blocked, n_nodes, range_end, next_round);
}

}  // namespace dctfp_host
