// dct-sim --cluster: single-linkage clusters at a cut-off = the connected components of the pairs that pass it, joined on the
// device in a lock-free union-find over parent[0 .. n_nodes):
//   tri_link_kernel     -- tri_filter_count_kernel's walk over an int32 tile of L1 values; every surviving entry (i, j) is a union;
//   link_pairs_kernel   -- the same union for a list of pairs;
//   rows_link_kernel    -- dct-sim --cluster --level domain: the nodes are fingerprint rows.  sad_tile's 128 x 128 contraction
//                          (sad_tile.hip.h) of two sets of rows; every pair of rows of different proteins within the bound is a union,
//                          straight from the accumulators: no distance is written anywhere;
//   flatten_kernel / labels_kernel -- after all linking, in launches of their own: every node under its root, labels[x] = root.
//
// The forest.  parent[x] <= x at all times; x is a root when parent[x] == x.  A union finds both roots and, if they differ, hooks
// the LARGER under the smaller with a compare-and-swap that expects the larger still to be a root; on failure it goes on from
// the value the CAS returned.  A find replaces parent[x] by an ancestor with an atomic min (path halving), which keeps both the
// invariant and the components.  Roots only ever get smaller parents, so the root of a finished component is its smallest
// member whatever the order in which waves ran: the labels are a property of the graph.
//
// Visibility (eight XCDs with private L2s, a vector L1 per CU that no other CU's store refreshes).  Inside a launch that links,
// EVERY access to parent is an agent-scope relaxed atomic -- load, CAS or min; no plain load or store, nothing through the
// scalar path.  No ordering is needed beyond that: a stale or late view of parent can only show a node as a root that no longer
// is one (parents change only from "self" to a smaller node, or from an ancestor to a further ancestor).  The CAS on such a
// node then fails -- it is decided at the one copy the atomics of all XCDs reach -- and the find continues from what it returned.
// So correctness never rests on when a write becomes visible, only on the atomicity of the hook.  No wave waits for another
// workgroup's progress: a failed CAS means another wave succeeded, and there are no flags, tickets or spin loops.
#define DCTFP_TEMPLATES_ONLY
#include "launch.h"
#include "sad_tile.hip.h"
#include "tri_walk.hip.h"
#include "union_find.hip.h"   // the forest: uf_find / uf_union, kLinkThreads

namespace {

using dctfp::kSadLds;
using dctfp::kSadTile;

// tri_filter_count_kernel's walk (one workgroup per row at a time, 16-byte loads, filter_quad).  Row r is protein i = row0 + r:
// a step without survivors -- the common case -- costs what the count's step costs, the ballots show it and the wave moves on;
// in a step with some, one lane finds i's root (once per step, carried to the next as the place to start from) and only the
// lanes with a surviving entry find j and hook.  The host has checked row0 + n_rows <= n_nodes and col0 + n_cols <= n_nodes.
__global__ __launch_bounds__(kFilterThreads) void tri_link_kernel(const TriTile t, int32_t* parent) {
    const int tid = threadIdx.x, lane = tid & 63;
    for (int64_t r = blockIdx.x; r < t.n_rows; r += gridDim.x) {
        const TriRow w = tri_row(t, r);
        int32_t above = (int32_t)(t.row0 + r);   // i, or an ancestor of i (wave-uniform)
        for (int64_t v0 = tri_begin(w); v0 < t.n_cols + w.shift; v0 += kFilterStep) {
            const int64_t v = v0 + 4 * tid;
            const Quad q = filter_quad(t, w, v, t.n_cols);
            if (__ballot(q.keep[0] || q.keep[1] || q.keep[2] || q.keep[3]) == 0) continue;
            int32_t root = 0;
            if (lane == 0) root = uf_find(parent, above);
            above = __shfl(root, 0);
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (q.keep[e]) uf_union(parent, above, (int32_t)(t.col0 + v - w.shift + e));
        }
    }
}

// The same union for pair n = (pi[n], pj[n]); a pair with an index outside [0, n_nodes) is skipped, as pair_lines_kernel skips it.
__global__ __launch_bounds__(kLinkThreads) void link_pairs_kernel(const int32_t* __restrict__ pi, const int32_t* __restrict__ pj, int64_t n_pairs,
                                                                  int32_t* parent, int64_t n_nodes) {
    const int64_t n = (int64_t)blockIdx.x * kLinkThreads + threadIdx.x;
    if (n >= n_pairs) return;
    const int64_t i = pi[n], j = pj[n];
    if (i < 0 || i >= n_nodes || j < 0 || j >= n_nodes || i == j) return;
    uf_union(parent, (int32_t)i, (int32_t)j);
}

// dct-sim --cluster --level domain.  Row r of a is node a0 + r, row c of b node b0 + c; one workgroup per 128 x 128 block of the
// pairs, left out before any load when it lies wholly on or left of the diagonal (its last column's node <= its first row's).
// The contraction is sad_tile's (sad_tile.hip.h); ALIGN = dctfp::sad_tile_align() of the rows, the fill it takes.
// The epilogue: a thread's 64 sums against the bound as a 64-bit mask (sad_keep_mask: bit 8 i + j, rows and columns beyond the sets
// masked out) and a wave-wide ballot, which in the common case shows no survivor anywhere.  Else the lanes with a bit walk theirs:
// node a < node b, owner[a] != owner[b] (rows of one protein never join), neither skipped, then uf_union.  The host has checked
// a0 + na <= n_nodes and b0 + nb <= n_nodes; owner and skip have n_nodes entries.
template <int ALIGN>
__global__ __launch_bounds__(256, 4) void rows_link_kernel(const int8_t* __restrict__ a, int64_t na, int64_t lda, int64_t a0,
                                                           const int8_t* __restrict__ b, int64_t nb, int64_t ldb, int64_t b0, int d,
                                                           const int32_t* __restrict__ owner, const uint8_t* __restrict__ skip, uint32_t cap,
                                                           uint32_t bound, int32_t* parent) {
    const int64_t r0 = (int64_t)blockIdx.y * kSadTile, c0 = (int64_t)blockIdx.x * kSadTile;
    const int rows_a = (int)min((int64_t)kSadTile, na - r0), rows_b = (int)min((int64_t)kSadTile, nb - c0);
    if (b0 + c0 + rows_b - 1 <= a0 + r0) return;   // (the whole workgroup: no pair of the block has node a < node b)
    __shared__ uint32_t sa[kSadLds];
    __shared__ uint32_t sb[kSadLds];
    const int ty = threadIdx.x >> 4, tx = threadIdx.x & 15;
    uint32_t acc[8][8] = {};
    dctfp::sad_tile<ALIGN>(a + r0 * lda, rows_a, lda, b + c0 * ldb, rows_b, ldb, d, sa, sb, acc);
    uint64_t keep = dctfp::sad_keep_mask(acc, cap, bound, rows_a, rows_b);
    if (__ballot(keep != 0) == 0) return;
    const int64_t node_a = a0 + r0 + ty * 8, node_b = b0 + c0 + tx * 8;
    while (keep) {
        const int bit = __builtin_ctzll(keep);
        keep &= keep - 1;
        const int64_t x = node_a + (bit >> 3), y = node_b + (bit & 7);
        if (x >= y || owner[x] == owner[y]) continue;
        if (skip && (skip[x] | skip[y])) continue;
        uf_union(parent, (int32_t)x, (int32_t)y);
    }
}

// After all linking, first launch: every node directly under its root.  Other threads shorten the same paths meanwhile, so
// parent is read and written as in the links (agent-scope atomics); no root changes in this launch, so the root found is final.
// Halving by every thread at once keeps the walk short whatever depth the forest came with.
__global__ __launch_bounds__(kLinkThreads) void flatten_kernel(int32_t* parent, int64_t n_nodes) {
    const int64_t x = (int64_t)blockIdx.x * kLinkThreads + threadIdx.x;
    if (x >= n_nodes) return;
    const int32_t root = uf_find(parent, (int32_t)x);
    if (root != (int32_t)x) __hip_atomic_fetch_min(parent + x, root, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Second launch: labels[x] = root of x.  This launch only reads parent (the kernel boundary separates it from every write), so
// plain loads will do; after flatten_kernel the walk is one step.
__global__ __launch_bounds__(kLinkThreads) void labels_kernel(const int32_t* __restrict__ parent, int64_t n_nodes, int32_t* __restrict__ labels) {
    const int64_t x = (int64_t)blockIdx.x * kLinkThreads + threadIdx.x;
    if (x >= n_nodes) return;
    int32_t r = (int32_t)x;
    for (;;) {
        const int32_t p = parent[r];
        if ((uint32_t)p >= (uint32_t)r) break;
        r = p;
    }
    labels[x] = r;
}

unsigned link_grid(int64_t n) { return (unsigned)((n + kLinkThreads - 1) / kLinkThreads); }

}  // namespace

namespace dctfp_host {

void launch_tri_link(const TriTile& t, int32_t* parent, hipStream_t stream) {
    hipLaunchKernelGGL(tri_link_kernel, dim3(filter_grid(t.n_rows)), dim3(kFilterThreads), 0, stream, t, parent);
}

void launch_link_pairs(const int32_t* pi, const int32_t* pj, int64_t n_pairs, int32_t* parent, int64_t n_nodes, hipStream_t stream) {
    hipLaunchKernelGGL(link_pairs_kernel, dim3(link_grid(n_pairs)), dim3(kLinkThreads), 0, stream, pi, pj, n_pairs, parent, n_nodes);
}

void launch_rows_link(const int8_t* a, int64_t na, int64_t lda, int64_t a0, const int8_t* b, int64_t nb, int64_t ldb, int64_t b0, int d,
                      const int32_t* owner, const uint8_t* skip, int32_t cap, int32_t bound, int32_t* parent, hipStream_t stream) {
    const dim3 grid((unsigned)((nb + kSadTile - 1) / kSadTile), (unsigned)((na + kSadTile - 1) / kSadTile));
    const int align = sad_tile_align(a, lda, b, ldb);
    auto* const kernel = align == 16 ? rows_link_kernel<16> : align == 4 ? rows_link_kernel<4> : rows_link_kernel<1>;
    hipLaunchKernelGGL(kernel, grid, dim3(256), 0, stream, a, na, lda, a0, b, nb, ldb, b0, d, owner, skip, (uint32_t)cap, (uint32_t)bound, parent);
}

void launch_cluster_labels(int32_t* parent, int64_t n_nodes, int32_t* labels, hipStream_t stream) {
    hipLaunchKernelGGL(flatten_kernel, dim3(link_grid(n_nodes)), dim3(kLinkThreads), 0, stream, parent, n_nodes);
    hipLaunchKernelGGL(labels_kernel, dim3(link_grid(n_nodes)), dim3(kLinkThreads), 0, stream, parent, n_nodes, labels);
}

}  // namespace dctfp_host

