// dct-sim --tree: the single-linkage tree of a file = the minimum spanning forest of the complete graph on its proteins under
// the strict edge order (key, i, j), key = min(L1, cap) <= bound, i < j -- Boruvka's algorithm over the implicit graph, in rounds:
//   tri_nearest_kernel -- tri_link_kernel's view of an int32 tile of L1 values (filter_quad); every surviving entry (i, j) whose
//                         ends lie in different components is a candidate for the lightest outgoing edge of BOTH components;
//   tree_hook_kernel   -- after all tiles of the round, in a launch of its own: every component appends its lightest outgoing edge
//                         to the edge list and joins its two ends in the union-find forest of k_cluster.hip.
// The host then takes the new labels (cluster_labels) and runs the next round, until a round appends nothing.
//
// State.  comp[x] (int32) = this round's label of node x = the smallest member of its component; best[c] (uint64, indexed by
// label) = the lightest outgoing edge of component c seen so far, packed key << 48 | i << 24 | j (key <= 32767, i < j < 2^24), so
// that unsigned 64-bit order is the edge order; all ones = none.  parent = the forest of k_cluster.hip.
//
// Visibility (eight XCDs with private L2s; the header of k_cluster.hip has the argument).  comp is written by an earlier launch
// and only read here: plain loads.  Inside tri_nearest_kernel best is touched by agent-scope relaxed atomics alone -- a load that
// skips a minimum which would change nothing, then the minimum.  best[c] only ever decreases within a round, so a stale value
// read by that load costs one redundant atomic and never a wrong result; the minimum itself is decided at the one copy the
// atomics of all XCDs reach.  The result is a minimum over a set the inputs alone fix: it does not depend on the order in which
// workgroups ran or on how the caller cut the triangle into tiles.  tree_hook_kernel reads best with plain loads (a launch of
// its own, after the tiles) and writes none of it -- the reset to "none" is a fill the launcher puts behind it on the stream, so
// that no thread reads another component's entry while its owner clears it.  No wave waits for another workgroup: no flags, no
// tickets, no spin loops.
//
// Atomics per tile.  A workgroup takes a band of kTreeBand rows x kFilterStep (1024) columns.  Row side: a row's survivors are
// reduced in the wave (shuffles) and across the four waves in LDS; one global minimum per (row, workgroup) at most.  Column side:
// an LDS minimum per column over the band's rows, then one global minimum per (column, workgroup) at most.  So a tile of
// R x C entries costs at most R ceil((C + 3) / 1024) + (C + 3) ceil(R / 64) global atomics -- under 2 % of its entries, and far
// fewer once best has settled (the load in front).
//
// No cycles.  The hooks of a round never close a cycle, because the order is strict: let components C1 -> C2 -> ... -> Ck -> C1
// each have chosen the edge e_t that leads to the next.  e_t also leaves C_(t+1), whose choice e_(t+1) is its lightest: e_(t+1)
// <= e_t.  Around the cycle all are equal, and equal keys are the same edge (i, j): k = 2 and both components chose one edge.
// That edge is appended once: the component with the higher label skips it when best of the other holds the identical key.
#define DCTFP_TEMPLATES_ONLY
#include "launch.h"
#include "tri_walk.hip.h"
#include "union_find.hip.h"   // the forest of k_cluster.hip: uf_union, kLinkThreads

namespace {

constexpr int kTreeBand = 64;                      // rows of a workgroup's band (6 bits of a column's packed minimum)
constexpr int kTreeCols = kFilterStep + 3;         // columns a band's step can touch: the rows' 16-byte shifts differ by up to 3
constexpr uint32_t kNone32 = 0xffffffffu;
constexpr unsigned long long kNoEdge = ~0ull;

__device__ inline unsigned long long pack_edge(int32_t key, int64_t i, int64_t j) {
    return (unsigned long long)(uint32_t)key << 48 | (unsigned long long)i << 24 | (unsigned long long)j;
}

// best[c] = min(best[c], edge): the minimum only when the value seen (possibly stale, never too small) does not rule it out.
__device__ inline void lower_best(unsigned long long* best, int32_t c, int64_t n_nodes, unsigned long long edge) {
    if ((uint32_t)c >= (uint64_t)n_nodes) return;   // (a label outside the nodes: the caller's comp is no labelling)
    if (__hip_atomic_load(best + c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) <= edge) return;
    __hip_atomic_fetch_min(best + c, edge, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// One workgroup per (band of kTreeBand rows, step of kFilterStep columns) at a time.  As in tri_link_kernel, `v` counts a row's
// columns from the 16-byte boundary at or below its first entry, so the columns of step v0 are v0 - shift .. v0 + 1023 - shift with
// the row's own shift: LDS slot s stands for column v0 - 3 + s.  s_comp = comp of those columns, s_col = their minimum over the
// band as key << 8 | row within the band, s_row = the rows' minimum over the step as key << 11 | slot -- both orders are the edge
// order restricted to one column / one row.  The host has checked row0 + n_rows <= n_nodes and col0 + n_cols <= n_nodes.
__global__ __launch_bounds__(kFilterThreads) void tri_nearest_kernel(const TriTile t, const int32_t* __restrict__ comp, unsigned long long* best,
                                                                      int64_t n_nodes, int64_t n_bands, int64_t n_steps) {
    __shared__ int32_t s_comp[kTreeCols];
    __shared__ uint32_t s_col[kTreeCols];
    __shared__ uint32_t s_row[kTreeBand];
    const int tid = threadIdx.x, lane = tid & 63;
    for (int64_t job = blockIdx.x; job < n_bands * n_steps; job += gridDim.x) {
        const int64_t r_lo = job / n_steps * kTreeBand, v0 = job % n_steps * kFilterStep;
        const int rows = (int)min((int64_t)kTreeBand, t.n_rows - r_lo);
        if (v0 + kFilterStep <= first_column(t, r_lo)) continue;   // (the whole step lies on or left of the diagonal)
        const int64_t c_lo = v0 - 3;                                        // column of slot 0
        __syncthreads();                                                    // (the previous job's flush has read the arrays)
        for (int s = tid; s < kTreeCols; s += kFilterThreads) {
            const int64_t c = c_lo + s;
            s_comp[s] = c >= 0 && c < t.n_cols ? comp[t.col0 + c] : -1;
            s_col[s] = kNone32;
        }
        if (tid < kTreeBand) s_row[tid] = kNone32;
        __syncthreads();
        for (int rl = 0; rl < rows; ++rl) {
            const int64_t r = r_lo + rl;
            if (v0 + kFilterStep <= first_column(t, r)) continue;
            const TriRow w = tri_row(t, r);
            const int32_t comp_i = comp[t.row0 + r];
            const Quad q = filter_quad(t, w, v0 + 4 * tid, t.n_cols);
            const int slot0 = 4 * tid + 3 - w.shift;                          // slot of the quad's first column v - shift
            uint32_t mine = kNone32;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if (!q.keep[e] || s_comp[slot0 + e] == comp_i) continue;
                mine = min(mine, (uint32_t)q.key[e] << 11 | (uint32_t)(slot0 + e));
                atomicMin(&s_col[slot0 + e], (uint32_t)q.key[e] << 8 | (uint32_t)rl);
            }
            if (__ballot(mine != kNone32) == 0) continue;
#pragma unroll
            for (int d = 32; d > 0; d >>= 1) mine = min(mine, (uint32_t)__shfl_xor((int)mine, d));
            if (lane == 0) atomicMin(&s_row[rl], mine);
        }
        __syncthreads();
        if (tid < rows && s_row[tid] != kNone32) {
            const int64_t i = t.row0 + r_lo + tid, j = t.col0 + c_lo + (s_row[tid] & 0x7ff);
            lower_best(best, comp[i], n_nodes, pack_edge((int32_t)(s_row[tid] >> 11), i, j));
        }
        for (int s = tid; s < kTreeCols; s += kFilterThreads)
            if (s_col[s] != kNone32) {
                const int64_t i = t.row0 + r_lo + (s_col[s] & 0xff), j = t.col0 + c_lo + s;
                lower_best(best, s_comp[s], n_nodes, pack_edge((int32_t)(s_col[s] >> 8), i, j));
            }
    }
}

// One thread per node c.  A root of this round's labelling whose component has an outgoing edge appends it at the slot an
// atomic counter hands out -- unless the other end's component, of a lower label, holds the identical edge and appends it
// itself -- and joins the two ends.  Nothing is written at or beyond max_edges (the host sizes the arrays to n - 1, which a
// forest cannot exceed); an entry of best that names no edge of c (no i < j < n_nodes with one end in c) is skipped.
__global__ __launch_bounds__(kLinkThreads) void tree_hook_kernel(const int32_t* __restrict__ comp, const unsigned long long* __restrict__ best,
                                                                 int32_t* parent, int64_t n_nodes, int32_t* __restrict__ edge_i,
                                                                 int32_t* __restrict__ edge_j, int32_t* __restrict__ edge_key, int32_t* counter,
                                                                 int64_t max_edges) {
    const int64_t c = (int64_t)blockIdx.x * kLinkThreads + threadIdx.x;
    if (c >= n_nodes || comp[c] != (int32_t)c) return;
    const unsigned long long e = best[c];
    if (e == kNoEdge) return;
    const int64_t i = (int64_t)(e >> 24 & 0xffffff), j = (int64_t)(e & 0xffffff);
    if (i >= j || j >= n_nodes) return;
    const int32_t ci = comp[i], cj = comp[j];
    if (ci == cj || (ci != (int32_t)c && cj != (int32_t)c)) return;
    const int32_t other = ci == (int32_t)c ? cj : ci;
    if ((uint32_t)other < (uint32_t)c && best[other] == e) return;          // (chosen from both sides: the lower label appends)
    const int32_t slot = __hip_atomic_fetch_add(counter, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (slot >= 0 && slot < max_edges) {
        edge_i[slot] = (int32_t)i;
        edge_j[slot] = (int32_t)j;
        edge_key[slot] = (int32_t)(e >> 48);
    }
    uf_union(parent, (int32_t)i, (int32_t)j);
}

}  // namespace

namespace dctfp_host {

void launch_tri_nearest(const TriTile& t, const int32_t* comp, uint64_t* best, int64_t n_nodes, hipStream_t stream) {
    const int64_t n_bands = (t.n_rows + kTreeBand - 1) / kTreeBand, n_steps = (t.n_cols + 3 + kFilterStep - 1) / kFilterStep;
    hipLaunchKernelGGL(tri_nearest_kernel, dim3(filter_grid(n_bands * n_steps)), dim3(kFilterThreads), 0, stream, t, comp,
                       reinterpret_cast<unsigned long long*>(best), n_nodes, n_bands, n_steps);
}

hipError_t launch_tree_hook(const int32_t* comp, uint64_t* best, int32_t* parent, int64_t n_nodes, int32_t* edge_i, int32_t* edge_j,
                            int32_t* edge_key, int32_t* counter, int64_t max_edges, hipStream_t stream) {
    hipLaunchKernelGGL(tree_hook_kernel, dim3((unsigned)((n_nodes + kLinkThreads - 1) / kLinkThreads)), dim3(kLinkThreads), 0, stream, comp,
                       reinterpret_cast<const unsigned long long*>(best), parent, n_nodes, edge_i, edge_j, edge_key, counter, max_edges);
    return hipMemsetAsync(best, 0xff, (size_t)n_nodes * sizeof(uint64_t), stream);   // every entry back to "none", behind the hooks
}

}  // namespace dctfp_host
