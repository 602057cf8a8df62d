// The walk over one row of a TriTile (tri_tile.hip.h).  Users: k_filter.hip (count and fill), k_cluster.hip (link), k_greedy.hip
// (mark) and k_tree.hip (nearest).  One workgroup per row at a time, 1024 columns per step, one 16-byte load per thread, and the
// rule that says which of a thread's four entries survive.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "tri_tile.hip.h"

namespace {

using dctfp::TriTile;

constexpr int kFilterThreads = 256;            // one workgroup per row at a time
constexpr int kFilterWaves = kFilterThreads / 64;
constexpr int kFilterStep = kFilterThreads * 4;   // columns per step: one 16-byte load per thread

// Row r of the tile as a walk sees it.  Row r is protein i = row0 + r, column c protein j = col0 + c; only j > i counts: c >= c_min.
// `shift` = the entries between the row's first one and the 16-byte boundary at or below it.
struct TriRow { const int32_t* row; int shift; int64_t c_min; bool empty; };

__device__ inline int64_t first_column(const TriTile& t, int64_t r) { return max((int64_t)0, t.row0 + r + 1 - t.col0); }

__device__ inline TriRow tri_row(const TriTile& t, int64_t r) {
    const int32_t* row = t.tile + r * t.ld;
    return {row, (int)((reinterpret_cast<uintptr_t>(row) >> 2) & 3u), first_column(t, r), t.row_empty && t.row_empty[r]};
}

// The first v0 of a row's step loop: the 16-byte boundary at or below column c_min (`v` is explained at filter_quad).
__device__ inline int64_t tri_begin(const TriRow& w) { return (w.c_min + w.shift) & ~(int64_t)3; }

// The four entries a thread looks at in one step and which of them survive.  `v` counts columns from the 16-byte boundary at
// or below the row's first entry, so that v % 4 == 0 is a 16-byte aligned address: a quad inside the row is one 16-byte load,
// the quads at the row's ends are read entry by entry.  Entry c = v - shift + e survives when c_min <= c < n_cols and
// min(L1, cap) <= bound, an empty protein on either side having key cap.  `n_cols` is the tile's, or less where a kernel narrows
// the row (greedy_tri_mark_kernel's range).  `key` is that min(L1, cap), for the kernels that rank the survivors (k_tree.hip); the
// others never read it and it costs them nothing.
struct Quad {
    bool keep[4];
    int32_t key[4];
};

// (the rule itself, with the pointers as __restrict__ arguments: struct members cannot carry the qualifier, and read through the
// structs every kernel of the family compiles to some 70 instructions more -- profiles/tri_walk/README.md)
__device__ inline Quad quad_of(const int32_t* __restrict__ row, int64_t v, int shift, int64_t c_min, int64_t n_cols, bool row_is_empty,
                               const uint8_t* __restrict__ col_empty, int32_t cap, int32_t bound) {
    Quad q;
    const int64_t c0 = v - shift;
    uint32_t x[4] = {0u, 0u, 0u, 0u};
    if (c0 >= 0 && c0 + 4 <= n_cols) {
        const uint4 w = *reinterpret_cast<const uint4*>(row + c0);
        x[0] = w.x;
        x[1] = w.y;
        x[2] = w.z;
        x[3] = w.w;
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (c0 + e >= 0 && c0 + e < n_cols) x[e] = (uint32_t)row[c0 + e];
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int64_t c = c0 + e;
        const bool inside = c >= c_min && c < n_cols;
        // (a negative value -- no L1 is -- counts as cap, as in select_count_kernel)
        const bool full = row_is_empty || x[e] >= (uint32_t)cap || (inside && col_empty && col_empty[c]);
        const int32_t key = full ? cap : (int32_t)x[e];
        q.keep[e] = inside && key <= bound;
        q.key[e] = key;
    }
    return q;
}

__device__ inline Quad filter_quad(const TriTile& t, const TriRow& w, int64_t v, int64_t n_cols) {
    return quad_of(w.row, v, w.shift, w.c_min, n_cols, w.empty, t.col_empty, t.cap, t.bound);
}

inline unsigned filter_grid(int64_t n_rows) { return (unsigned)min(n_rows, (int64_t)1 << 20); }

}  // namespace
