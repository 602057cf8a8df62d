// The walk over a row of an int32 L1 tile that the kernels of the all-against-all cut-offs share (k_filter.hip: count and fill;
// k_cluster.hip: link; k_greedy.hip: mark; k_tree.hip: nearest): one workgroup per row at a time, 1024 columns per step, one 16-byte load per thread, and the rule that
// says which of a thread's four entries survive.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace {

constexpr int kFilterThreads = 256;            // one workgroup per row at a time
constexpr int kFilterWaves = kFilterThreads / 64;
constexpr int kFilterStep = kFilterThreads * 4;   // columns per step: one 16-byte load per thread

// The four entries a thread looks at in one step and which of them survive.  `v` counts columns from the 16-byte boundary at
// or below the row's first entry (`shift` = entries between the two), so that v % 4 == 0 is a 16-byte aligned address: a quad
// inside the row is one 16-byte load, the quads at the row's ends are read entry by entry.  Entry c survives when
// c_min <= c < n_cols and min(L1, cap) <= bound, an empty protein on either side having key cap.  `key` is that min(L1, cap), for
// the kernels that rank the survivors (k_tree.hip); the others never read it and it costs them nothing.
struct Quad {
    bool keep[4];
    int32_t key[4];
};

__device__ inline Quad filter_quad(const int32_t* __restrict__ row, int64_t v, int shift, int64_t c_min, int64_t n_cols, bool row_is_empty,
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

// Row r of the tile is protein i = row0 + r, column c protein j = col0 + c; only j > i counts: c >= c_min.
__device__ inline int64_t first_column(int64_t row0, int64_t r, int64_t col0) { return max((int64_t)0, row0 + r + 1 - col0); }

__device__ inline int row_shift(const int32_t* row) { return (int)((reinterpret_cast<uintptr_t>(row) >> 2) & 3u); }

inline unsigned filter_grid(int64_t n_rows) { return (unsigned)min(n_rows, (int64_t)1 << 20); }

}  // namespace
