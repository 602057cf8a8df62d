// dct-sim --domain-map: every matched fingerprint pair behind a result line, not only the best one:
//   pair_row_best_kernel  -- per protein pair, for EVERY fingerprint row of either protein the nearest row of the other protein
//                            (its L1 and its index): pair_min_kernel's contraction, walked twice with the roles swapped;
//   pair_map_lines_kernel -- pair_lines_kernel<true>'s line with one more field, the map of the rows within a bound:
//                            "{id_i} {id_j} {a} {b} {label_a} {label_b} {side}/{side}\n", side = "-" or the entries
//                            "{label}={label of the counterpart}:{score}" of the matched rows in row order, joined by ";".
//                            <false> writes every line's byte length, <true> the text at the caller's prefix sum of those
//                            lengths (tri_filter_count / tri_filter_fill's idiom): both run one body, so a length cannot
//                            disagree with the text.
// No LDS, no atomics; every store is checked against the caller's buffer sizes.
#define DCTFP_TEMPLATES_ONLY
#include "launch.h"

namespace {

constexpr int kPairWaves = 4;                  // protein pairs per workgroup (one wave each), as pair_min_kernel
constexpr int kLineLanes = 16;                 // lanes per result line, as pair_lines_kernel
constexpr int kLineThreads = 256;
constexpr int kScoreRows = 17002;
constexpr uint32_t kFlip = 0x80808080u;        // signed -> unsigned order, |x - y| unchanged

__device__ inline uint32_t bytes4(const int8_t* p, int d, int k, bool aligned) {
    const int byte0 = 4 * k, valid = min(4, d - byte0);
    return (aligned && valid == 4) ? *reinterpret_cast<const uint32_t*>(p + byte0) : dctfp::load_bytes4(p + byte0, valid);
}

__device__ inline uint32_t wave_sum(uint32_t s) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    return s;
}

// One side of a pair: for every row i of x[x0, x1) the smallest L1 to the rows of y[y0, y1) and the row (counted from y0) it
// was found at, to out_l1[i - x0] / out_arg[i - x0]; 0x7fffffff and -1 where y has no rows.  pair_min_kernel's loop: the x row in
// two registers per lane and four y rows in flight for rows of up to 512 bytes, the general loop above.  After wave_sum every
// lane holds the sum, so the comparison is wave-uniform; it is made in ascending order of the y row with `<`: among equal L1
// values the lowest row stands, whatever the unroll.
template <bool ALIGNED>
__device__ __forceinline__ void row_best_side(const int8_t* __restrict__ x, int64_t ldx, int64_t x0, int64_t x1, const int8_t* __restrict__ y,
                                              int64_t ldy, int64_t y0, int64_t y1, int d, int lane, int32_t* __restrict__ out_l1,
                                              int32_t* __restrict__ out_arg) {
    const int nd = (d + 3) / 4;
    const bool has0 = lane < nd, has1 = lane + 64 < nd;
    for (int64_t i = x0; i < x1; ++i) {
        const int8_t* rx = x + i * ldx;
        int32_t mn = 0x7fffffff, arg = -1;
        if (nd <= 128) {
            const uint32_t vx0 = has0 ? bytes4(rx, d, lane, ALIGNED) ^ kFlip : 0u;
            const uint32_t vx1 = has1 ? bytes4(rx, d, lane + 64, ALIGNED) ^ kFlip : 0u;
            for (int64_t j = y0; j < y1; j += 4) {
                uint32_t s[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    s[u] = 0;
                    if (j + u < y1) {
                        const int8_t* ry = y + (j + u) * ldy;
                        if (has0) s[u] = dctfp::sad_dword(vx0, bytes4(ry, d, lane, ALIGNED) ^ kFlip, s[u]);
                        if (has1) s[u] = dctfp::sad_dword(vx1, bytes4(ry, d, lane + 64, ALIGNED) ^ kFlip, s[u]);
                    }
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) s[u] = wave_sum(s[u]);
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    if (j + u < y1 && (int32_t)s[u] < mn) {
                        mn = (int32_t)s[u];
                        arg = (int32_t)(j + u - y0);
                    }
            }
        } else {
            for (int64_t j = y0; j < y1; ++j) {
                const int8_t* ry = y + j * ldy;
                uint32_t s = 0;
                for (int k = lane; k < nd; k += 64) s = dctfp::sad_dword(bytes4(rx, d, k, ALIGNED) ^ kFlip, bytes4(ry, d, k, ALIGNED) ^ kFlip, s);
                const int32_t v = (int32_t)wave_sum(s);
                if (v < mn) {
                    mn = v;
                    arg = (int32_t)(j - y0);
                }
            }
        }
        if (lane == 0) {
            out_l1[i - x0] = mn;
            out_arg[i - x0] = arg;
        }
    }
}

// One wave per protein pair (pa, pb) with k and m fingerprint rows: the results lie at [row_off[p], row_off[p + 1]) of out_l1 /
// out_arg, first the k rows of pa against pb, then the m rows of pb against pa.  A pair with an index outside the files, a range
// whose width is not k + m or that is not within [0, out_len] writes nothing.
template <bool ALIGNED>
__global__ __launch_bounds__(kPairWaves * 64) void pair_row_best_kernel(const int32_t* __restrict__ pairs, int64_t n_pairs,
                                                                        const int8_t* __restrict__ a, int64_t lda, const int64_t* __restrict__ idx_a,
                                                                        int64_t npa, const int8_t* __restrict__ b, int64_t ldb,
                                                                        const int64_t* __restrict__ idx_b, int64_t npb, int d,
                                                                        const int64_t* __restrict__ row_off, int64_t out_len,
                                                                        int32_t* __restrict__ out_l1, int32_t* __restrict__ out_arg) {
    const int lane = threadIdx.x & 63;
    const int64_t p = (int64_t)blockIdx.x * kPairWaves + (threadIdx.x >> 6);
    if (p >= n_pairs) return;
    const int32_t pa = pairs[2 * p], pb = pairs[2 * p + 1];
    if (pa < 0 || pa >= npa || pb < 0 || pb >= npb) return;
    const int64_t a0 = idx_a[pa], a1 = idx_a[pa + 1], b0 = idx_b[pb], b1 = idx_b[pb + 1];
    const int64_t at = row_off[p], end = row_off[p + 1];
    if (at < 0 || end > out_len || end - at != (a1 - a0) + (b1 - b0)) return;
    for (int side = 0; side < 2; ++side) {   // (the pair is walked twice with the roles swapped: one body, not two inlined copies)
        const bool first = side == 0;
        const int64_t to = first ? at : at + (a1 - a0);
        row_best_side<ALIGNED>(first ? a : b, first ? lda : ldb, first ? a0 : b0, first ? a1 : b1, first ? b : a, first ? ldb : lda,
                               first ? b0 : a0, first ? b1 : a1, d, lane, out_l1 + to, out_arg + to);
    }
}

// What pair_map_lines_kernel reads, beyond the line's own (i, j, mn, last, la, lb).
struct MapText {
    const uint8_t* __restrict__ ids;
    const int64_t* __restrict__ id_off;
    int64_t n_ids;
    const uint8_t* __restrict__ labels;
    const int64_t* __restrict__ label_off;
    int64_t n_labels;
    const char* __restrict__ table;
    const int64_t* __restrict__ first_row;   // (n_ids + 1): protein p's rows are the labels first_row[p] .. first_row[p + 1] - 1
    const int64_t* __restrict__ row_off;     // pair_row_best_kernel's
    int64_t n_rows;                          // the entries of row_l1 / row_arg
    const int32_t* __restrict__ row_l1;
    const int32_t* __restrict__ row_arg;
    int32_t bound;
};

// `len` bytes from src to dst + at, if WRITE; at + len.  (One lane writes a whole piece: the pieces of a line go round the lanes.)
template <bool WRITE>
__device__ inline int64_t put(uint8_t* __restrict__ dst, int64_t at, const uint8_t* __restrict__ src, int64_t len, bool mine) {
    if constexpr (WRITE)
        if (mine)
            for (int64_t o = 0; o < len; ++o) dst[at + o] = src[o];
    return at + len;
}

template <bool WRITE>
__device__ inline int64_t put1(uint8_t* __restrict__ dst, int64_t at, uint8_t ch, bool mine) {
    if constexpr (WRITE)
        if (mine) dst[at] = ch;
    return at + 1;
}

// One side of the map from byte `at` of the line: the matched rows (L1 <= bound) of the k rows of protein `self` (labels from
// self0, results from r0) against the m rows of `other`, "-" if none.  Every lane walks all rows and so knows where every entry
// starts; entry number e is written by lane e % 16.  Returns the byte after the side, -1 for a counterpart or a label out of range.
template <bool WRITE>
__device__ inline int64_t map_side(const MapText& t, uint8_t* __restrict__ dst, int64_t at, int64_t self0, int64_t k, int64_t other0, int64_t m,
                                   int64_t r0, int sub) {
    int64_t entries = 0;
    for (int64_t r = 0; r < k; ++r) {
        const int32_t l1 = t.row_l1[r0 + r], arg = t.row_arg[r0 + r];
        if (l1 < 0 || l1 > t.bound) continue;
        if (arg < 0 || arg >= m) return -1;
        const int64_t x = self0 + r, y = other0 + arg;
        if (x < 0 || x >= t.n_labels || y < 0 || y >= t.n_labels) return -1;
        const bool mine = (int)(entries % kLineLanes) == sub;
        if (entries) at = put1<WRITE>(dst, at, ';', mine);
        at = put<WRITE>(dst, at, t.labels + t.label_off[x], t.label_off[x + 1] - t.label_off[x], mine);
        at = put1<WRITE>(dst, at, '=', mine);
        at = put<WRITE>(dst, at, t.labels + t.label_off[y], t.label_off[y + 1] - t.label_off[y], mine);
        at = put1<WRITE>(dst, at, ':', mine);
        at = put<WRITE>(dst, at, reinterpret_cast<const uint8_t*>(t.table) + 5 * (int64_t)min((uint32_t)l1, (uint32_t)(kScoreRows - 1)), 5, mine);
        ++entries;
    }
    if (entries == 0) at = put1<WRITE>(dst, at, '-', sub == 0);
    return at;
}

// The map field and the newline of line (i, j), results at [r0, r0 + k + m), from byte `at`: " {side}/{side}\n".  Returns the byte
// after the line, -1 as map_side.
template <bool WRITE>
__device__ inline int64_t map_tail(const MapText& t, uint8_t* __restrict__ dst, int64_t at, int64_t i, int64_t j, int64_t r0, int sub) {
    const int64_t i0 = t.first_row[i], k = t.first_row[i + 1] - i0, j0 = t.first_row[j], m = t.first_row[j + 1] - j0;
    at = put1<WRITE>(dst, at, ' ', sub == 0);
    at = map_side<WRITE>(t, dst, at, i0, k, j0, m, r0, sub);
    if (at < 0) return -1;
    at = put1<WRITE>(dst, at, '/', sub == 0);
    at = map_side<WRITE>(t, dst, at, j0, m, i0, k, r0 + k, sub);
    if (at < 0) return -1;
    return put1<WRITE>(dst, at, '\n', sub == 0);
}

// Sixteen lanes per line, byte stores, any id or label length.  FILL = false: out_count[n] = the bytes of line n, 0 for a line that
// would not be written; nothing else is stored.  FILL = true: the line from byte line_off[n] of out.  A line with a protein or
// label index out of range, results that are not k + m entries within [0, n_rows], or an end beyond out_bytes is not written.
template <bool FILL>
__global__ __launch_bounds__(kLineThreads) void pair_map_lines_kernel(int64_t n_lines, const int32_t* __restrict__ pi, const int32_t* __restrict__ pj,
                                                                      const int32_t* __restrict__ mn, const int32_t* __restrict__ last,
                                                                      const int32_t* __restrict__ la, const int32_t* __restrict__ lb, const MapText t,
                                                                      const int64_t* __restrict__ line_off, uint8_t* __restrict__ out,
                                                                      int64_t out_bytes, int64_t* __restrict__ out_count) {
    const int64_t g = (int64_t)blockIdx.x * kLineThreads + threadIdx.x;
    const int64_t n = g / kLineLanes;
    const int sub = (int)(g % kLineLanes);
    if (n >= n_lines) return;
    int64_t total = 0;   // (the line's length; 0 = not written)
    const int64_t i = pi[n], j = pj[n], x = la[n], y = lb[n];
    int64_t len_i = 0, len_j = 0, len_x = 0, len_y = 0, r0 = 0, head = 0;
    if (i >= 0 && i < t.n_ids && j >= 0 && j < t.n_ids && x >= 0 && x < t.n_labels && y >= 0 && y < t.n_labels) {
        r0 = t.row_off[n];
        const int64_t rows = (t.first_row[i + 1] - t.first_row[i]) + (t.first_row[j + 1] - t.first_row[j]);
        if (r0 >= 0 && t.row_off[n + 1] <= t.n_rows && t.row_off[n + 1] - r0 == rows) {
            len_i = t.id_off[i + 1] - t.id_off[i], len_j = t.id_off[j + 1] - t.id_off[j];
            len_x = t.label_off[x + 1] - t.label_off[x], len_y = t.label_off[y + 1] - t.label_off[y];
            head = len_i + len_j + 14 + len_x + len_y + 1;   // (pair_lines_kernel<true>'s line without its newline)
            total = max(map_tail<false>(t, nullptr, head, i, j, r0, sub), (int64_t)0);
        }
    }
    if constexpr (!FILL) {
        if (sub == 0) out_count[n] = total;
        return;
    } else {
        const int64_t at = line_off[n];
        if (total == 0 || at < 0 || at + total > out_bytes) return;
        const int64_t off_i = t.id_off[i], off_j = t.id_off[j], off_x = t.label_off[x], off_y = t.label_off[y];
        const char* __restrict__ ta = t.table + 5 * (int64_t)min((uint32_t)mn[n], (uint32_t)(kScoreRows - 1));
        const char* __restrict__ tb = t.table + 5 * (int64_t)(kScoreRows + min((uint32_t)last[n], (uint32_t)(kScoreRows - 1)));
        const int64_t tail0 = len_i + 1 + len_j;   // " a.aaa b.bbb", then " {label_a} {label_b}"
        const int64_t x0 = tail0 + 13, y0 = x0 + len_x + 1;
        for (int64_t o = sub; o < head; o += kLineLanes) {
            uint8_t ch;
            if (o < len_i) ch = t.ids[off_i + o];
            else if (o == len_i) ch = ' ';
            else if (o < tail0) ch = t.ids[off_j + (o - len_i - 1)];
            else if (o < x0 - 1) {
                const int k = (int)(o - tail0);
                ch = k == 0 || k == 6 ? (uint8_t)' ' : k < 6 ? (uint8_t)ta[k - 1] : (uint8_t)tb[k - 7];
            } else if (o < x0) ch = ' ';
            else if (o < y0 - 1) ch = t.labels[off_x + (o - x0)];
            else if (o < y0) ch = ' ';
            else ch = t.labels[off_y + (o - y0)];
            out[at + o] = ch;
        }
        map_tail<true>(t, out + at, head, i, j, r0, sub);
    }
}

}  // namespace

namespace dctfp_host {

void launch_pair_row_best(const int32_t* pairs, int64_t n_pairs, const int8_t* a, int64_t lda, const int64_t* idx_a, int64_t npa,
                          const int8_t* b, int64_t ldb, const int64_t* idx_b, int64_t npb, int d, const int64_t* row_off, int64_t out_len,
                          int32_t* out_l1, int32_t* out_arg, hipStream_t stream) {
    const bool aligned = ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | (uintptr_t)lda | (uintptr_t)ldb) & 3u) == 0;
    const dim3 grid((unsigned)((n_pairs + kPairWaves - 1) / kPairWaves));
    if (aligned)
        hipLaunchKernelGGL((pair_row_best_kernel<true>), grid, dim3(kPairWaves * 64), 0, stream, pairs, n_pairs, a, lda, idx_a, npa, b, ldb, idx_b,
                           npb, d, row_off, out_len, out_l1, out_arg);
    else
        hipLaunchKernelGGL((pair_row_best_kernel<false>), grid, dim3(kPairWaves * 64), 0, stream, pairs, n_pairs, a, lda, idx_a, npa, b, ldb, idx_b,
                           npb, d, row_off, out_len, out_l1, out_arg);
}

void launch_pair_map_lines(int64_t n_lines, const int32_t* pi, const int32_t* pj, const int32_t* mn, const int32_t* last, const int32_t* la,
                           const int32_t* lb, const uint8_t* ids, const int64_t* id_off, int64_t n_ids, const uint8_t* labels,
                           const int64_t* label_off, int64_t n_labels, const char* table, const int64_t* first_row, const int64_t* row_off,
                           int64_t n_rows, const int32_t* row_l1, const int32_t* row_arg, int32_t bound, const int64_t* line_off, uint8_t* out,
                           int64_t out_bytes, int64_t* out_count, hipStream_t stream) {
    const MapText t{ids, id_off, n_ids, labels, label_off, n_labels, table, first_row, row_off, n_rows, row_l1, row_arg, bound};
    const int64_t threads = n_lines * kLineLanes;
    const dim3 grid((unsigned)((threads + kLineThreads - 1) / kLineThreads));
    if (out_count)
        hipLaunchKernelGGL((pair_map_lines_kernel<false>), grid, dim3(kLineThreads), 0, stream, n_lines, pi, pj, mn, last, la, lb, t, line_off, out,
                           out_bytes, out_count);
    else
        hipLaunchKernelGGL((pair_map_lines_kernel<true>), grid, dim3(kLineThreads), 0, stream, n_lines, pi, pj, mn, last, la, lb, t, line_off, out,
                           out_bytes, out_count);
}

}  // namespace dctfp_host
