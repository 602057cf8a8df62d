// dct-sim all-against-all with score cut-offs (--min-domain / --min-global): the pairs of the upper triangle that pass a
// cut-off, selected on the device in output order, and the result lines of those pairs only:
//   tri_filter_count_kernel -- per row of an int32 tile of L1 values: #(entries right of the diagonal with key <= bound);
//   tri_filter_fill_kernel  -- those entries' (i, j), compacted in column order at the caller's prefix sum of the counts;
//   pair_lines_kernel       -- "{id_i} {id_j} {a} {b}\n" for a list of pairs at caller-computed offsets (sim_lines_kernel's text,
//                              without its closed form for the dense row); <LABELS = true>: the same lines with the labels of
//                              DCTdomain's fingerprint pair behind the scores (--domains).
// No global atomic decides a position: a row's survivors go out in column order within one workgroup, rows at their offsets.
#define DCTFP_TEMPLATES_ONLY
#include "launch.h"
#include "tri_walk.hip.h"   // TriTile, the row walk and filter_quad

namespace {

constexpr int kLineLanes = 16;                 // lanes per result line
constexpr int kLineThreads = 256;
constexpr int kScoreRows = 17002;

// out_count[r] = #survivors of row r.  One workgroup per row (rows loop over the grid), 1024 columns per step, a ballot and a
// population count per entry of the quad, the waves' sums through LDS.
__global__ __launch_bounds__(kFilterThreads) void tri_filter_count_kernel(const TriTile t, int32_t* __restrict__ out_count) {
    __shared__ int32_t wsum[kFilterWaves];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int64_t r = blockIdx.x; r < t.n_rows; r += gridDim.x) {
        const TriRow w = tri_row(t, r);
        int32_t n = 0;   // (wave-uniform)
        for (int64_t v0 = tri_begin(w); v0 < t.n_cols + w.shift; v0 += kFilterStep) {
            const Quad q = filter_quad(t, w, v0 + 4 * tid, t.n_cols);
#pragma unroll
            for (int e = 0; e < 4; ++e) n += __popcll(__ballot(q.keep[e]));
        }
        if (lane == 0) wsum[wave] = n;
        __syncthreads();
        if (tid == 0) {
            int32_t s = 0;
            for (int k = 0; k < kFilterWaves; ++k) s += wsum[k];
            out_count[r] = s;
        }
        __syncthreads();   // (wsum is rewritten for the next row)
    }
}

// The survivors of row r, in column order, to out_i / out_j [offsets[r], offsets[r + 1]) as global protein indices.  Same walk
// as the count; a thread's place within a step = the survivors of the lanes below it (ballots) + of the waves below it (LDS,
// double buffered: one barrier per step) + of its own earlier entries.  Nothing is written at or beyond out_len, nor beyond
// the row's range.
__global__ __launch_bounds__(kFilterThreads) void tri_filter_fill_kernel(const TriTile t, const int64_t* __restrict__ offsets, int64_t out_len,
                                                                          int32_t* __restrict__ out_i, int32_t* __restrict__ out_j) {
    __shared__ int32_t wtot[2][kFilterWaves];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned long long below = (1ull << lane) - 1;
    int64_t step = 0;   // (over all rows of this workgroup: the LDS buffers alternate)
    for (int64_t r = blockIdx.x; r < t.n_rows; r += gridDim.x) {
        const TriRow w = tri_row(t, r);
        const int64_t base = offsets[r], len = min(offsets[r + 1], out_len) - base;
        int64_t done = 0;
        for (int64_t v0 = tri_begin(w); v0 < t.n_cols + w.shift && done < len; v0 += kFilterStep, ++step) {
            const int64_t v = v0 + 4 * tid;
            const Quad q = filter_quad(t, w, v, t.n_cols);
            int32_t before = 0, mine = 0;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const unsigned long long b = __ballot(q.keep[e]);
                before += __popcll(b & below);
                mine += __popcll(b);
            }
            const int buf = (int)(step & 1);
            if (lane == 0) wtot[buf][wave] = mine;
            __syncthreads();
            int32_t total = 0;
            for (int k = 0; k < kFilterWaves; ++k) {
                const int32_t n = wtot[buf][k];
                if (k < wave) before += n;
                total += n;
            }
            int64_t pos = done + before;
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (q.keep[e]) {
                    if (pos < len) {
                        out_i[base + pos] = (int32_t)(t.row0 + r);
                        out_j[base + pos] = (int32_t)(t.col0 + v - w.shift + e);
                    }
                    ++pos;
                }
            done += total;
        }
    }
}

// Line n = "{id_i} {id_j} {a} {b}\n" from byte line_off[n] of out: i = pi[n], j = pj[n], a / b = the five bytes of rows
// min(mn[n], 17001) / min(last[n], 17001) of the two halves of the score table (sim_lines_kernel's).  Sixteen lanes per line,
// lane l writing bytes l, l + 16, ...: byte stores, any id length, any alignment.  A line with an index outside [0, n_ids) or
// an end beyond out_bytes is not written.
// LABELS (dctfp_pair_domain_lines): two more fields, "{id_i} {id_j} {a} {b} {label_a} {label_b}\n", label x = bytes
// [label_off[x], label_off[x + 1]) of `labels` for x = la[n] / lb[n] -- a row of the file's label table (one entry per fingerprint
// row, then the "no pair" entry); a line with a label index outside [0, n_labels) is not written either.  Without LABELS the
// four label arguments are not read.
template <bool LABELS>
__global__ __launch_bounds__(kLineThreads) void pair_lines_kernel(int64_t n_lines, const int32_t* __restrict__ pi, const int32_t* __restrict__ pj,
                                                                  const int32_t* __restrict__ mn, const int32_t* __restrict__ last,
                                                                  const int32_t* __restrict__ la, const int32_t* __restrict__ lb,
                                                                  const uint8_t* __restrict__ ids, const int64_t* __restrict__ id_off,
                                                                  int64_t n_ids, const uint8_t* __restrict__ labels,
                                                                  const int64_t* __restrict__ label_off, int64_t n_labels,
                                                                  const char* __restrict__ table, const int64_t* __restrict__ line_off,
                                                                  uint8_t* __restrict__ out, int64_t out_bytes) {
    const int64_t t = (int64_t)blockIdx.x * kLineThreads + threadIdx.x;
    const int64_t n = t / kLineLanes;
    const int sub = (int)(t % kLineLanes);
    if (n >= n_lines) return;
    const int64_t i = pi[n], j = pj[n];
    if (i < 0 || i >= n_ids || j < 0 || j >= n_ids) return;
    int64_t x = 0, y = 0, off_x = 0, len_x = 0, off_y = 0, len_y = 0;   // (the labels: two empty ones without LABELS)
    if constexpr (LABELS) {
        x = la[n], y = lb[n];
        if (x < 0 || x >= n_labels || y < 0 || y >= n_labels) return;
    }
    const int64_t off_i = id_off[i], len_i = id_off[i + 1] - off_i, off_j = id_off[j], len_j = id_off[j + 1] - off_j;
    if constexpr (LABELS) off_x = label_off[x], len_x = label_off[x + 1] - off_x, off_y = label_off[y], len_y = label_off[y + 1] - off_y;
    const int64_t at = line_off[n], total = len_i + len_j + 14 + (LABELS ? len_x + len_y + 2 : 0);
    if (at < 0 || at + total > out_bytes) return;
    const char* __restrict__ ta = table + 5 * (int64_t)min((uint32_t)mn[n], (uint32_t)(kScoreRows - 1));
    const char* __restrict__ tb = table + 5 * (int64_t)(kScoreRows + min((uint32_t)last[n], (uint32_t)(kScoreRows - 1)));
    const int64_t tail0 = len_i + 1 + len_j;   // " a.aaa b.bbb", then "\n" or " {label_a} {label_b}\n"
    const int64_t x0 = tail0 + 13, y0 = x0 + len_x + 1;
    for (int64_t o = sub; o < total; o += kLineLanes) {
        uint8_t ch;
        if (o < len_i) ch = ids[off_i + o];
        else if (o == len_i) ch = ' ';
        else if (o < tail0) ch = ids[off_j + (o - len_i - 1)];
        else if (!LABELS || o < x0 - 1) {
            const int k = (int)(o - tail0);
            ch = k == 0 || k == 6 ? (uint8_t)' ' : !LABELS && k == 12 ? (uint8_t)'\n' : k < 6 ? (uint8_t)ta[k - 1] : (uint8_t)tb[k - 7];
        } else if (o < x0) ch = ' ';
        else if (o < y0 - 1) ch = labels[off_x + (o - x0)];
        else if (o < y0) ch = ' ';
        else if (o < total - 1) ch = labels[off_y + (o - y0)];
        else ch = '\n';
        out[at + o] = ch;
    }
}

}  // namespace

namespace dctfp_host {

void launch_tri_filter_count(const TriTile& t, int32_t* out_count, hipStream_t stream) {
    hipLaunchKernelGGL(tri_filter_count_kernel, dim3(filter_grid(t.n_rows)), dim3(kFilterThreads), 0, stream, t, out_count);
}

void launch_tri_filter_fill(const TriTile& t, const int64_t* offsets, int64_t out_len, int32_t* out_i, int32_t* out_j, hipStream_t stream) {
    hipLaunchKernelGGL(tri_filter_fill_kernel, dim3(filter_grid(t.n_rows)), dim3(kFilterThreads), 0, stream, t, offsets, out_len, out_i, out_j);
}

void launch_pair_domain_lines(int64_t n_lines, const int32_t* pi, const int32_t* pj, const int32_t* mn, const int32_t* last, const int32_t* la,
                              const int32_t* lb, const uint8_t* ids, const int64_t* id_off, int64_t n_ids, const uint8_t* labels,
                              const int64_t* label_off, int64_t n_labels, const char* table, const int64_t* line_off, uint8_t* out,
                              int64_t out_bytes, hipStream_t stream) {
    const int64_t threads = n_lines * kLineLanes;
    const dim3 grid((unsigned)((threads + kLineThreads - 1) / kLineThreads));
    if (labels)
        hipLaunchKernelGGL((pair_lines_kernel<true>), grid, dim3(kLineThreads), 0, stream, n_lines, pi, pj, mn, last, la, lb, ids, id_off, n_ids,
                           labels, label_off, n_labels, table, line_off, out, out_bytes);
    else
        hipLaunchKernelGGL((pair_lines_kernel<false>), grid, dim3(kLineThreads), 0, stream, n_lines, pi, pj, mn, last, la, lb, ids, id_off, n_ids,
                           labels, label_off, n_labels, table, line_off, out, out_bytes);
}

}  // namespace dctfp_host
