// Protein-level search (dct-sim --db / --pair, src/dct-sim.py:86-156) without the all-against-all block matrix:
//   pair_min_kernel      -- DCTdomain / DCTglobal L1 of a list of protein pairs, read straight from the fingerprints, and
//                           (ARG) the fingerprint pair DCTdomain came from;
//   select_count_kernel  -- per row of a last-row distance tile: how many hits the reference prints, and where the cut is;
//   select_fill_kernel   -- the hits themselves, compacted into a ragged array at host-computed offsets;
//   select_order_kernel  -- each row's hits in the reference's order (key ascending, ties by column), rows of <= 1024 hits;
//   sim_lines_kernel     -- all_sim's result lines (src/dct-sim.py:158-176) as text, from a (min, last) tile.
#define DCTFP_TEMPLATES_ONLY
#include "launch.h"

namespace {

constexpr int kPairWaves = 4;        // protein pairs per workgroup (one wave each)
constexpr int32_t kFullScale = 17000;   // the L1 of similarity 0 (src/dct-sim.py:24)
constexpr int kSelThreads = 1024;    // one workgroup per row in the selection
constexpr int kSelWaves = kSelThreads / 64;
constexpr int kBinsPerThread = 17;   // the key histogram: 17 bins per thread, keys 0 .. 17407

__device__ inline uint32_t bytes4(const int8_t* p, int d, int k, bool aligned) {
    const int byte0 = 4 * k, valid = min(4, d - byte0);
    return (aligned && valid == 4) ? *reinterpret_cast<const uint32_t*>(p + byte0) : dctfp::load_bytes4(p + byte0, valid);
}

__device__ inline uint32_t wave_sum(uint32_t s) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    return s;
}

// One wave per protein pair (pa, pb): the L1 of every fingerprint of pa against every fingerprint of pb, 64 lanes over the
// dwords of one fingerprint pair (v_sad_u8 on the sign-flipped bytes, as l1_matrix_kernel), summed across the wave; the minimum
// and the last (whole protein x whole protein) value are kept -- block_min_kernel's two numbers, without the distance matrix.
// Rows of up to 512 bytes (every fingerprint file: 480) keep the pa row in two registers per lane and read four pb rows per
// step, so that a wave has eight loads in flight instead of two.  An empty protein on either side leaves 0x7fffffff in both
// outputs (block_min_kernel's fill); a pair index outside [0, npa) x [0, npb) writes -1 to both.
// ARG (dctfp_pair_argmin): also where the minimum was, as row indices within the two proteins -- the reference's loop
// (src/dct-sim.py:42-50) replaces its maximum on `s > maxs` only, so among equal L1 values the first in (row of pa, row of pb)
// order stands.  After wave_sum every lane holds the sum, so the comparison is wave-uniform; it is made once per fingerprint
// pair in exactly that order (i, then j + u with u ascending), with `<`: the unroll cannot change which pair wins.  No pair
// (-1, -1) when the minimum is 17000 or more -- similarity 0 never exceeds the loop's starting 0 -- which covers the empty sides.
template <bool ALIGNED, bool ARG>
__global__ __launch_bounds__(kPairWaves * 64) void pair_min_kernel(const int32_t* __restrict__ pairs, int64_t n_pairs,
                                                                   const int8_t* __restrict__ a, int64_t lda, const int64_t* __restrict__ idx_a,
                                                                   int64_t npa, const int8_t* __restrict__ b, int64_t ldb,
                                                                   const int64_t* __restrict__ idx_b, int64_t npb, int d,
                                                                   int32_t* __restrict__ out_min, int32_t* __restrict__ out_last,
                                                                   int32_t* __restrict__ out_arg_a, int32_t* __restrict__ out_arg_b) {
    const int lane = threadIdx.x & 63;
    const int64_t p = (int64_t)blockIdx.x * kPairWaves + (threadIdx.x >> 6);
    if (p >= n_pairs) return;
    const int32_t pa = pairs[2 * p], pb = pairs[2 * p + 1];
    if (pa < 0 || pa >= npa || pb < 0 || pb >= npb) {
        if (lane == 0) {
            out_min[p] = out_last[p] = -1;
            if constexpr (ARG) out_arg_a[p] = out_arg_b[p] = -1;
        }
        return;
    }
    const int64_t a0 = idx_a[pa], a1 = idx_a[pa + 1], b0 = idx_b[pb], b1 = idx_b[pb + 1];
    constexpr uint32_t kFlip = 0x80808080u;   // signed -> unsigned order, |x - y| unchanged
    const int nd = (d + 3) / 4;
    int32_t mn = 0x7fffffff, last = 0x7fffffff;
    int32_t arg_a = -1, arg_b = -1;
    if (nd <= 128) {
        const bool has0 = lane < nd, has1 = lane + 64 < nd;
        for (int64_t i = a0; i < a1; ++i) {
            const int8_t* ra = a + i * lda;
            const uint32_t va0 = has0 ? bytes4(ra, d, lane, ALIGNED) ^ kFlip : 0u;
            const uint32_t va1 = has1 ? bytes4(ra, d, lane + 64, ALIGNED) ^ kFlip : 0u;
            for (int64_t j = b0; j < b1; j += 4) {
                uint32_t s[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    s[u] = 0;
                    if (j + u < b1) {
                        const int8_t* rb = b + (j + u) * ldb;
                        if (has0) s[u] = __builtin_amdgcn_sad_u8(va0, bytes4(rb, d, lane, ALIGNED) ^ kFlip, s[u]);
                        if (has1) s[u] = __builtin_amdgcn_sad_u8(va1, bytes4(rb, d, lane + 64, ALIGNED) ^ kFlip, s[u]);
                    }
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) s[u] = wave_sum(s[u]);
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    if (j + u < b1) {
                        last = (int32_t)s[u];
                        if constexpr (ARG) {
                            if (last < mn) {
                                arg_a = (int32_t)(i - a0);
                                arg_b = (int32_t)(j + u - b0);
                            }
                        }
                        mn = min(mn, last);
                    }
            }
        }
    } else {
        for (int64_t i = a0; i < a1; ++i) {
            const int8_t* ra = a + i * lda;
            for (int64_t j = b0; j < b1; ++j) {
                const int8_t* rb = b + j * ldb;
                uint32_t s = 0;
                for (int k = lane; k < nd; k += 64) s = __builtin_amdgcn_sad_u8(bytes4(ra, d, k, ALIGNED) ^ kFlip, bytes4(rb, d, k, ALIGNED) ^ kFlip, s);
                last = (int32_t)wave_sum(s);
                if constexpr (ARG) {
                    if (last < mn) {
                        arg_a = (int32_t)(i - a0);
                        arg_b = (int32_t)(j - b0);
                    }
                }
                mn = min(mn, last);
            }
        }
    }
    if (lane == 0) {
        out_min[p] = mn;
        out_last[p] = last;
        if constexpr (ARG) {
            const bool none = mn >= kFullScale;
            out_arg_a[p] = none ? -1 : arg_a;
            out_arg_b[p] = none ? -1 : arg_b;
        }
    }
}

// key of one entry: min(L1, cap); an empty protein on either side (no last row) is `cap` against everything.  (A negative
// value -- no L1 is -- counts as cap, so that no key can index outside the histogram.)
__device__ inline int32_t entry_key(const int32_t* __restrict__ row, const uint8_t* __restrict__ col_empty, int64_t c, int32_t cap) {
    const uint32_t v = (uint32_t)row[c];
    return (v >= (uint32_t)cap || (col_empty && col_empty[c])) ? cap : (int32_t)v;
}

// One workgroup per row: the histogram of the keys in LDS (key == cap counted in registers: unrelated proteins are mostly
// there, and one LDS bin would serialise them), then
//   c = #(key <= bound),  m = min(n_cols, max(top, c))            -- the reference prints m hits (src/dct-sim.py:150-152),
//   V = the smallest key with #(key <= V) >= m,  need = m - #(key < V)   -- the hits are key < V and the first `need` key == V.
// out_count[r] = m, out_cut[2 r] = V, out_cut[2 r + 1] = need.
__global__ __launch_bounds__(kSelThreads) void select_count_kernel(const int32_t* __restrict__ dist, int64_t ld, int64_t n_cols,
                                                                    const uint8_t* __restrict__ row_empty, const uint8_t* __restrict__ col_empty,
                                                                    int32_t cap, int32_t bound, int32_t top, int32_t* __restrict__ out_count,
                                                                    int32_t* __restrict__ out_cut) {
    __shared__ int32_t hist[kSelThreads * kBinsPerThread];
    __shared__ int32_t wtot[kSelWaves], wbound[kSelWaves];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t r = blockIdx.x;
    for (int q = tid; q < kSelThreads * kBinsPerThread; q += kSelThreads) hist[q] = 0;
    __syncthreads();
    uint32_t full = 0;
    if (row_empty && row_empty[r]) {
        full = tid < n_cols ? (uint32_t)((n_cols - 1 - tid) / kSelThreads + 1) : 0u;
    } else {
        const int32_t* row = dist + r * ld;
        for (int64_t c = tid; c < n_cols; c += kSelThreads) {
            const int32_t key = entry_key(row, col_empty, c, cap);
            if (key == cap) ++full;
            else atomicAdd(&hist[key], 1);
        }
    }
    full = wave_sum(full);
    if (lane == 0) atomicAdd(&hist[cap], (int32_t)full);
    __syncthreads();
    int32_t s = 0, s_bound = 0;
    for (int q = 0; q < kBinsPerThread; ++q) {
        const int bin = tid * kBinsPerThread + q;
        const int32_t h = hist[bin];
        s += h;
        if (bin <= bound) s_bound += h;
    }
    int32_t incl = s;   // inclusive scan of the per-thread sums over the wave ...
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int32_t t = __shfl_up(incl, o);
        if (lane >= o) incl += t;
    }
    s_bound = (int32_t)wave_sum((uint32_t)s_bound);
    if (lane == 63) wtot[wave] = incl;
    if (lane == 0) wbound[wave] = s_bound;
    __syncthreads();
    int32_t before = 0, c_bound = 0;   // ... and over the waves
    for (int w = 0; w < kSelWaves; ++w) {
        if (w < wave) before += wtot[w];
        c_bound += wbound[w];
    }
    const int32_t pre = before + incl - s;
    const int32_t m = (int32_t)min(n_cols, (int64_t)max(top, c_bound));
    if (pre < m && m <= pre + s) {   // exactly one thread: the one whose bins hold the m-th key
        int32_t cum = pre;
        for (int q = 0; q < kBinsPerThread; ++q) {
            const int bin = tid * kBinsPerThread + q;
            const int32_t h = hist[bin];
            if (cum + h >= m) {
                out_cut[2 * r] = bin;
                out_cut[2 * r + 1] = m - cum;
                break;
            }
            cum += h;
        }
    }
    if (tid == 0) out_count[r] = m;
}

// One workgroup per row, 1024 columns per step: the entries with key < V and the first `need` entries with key == V, written in
// column order to [offsets[r], offsets[r + 1]) -- a ballot + popcount scan per wave, the 16 wave totals through LDS (double
// buffered: one barrier per step).  The scan stops as soon as the row's m entries are out.
__global__ __launch_bounds__(kSelThreads) void select_fill_kernel(const int32_t* __restrict__ dist, int64_t ld, int64_t n_cols,
                                                                   const uint8_t* __restrict__ row_empty, const uint8_t* __restrict__ col_empty,
                                                                   int32_t cap, const int32_t* __restrict__ cut, const int64_t* __restrict__ offsets,
                                                                   int32_t* __restrict__ out_key, int32_t* __restrict__ out_col) {
    __shared__ int32_t wlt[2][kSelWaves], weq[2][kSelWaves];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t r = blockIdx.x;
    const int32_t V = cut[2 * r], need = cut[2 * r + 1];
    const int64_t base = offsets[r], len = offsets[r + 1] - base;
    const bool empty_row = row_empty && row_empty[r];
    const int32_t* row = dist + r * ld;
    const unsigned long long below = (1ull << lane) - 1;
    int64_t done = 0;
    int32_t eq_seen = 0;
    for (int64_t c0 = 0, step = 0; c0 < n_cols && done < len; c0 += kSelThreads, ++step) {
        const int64_t c = c0 + tid;
        const bool valid = c < n_cols;
        const int32_t key = !valid || empty_row ? cap : entry_key(row, col_empty, c, cap);
        const bool lt = valid && key < V, eq = valid && key == V;
        const unsigned long long blt = __ballot(lt), beq = __ballot(eq);
        const int buf = (int)(step & 1);
        if (lane == 0) {
            wlt[buf][wave] = __popcll(blt);
            weq[buf][wave] = __popcll(beq);
        }
        __syncthreads();
        int32_t lt_before = __popcll(blt & below), eq_before = __popcll(beq & below), lt_tot = 0, eq_tot = 0;
        for (int w = 0; w < kSelWaves; ++w) {
            const int32_t l = wlt[buf][w], e = weq[buf][w];
            if (w < wave) {
                lt_before += l;
                eq_before += e;
            }
            lt_tot += l;
            eq_tot += e;
        }
        const int32_t need_left = max(0, need - eq_seen);
        if (lt || (eq && eq_before < need_left)) {
            const int64_t pos = done + lt_before + min(eq_before, need_left);
            if (pos < len) {
                out_key[base + pos] = key;
                out_col[base + pos] = (int32_t)c;
            }
        }
        done += lt_tot + min(eq_tot, need_left);
        eq_seen += eq_tot;
    }
}

// Each row's (key, column) pairs ascending by key, ties by column -- row_order_kernel's bitonic network on ragged rows.  Rows
// of more than N entries are left as they are (in column order; the caller orders those).
template <int N>
__global__ __launch_bounds__(N / 2) void select_order_kernel(int32_t* __restrict__ key, int32_t* __restrict__ col, const int64_t* __restrict__ offsets) {
    __shared__ unsigned long long keys[N];
    const int64_t base = offsets[blockIdx.x], k = offsets[blockIdx.x + 1] - base;
    if (k <= 1 || k > N) return;
    int32_t* __restrict__ v = key + base;
    int32_t* __restrict__ c = col + base;
    for (int p = threadIdx.x; p < N; p += N / 2)
        keys[p] = p < k ? ((unsigned long long)(uint32_t)v[p] << 32) | (uint32_t)c[p] : ~0ull;
    __syncthreads();
    for (int size = 2; size <= N; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            const int q = threadIdx.x;
            const int lo = ((q & ~(stride - 1)) << 1) | (q & (stride - 1));
            const int hi = lo | stride;
            const bool up = (lo & size) == 0;
            const unsigned long long x = keys[lo], y = keys[hi];
            if ((x > y) == up) {
                keys[lo] = y;
                keys[hi] = x;
            }
            __syncthreads();
        }
    }
    for (int p = threadIdx.x; p < k; p += N / 2) {
        v[p] = (int32_t)(keys[p] >> 32);
        c[p] = (int32_t)(uint32_t)keys[p];
    }
}

// ---- all_sim's result lines.  Line (i, j) is "{id_i} {id_j} {a} {b}\n", len_i + len_j + 14 bytes, a / b the five characters
// of the score table for min / last (rows 0 .. 17000 = that L1, row 17001 = every larger value).  Row i prints j = i + 1 .. n - 1
// contiguously from row_base[r]; the line of column j starts (j - (i + 1)) (len_i + 14) + (P[j] - P[i + 1]) bytes later
// (P = id_off), so every workgroup knows where its bytes go without a scan over lines.
constexpr int kLineThreads = 256;    // one workgroup per (row, run of 256 columns)
constexpr int kIdStage = 4096;       // id bytes staged in LDS (longer: read from global memory)
constexpr int kScoreRows = 17002;

// The byte at offset o of a line: id_i, ' ', id_j, then the 13-byte tail " a.aaa b.bbb\n".
__device__ inline uint32_t line_byte(int64_t o, int64_t len_i, int64_t len_j, const uint8_t* si, const uint8_t* sj, const uint8_t* tail) {
    if (o < len_i) return si[o];
    if (o == len_i) return ' ';
    o -= len_i + 1;
    return o < len_j ? sj[o] : tail[o - len_j];
}

// One workgroup per (row r, run of up to 256 columns of the tile): the run's lines are one contiguous byte range.  Its line
// starts and score tails go to LDS (and the ids, when short), then the threads fill the range 16 aligned bytes at a time --
// whole words with one 16-byte store, only the first and last word of the range byte by byte (the neighbouring runs own the
// rest of those words).  Rows loop over gridDim.y.  Writes exactly [row_base[r] + start of the run's first line, ... + run bytes).
__global__ __launch_bounds__(kLineThreads) void sim_lines_kernel(const int32_t* __restrict__ mn, const int32_t* __restrict__ last, int64_t ld,
                                                                 int64_t n_rows, int64_t row0, int64_t col0, int64_t n_cols,
                                                                 const uint8_t* __restrict__ ids, const int64_t* __restrict__ id_off,
                                                                 const char* __restrict__ table, const int64_t* __restrict__ row_base,
                                                                 uint8_t* __restrict__ out) {
    __shared__ int64_t start[kLineThreads + 1];          // line starts, relative to the run's first byte
    __shared__ uint8_t tail[kLineThreads][16];
    __shared__ uint8_t stage_i[kIdStage], stage_j[kIdStage];
    const int tid = threadIdx.x;
    const int64_t c_lo = (int64_t)blockIdx.x * kLineThreads;
    for (int64_t r = blockIdx.y; r < n_rows; r += gridDim.y) {
        const int64_t i = row0 + r, js = i + 1;
        const int64_t j_lo = max(col0 + c_lo, js), j_hi = col0 + min(c_lo + kLineThreads, n_cols);
        if (j_lo >= j_hi) continue;                       // (uniform: the run lies left of the diagonal)
        const int64_t cnt = j_hi - j_lo;
        const int64_t off_i = id_off[i], len_i = id_off[i + 1] - off_i, pj0 = id_off[j_lo], len_js = id_off[j_hi] - pj0;
        const int64_t run0 = row_base[r] + (j_lo - js) * (len_i + 14) + (pj0 - id_off[js]);
        if (tid < cnt) {
            start[tid] = tid * (len_i + 14) + (id_off[j_lo + tid] - pj0);
            const int64_t c = j_lo + tid - col0;
            const uint32_t a = min((uint32_t)mn[r * ld + c], (uint32_t)(kScoreRows - 1));
            const uint32_t b = min((uint32_t)last[r * ld + c], (uint32_t)(kScoreRows - 1));
            uint8_t* t = tail[tid];
            t[0] = ' ';
            t[6] = ' ';
            t[12] = '\n';
#pragma unroll
            for (int k = 0; k < 5; ++k) {
                t[1 + k] = (uint8_t)table[5 * a + k];
                t[7 + k] = (uint8_t)table[5 * (kScoreRows + b) + k];
            }
        }
        if (tid == 0) start[cnt] = cnt * (len_i + 14) + len_js;
        const bool stage_ok_i = len_i <= kIdStage, stage_ok_j = len_js <= kIdStage;
        if (stage_ok_i)
            for (int64_t k = tid; k < len_i; k += kLineThreads) stage_i[k] = ids[off_i + k];
        if (stage_ok_j)
            for (int64_t k = tid; k < len_js; k += kLineThreads) stage_j[k] = ids[pj0 + k];
        __syncthreads();
        const uint8_t* si = stage_ok_i ? stage_i : ids + off_i;
        const uint8_t* sj = stage_ok_j ? stage_j : ids + pj0;
        const int64_t total = start[cnt];
        uint8_t* g = out + run0;
        const int64_t head = (int64_t)(reinterpret_cast<uintptr_t>(g) & 15u);   // bytes of the first word before the range
        const int64_t n_words = (head + total + 15) / 16;
        for (int64_t w = tid; w < n_words; w += kLineThreads) {
            const int64_t p0 = 16 * w - head;                   // range offset of the word's first byte (may be < 0)
            // the line holding max(p0, 0): the last l with start[l] <= it
            const int64_t q = max(p0, (int64_t)0);
            int lo = 0, hi = (int)cnt - 1;
            while (lo < hi) {
                const int mid = (lo + hi + 1) >> 1;
                if (start[mid] <= q) lo = mid;
                else hi = mid - 1;
            }
            int l = lo;
            int64_t ls = start[l], le = start[l + 1];
            uint32_t word[4] = {0u, 0u, 0u, 0u};
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                const int64_t p = p0 + k;
                if (p >= 0 && p < total) {
                    while (p >= le) {
                        ++l;
                        ls = le;
                        le = start[l + 1];
                    }
                    const int64_t len_j = le - ls - len_i - 14;
                    const uint32_t ch = line_byte(p - ls, len_i, len_j, si, sj + (ls - l * (len_i + 14)), tail[l]);
                    word[k >> 2] |= ch << (8 * (k & 3));
                }
            }
            if (p0 >= 0 && p0 + 16 <= total) {
                *reinterpret_cast<uint4*>(g + p0) = make_uint4(word[0], word[1], word[2], word[3]);
            } else {
#pragma unroll
                for (int k = 0; k < 16; ++k)
                    if (p0 + k >= 0 && p0 + k < total) g[p0 + k] = (uint8_t)(word[k >> 2] >> (8 * (k & 3)));
            }
        }
        __syncthreads();                                    // (LDS is refilled for the next row)
    }
}

}  // namespace

namespace dctfp_host {

template <bool ARG>
static void launch_pair_kernel(const int32_t* pairs, int64_t n_pairs, const int8_t* a, int64_t lda, const int64_t* idx_a, int64_t npa,
                               const int8_t* b, int64_t ldb, const int64_t* idx_b, int64_t npb, int d, int32_t* out_min, int32_t* out_last,
                               int32_t* out_arg_a, int32_t* out_arg_b, hipStream_t stream) {
    const bool aligned = ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | (uintptr_t)lda | (uintptr_t)ldb) & 3u) == 0;
    const dim3 grid((unsigned)((n_pairs + kPairWaves - 1) / kPairWaves));
    if (aligned)
        hipLaunchKernelGGL((pair_min_kernel<true, ARG>), grid, dim3(kPairWaves * 64), 0, stream, pairs, n_pairs, a, lda, idx_a, npa, b, ldb,
                           idx_b, npb, d, out_min, out_last, out_arg_a, out_arg_b);
    else
        hipLaunchKernelGGL((pair_min_kernel<false, ARG>), grid, dim3(kPairWaves * 64), 0, stream, pairs, n_pairs, a, lda, idx_a, npa, b, ldb,
                           idx_b, npb, d, out_min, out_last, out_arg_a, out_arg_b);
}

void launch_pair_argmin(const int32_t* pairs, int64_t n_pairs, const int8_t* a, int64_t lda, const int64_t* idx_a, int64_t npa,
                        const int8_t* b, int64_t ldb, const int64_t* idx_b, int64_t npb, int d, int32_t* out_min, int32_t* out_last,
                        int32_t* out_arg_a, int32_t* out_arg_b, hipStream_t stream) {
    if (out_arg_a)
        launch_pair_kernel<true>(pairs, n_pairs, a, lda, idx_a, npa, b, ldb, idx_b, npb, d, out_min, out_last, out_arg_a, out_arg_b, stream);
    else
        launch_pair_kernel<false>(pairs, n_pairs, a, lda, idx_a, npa, b, ldb, idx_b, npb, d, out_min, out_last, nullptr, nullptr, stream);
}

int select_max_cap() { return kSelThreads * kBinsPerThread - 1; }

void launch_select_count(const int32_t* dist, int64_t n_rows, int64_t n_cols, int64_t ld, const uint8_t* row_empty, const uint8_t* col_empty,
                         int32_t cap, int32_t bound, int32_t top, int32_t* out_count, int32_t* out_cut, hipStream_t stream) {
    hipLaunchKernelGGL(select_count_kernel, dim3((unsigned)n_rows), dim3(kSelThreads), 0, stream, dist, ld, n_cols, row_empty, col_empty, cap,
                       bound, top, out_count, out_cut);
}

void launch_select_fill(const int32_t* dist, int64_t n_rows, int64_t n_cols, int64_t ld, const uint8_t* row_empty, const uint8_t* col_empty,
                        int32_t cap, const int32_t* cut, const int64_t* offsets, int32_t max_count, int32_t* out_key, int32_t* out_col,
                        hipStream_t stream) {
    hipLaunchKernelGGL(select_fill_kernel, dim3((unsigned)n_rows), dim3(kSelThreads), 0, stream, dist, ld, n_cols, row_empty, col_empty, cap, cut,
                       offsets, out_key, out_col);
    if (max_count <= 1) return;
    if (max_count <= 128) hipLaunchKernelGGL((select_order_kernel<128>), dim3((unsigned)n_rows), dim3(64), 0, stream, out_key, out_col, offsets);
    else if (max_count <= 256) hipLaunchKernelGGL((select_order_kernel<256>), dim3((unsigned)n_rows), dim3(128), 0, stream, out_key, out_col, offsets);
    else hipLaunchKernelGGL((select_order_kernel<1024>), dim3((unsigned)n_rows), dim3(512), 0, stream, out_key, out_col, offsets);
}

void launch_sim_lines(const int32_t* mn, const int32_t* last, int64_t ld, int64_t n_rows, int64_t row0, int64_t col0, int64_t n_cols,
                      const uint8_t* ids, const int64_t* id_off, const char* table, const int64_t* row_base, uint8_t* out, hipStream_t stream) {
    const dim3 grid((unsigned)((n_cols + kLineThreads - 1) / kLineThreads), (unsigned)min(n_rows, (int64_t)65535));
    hipLaunchKernelGGL(sim_lines_kernel, grid, dim3(kLineThreads), 0, stream, mn, last, ld, n_rows, row0, col0, n_cols, ids, id_off, table,
                       row_base, out);
}

}  // namespace dctfp_host
