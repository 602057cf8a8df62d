// query_db at database scale (src/query_db.py:17-91) without a distance matrix in HBM:
//   l1_knn_kernel      -- the L1 distances of a 128-row query tile against a slice of the database (sad_tile's
//                         contraction, in a copy of its own) and, fused behind them, each row's k nearest: keys below the row's threshold go to a
//                         small LDS ring, a full ring is merged into the row's sorted k-list in global scratch;
//   knn_merge2_kernel  -- two sorted k-lists of a row -> one (the slices of the database, pairwise);
//   query_rank_kernel  -- the protein-level ranking of ranked_hits (src/query_db.py:33-40) from the sorted hit lists;
//   query_lines_kernel -- the hit lines as UTF-8 text at host-computed offsets.
// Key of a hit: (distance << 32) | column -- unique per row, so the order is total and every selection strategy agrees with
// row_select(l1_matrix(q, b), k): ascending distance, ties to the lower database row.
#define DCTFP_TEMPLATES_ONLY
#include "launch.h"

namespace {

using dctfp::kSadKC;
using dctfp::kSadLD;
using dctfp::kSadLds;
using dctfp::load_bytes4;
using dctfp::sad_b_slot;
using dctfp::v4u32;

// l1_knn_kernel keeps a copy of its own of sad_tile<16> (sad_tile.hip.h): it sits at the register ceiling, and through the shared
// function (290 registers instead of 294) every k = 1024 configuration of tools/query_db_bench.py measured 0.7 - 1.4 % slower than
// the parent's five runs, whose spread is 0.05 % (the k = 100 ones 1 - 2 % faster; profiles/sad_tile/README.md).  A fix to the
// tile is made there AND here.  The layout numbers (kSadKC, kSadLD, sad_b_slot) are the header's.
constexpr int kTile = dctfp::kSadTile;  // query rows and database columns per block: the tile's, and the size of the row state
constexpr int kRing = 32;             // candidate slots per row in LDS
constexpr unsigned long long kNone = ~0ull;

// LDS of l1_knn_kernel: 2 x 18 KiB operand tiles + 32 KiB ring + 2.5 KiB row state = 70.5 KiB (two workgroups per CU by LDS).
// Registers bind first: 256 VGPRs + 38 AGPRs = one wave per SIMD, one workgroup per CU.  A bound of two workgroups makes the
// compiler spill to scratch, so none is asked for.
__global__ __launch_bounds__(256, 1) void l1_knn_kernel(const int8_t* __restrict__ a, int64_t na, int64_t lda, const int8_t* __restrict__ b,
                                                        int64_t nb, int64_t ldb, int d, int k, int64_t slice_cols, int n_slices,
                                                        unsigned long long* __restrict__ work, unsigned long long* __restrict__ cand,
                                                        int32_t* __restrict__ out_val, int32_t* __restrict__ out_idx, int64_t col0, int k_eff) {
    __shared__ uint32_t sa[kSadLds];
    __shared__ uint32_t sb[kSadLds];
    __shared__ unsigned long long ring[kTile][kRing];
    __shared__ unsigned long long tau[kTile];   // the row's k-th key (kNone while its list holds fewer than k)
    __shared__ int cnt[kTile];                  // ring entries (attempts beyond kRing included)
    __shared__ int len[kTile];                  // k-list length
    __shared__ int cur[kTile];                  // which of the row's two work lists holds it
    __shared__ int sflag;
    const int tid = threadIdx.x;
    const int64_t r0 = (int64_t)blockIdx.y * kTile;
    const int s = blockIdx.x;
    const int64_t cs0 = (int64_t)s * slice_cols, cs1 = min(nb, cs0 + slice_cols);
    const int rows_a = (int)min((int64_t)kTile, na - r0);
    if (tid < kTile) {
        tau[tid] = kNone;
        cnt[tid] = 0;
        len[tid] = 0;
        cur[tid] = 0;
    }
    if (tid == 0) sflag = 0;
    // the work lists of (row, slice): two of k keys each
    auto list = [&](int row, int which) { return work + (((r0 + row) * n_slices + s) * 2 + which) * (int64_t)k; };

    // ring -> sorted k-list, every row with ring entries: sort the ring (bitonic, padded with kNone), then the merged position of
    // a ring key is its slot + #list keys below it, of a list key its index + #ring keys below it (keys are unique)
    auto flush = [&]() {
        // below[row][j] = #list keys below ring key j; it lives in sa, which is free between the contraction and the next fill
        int* below = reinterpret_cast<int*>(sa);
        __syncthreads();
        for (int p = tid; p < kTile * kRing; p += 256) {
            const int row = p / kRing, q = p % kRing;
            below[p] = 0;
            if (cnt[row] > 0 && q >= min(cnt[row], kRing)) ring[row][q] = kNone;
        }
        __syncthreads();
        for (int size = 2; size <= kRing; size <<= 1) {
            for (int stride = size >> 1; stride > 0; stride >>= 1) {
                for (int p = tid; p < kTile * kRing / 2; p += 256) {
                    const int row = p / (kRing / 2), q = p % (kRing / 2);
                    if (cnt[row] == 0) continue;
                    const int lo = ((q & ~(stride - 1)) << 1) | (q & (stride - 1));
                    const int hi = lo | stride;
                    const bool up = (lo & size) == 0;
                    const unsigned long long x = ring[row][lo], y = ring[row][hi];
                    if ((x > y) == up) {
                        ring[row][lo] = y;
                        ring[row][hi] = x;
                    }
                }
                __syncthreads();
            }
        }
        // #ring keys below x: a binary search in LDS
        auto rank_in_ring = [&](int row, int m, unsigned long long x) {
            int lo = 0, hi = m;
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (ring[row][mid] < x) lo = mid + 1;
                else hi = mid;
            }
            return lo;
        };
        // list keys (rows with an empty ring keep their list as it is): key i moves to i + #ring keys below it; and since
        // list key i is below ring key j exactly when that count is <= j, key i sets below[j] = i + 1 for j from its count up
        // to the next key's.  Reads of the list are coalesced; no search in global memory.
        for (int64_t p = tid; p < (int64_t)rows_a * k; p += 256) {
            const int row = (int)(p / k), i = (int)(p % k);
            const int m = min(cnt[row], kRing), n = len[row];
            if (m == 0 || i >= n) continue;
            const unsigned long long* __restrict__ src = list(row, cur[row]);
            unsigned long long* __restrict__ dst = list(row, cur[row] ^ 1);
            const unsigned long long x = src[i];
            const int lo = rank_in_ring(row, m, x);
            const int pos = i + lo;
            if (pos < k) dst[pos] = x;
            if (pos == k - 1) tau[row] = x;
            const int hi = i + 1 < n ? rank_in_ring(row, m, src[i + 1]) : m;
            for (int j = lo; j < hi; ++j) below[row * kRing + j] = i + 1;
        }
        __syncthreads();
        for (int p = tid; p < rows_a * kRing; p += 256) {   // ring keys: slot + #list keys below
            const int row = p / kRing, j = p % kRing;
            if (j >= min(cnt[row], kRing)) continue;
            const unsigned long long x = ring[row][j];
            const int pos = j + below[p];
            if (pos < k) list(row, cur[row] ^ 1)[pos] = x;
            if (pos == k - 1) tau[row] = x;
        }
        // the lists are read by other waves of the workgroup in the next flush / the output: the stores must reach L2 and
        // the readers' L1 lines (possibly from an earlier flush) must go -- a workgroup-scope barrier promises neither
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        __syncthreads();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        if (tid < kTile && cnt[tid] > 0) {
            len[tid] = min(k, len[tid] + min(cnt[tid], kRing));
            cur[tid] ^= 1;
            cnt[tid] = 0;
        }
        __syncthreads();
    };

    const int ty = tid >> 4, tx = tid & 15;
    const int seg = tid & 7, frow = tid >> 3;
    const v4u32 flip = {0x80808080u, 0x80808080u, 0x80808080u, 0x80808080u};  // signed -> unsigned order, |x - y| unchanged
    const int8_t* __restrict__ abase = a + r0 * lda;
    const uint32_t lda32 = (uint32_t)lda, ldb32 = (uint32_t)ldb;
    const int d16 = d & ~15;
    for (int64_t c0 = cs0; c0 < cs1; c0 += kTile) {
        const int8_t* __restrict__ bbase = b + c0 * ldb;
        const int rows_b = (int)min((int64_t)kTile, cs1 - c0);
        uint32_t acc[8][8] = {};
        auto contract = [&](int kn) {
            for (int kk = 0; kk < kn; kk += 4) {
                v4u32 av[8];
#pragma unroll
                for (int i = 0; i < 8; ++i) av[i] = *reinterpret_cast<const v4u32*>(&sa[(ty * 8 + i) * kSadLD + kk]);
#pragma unroll
                for (int h = 0; h < 4; ++h) {
                    v4u32 bv[2];
#pragma unroll
                    for (int j = 0; j < 2; ++j) bv[j] = *reinterpret_cast<const v4u32*>(&sb[((2 * h + j) * 16 + tx) * kSadLD + kk]);
#pragma unroll
                    for (int q = 0; q < 4; ++q)
#pragma unroll
                        for (int i = 0; i < 8; ++i)
#pragma unroll
                            for (int j = 0; j < 2; ++j) acc[i][2 * h + j] = __builtin_amdgcn_sad_u8(av[i][q], bv[j][q], acc[i][2 * h + j]);
                }
            }
        };
        for (int byte0 = 0; byte0 < d16; byte0 += kSadKC * 4) {
            const int my0 = byte0 + seg * 16;
            const bool have = my0 < d16;
            __syncthreads();
            {
                v4u32 va[kTile / 32], vb[kTile / 32];
#pragma unroll
                for (int i = 0; i < kTile / 32; ++i) {
                    const int r = frow + 32 * i;
                    va[i] = flip;
                    vb[i] = flip;
                    if (have && r < rows_a) va[i] = *reinterpret_cast<const v4u32*>(abase + ((uint32_t)r * lda32 + (uint32_t)my0));
                    if (have && r < rows_b) vb[i] = *reinterpret_cast<const v4u32*>(bbase + ((uint32_t)r * ldb32 + (uint32_t)my0));
                }
#pragma unroll
                for (int i = 0; i < kTile / 32; ++i) {
                    const int r = frow + 32 * i;
                    *reinterpret_cast<v4u32*>(&sa[r * kSadLD + seg * 4]) = va[i] ^ flip;
                    *reinterpret_cast<v4u32*>(&sb[sad_b_slot(r) * kSadLD + seg * 4]) = vb[i] ^ flip;
                }
            }
            __syncthreads();
            contract(min(kSadKC, (d16 - byte0) >> 2));
        }
        if (d16 < d) {   // the 1..15 bytes the fingerprints end with
            __syncthreads();
            if (tid < kTile) {
                const int r = tid;
                v4u32 va = flip, vb = flip;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int n = min(4, d - d16 - 4 * q);
                    if (n > 0 && r < rows_a) va[q] = load_bytes4(abase + ((uint32_t)r * lda32 + (uint32_t)(d16 + 4 * q)), n);
                    if (n > 0 && r < rows_b) vb[q] = load_bytes4(bbase + ((uint32_t)r * ldb32 + (uint32_t)(d16 + 4 * q)), n);
                }
                *reinterpret_cast<v4u32*>(&sa[r * kSadLD]) = va ^ flip;
                *reinterpret_cast<v4u32*>(&sb[sad_b_slot(r) * kSadLD]) = vb ^ flip;
            }
            __syncthreads();
            contract(4);
        }
        // selection: acc[i][j] = distance of row ty * 8 + i to column c0 + tx * 8 + j (slice-relative key column)
        const uint32_t cbase = (uint32_t)(c0 - cs0) + tx * 8;
        auto key = [&](int i, int j) { return ((unsigned long long)acc[i][j] << 32) | (cbase + j); };
        unsigned long long pend = 0;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int row = ty * 8 + i;
            if (row >= rows_a) continue;
            const unsigned long long t = tau[row];
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (tx * 8 + j < rows_b && key(i, j) < t) pend |= 1ull << (i * 8 + j);
        }
        while (true) {
#pragma unroll
            for (int i = 0; i < 8; ++i)
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const unsigned long long bit = 1ull << (i * 8 + j);
                    if (!(pend & bit)) continue;
                    const int row = ty * 8 + i;
                    const int pos = atomicAdd(&cnt[row], 1);
                    if (pos < kRing) {
                        ring[row][pos] = key(i, j);
                        pend &= ~bit;
                    }
                }
            if (pend) sflag = 1;
            __syncthreads();
            const bool again = sflag != 0;
            __syncthreads();
            if (!again) break;
            if (tid == 0) sflag = 0;
            flush();
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const unsigned long long t = tau[ty * 8 + i];
#pragma unroll
                for (int j = 0; j < 8; ++j)
                    if ((pend >> (i * 8 + j)) & 1ull && !(key(i, j) < t)) pend &= ~(1ull << (i * 8 + j));
            }
        }
    }
    flush();
    // the row's list out: straight to (out_val, out_idx) with one slice, else to the candidate lists of the merge
    for (int row = 0; row < rows_a; ++row) {
        const int n = len[row];
        const unsigned long long* __restrict__ src = list(row, cur[row]);
        if (n_slices == 1) {
            for (int i = tid; i < k_eff; i += 256) {
                const unsigned long long x = src[i];   // (n == k_eff here)
                out_val[(r0 + row) * k_eff + i] = (int32_t)(x >> 32);
                out_idx[(r0 + row) * k_eff + i] = (int32_t)((int64_t)(uint32_t)x + col0);
            }
        } else {
            unsigned long long* __restrict__ dst = cand + ((r0 + row) * n_slices + s) * (int64_t)k;
            for (int i = tid; i < k; i += 256) {
                unsigned long long x = kNone;
                if (i < n) x = src[i] + ((unsigned long long)(uint32_t)cs0);   // (slice-relative -> block column)
                dst[i] = x;
            }
        }
    }
}

// List 2p and 2p + 1 of every row (n_in lists of k keys, padded with kNone) -> list p of the output (n_out = ceil(n_in / 2)):
// a key of the first list goes to its index + #keys of the second below it, one of the second to its index + #keys of the first
// not above it (so that padding lands behind everything).  n_out == 1: the final list straight to (out_val, out_idx).
__global__ __launch_bounds__(256) void knn_merge2_kernel(const unsigned long long* __restrict__ in, int n_in, int k,
                                                         unsigned long long* __restrict__ out, int32_t* __restrict__ out_val,
                                                         int32_t* __restrict__ out_idx, int64_t col0, int k_eff) {
    const int64_t row = blockIdx.x;
    const int p = blockIdx.y, n_out = gridDim.y;
    const unsigned long long* __restrict__ A = in + (row * n_in + 2 * p) * (int64_t)k;
    const bool pair = 2 * p + 1 < n_in;
    const unsigned long long* __restrict__ B = A + k;
    for (int t = threadIdx.x; t < (pair ? 2 * k : k); t += blockDim.x) {
        const bool first = t < k;
        const int i = first ? t : t - k;
        const unsigned long long x = first ? A[i] : B[i];
        int pos = i;
        if (pair) {
            const unsigned long long* __restrict__ other = first ? B : A;
            int lo = 0, hi = k;
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (first ? other[mid] < x : other[mid] <= x) lo = mid + 1;
                else hi = mid;
            }
            pos += lo;
        }
        if (pos >= k) continue;
        if (n_out == 1) {
            if (pos < k_eff) {
                out_val[row * k_eff + pos] = (int32_t)(x >> 32);
                out_idx[row * k_eff + pos] = (int32_t)((int64_t)(uint32_t)x + col0);
            }
        } else {
            out[(row * n_out + p) * (int64_t)k + pos] = x;
        }
    }
}

// ranked_hits (src/query_db.py:33-40) for every protein at once: protein p owns fingerprint rows [qoff[p], qoff[p+1]) of the
// (n_rows, k) sorted hit lists; hit (i, j) -- fingerprint i of the protein, rank j in its list -- goes to rank
// j + sum over the protein's other lists of #(distance < mine) (lists before i: <=), i.e. the stable order by
// (distance, fingerprint, hit).  Ranks below min(khits, f k) are written at line_base[p] + rank.  One thread per hit;
// rows with prot_of_row < 0 are skipped.
__global__ __launch_bounds__(256) void query_rank_kernel(const int32_t* __restrict__ val, const int32_t* __restrict__ idx, int64_t n_rows, int k,
                                                         const int64_t* __restrict__ qoff, const int32_t* __restrict__ prot_of_row,
                                                         const int64_t* __restrict__ line_base, int khits, int32_t* __restrict__ out_qrow,
                                                         int32_t* __restrict__ out_drow, int32_t* __restrict__ out_dist) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_rows * k) return;
    const int64_t r = t / k;
    const int j = (int)(t % k);
    const int p = prot_of_row[r];
    if (p < 0) return;                     // (a protein the caller ranks on the host)
    const int64_t q0 = qoff[p], q1 = qoff[p + 1];
    const int32_t x = val[t];
    int64_t rank = j;
    for (int64_t o = q0; o < q1; ++o) {
        if (o == r) continue;
        const int32_t* __restrict__ v = val + o * k;
        const bool le = o < r;
        int lo = 0, hi = k;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (le ? v[mid] <= x : v[mid] < x) lo = mid + 1;
            else hi = mid;
        }
        rank += lo;
        if (rank >= khits) return;
    }
    if (rank >= khits) return;
    const int64_t at = line_base[p] + rank;
    out_qrow[at] = (int32_t)r;
    out_drow[at] = idx[t];
    out_dist[at] = x;
}

// Line n: "Query: {qpid} {qdom}, Result {rank}: {dpid} {ddom}, Similarity: {score}\n" from byte line_off[n] of out (the
// host's prefix sum of the lengths).  Strings: q / d pids and domains as concatenated UTF-8 bytes with int64 prefix offsets per
// row; the score of distance x is bytes [score_off[x], score_off[x + 1]) of score_txt.  One thread per line, byte stores.
struct Piece {
    const uint8_t* p;
    int64_t n;
};

__device__ inline int64_t put(uint8_t* __restrict__ o, int64_t at, Piece s) {
    for (int64_t c = 0; c < s.n; ++c) o[at + c] = s.p[c];
    return at + s.n;
}

__global__ __launch_bounds__(256) void query_lines_kernel(int64_t n_lines, const int32_t* __restrict__ qrow, const int32_t* __restrict__ drow,
                                                          const int32_t* __restrict__ dist, const int32_t* __restrict__ rank,
                                                          const uint8_t* __restrict__ q_txt, const int64_t* __restrict__ q_pid_off,
                                                          const int64_t* __restrict__ q_dom_off, const uint8_t* __restrict__ d_txt,
                                                          const int64_t* __restrict__ d_pid_off, const int64_t* __restrict__ d_dom_off,
                                                          const uint8_t* __restrict__ score_txt, const int64_t* __restrict__ score_off,
                                                          const int64_t* __restrict__ line_off, uint8_t* __restrict__ out) {
    const int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= n_lines) return;
    static constexpr uint8_t k0[] = "Query: ", k1[] = ", Result ", k2[] = ": ", k3[] = ", Similarity: ";
    const int64_t qr = qrow[n], dr = drow[n];
    int64_t at = line_off[n];
    at = put(out, at, {k0, 7});
    at = put(out, at, {q_txt + q_pid_off[qr], q_pid_off[qr + 1] - q_pid_off[qr]});
    out[at++] = ' ';
    at = put(out, at, {q_txt + q_dom_off[qr], q_dom_off[qr + 1] - q_dom_off[qr]});
    at = put(out, at, {k1, 9});
    char dig[12];
    int nd = 0;
    for (uint32_t v = (uint32_t)rank[n]; nd == 0 || v; v /= 10) dig[nd++] = (char)('0' + v % 10);
    while (nd) out[at++] = (uint8_t)dig[--nd];
    at = put(out, at, {k2, 2});
    at = put(out, at, {d_txt + d_pid_off[dr], d_pid_off[dr + 1] - d_pid_off[dr]});
    out[at++] = ' ';
    at = put(out, at, {d_txt + d_dom_off[dr], d_dom_off[dr + 1] - d_dom_off[dr]});
    at = put(out, at, {k3, 14});
    const int64_t x = dist[n];
    at = put(out, at, {score_txt + score_off[x], score_off[x + 1] - score_off[x]});
    out[at] = '\n';
}

}  // namespace

namespace dctfp_host {

int knn_slices(int64_t na, int64_t nb, int k) {
    // about two workgroups per CU in all (one runs per CU at a time); a slice keeps at least 64 column blocks and 16 k columns,
    // so that its first k columns -- every one of them enters the list -- stay a small part of its work
    const int64_t tiles = (na + kTile - 1) / kTile, blocks = (nb + kTile - 1) / kTile;
    int64_t s = (512 + tiles - 1) / tiles;
    s = min(s, max((int64_t)1, blocks / 64));
    s = min(s, max((int64_t)1, nb / (16 * (int64_t)k)));
    return (int)max((int64_t)1, min(s, (int64_t)4096));
}

size_t knn_scratch_bytes(int64_t na, int k, int n_slices) {
    size_t keys = (size_t)na * n_slices * 2 * k;                          // work lists
    if (n_slices > 1) keys += (size_t)na * n_slices * k + (size_t)na * ((n_slices + 1) / 2) * k;   // candidates + merge
    return keys * sizeof(unsigned long long);
}

int launch_l1_knn(const int8_t* a, int64_t na, int64_t lda, const int8_t* b, int64_t nb, int64_t ldb, int d, int k, int n_slices,
                  void* scratch, int32_t* out_val, int32_t* out_idx, int64_t col0, hipStream_t stream) {
    const int k_eff = (int)min((int64_t)k, nb);
    const int64_t blocks = (nb + kTile - 1) / kTile;
    const int64_t slice_cols = (blocks + n_slices - 1) / n_slices * kTile;
    const int S = (int)((nb + slice_cols - 1) / slice_cols);   // (slices that own a column)
    unsigned long long* work = (unsigned long long*)scratch;
    unsigned long long* cand = work + (size_t)na * S * 2 * k;
    unsigned long long* cand2 = cand + (size_t)na * S * k;
    const dim3 grid((unsigned)S, (unsigned)((na + kTile - 1) / kTile));
    hipLaunchKernelGGL(l1_knn_kernel, grid, dim3(256), 0, stream, a, na, lda, b, nb, ldb, d, k, slice_cols, S, work, cand, out_val, out_idx,
                       col0, k_eff);
    int n_in = S;
    unsigned long long* src = cand;
    unsigned long long* dst = cand2;
    while (n_in > 1) {
        const int n_out = (n_in + 1) / 2;
        hipLaunchKernelGGL(knn_merge2_kernel, dim3((unsigned)na, (unsigned)n_out), dim3(256), 0, stream, src, n_in, k, dst, out_val, out_idx,
                           col0, k_eff);
        n_in = n_out;
        std::swap(src, dst);
    }
    return S;
}

void launch_query_rank(const int32_t* val, const int32_t* idx, int64_t n_rows, int k, const int64_t* qoff, const int32_t* prot_of_row,
                       const int64_t* line_base, int khits, int32_t* out_qrow, int32_t* out_drow, int32_t* out_dist, hipStream_t stream) {
    const int64_t n = n_rows * k;
    hipLaunchKernelGGL(query_rank_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, val, idx, n_rows, k, qoff, prot_of_row,
                       line_base, khits, out_qrow, out_drow, out_dist);
}

void launch_query_lines(int64_t n_lines, const int32_t* qrow, const int32_t* drow, const int32_t* dist, const int32_t* rank,
                        const uint8_t* q_txt, const int64_t* q_pid_off, const int64_t* q_dom_off, const uint8_t* d_txt, const int64_t* d_pid_off,
                        const int64_t* d_dom_off, const uint8_t* score_txt, const int64_t* score_off, const int64_t* line_off, uint8_t* out,
                        hipStream_t stream) {
    hipLaunchKernelGGL(query_lines_kernel, dim3((unsigned)((n_lines + 255) / 256)), dim3(256), 0, stream, n_lines, qrow, drow, dist, rank, q_txt,
                       q_pid_off, q_dom_off, d_txt, d_pid_off, d_dom_off, score_txt, score_off, line_off, out);
}

}  // namespace dctfp_host
