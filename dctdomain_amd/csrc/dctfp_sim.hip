// libdctfp.so -- the stateless exports of include/dctfp.h behind dct-sim and query_db, include/dctfp_linkage.h and
// include/dctfp_silhouette.h.
// Each checks its arguments, takes the context's mutex and makes the launches of one kernel family.  Of the context they read
// mu, device, n_cu, scratch and the options l1_kernel / row_select, and dctfp_l1_knn writes last_knn_slices / knn_calls.
// Built once and linked into both libraries (not in build_ext.TWIN_UNITS): see dctfp_host.h.
#define DCTFP_TEMPLATES_ONLY   // (the plain kernels of kernels.hip.h are defined in dctfp.hip; the three launched here: below)
#include "dctfp.h"
#include "dctfp_linkage.h"
#include "dctfp_silhouette.h"

#include "dctfp_host.h"
#include "tri_tile.hip.h"   // (TriTile; the kernels that scan one include tri_walk.hip.h or band_walk.hip.h)

namespace dctfp {
// (a launch needs the declaration alone; a signature that strays from kernels.hip.h fails to link)
__global__ void l1_matrix16_kernel(const int8_t* a, int64_t na, int64_t lda, const int8_t* b, int64_t nb, int64_t ldb, int d, int32_t* out,
                                   int64_t ldo);
__global__ void block_min_kernel(const int32_t* dist, int64_t ldo, const int64_t* idx_a, int64_t npa, const int64_t* idx_b, int64_t npb,
                                 int32_t* out_min, int32_t* out_last);
__global__ void row_select_kernel(const int32_t* dist, int64_t ld, int64_t n_cols, int k, int32_t* out_val, int32_t* out_idx);
}  // namespace dctfp

using namespace dctfp;
using namespace dctfp_host;

namespace {

// Whether ONE launch takes n items at `per` items to a workgroup of `threads`: HIP launches nothing whose gridDim.x * blockDim.x
// reaches 2^32 (hip_runtime_api.h, hipModuleLaunchKernel), so a grid has at most (2^32 - 1) / threads workgroups.  Written so
// that no n overflows; launch_items(per, threads) is the number the messages and include/dctfp.h state.
constexpr int64_t launch_items(int64_t per, int64_t threads) { return (int64_t)(0xffffffffu / threads) * per; }
constexpr bool one_launch(int64_t n, int64_t per, int64_t threads) { return n <= launch_items(per, threads); }
// Whether the `count` entries from `first` on lie within [0, n), for arguments that are not negative: first + count may not be formed,
// an int64 near its end wraps and the check passes (the kernels bound no index: what passes here is what they touch).
constexpr bool range_within(int64_t first, int64_t count, int64_t n) { return count <= n && first <= n - count; }

// The tail of an export that makes one launch: on the context's device, and what the launch left as the last error.
template <typename Launch> int on_device(dctfp_ctx* ctx, Launch launch) {
    HIP_TRY(hipSetDevice(ctx->device)); launch(); HIP_TRY(hipGetLastError()); return DCTFP_OK;
}

}  // namespace

extern "C" {

int dctfp_l1_matrix(dctfp_ctx* ctx, const int8_t* a, int64_t na, int64_t lda, const int8_t* b, int64_t nb, int64_t ldb,
                    int32_t d, int32_t* out, int64_t ldo, void* stream_v) try {
    if (!ctx || !a || !b || !out) return fail(DCTFP_ERR_INVALID, "dctfp_l1_matrix: NULL argument");
    std::lock_guard<std::mutex> lock(ctx->mu);
    if (na < 0 || nb < 0 || d < 1 || lda < d || ldb < d || ldo < nb) return fail(DCTFP_ERR_INVALID, "dctfp_l1_matrix: bad shape");
    if (na == 0 || nb == 0) return DCTFP_OK;
    if (na > 65535 * 128) return fail(DCTFP_ERR_LIMIT, "dctfp_l1_matrix: more than 8M rows per call");
    // (128 columns to a 256-thread workgroup along gridDim.x)
    if (!one_launch(nb, 128, 256)) return fail(DCTFP_ERR_LIMIT, "dctfp_l1_matrix: more than %lld columns per call", (long long)launch_items(128, 256));
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t stream = (hipStream_t)stream_v;
    dim3 grid((unsigned)((nb + 127) / 128), (unsigned)((na + 127) / 128));  // 128 x 128 distances per workgroup (l1_matrix_kernel)
    const int align = sad_tile_align(a, lda, b, ldb);   // (sad_tile.hip.h: 16, 4 or 1)
    if (align == 16 && ctx->opt_l1_kernel != 1) hipLaunchKernelGGL(l1_matrix16_kernel, grid, dim3(256), 0, stream, a, na, lda, b, nb, ldb, d, out, ldo);
    else if (align >= 4) hipLaunchKernelGGL((l1_matrix_kernel<true>), grid, dim3(256), 0, stream, a, na, lda, b, nb, ldb, d, out, ldo);
    else hipLaunchKernelGGL((l1_matrix_kernel<false>), grid, dim3(256), 0, stream, a, na, lda, b, nb, ldb, d, out, ldo);
    HIP_TRY(hipGetLastError());
    return DCTFP_OK;
} DCTFP_GUARD("dctfp_l1_matrix")

int dctfp_block_min(dctfp_ctx* ctx, const int32_t* dist, int64_t ldo, const int64_t* idx_a, int64_t npa,
                    const int64_t* idx_b, int64_t npb, int32_t* out_min, int32_t* out_last, void* stream_v) try {
    if (!ctx || !dist || !idx_a || !idx_b || !out_min || !out_last) return fail(DCTFP_ERR_INVALID, "dctfp_block_min: NULL argument");
    std::lock_guard<std::mutex> lock(ctx->mu);
    if (npa < 0 || npb < 0) return fail(DCTFP_ERR_INVALID, "dctfp_block_min: negative count");
    if (npa == 0 || npb == 0) return DCTFP_OK;
    // (one thread per protein pair in 256-thread workgroups)
    if (npa > launch_items(256, 256) / npb)
        return fail(DCTFP_ERR_LIMIT, "dctfp_block_min: more than %lld protein pairs (npa x npb) per call", (long long)launch_items(256, 256));
    const int64_t total = npa * npb;
    return on_device(ctx, [&] {
        hipLaunchKernelGGL(block_min_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream_v, dist, ldo,
                           idx_a, npa, idx_b, npb, out_min, out_last);
    });
} DCTFP_GUARD("dctfp_block_min")

int dctfp_row_select(dctfp_ctx* ctx, const int32_t* dist, int64_t n_rows, int64_t n_cols, int64_t ld, int32_t k,
                     int32_t* out_val, int32_t* out_idx, void* stream_v) try {
    if (!ctx || !dist || !out_val || !out_idx) return fail(DCTFP_ERR_INVALID, "dctfp_row_select: NULL argument");
    std::lock_guard<std::mutex> lock(ctx->mu);
    if (n_rows < 0 || n_cols < 1 || ld < n_cols || k < 1 || k > n_cols) return fail(DCTFP_ERR_INVALID, "dctfp_row_select: bad shape");
    if (n_rows == 0) return DCTFP_OK;
    // (one workgroup of up to 1024 threads to a row)
    if (!one_launch(n_rows, 1, 1024)) return fail(DCTFP_ERR_LIMIT, "dctfp_row_select: more than %lld rows per call", (long long)launch_items(1, 1024));
    if (n_cols > 0x7fffffff) return fail(DCTFP_ERR_LIMIT, "dctfp_row_select: more than 2^31 - 1 columns (out_idx is int32)");
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t stream = (hipStream_t)stream_v;
    Hold scratch{ctx->scratch, stream};   // (given back when the candidates were used: the destructor)
    // The row (or a segment of it) in the registers of one workgroup, read once (row_select_reg_kernel); longer rows in segments
    // whose k candidates each a second launch selects from.  Large k, or more candidates than one workgroup holds: the radix
    // select, which reads its row six times but has no limit.
    constexpr int kPer = 40;
    constexpr int64_t kSeg = 1024 * kPer;
    const int64_t n_seg = (n_cols + kSeg - 1) / kSeg;
    const bool reg_ok = ctx->opt_row_select != 1 && k <= 1024 && one_launch(n_rows * n_seg, 1, 512) && (n_seg == 1 || n_seg * k <= kSeg);
    if (reg_ok && n_seg == 1) {
        hipLaunchKernelGGL((row_select_reg_kernel<2 * kPer, false, 512>), dim3((unsigned)n_rows), dim3(512), 0, stream, dist, (const int32_t*)nullptr,
                           ld, n_cols, kSeg, (int64_t)1, (int)k, out_val, out_idx);
    } else if (reg_ok) {
        const int64_t n_in = n_seg * k;                       // candidates per row
        int rc = scratch.take((size_t)n_rows * n_in * 2 * sizeof(int32_t), stream);
        if (rc) return rc;
        int32_t* cand_val = (int32_t*)scratch.p();
        int32_t* cand_idx = cand_val + (size_t)n_rows * n_in;
        hipLaunchKernelGGL((row_select_reg_kernel<2 * kPer, false, 512>), dim3((unsigned)(n_rows * n_seg)), dim3(512), 0, stream, dist,
                           (const int32_t*)nullptr, ld, n_cols, kSeg, n_seg, (int)k, cand_val, cand_idx);
        hipLaunchKernelGGL((row_select_reg_kernel<kPer, true, 1024>), dim3((unsigned)n_rows), dim3(1024), 0, stream, (const int32_t*)cand_val,
                           (const int32_t*)cand_idx, n_in, n_in, n_in, (int64_t)1, (int)k, out_val, out_idx);
    } else {
        hipLaunchKernelGGL(row_select_kernel, dim3((unsigned)n_rows), dim3(1024), 0, stream, dist, ld, n_cols, k, out_val, out_idx);
    }
    HIP_TRY(hipGetLastError());
    return scratch.armed ? scratch.give_back() : DCTFP_OK;
} DCTFP_GUARD("dctfp_row_select")

int dctfp_row_order(dctfp_ctx* ctx, int32_t* val, int32_t* idx, int64_t n_rows, int32_t k, void* stream_v) try {
    if (!ctx || !val || !idx) return fail(DCTFP_ERR_INVALID, "dctfp_row_order: NULL argument");
    std::lock_guard<std::mutex> lock(ctx->mu);
    if (n_rows < 0 || k < 1) return fail(DCTFP_ERR_INVALID, "dctfp_row_order: bad shape");
    if (k > 1024) return fail(DCTFP_ERR_LIMIT, "dctfp_row_order: more than 1024 entries per row (order them on the host)");
    // (one workgroup of up to 512 threads to a row)
    if (!one_launch(n_rows, 1, 512)) return fail(DCTFP_ERR_LIMIT, "dctfp_row_order: more than %lld rows per call", (long long)launch_items(1, 512));
    if (n_rows == 0 || k == 1) return DCTFP_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t stream = (hipStream_t)stream_v;
    if (k <= 128) hipLaunchKernelGGL((row_order_kernel<128>), dim3((unsigned)n_rows), dim3(64), 0, stream, val, idx, (int)k);
    else if (k <= 256) hipLaunchKernelGGL((row_order_kernel<256>), dim3((unsigned)n_rows), dim3(128), 0, stream, val, idx, (int)k);
    else hipLaunchKernelGGL((row_order_kernel<1024>), dim3((unsigned)n_rows), dim3(512), 0, stream, val, idx, (int)k);
    HIP_TRY(hipGetLastError());
    return DCTFP_OK;
} DCTFP_GUARD("dctfp_row_order")

// dctfp_pair_min (out_arg_a = out_arg_b = NULL) and dctfp_pair_argmin: `name` = the export, for its messages.
static int pair_min_call(const char* name, dctfp_ctx* ctx, const int32_t* pairs, int64_t n_pairs, const int8_t* a, int64_t lda,
                         const int64_t* idx_a, int64_t npa, const int8_t* b, int64_t ldb, const int64_t* idx_b, int64_t npb, int32_t d,
                         int32_t* out_min, int32_t* out_last, int32_t* out_arg_a, int32_t* out_arg_b, void* stream_v) {
    if (!ctx || !pairs || !a || !idx_a || !b || !idx_b || !out_min || !out_last) return fail(DCTFP_ERR_INVALID, "%s: NULL argument", name);
    std::lock_guard<std::mutex> lock(ctx->mu);
    if (n_pairs < 0 || npa < 0 || npb < 0 || d < 1 || lda < d || ldb < d) return fail(DCTFP_ERR_INVALID, "%s: bad shape", name);
    if (npa > 0x7fffffff || npb > 0x7fffffff) return fail(DCTFP_ERR_LIMIT, "%s: more than 2^31 - 1 proteins on a side", name);
    // (four pairs to a 256-thread workgroup)
    if (!one_launch(n_pairs, 4, 256)) return fail(DCTFP_ERR_LIMIT, "%s: more than %lld pairs per call", name, (long long)launch_items(4, 256));
    if (n_pairs == 0) return DCTFP_OK;
    return on_device(ctx, [&] {
        launch_pair_argmin(pairs, n_pairs, a, lda, idx_a, npa, b, ldb, idx_b, npb, d, out_min, out_last, out_arg_a, out_arg_b, (hipStream_t)stream_v);
    });
}

int dctfp_pair_min(dctfp_ctx* ctx, const int32_t* pairs, int64_t n_pairs, const int8_t* a, int64_t lda, const int64_t* idx_a, int64_t npa,
                   const int8_t* b, int64_t ldb, const int64_t* idx_b, int64_t npb, int32_t d, int32_t* out_min, int32_t* out_last,
                   void* stream_v) try {
    return pair_min_call("dctfp_pair_min", ctx, pairs, n_pairs, a, lda, idx_a, npa, b, ldb, idx_b, npb, d, out_min, out_last, nullptr, nullptr,
                         stream_v);
} DCTFP_GUARD("dctfp_pair_min")

int dctfp_pair_argmin(dctfp_ctx* ctx, const int32_t* pairs, int64_t n_pairs, const int8_t* a, int64_t lda, const int64_t* idx_a, int64_t npa,
                      const int8_t* b, int64_t ldb, const int64_t* idx_b, int64_t npb, int32_t d, int32_t* out_min, int32_t* out_last,
                      int32_t* out_arg_a, int32_t* out_arg_b, void* stream_v) try {
    if (!out_arg_a || !out_arg_b) return fail(DCTFP_ERR_INVALID, "dctfp_pair_argmin: NULL argument");
    return pair_min_call("dctfp_pair_argmin", ctx, pairs, n_pairs, a, lda, idx_a, npa, b, ldb, idx_b, npb, d, out_min, out_last, out_arg_a,
                         out_arg_b, stream_v);
} DCTFP_GUARD("dctfp_pair_argmin")

int dctfp_pair_row_best(dctfp_ctx* ctx, const int32_t* pairs, int64_t n_pairs, const int8_t* a, int64_t lda, const int64_t* idx_a, int64_t npa,
                        const int8_t* b, int64_t ldb, const int64_t* idx_b, int64_t npb, int32_t d, const int64_t* row_off, int64_t out_len,
                        int32_t* out_l1, int32_t* out_arg, void* stream_v) try {
    if (!ctx || !pairs || !a || !idx_a || !b || !idx_b || !row_off || !out_l1 || !out_arg)
        return fail(DCTFP_ERR_INVALID, "dctfp_pair_row_best: NULL argument");
    std::lock_guard<std::mutex> lock(ctx->mu);
    if (n_pairs < 0 || npa < 0 || npb < 0 || d < 1 || lda < d || ldb < d || out_len < 0) return fail(DCTFP_ERR_INVALID, "dctfp_pair_row_best: bad shape");
    if (npa > 0x7fffffff || npb > 0x7fffffff) return fail(DCTFP_ERR_LIMIT, "dctfp_pair_row_best: more than 2^31 - 1 proteins on a side");
    if (!one_launch(n_pairs, 4, 256))
        return fail(DCTFP_ERR_LIMIT, "dctfp_pair_row_best: more than %lld pairs per call", (long long)launch_items(4, 256));
    if (n_pairs == 0) return DCTFP_OK;
    return on_device(ctx, [&] {
        launch_pair_row_best(pairs, n_pairs, a, lda, idx_a, npa, b, ldb, idx_b, npb, d, row_off, out_len, out_l1, out_arg, (hipStream_t)stream_v);
    });
} DCTFP_GUARD("dctfp_pair_row_best")

int dctfp_protein_min(dctfp_ctx* ctx, const int8_t* a, int64_t lda, const int64_t* idx_a, int64_t npa, const int8_t* b, int64_t ldb,
                      const int64_t* idx_b, int64_t npb, int32_t d, int32_t* out, int64_t ldo, void* stream_v) try {
    if (!ctx || !a || !idx_a || !b || !idx_b || !out) return fail(DCTFP_ERR_INVALID, "dctfp_protein_min: NULL argument");
    std::lock_guard<std::mutex> lock(ctx->mu);
    if (npa < 0 || npb < 0 || d < 1 || lda < d || ldb < d || ldo < npb) return fail(DCTFP_ERR_INVALID, "dctfp_protein_min: bad shape");
    if (npa > 0x7fffffff || npb > 0x7fffffff) return fail(DCTFP_ERR_LIMIT, "dctfp_protein_min: more than 2^31 - 1 proteins on a side");
    if (d > 512) return fail(DCTFP_ERR_LIMIT, "dctfp_protein_min: rows above 512 bytes (use l1_matrix + block_min)");
    if (sad_tile_align(a, lda, b, ldb) != 16)
        return fail(DCTFP_ERR_LIMIT, "dctfp_protein_min: rows not on 16-byte boundaries or 2^24 bytes apart (use l1_matrix + block_min)");
    if (npa == 0 || npb == 0) return DCTFP_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t stream = (hipStream_t)stream_v;
    Hold scratch{ctx->scratch, stream};   // the two block plans: given back after the kernel
    int rc = scratch.take(protein_plan_bytes(npa) + protein_plan_bytes(npb), stream);
    if (rc) return rc;
    // (a persistent grid: two workgroups per CU, what the kernel's 202 VGPRs allow)
    launch_protein_min(a, lda, idx_a, npa, b, ldb, idx_b, npb, d, out, ldo, scratch.p(), 2 * ctx->n_cu, stream);
    HIP_TRY(hipGetLastError());
    return scratch.give_back();
} DCTFP_GUARD("dctfp_protein_min")

int dctfp_protein_cover(dctfp_ctx* ctx, const int8_t* a, int64_t lda, const int64_t* idx_a, int64_t npa, const int32_t* w_a, const int32_t* need_a,
                        const int8_t* b, int64_t ldb, const int64_t* idx_b, int64_t npb, const int32_t* w_b, const int32_t* need_b, int32_t d,
                        int32_t bound, int32_t* out, int64_t ldo, void* stream_v) try {
    if (!ctx || !a || !idx_a || !w_a || !need_a || !b || !idx_b || !w_b || !need_b || !out)
        return fail(DCTFP_ERR_INVALID, "dctfp_protein_cover: NULL argument");
    std::lock_guard<std::mutex> lock(ctx->mu);
    if (npa < 0 || npb < 0 || d < 1 || lda < d || ldb < d || ldo < npb) return fail(DCTFP_ERR_INVALID, "dctfp_protein_cover: bad shape");
    if (bound > 0x7ffffffe) return fail(DCTFP_ERR_INVALID, "dctfp_protein_cover: bound above 0x7ffffffe");
    if (npa > 0x7fffffff || npb > 0x7fffffff) return fail(DCTFP_ERR_LIMIT, "dctfp_protein_cover: more than 2^31 - 1 proteins on a side");
    if (d > 512) return fail(DCTFP_ERR_LIMIT, "dctfp_protein_cover: rows above 512 bytes");
    if (sad_tile_align(a, lda, b, ldb) != 16)
        return fail(DCTFP_ERR_LIMIT, "dctfp_protein_cover: rows not on 16-byte boundaries or 2^24 bytes apart");
    if (npa == 0 || npb == 0) return DCTFP_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t stream = (hipStream_t)stream_v;
    Hold scratch{ctx->scratch, stream};   // the two block plans: given back after the kernel
    int rc = scratch.take(protein_plan_bytes(npa) + protein_plan_bytes(npb), stream);
    if (rc) return rc;
    launch_protein_cover(a, lda, idx_a, npa, w_a, need_a, b, ldb, idx_b, npb, w_b, need_b, d, bound, out, ldo, scratch.p(), 2 * ctx->n_cu, stream);
    HIP_TRY(hipGetLastError());
    return scratch.give_back();
} DCTFP_GUARD("dctfp_protein_cover")

int dctfp_select_count(dctfp_ctx* ctx, const int32_t* dist, int64_t n_rows, int64_t n_cols, int64_t ld, const uint8_t* row_empty,
                       const uint8_t* col_empty, int32_t cap, int32_t bound, int32_t top, int32_t* out_count, int32_t* out_cut,
                       void* stream_v) try {
    if (!ctx || !dist || !out_count || !out_cut) return fail(DCTFP_ERR_INVALID, "dctfp_select_count: NULL argument");
    std::lock_guard<std::mutex> lock(ctx->mu);
    if (n_rows < 0 || n_cols < 1 || ld < n_cols || top < 1 || cap < 0 || bound < -1 || bound > cap)
        return fail(DCTFP_ERR_INVALID, "dctfp_select_count: bad shape or bound");
    if (cap > select_max_cap()) return fail(DCTFP_ERR_LIMIT, "dctfp_select_count: cap above %d", select_max_cap());
    // (one 1024-thread workgroup to a row)
    if (!one_launch(n_rows, 1, 1024) || n_cols > 0x7fffffff)
        return fail(DCTFP_ERR_LIMIT, "dctfp_select_count: more than %lld rows per call or 2^31 - 1 columns", (long long)launch_items(1, 1024));
    if (n_rows == 0) return DCTFP_OK;
    return on_device(ctx, [&] { launch_select_count(dist, n_rows, n_cols, ld, row_empty, col_empty, cap, bound, top, out_count, out_cut, (hipStream_t)stream_v); });
} DCTFP_GUARD("dctfp_select_count")

int dctfp_select_fill(dctfp_ctx* ctx, const int32_t* dist, int64_t n_rows, int64_t n_cols, int64_t ld, const uint8_t* row_empty,
                      const uint8_t* col_empty, int32_t cap, const int32_t* cut, const int64_t* offsets, int32_t max_count, int32_t* out_key,
                      int32_t* out_col, void* stream_v) try {
    if (!ctx || !dist || !cut || !offsets || !out_key || !out_col) return fail(DCTFP_ERR_INVALID, "dctfp_select_fill: NULL argument");
    std::lock_guard<std::mutex> lock(ctx->mu);
    if (n_rows < 0 || n_cols < 1 || ld < n_cols || cap < 0 || max_count < 0) return fail(DCTFP_ERR_INVALID, "dctfp_select_fill: bad shape");
    if (cap > select_max_cap()) return fail(DCTFP_ERR_LIMIT, "dctfp_select_fill: cap above %d", select_max_cap());
    if (!one_launch(n_rows, 1, 1024) || n_cols > 0x7fffffff)
        return fail(DCTFP_ERR_LIMIT, "dctfp_select_fill: more than %lld rows per call or 2^31 - 1 columns", (long long)launch_items(1, 1024));
    if (n_rows == 0) return DCTFP_OK;
    return on_device(ctx, [&] {
        launch_select_fill(dist, n_rows, n_cols, ld, row_empty, col_empty, cap, cut, offsets, max_count, out_key, out_col, (hipStream_t)stream_v);
    });
} DCTFP_GUARD("dctfp_select_fill")

int dctfp_sim_lines(dctfp_ctx* ctx, const int32_t* mn, const int32_t* last, int64_t ld, int64_t n_rows, int64_t row0, int64_t col0,
                    int64_t n_cols, const uint8_t* ids, const int64_t* id_off, const char* table, const int64_t* row_base, uint8_t* out,
                    void* stream_v) try {
    if (!ctx || !mn || !last || !ids || !id_off || !table || !row_base || !out) return fail(DCTFP_ERR_INVALID, "dctfp_sim_lines: NULL argument");
    std::lock_guard<std::mutex> lock(ctx->mu);
    if (n_rows < 0 || n_cols < 0 || ld < n_cols || row0 < 0 || col0 < 0) return fail(DCTFP_ERR_INVALID, "dctfp_sim_lines: bad shape");
    // (one 256-thread workgroup per 256 columns)
    if (!one_launch(n_cols, 256, 256)) return fail(DCTFP_ERR_LIMIT, "dctfp_sim_lines: more than 2^32 - 256 columns per call");
    if (n_rows == 0 || n_cols == 0) return DCTFP_OK;
    return on_device(ctx, [&] { launch_sim_lines(mn, last, ld, n_rows, row0, col0, n_cols, ids, id_off, table, row_base, out, (hipStream_t)stream_v); });
} DCTFP_GUARD("dctfp_sim_lines")

// What the five exports that scan a tile (count, fill, link, mark, nearest) ask of it; `name` = the export, for the message.
static int check_tri_tile(const char* name, const TriTile& t) {
    if (t.n_rows < 0 || t.n_cols < 0 || t.ld < t.n_cols || t.row0 < 0 || t.col0 < 0 || t.cap < 0 || t.bound < -1 || t.bound > t.cap ||
        (reinterpret_cast<uintptr_t>(t.tile) & 3u) != 0)
        return fail(DCTFP_ERR_INVALID, "%s: bad shape, bound or alignment", name);
    return DCTFP_OK;
}

// ... and of the node arrays beside it: every (i, j) a kernel can form lies inside the tile, so the nodes are bounded here, on the
// host, and not on the device.
static int check_tri_nodes(const char* name, const TriTile& t, int64_t n_nodes) {
    if (n_nodes < 0 || !range_within(t.row0, t.n_rows, n_nodes) || !range_within(t.col0, t.n_cols, n_nodes))
        return fail(DCTFP_ERR_INVALID, "%s: the tile names proteins outside the nodes", name);
    return DCTFP_OK;
}

int dctfp_tri_filter_count(dctfp_ctx* ctx, const int32_t* tile, int64_t n_rows, int64_t n_cols, int64_t ld, int64_t row0, int64_t col0,
                           const uint8_t* row_empty, const uint8_t* col_empty, int32_t cap, int32_t bound, int32_t* out_count,
                           void* stream_v) try {
    if (!ctx || !tile || !out_count) return fail(DCTFP_ERR_INVALID, "dctfp_tri_filter_count: NULL argument");
    std::lock_guard<std::mutex> lock(ctx->mu);
    const TriTile t{tile, n_rows, n_cols, ld, row0, col0, row_empty, col_empty, cap, bound};
    RC_TRY(check_tri_tile("dctfp_tri_filter_count", t));
    if (!range_within(row0, n_rows, 0x7fffffff) || !range_within(col0, n_cols, 0x7fffffff))
        return fail(DCTFP_ERR_LIMIT, "dctfp_tri_filter_count: protein indices above 2^31 - 1");
    if (n_rows == 0) return DCTFP_OK;   // (n_cols == 0 still launches: the counts are zeros, written)
    return on_device(ctx, [&] { launch_tri_filter_count(t, out_count, (hipStream_t)stream_v); });
} DCTFP_GUARD("dctfp_tri_filter_count")

int dctfp_tri_filter_fill(dctfp_ctx* ctx, const int32_t* tile, int64_t n_rows, int64_t n_cols, int64_t ld, int64_t row0, int64_t col0,
                          const uint8_t* row_empty, const uint8_t* col_empty, int32_t cap, int32_t bound, const int64_t* offsets,
                          int64_t out_len, int32_t* out_i, int32_t* out_j, void* stream_v) try {
    if (!ctx || !tile || !offsets || !out_i || !out_j) return fail(DCTFP_ERR_INVALID, "dctfp_tri_filter_fill: NULL argument");
    std::lock_guard<std::mutex> lock(ctx->mu);
    const TriTile t{tile, n_rows, n_cols, ld, row0, col0, row_empty, col_empty, cap, bound};
    RC_TRY(check_tri_tile("dctfp_tri_filter_fill", t));
    if (out_len < 0) return fail(DCTFP_ERR_INVALID, "dctfp_tri_filter_fill: negative out_len");
    if (!range_within(row0, n_rows, 0x7fffffff) || !range_within(col0, n_cols, 0x7fffffff))
        return fail(DCTFP_ERR_LIMIT, "dctfp_tri_filter_fill: protein indices above 2^31 - 1");
    if (n_rows == 0 || n_cols == 0 || out_len == 0) return DCTFP_OK;
    return on_device(ctx, [&] { launch_tri_filter_fill(t, offsets, out_len, out_i, out_j, (hipStream_t)stream_v); });
} DCTFP_GUARD("dctfp_tri_filter_fill")

// dctfp_pair_lines (labels = NULL: la, lb, label_off unused) and dctfp_pair_domain_lines: `name` = the export, for its messages.
static int pair_lines_call(const char* name, dctfp_ctx* ctx, int64_t n_lines, const int32_t* pi, const int32_t* pj, const int32_t* mn,
                           const int32_t* last, const int32_t* la, const int32_t* lb, const uint8_t* ids, const int64_t* id_off, int64_t n_ids,
                           const uint8_t* labels, const int64_t* label_off, int64_t n_labels, const char* table, const int64_t* line_off,
                           uint8_t* out, int64_t out_bytes, void* stream_v) {
    if (!ctx || !pi || !pj || !mn || !last || !ids || !id_off || !table || !line_off || !out)
        return fail(DCTFP_ERR_INVALID, "%s: NULL argument", name);
    std::lock_guard<std::mutex> lock(ctx->mu);
    if (n_lines < 0 || n_ids < 0 || n_labels < 0 || out_bytes < 0) return fail(DCTFP_ERR_INVALID, "%s: bad shape", name);
    // (sixteen lanes per line: sixteen lines to a 256-thread workgroup)
    if (!one_launch(n_lines, 16, 256)) return fail(DCTFP_ERR_LIMIT, "%s: more than %lld lines per call", name, (long long)launch_items(16, 256));
    if (n_lines == 0) return DCTFP_OK;
    return on_device(ctx, [&] {
        launch_pair_domain_lines(n_lines, pi, pj, mn, last, la, lb, ids, id_off, n_ids, labels, label_off, n_labels, table, line_off, out,
                                 out_bytes, (hipStream_t)stream_v);
    });
}

int dctfp_pair_lines(dctfp_ctx* ctx, int64_t n_lines, const int32_t* pi, const int32_t* pj, const int32_t* mn, const int32_t* last,
                     const uint8_t* ids, const int64_t* id_off, int64_t n_ids, const char* table, const int64_t* line_off, uint8_t* out,
                     int64_t out_bytes, void* stream_v) try {
    return pair_lines_call("dctfp_pair_lines", ctx, n_lines, pi, pj, mn, last, nullptr, nullptr, ids, id_off, n_ids, nullptr, nullptr, 0, table,
                           line_off, out, out_bytes, stream_v);
} DCTFP_GUARD("dctfp_pair_lines")

int dctfp_pair_domain_lines(dctfp_ctx* ctx, int64_t n_lines, const int32_t* pi, const int32_t* pj, const int32_t* mn, const int32_t* last,
                            const int32_t* la, const int32_t* lb, const uint8_t* ids, const int64_t* id_off, int64_t n_ids,
                            const uint8_t* labels, const int64_t* label_off, int64_t n_labels, const char* table, const int64_t* line_off,
                            uint8_t* out, int64_t out_bytes, void* stream_v) try {
    if (!la || !lb || !labels || !label_off) return fail(DCTFP_ERR_INVALID, "dctfp_pair_domain_lines: NULL argument");
    return pair_lines_call("dctfp_pair_domain_lines", ctx, n_lines, pi, pj, mn, last, la, lb, ids, id_off, n_ids, labels, label_off, n_labels,
                           table, line_off, out, out_bytes, stream_v);
} DCTFP_GUARD("dctfp_pair_domain_lines")

int dctfp_pair_map_lines(dctfp_ctx* ctx, int64_t n_lines, const int32_t* pi, const int32_t* pj, const int32_t* mn, const int32_t* last,
                         const int32_t* la, const int32_t* lb, const uint8_t* ids, const int64_t* id_off, int64_t n_ids, const uint8_t* labels,
                         const int64_t* label_off, int64_t n_labels, const char* table, const int64_t* line_off, uint8_t* out,
                         int64_t out_bytes, const int64_t* row_off, int64_t n_rows, const int32_t* row_l1, const int32_t* row_arg,
                         const int64_t* first_row, int32_t bound, int64_t* out_count, void* stream_v) try {
    if (!ctx || !pi || !pj || !mn || !last || !la || !lb || !ids || !id_off || !labels || !label_off || !table || !row_off || !row_l1 ||
        !row_arg || !first_row || (!out_count && (!line_off || !out)))
        return fail(DCTFP_ERR_INVALID, "dctfp_pair_map_lines: NULL argument");
    std::lock_guard<std::mutex> lock(ctx->mu);
    if (n_lines < 0 || n_ids < 0 || n_labels < 0 || out_bytes < 0 || n_rows < 0) return fail(DCTFP_ERR_INVALID, "dctfp_pair_map_lines: bad shape");
    // (a matched row prints the score of its L1 from the table: no bound at or above similarity 0, dctfp_pair_argmin's "no pair")
    if (bound >= 17000) return fail(DCTFP_ERR_INVALID, "dctfp_pair_map_lines: the bound must be below 17000");
    // (dctfp_pair_lines' grid: sixteen lanes per line in 256-thread workgroups)
    if (!one_launch(n_lines, 16, 256))
        return fail(DCTFP_ERR_LIMIT, "dctfp_pair_map_lines: more than %lld lines per call", (long long)launch_items(16, 256));
    if (n_lines == 0) return DCTFP_OK;
    return on_device(ctx, [&] {
        launch_pair_map_lines(n_lines, pi, pj, mn, last, la, lb, ids, id_off, n_ids, labels, label_off, n_labels, table, first_row, row_off, n_rows,
                              row_l1, row_arg, bound, line_off, out, out_bytes, out_count, (hipStream_t)stream_v);
    });
} DCTFP_GUARD("dctfp_pair_map_lines")

int dctfp_tri_link(dctfp_ctx* ctx, const int32_t* tile, int64_t n_rows, int64_t n_cols, int64_t ld, int64_t row0, int64_t col0,
                   const uint8_t* row_empty, const uint8_t* col_empty, int32_t cap, int32_t bound, int32_t* parent, int64_t n_nodes,
                   void* stream_v) try {
    if (!ctx || !tile || !parent) return fail(DCTFP_ERR_INVALID, "dctfp_tri_link: NULL argument");
    std::lock_guard<std::mutex> lock(ctx->mu);
    const TriTile t{tile, n_rows, n_cols, ld, row0, col0, row_empty, col_empty, cap, bound};
    RC_TRY(check_tri_tile("dctfp_tri_link", t));
    if (n_nodes > 0x7fffffff) return fail(DCTFP_ERR_LIMIT, "dctfp_tri_link: more than 2^31 - 1 nodes");
    RC_TRY(check_tri_nodes("dctfp_tri_link", t, n_nodes));
    if (n_rows == 0 || n_cols == 0 || n_nodes == 0) return DCTFP_OK;
    return on_device(ctx, [&] { launch_tri_link(t, parent, (hipStream_t)stream_v); });
} DCTFP_GUARD("dctfp_tri_link")

int dctfp_link_pairs(dctfp_ctx* ctx, const int32_t* pi, const int32_t* pj, int64_t n_pairs, int32_t* parent, int64_t n_nodes,
                     void* stream_v) try {
    if (!ctx || !parent || ((!pi || !pj) && n_pairs > 0)) return fail(DCTFP_ERR_INVALID, "dctfp_link_pairs: NULL argument");
    std::lock_guard<std::mutex> lock(ctx->mu);
    if (n_pairs < 0 || n_nodes < 0) return fail(DCTFP_ERR_INVALID, "dctfp_link_pairs: bad shape");
    // (one thread per pair in 256-thread workgroups: 2^31 pairs are 2^23 workgroups, 2^31 threads)
    if (n_nodes > 0x7fffffff || n_pairs > (int64_t)1 << 31) return fail(DCTFP_ERR_LIMIT, "dctfp_link_pairs: more than 2^31 - 1 nodes or 2^31 pairs per call");
    if (n_pairs == 0 || n_nodes == 0) return DCTFP_OK;
    return on_device(ctx, [&] { launch_link_pairs(pi, pj, n_pairs, parent, n_nodes, (hipStream_t)stream_v); });
} DCTFP_GUARD("dctfp_link_pairs")

int dctfp_cluster_labels(dctfp_ctx* ctx, int32_t* parent, int64_t n_nodes, int32_t* labels, void* stream_v) try {
    if (!ctx || !parent || !labels) return fail(DCTFP_ERR_INVALID, "dctfp_cluster_labels: NULL argument");
    std::lock_guard<std::mutex> lock(ctx->mu);
    if (n_nodes < 0) return fail(DCTFP_ERR_INVALID, "dctfp_cluster_labels: bad shape");
    if (n_nodes > 0x7fffffff) return fail(DCTFP_ERR_LIMIT, "dctfp_cluster_labels: more than 2^31 - 1 nodes");
    if (n_nodes == 0) return DCTFP_OK;
    return on_device(ctx, [&] { launch_cluster_labels(parent, n_nodes, labels, (hipStream_t)stream_v); });
} DCTFP_GUARD("dctfp_cluster_labels")

int dctfp_rows_link(dctfp_ctx* ctx, const int8_t* a, int64_t na, int64_t lda, int64_t a0, const int8_t* b, int64_t nb, int64_t ldb, int64_t b0,
                    int32_t d, const int32_t* owner, const uint8_t* skip, int32_t cap, int32_t bound, int32_t* parent, int64_t n_nodes,
                    void* stream_v) try {
    if (!ctx || !a || !b || !owner || !parent) return fail(DCTFP_ERR_INVALID, "dctfp_rows_link: NULL argument");
    std::lock_guard<std::mutex> lock(ctx->mu);
    if (na < 0 || nb < 0 || d < 1 || lda < d || ldb < d || a0 < 0 || b0 < 0 || cap < 0 || bound < 0 || n_nodes < 0)
        return fail(DCTFP_ERR_INVALID, "dctfp_rows_link: bad shape or bound");
    if (n_nodes > 0x7fffffff) return fail(DCTFP_ERR_LIMIT, "dctfp_rows_link: more than 2^31 - 1 nodes");
    // (every node the kernel can form is a row of a or b: bounded here, not on the device)
    if (!range_within(a0, na, n_nodes) || !range_within(b0, nb, n_nodes)) return fail(DCTFP_ERR_INVALID, "dctfp_rows_link: the rows name nodes outside parent");
    if (na == 0 || nb == 0) return DCTFP_OK;
    if (na > 65535 * 128) return fail(DCTFP_ERR_LIMIT, "dctfp_rows_link: more than 8M rows of a per call");
    // (128 rows of b to a 256-thread workgroup along gridDim.x)
    if (!one_launch(nb, 128, 256)) return fail(DCTFP_ERR_LIMIT, "dctfp_rows_link: more than %lld rows of b per call", (long long)launch_items(128, 256));
    return on_device(ctx, [&] { launch_rows_link(a, na, lda, a0, b, nb, ldb, b0, d, owner, skip, cap, bound, parent, (hipStream_t)stream_v); });
} DCTFP_GUARD("dctfp_rows_link")

int dctfp_rows_assign(dctfp_ctx* ctx, const int8_t* a, int64_t na, int64_t lda, const int32_t* value_a, int64_t a0, const int8_t* b, int64_t nb,
                      int64_t ldb, const int32_t* slot_b, int64_t b0, int32_t d, int32_t cap, int32_t bound, int32_t* assign, int64_t n_assign,
                      void* stream_v) try {
    if (!ctx || !a || !b || !assign) return fail(DCTFP_ERR_INVALID, "dctfp_rows_assign: NULL argument");
    std::lock_guard<std::mutex> lock(ctx->mu);
    if (na < 0 || nb < 0 || d < 1 || lda < d || ldb < d || a0 < 0 || b0 < 0 || cap < 0 || bound < 0 || n_assign < 0)
        return fail(DCTFP_ERR_INVALID, "dctfp_rows_assign: bad shape or bound");
    if (n_assign > 0x7fffffff) return fail(DCTFP_ERR_LIMIT, "dctfp_rows_assign: more than 2^31 - 1 entries of assign");
    if (na == 0 || nb == 0 || n_assign == 0) return DCTFP_OK;
    if (na > 65535 * 128) return fail(DCTFP_ERR_LIMIT, "dctfp_rows_assign: more than 8M rows of a per call");
    // (128 rows of b to a 256-thread workgroup along gridDim.x)
    if (!one_launch(nb, 128, 256)) return fail(DCTFP_ERR_LIMIT, "dctfp_rows_assign: more than %lld rows of b per call", (long long)launch_items(128, 256));
    // (slots and values are bounded on the device: the host cannot see value_a and slot_b)
    return on_device(ctx, [&] { launch_rows_assign(a, na, lda, value_a, a0, b, nb, ldb, slot_b, b0, d, cap, bound, assign, n_assign, (hipStream_t)stream_v); });
} DCTFP_GUARD("dctfp_rows_assign")

int dctfp_tri_nearest(dctfp_ctx* ctx, const int32_t* tile, int64_t n_rows, int64_t n_cols, int64_t ld, int64_t row0, int64_t col0,
                      const uint8_t* row_empty, const uint8_t* col_empty, int32_t cap, int32_t bound, const int32_t* comp, uint64_t* best,
                      int64_t n_nodes, void* stream_v) try {
    // (the packed edge: 15 bits of key, 24 bits for each end -- said first: it holds whatever the other arguments are)
    if (n_nodes > (int64_t)1 << 24 || cap > 0x7fff) return fail(DCTFP_ERR_LIMIT, "dctfp_tri_nearest: more than 2^24 nodes or a cap above 32767");
    if (!ctx || !tile || !comp || !best) return fail(DCTFP_ERR_INVALID, "dctfp_tri_nearest: NULL argument");
    std::lock_guard<std::mutex> lock(ctx->mu);
    const TriTile t{tile, n_rows, n_cols, ld, row0, col0, row_empty, col_empty, cap, bound};
    RC_TRY(check_tri_tile("dctfp_tri_nearest", t));
    if ((reinterpret_cast<uintptr_t>(best) & 7u) != 0) return fail(DCTFP_ERR_INVALID, "dctfp_tri_nearest: best is not 8-byte aligned");
    RC_TRY(check_tri_nodes("dctfp_tri_nearest", t, n_nodes));
    if (n_rows == 0 || n_cols == 0 || n_nodes == 0) return DCTFP_OK;
    return on_device(ctx, [&] { launch_tri_nearest(t, comp, best, n_nodes, (hipStream_t)stream_v); });
} DCTFP_GUARD("dctfp_tri_nearest")

int dctfp_tree_hook(dctfp_ctx* ctx, const int32_t* comp, uint64_t* best, int32_t* parent, int64_t n_nodes, int32_t* edge_i, int32_t* edge_j,
                    int32_t* edge_key, int32_t* counter, int64_t max_edges, void* stream_v) try {
    if (n_nodes > (int64_t)1 << 24) return fail(DCTFP_ERR_LIMIT, "dctfp_tree_hook: more than 2^24 nodes");
    if (!ctx || !comp || !best || !parent || !counter || ((!edge_i || !edge_j || !edge_key) && max_edges > 0))
        return fail(DCTFP_ERR_INVALID, "dctfp_tree_hook: NULL argument");
    std::lock_guard<std::mutex> lock(ctx->mu);
    if (n_nodes < 0 || max_edges < 0 || (reinterpret_cast<uintptr_t>(best) & 7u) != 0) return fail(DCTFP_ERR_INVALID, "dctfp_tree_hook: bad shape or alignment");
    if (n_nodes == 0) return DCTFP_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(launch_tree_hook(comp, best, parent, n_nodes, edge_i, edge_j, edge_key, counter, max_edges, (hipStream_t)stream_v));
    HIP_TRY(hipGetLastError());
    return DCTFP_OK;
} DCTFP_GUARD("dctfp_tree_hook")

// ---- include/dctfp_linkage.h: the two kernels of complete- and average-linkage clustering (k_linkage.hip)
int dctfp_linkage_version(void) { return DCTFP_LINKAGE_VERSION; }

// What both exports ask of the matrix; `name` = the export, for the message.  The limit first: it holds whatever else is passed.
static int check_linkage_matrix(const char* name, const void* mat, int32_t wide, int64_t n, int64_t ld) {
    if (n > DCTFP_LINKAGE_MAX_N) return fail(DCTFP_ERR_LIMIT, "%s: more than %d nodes", name, DCTFP_LINKAGE_MAX_N);
    if (!mat) return fail(DCTFP_ERR_INVALID, "%s: NULL argument", name);
    if (wide < 0 || wide > 1) return fail(DCTFP_ERR_INVALID, "%s: wide is 0 (int32 entries) or 1 (int64)", name);
    if (n < 0 || ld < n) return fail(DCTFP_ERR_INVALID, "%s: bad shape (n < 0 or ld < n)", name);
    if ((reinterpret_cast<uintptr_t>(mat) & (wide ? 7u : 3u)) != 0) return fail(DCTFP_ERR_INVALID, "%s: the matrix is not aligned to its entries", name);
    return DCTFP_OK;
}

int dctfp_linkage_nearest(dctfp_ctx* ctx, const void* mat, int32_t wide, int64_t n, int64_t ld, const int32_t* size, const int32_t* live,
                          int64_t n_live, int32_t bound, int32_t* nn, void* stream_v) try {
    if (n > DCTFP_LINKAGE_MAX_N || bound > DCTFP_LINKAGE_MAX_BOUND)
        return fail(DCTFP_ERR_LIMIT, "dctfp_linkage_nearest: more than %d nodes or a bound above %d", DCTFP_LINKAGE_MAX_N, DCTFP_LINKAGE_MAX_BOUND);
    if (!ctx || !size || !live || !nn) return fail(DCTFP_ERR_INVALID, "dctfp_linkage_nearest: NULL argument");
    RC_TRY(check_linkage_matrix("dctfp_linkage_nearest", mat, wide, n, ld));
    std::lock_guard<std::mutex> lock(ctx->mu);
    if (n_live < 0 || n_live > n || bound < -1) return fail(DCTFP_ERR_INVALID, "dctfp_linkage_nearest: a live list of %lld ids for %lld nodes, or a bound below -1", (long long)n_live, (long long)n);
    if (((reinterpret_cast<uintptr_t>(size) | reinterpret_cast<uintptr_t>(live) | reinterpret_cast<uintptr_t>(nn)) & 3u) != 0)
        return fail(DCTFP_ERR_INVALID, "dctfp_linkage_nearest: size, live or nn is not 4-byte aligned");
    if (n == 0 || n_live == 0) return DCTFP_OK;
    // (one workgroup per live row: at most 46340 of them)
    return on_device(ctx, [&] { launch_linkage_nearest(mat, wide, n, ld, size, live, n_live, bound, nn, (hipStream_t)stream_v); });
} DCTFP_GUARD("dctfp_linkage_nearest")

int dctfp_linkage_merge(dctfp_ctx* ctx, void* mat, int32_t wide, int64_t n, int64_t ld, const int32_t* size, const int32_t* partner,
                        const int32_t* keep, int64_t n_keep, void* stream_v) try {
    if (n > DCTFP_LINKAGE_MAX_N) return fail(DCTFP_ERR_LIMIT, "dctfp_linkage_merge: more than %d nodes", DCTFP_LINKAGE_MAX_N);
    if (!ctx || !size || !partner || !keep) return fail(DCTFP_ERR_INVALID, "dctfp_linkage_merge: NULL argument");
    RC_TRY(check_linkage_matrix("dctfp_linkage_merge", mat, wide, n, ld));
    std::lock_guard<std::mutex> lock(ctx->mu);
    if (n_keep < 0 || n_keep > n / 2) return fail(DCTFP_ERR_INVALID, "dctfp_linkage_merge: %lld pairs of %lld nodes", (long long)n_keep, (long long)n);
    if (((reinterpret_cast<uintptr_t>(size) | reinterpret_cast<uintptr_t>(partner) | reinterpret_cast<uintptr_t>(keep)) & 3u) != 0)
        return fail(DCTFP_ERR_INVALID, "dctfp_linkage_merge: size, partner or keep is not 4-byte aligned");
    if (n == 0 || n_keep == 0) return DCTFP_OK;
    // (the grid: ceil(n / 256) x n_keep workgroups, n_keep <= 23170 < 65536)
    return on_device(ctx, [&] { launch_linkage_merge(mat, wide, n, ld, size, partner, keep, n_keep, (hipStream_t)stream_v); });
} DCTFP_GUARD("dctfp_linkage_merge")

// What the five exports of the band walk over a triangle (band_walk.hip.h) ask of the tile and of n_nodes; `name` = the export, for the
// message.  The arrays beside the tile are checked by the export that knows them.
static int check_band_tile(const char* name, const TriTile& t, int64_t n_nodes) {
    if (t.n_rows < 0 || t.n_cols < 0 || t.ld < t.n_cols || t.row0 < 0 || t.col0 < 0 || t.cap < 0 || t.bound < -1 || t.bound > t.cap)
        return fail(DCTFP_ERR_INVALID, "%s: bad shape, cap or bound", name);
    if ((reinterpret_cast<uintptr_t>(t.tile) & 3u) != 0) return fail(DCTFP_ERR_INVALID, "%s: the tile is not 4-byte aligned", name);
    if (n_nodes < 0 || n_nodes > 0x7fffffff) return fail(DCTFP_ERR_INVALID, "%s: n_nodes must lie in 0 .. 2^31 - 1", name);
    // (every index the kernel can form lies inside the tile and the arrays: bounded here, on the host, and not on the device)
    if (t.n_rows > n_nodes || t.row0 > n_nodes - t.n_rows || t.n_cols > n_nodes || t.col0 > n_nodes - t.n_cols)
        return fail(DCTFP_ERR_INVALID, "%s: the tile names proteins outside the arrays", name);
    return DCTFP_OK;
}

int dctfp_rect_best(dctfp_ctx* ctx, const int32_t* tile, int64_t n_rows, int64_t n_cols, int64_t ld, int64_t row0, int64_t col0,
                    const uint8_t* row_empty, const uint8_t* col_empty, int32_t cap, int32_t bound, uint64_t* best_row, int64_t n_a,
                    uint64_t* best_col, int64_t n_b, void* stream_v) try {
    if (!ctx || !tile || !best_row || !best_col) return fail(DCTFP_ERR_INVALID, "dctfp_rect_best: NULL argument");
    std::lock_guard<std::mutex> lock(ctx->mu);
    // (a rectangle, not a tile of the triangle: its own few conditions)
    if (n_rows < 0 || n_cols < 0 || ld < n_cols || row0 < 0 || col0 < 0 || cap < 0 || bound < -1 || bound > cap)
        return fail(DCTFP_ERR_INVALID, "dctfp_rect_best: bad shape or bound");
    if (((reinterpret_cast<uintptr_t>(tile) & 3u) | ((reinterpret_cast<uintptr_t>(best_row) | reinterpret_cast<uintptr_t>(best_col)) & 7u)) != 0)
        return fail(DCTFP_ERR_INVALID, "dctfp_rect_best: the tile is not 4-byte aligned or best_row / best_col not 8-byte aligned");
    if (cap > rect_best_max_cap())
        return fail(DCTFP_ERR_INVALID, "dctfp_rect_best: a cap above %d does not fit the packed minima of a row", rect_best_max_cap());
    if (n_a < 0 || n_b < 0 || n_a > 0x7fffffff || n_b > 0x7fffffff) return fail(DCTFP_ERR_INVALID, "dctfp_rect_best: n_a and n_b must lie in 0 .. 2^31 - 1");
    // (every index the kernel can form lies inside the tile: bounded here, on the host, and not on the device)
    if (!range_within(row0, n_rows, n_a) || !range_within(col0, n_cols, n_b))
        return fail(DCTFP_ERR_INVALID, "dctfp_rect_best: the tile names proteins outside best_row / best_col");
    if (n_rows == 0 || n_cols == 0) return DCTFP_OK;
    return on_device(ctx, [&] {
        launch_rect_best(TriTile{tile, n_rows, n_cols, ld, row0, col0, row_empty, col_empty, cap, bound}, best_row, best_col, (hipStream_t)stream_v);
    });
} DCTFP_GUARD("dctfp_rect_best")

int dctfp_label_sums(dctfp_ctx* ctx, const int32_t* tile, int64_t n_rows, int64_t n_cols, int64_t ld, int64_t row0, int64_t col0,
                     const uint8_t* row_empty, const uint8_t* col_empty, int32_t cap, int32_t bound, const int32_t* labels, uint64_t* sums,
                     int64_t n_nodes, void* stream_v) try {
    (void)bound;   // (a sum has no cut-off: every pair of one label counts, with its key -- the tile's bound is its cap)
    if (!ctx || !tile || !labels || !sums) return fail(DCTFP_ERR_INVALID, "dctfp_label_sums: NULL argument");
    std::lock_guard<std::mutex> lock(ctx->mu);
    const TriTile t{tile, n_rows, n_cols, ld, row0, col0, row_empty, col_empty, cap, cap};
    RC_TRY(check_band_tile("dctfp_label_sums", t, n_nodes));
    if ((reinterpret_cast<uintptr_t>(labels) & 3u) != 0 || (reinterpret_cast<uintptr_t>(sums) & 7u) != 0)
        return fail(DCTFP_ERR_INVALID, "dctfp_label_sums: the labels are not 4-byte aligned or sums is not 8-byte aligned");
    if (cap > label_sums_max_cap())
        return fail(DCTFP_ERR_INVALID, "dctfp_label_sums: a cap above %d does not fit the 32-bit partial sums of a row", label_sums_max_cap());
    if (n_rows == 0 || n_cols == 0) return DCTFP_OK;
    return on_device(ctx, [&] { launch_label_sums(t, labels, sums, (hipStream_t)stream_v); });
} DCTFP_GUARD("dctfp_label_sums")

int dctfp_tri_degree(dctfp_ctx* ctx, const int32_t* tile, int64_t n_rows, int64_t n_cols, int64_t ld, int64_t row0, int64_t col0,
                     const uint8_t* row_empty, const uint8_t* col_empty, int32_t cap, int32_t bound, uint32_t* deg, int64_t n_nodes,
                     void* stream_v) try {
    if (!ctx || !tile || !deg) return fail(DCTFP_ERR_INVALID, "dctfp_tri_degree: NULL argument");
    std::lock_guard<std::mutex> lock(ctx->mu);
    const TriTile t{tile, n_rows, n_cols, ld, row0, col0, row_empty, col_empty, cap, bound};
    RC_TRY(check_band_tile("dctfp_tri_degree", t, n_nodes));
    if ((reinterpret_cast<uintptr_t>(deg) & 3u) != 0) return fail(DCTFP_ERR_INVALID, "dctfp_tri_degree: deg is not 4-byte aligned");
    if (n_rows == 0 || n_cols == 0) return DCTFP_OK;
    return on_device(ctx, [&] { launch_tri_degree(t, deg, (hipStream_t)stream_v); });
} DCTFP_GUARD("dctfp_tri_degree")

int dctfp_tri_link_core(dctfp_ctx* ctx, const int32_t* tile, int64_t n_rows, int64_t n_cols, int64_t ld, int64_t row0, int64_t col0,
                        const uint8_t* row_empty, const uint8_t* col_empty, int32_t cap, int32_t bound, const uint8_t* core, int32_t* parent,
                        int32_t* nearest, int64_t n_nodes, void* stream_v) try {
    if (!ctx || !tile || !core || !parent || !nearest) return fail(DCTFP_ERR_INVALID, "dctfp_tri_link_core: NULL argument");
    std::lock_guard<std::mutex> lock(ctx->mu);
    const TriTile t{tile, n_rows, n_cols, ld, row0, col0, row_empty, col_empty, cap, bound};
    RC_TRY(check_band_tile("dctfp_tri_link_core", t, n_nodes));
    if (((reinterpret_cast<uintptr_t>(parent) | reinterpret_cast<uintptr_t>(nearest)) & 3u) != 0)
        return fail(DCTFP_ERR_INVALID, "dctfp_tri_link_core: parent or nearest is not 4-byte aligned");
    if (n_rows == 0 || n_cols == 0) return DCTFP_OK;
    return on_device(ctx, [&] { launch_tri_link_core(t, core, parent, nearest, (hipStream_t)stream_v); });
} DCTFP_GUARD("dctfp_tri_link_core")

// dct-sim --auc1 (k_auc.hip)
int dctfp_tri_first_fp(dctfp_ctx* ctx, const int32_t* tile, int64_t n_rows, int64_t n_cols, int64_t ld, int64_t row0, int64_t col0,
                       const uint8_t* row_empty, const uint8_t* col_empty, int32_t cap, int32_t bound, const int32_t* fam, uint64_t* first,
                       int64_t n_nodes, void* stream_v) try {
    if (!ctx || !tile || !fam || !first) return fail(DCTFP_ERR_INVALID, "dctfp_tri_first_fp: NULL argument");
    std::lock_guard<std::mutex> lock(ctx->mu);
    const TriTile t{tile, n_rows, n_cols, ld, row0, col0, row_empty, col_empty, cap, bound};
    RC_TRY(check_band_tile("dctfp_tri_first_fp", t, n_nodes));
    if ((reinterpret_cast<uintptr_t>(fam) & 3u) != 0 || (reinterpret_cast<uintptr_t>(first) & 7u) != 0)
        return fail(DCTFP_ERR_INVALID, "dctfp_tri_first_fp: fam is not 4-byte aligned or first not 8-byte aligned");
    if (cap > rect_best_max_cap())
        return fail(DCTFP_ERR_INVALID, "dctfp_tri_first_fp: a cap above %d does not fit the packed minima of a row", rect_best_max_cap());
    if (n_rows == 0 || n_cols == 0) return DCTFP_OK;
    return on_device(ctx, [&] { launch_tri_first_fp(t, fam, first, (hipStream_t)stream_v); });
} DCTFP_GUARD("dctfp_tri_first_fp")

int dctfp_tri_tp_before(dctfp_ctx* ctx, const int32_t* tile, int64_t n_rows, int64_t n_cols, int64_t ld, int64_t row0, int64_t col0,
                        const uint8_t* row_empty, const uint8_t* col_empty, int32_t cap, int32_t bound, const int32_t* fam,
                        const uint64_t* first, uint32_t* tp, int64_t n_nodes, void* stream_v) try {
    if (!ctx || !tile || !fam || !first || !tp) return fail(DCTFP_ERR_INVALID, "dctfp_tri_tp_before: NULL argument");
    std::lock_guard<std::mutex> lock(ctx->mu);
    const TriTile t{tile, n_rows, n_cols, ld, row0, col0, row_empty, col_empty, cap, bound};
    RC_TRY(check_band_tile("dctfp_tri_tp_before", t, n_nodes));
    if (((reinterpret_cast<uintptr_t>(fam) | reinterpret_cast<uintptr_t>(tp)) & 3u) != 0 || (reinterpret_cast<uintptr_t>(first) & 7u) != 0)
        return fail(DCTFP_ERR_INVALID, "dctfp_tri_tp_before: fam or tp is not 4-byte aligned or first not 8-byte aligned");
    if (n_rows == 0 || n_cols == 0) return DCTFP_OK;
    return on_device(ctx, [&] { launch_tri_tp_before(t, fam, first, tp, (hipStream_t)stream_v); });
} DCTFP_GUARD("dctfp_tri_tp_before")

// dct-sim --hist (k_hist.hip)
int dctfp_tri_hist(dctfp_ctx* ctx, const int32_t* tile, int64_t n_rows, int64_t n_cols, int64_t ld, int64_t row0, int64_t col0,
                   const uint8_t* row_empty, const uint8_t* col_empty, int32_t cap, int32_t bound, const int32_t* fam, int64_t n_nodes,
                   uint64_t* hist, void* stream_v) try {
    if (!ctx || !tile || !hist) return fail(DCTFP_ERR_INVALID, "dctfp_tri_hist: NULL argument");
    std::lock_guard<std::mutex> lock(ctx->mu);
    // (one array for the whole grid, not an array per protein: its own few conditions)
    if (n_rows < 0 || n_cols < 0 || ld < n_cols || row0 < 0 || col0 < 0 || cap < 0 || bound < -1 || bound > cap)
        return fail(DCTFP_ERR_INVALID, "dctfp_tri_hist: bad shape, cap or bound");
    if (((reinterpret_cast<uintptr_t>(tile) | reinterpret_cast<uintptr_t>(fam)) & 3u) != 0 || (reinterpret_cast<uintptr_t>(hist) & 7u) != 0)
        return fail(DCTFP_ERR_INVALID, "dctfp_tri_hist: the tile or fam is not 4-byte aligned or hist not 8-byte aligned");
    if (cap > tri_hist_max_cap())
        return fail(DCTFP_ERR_INVALID, "dctfp_tri_hist: a cap above %d does not fit the counters of two classes in the LDS of a CU", tri_hist_max_cap());
    if (n_nodes < 0 || n_nodes > 0x7fffffff) return fail(DCTFP_ERR_INVALID, "dctfp_tri_hist: n_nodes must lie in 0 .. 2^31 - 1");
    // (every index the kernel can form lies inside the tile and fam: bounded here, on the host, and not on the device)
    if (n_rows > n_nodes || row0 > n_nodes - n_rows || n_cols > n_nodes || col0 > n_nodes - n_cols)
        return fail(DCTFP_ERR_INVALID, "dctfp_tri_hist: the tile names proteins outside fam");
    if (n_rows == 0 || n_cols == 0) return DCTFP_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    LaunchError le;
    RC_TRY(launcher_rc(launch_tri_hist(TriTile{tile, n_rows, n_cols, ld, row0, col0, row_empty, col_empty, cap, bound}, fam, hist,
                                       (hipStream_t)stream_v, &le), le));
    HIP_TRY(hipGetLastError());
    return DCTFP_OK;
} DCTFP_GUARD("dctfp_tri_hist")

// dct-sim --db --zscore (k_moments.hip)
int dctfp_rect_moments(dctfp_ctx* ctx, const int32_t* tile, int64_t n_rows, int64_t n_cols, int64_t ld, int64_t row0, int64_t col0,
                       const uint8_t* row_empty, const uint8_t* col_empty, int32_t cap, int32_t bound, uint64_t* row_mom, int64_t n_a,
                       uint64_t* col_mom, int64_t n_b, void* stream_v) try {
    (void)bound;   // (a moment has no cut-off: cap is the exclusion limit and nothing else is compared)
    if (!ctx || !tile) return fail(DCTFP_ERR_INVALID, "dctfp_rect_moments: NULL argument");
    if (!row_mom && !col_mom) return fail(DCTFP_ERR_INVALID, "dctfp_rect_moments: row_mom and col_mom are both NULL");
    std::lock_guard<std::mutex> lock(ctx->mu);
    // (a rectangle with three words per protein, either side optional: its own few conditions)
    if (n_rows < 0 || n_cols < 0 || n_rows > 0x7fffffff || n_cols > 0x7fffffff || ld < n_cols || row0 < 0 || col0 < 0 || row0 > 0x7fffffff ||
        col0 > 0x7fffffff || cap < 0)
        return fail(DCTFP_ERR_INVALID, "dctfp_rect_moments: bad shape or cap");
    if (((reinterpret_cast<uintptr_t>(tile) & 3u) | ((reinterpret_cast<uintptr_t>(row_mom) | reinterpret_cast<uintptr_t>(col_mom)) & 7u)) != 0)
        return fail(DCTFP_ERR_INVALID, "dctfp_rect_moments: the tile is not 4-byte aligned or row_mom / col_mom not 8-byte aligned");
    if (cap > rect_moments_max_cap())
        return fail(DCTFP_ERR_INVALID, "dctfp_rect_moments: a cap above %d does not fit the 32-bit partial sums of a row", rect_moments_max_cap());
    if (n_a < 0 || n_b < 0 || n_a > 0x7fffffff || n_b > 0x7fffffff) return fail(DCTFP_ERR_INVALID, "dctfp_rect_moments: n_a and n_b must lie in 0 .. 2^31 - 1");
    // (every index the kernel can form lies inside the tile and the arrays it was given: bounded here, on the host, and not on the device)
    if ((row_mom && !range_within(row0, n_rows, n_a)) || (col_mom && !range_within(col0, n_cols, n_b)))
        return fail(DCTFP_ERR_INVALID, "dctfp_rect_moments: the tile names proteins outside row_mom / col_mom");
    // a row's words add up over the columns it meets and a column's over its rows: n_b resp. n_a of them, at least this tile's
    if (cap > 1) {
        const unsigned __int128 sq = (unsigned __int128)(cap - 1) * (unsigned __int128)(cap - 1), most = ~(uint64_t)0;
        const int64_t over_cols = std::max(n_b, col0 + n_cols), over_rows = std::max(n_a, row0 + n_rows);
        if ((row_mom && sq * (unsigned __int128)over_cols > most) || (col_mom && sq * (unsigned __int128)over_rows > most))
            return fail(DCTFP_ERR_INVALID, "dctfp_rect_moments: n x (cap - 1)^2 does not fit the 64 bits of a sum of squares");
    }
    if (n_rows == 0 || n_cols == 0) return DCTFP_OK;
    return on_device(ctx, [&] {
        launch_rect_moments(TriTile{tile, n_rows, n_cols, ld, row0, col0, row_empty, col_empty, cap, cap}, row_mom, n_a, col_mom, n_b,
                            (hipStream_t)stream_v);
    });
} DCTFP_GUARD("dctfp_rect_moments")

// python -m dctdomain_amd.cluster_quality (k_silhouette.hip; include/dctfp_silhouette.h)
int dctfp_silhouette_version(void) { return DCTFP_SILHOUETTE_VERSION; }

int dctfp_silhouette_rows(dctfp_ctx* ctx, const int32_t* tile, int64_t n_rows, int64_t n_cols, int64_t ld, int64_t row0, int64_t col0,
                          const uint8_t* row_empty, const uint8_t* col_empty, int32_t cap, const int32_t* cid, const int32_t* size,
                          const int32_t* first, int64_t n_clusters, int32_t pass_clusters, uint64_t* own_sum, uint64_t* near_sum,
                          int32_t* near_size, int32_t* near_first, int64_t n_nodes, void* stream_v) try {
    static_assert(DCTFP_SILHOUETTE_MAX_CAP == 1 << 22 && DCTFP_SILHOUETTE_MAX_PASS_CLUSTERS == 4096, "the header states the kernel's limits");
    // the limits first: they hold whatever else is passed
    if (cap > silhouette_max_cap())
        return fail(DCTFP_ERR_LIMIT, "dctfp_silhouette_rows: a cap above %d does not keep a sum below 2^53", silhouette_max_cap());
    if (pass_clusters > silhouette_max_pass())
        return fail(DCTFP_ERR_LIMIT, "dctfp_silhouette_rows: more than %d clusters to a pass do not fit the LDS of a workgroup", silhouette_max_pass());
    if (n_nodes > 0x7fffffff) return fail(DCTFP_ERR_LIMIT, "dctfp_silhouette_rows: n_nodes must lie in 0 .. 2^31 - 1");
    if (!ctx || !tile || !cid || !own_sum || !near_sum || !near_size || !near_first)
        return fail(DCTFP_ERR_INVALID, "dctfp_silhouette_rows: NULL argument");
    std::lock_guard<std::mutex> lock(ctx->mu);
    // (a full row per workgroup and four words per protein: its own few conditions)
    if (n_rows < 0 || n_cols < 0 || ld < n_cols || row0 < 0 || col0 < 0 || cap < 0 || n_nodes < 0)
        return fail(DCTFP_ERR_INVALID, "dctfp_silhouette_rows: bad shape or cap");
    if (pass_clusters < 1) return fail(DCTFP_ERR_INVALID, "dctfp_silhouette_rows: pass_clusters must lie in 1 .. %d", silhouette_max_pass());
    if (n_clusters < 0 || n_clusters > n_nodes / 2)
        return fail(DCTFP_ERR_INVALID, "dctfp_silhouette_rows: %lld clusters of two or more members among %lld proteins", (long long)n_clusters, (long long)n_nodes);
    if (n_clusters > 0 && (!size || !first)) return fail(DCTFP_ERR_INVALID, "dctfp_silhouette_rows: NULL size or first with clusters to read");
    if (((reinterpret_cast<uintptr_t>(tile) | reinterpret_cast<uintptr_t>(cid) | reinterpret_cast<uintptr_t>(size) | reinterpret_cast<uintptr_t>(first) |
          reinterpret_cast<uintptr_t>(near_size) | reinterpret_cast<uintptr_t>(near_first)) & 3u) != 0 ||
        ((reinterpret_cast<uintptr_t>(own_sum) | reinterpret_cast<uintptr_t>(near_sum)) & 7u) != 0)
        return fail(DCTFP_ERR_INVALID, "dctfp_silhouette_rows: the tile or an int32 array is not 4-byte aligned or own_sum / near_sum not 8-byte aligned");
    // (every index the kernel can form lies inside the tile and the arrays of n_nodes entries: bounded here, on the host, and not on
    // the device -- but for cid's values, which the caller vouches for: include/dctfp_silhouette.h)
    if (!range_within(row0, n_rows, n_nodes) || !range_within(col0, n_cols, n_nodes))
        return fail(DCTFP_ERR_INVALID, "dctfp_silhouette_rows: the tile names proteins outside the arrays of n_nodes entries");
    if (n_rows == 0 || n_cols == 0) return DCTFP_OK;
    return on_device(ctx, [&] {
        launch_silhouette_rows(TriTile{tile, n_rows, n_cols, ld, row0, col0, row_empty, col_empty, cap, cap}, cid, size, first,
                               (int32_t)n_clusters, pass_clusters, own_sum, near_sum, near_size, near_first, (hipStream_t)stream_v);
    });
} DCTFP_GUARD("dctfp_silhouette_rows")

int dctfp_greedy_decide(dctfp_ctx* ctx, int32_t* assign, int32_t* state, const int32_t* blocked, int64_t n_nodes, int64_t i0, int64_t i1,
                        int32_t round, int64_t* undecided, void* stream_v) try {
    if (!ctx || !assign || !state || !blocked || !undecided) return fail(DCTFP_ERR_INVALID, "dctfp_greedy_decide: NULL argument");
    std::lock_guard<std::mutex> lock(ctx->mu);
    if (n_nodes < 0 || i0 < 0 || i1 < i0 || round < 0) return fail(DCTFP_ERR_INVALID, "dctfp_greedy_decide: bad shape or round");
    if (n_nodes > 0x7fffffff) return fail(DCTFP_ERR_LIMIT, "dctfp_greedy_decide: more than 2^31 - 1 nodes");
    if (i1 > n_nodes) return fail(DCTFP_ERR_INVALID, "dctfp_greedy_decide: the range names proteins outside the nodes");
    if (i1 == i0) return DCTFP_OK;
    return on_device(ctx, [&] {
        launch_greedy_decide(assign, state, blocked, i0, i1, round, reinterpret_cast<unsigned long long*>(undecided), (hipStream_t)stream_v);
    });
} DCTFP_GUARD("dctfp_greedy_decide")

int dctfp_greedy_tri_mark(dctfp_ctx* ctx, const int32_t* tile, int64_t n_rows, int64_t n_cols, int64_t ld, int64_t row0, int64_t col0,
                          const uint8_t* row_empty, const uint8_t* col_empty, int32_t cap, int32_t bound, int32_t* assign, const int32_t* state,
                          int32_t* blocked, int64_t n_nodes, int64_t range_end, int32_t next_round, void* stream_v) try {
    if (!ctx || !tile || !assign || !state || !blocked) return fail(DCTFP_ERR_INVALID, "dctfp_greedy_tri_mark: NULL argument");
    std::lock_guard<std::mutex> lock(ctx->mu);
    const TriTile t{tile, n_rows, n_cols, ld, row0, col0, row_empty, col_empty, cap, bound};
    RC_TRY(check_tri_tile("dctfp_greedy_tri_mark", t));
    if (range_end < 0 || next_round < 1) return fail(DCTFP_ERR_INVALID, "dctfp_greedy_tri_mark: bad range or round");
    if (n_nodes > 0x7fffffff) return fail(DCTFP_ERR_LIMIT, "dctfp_greedy_tri_mark: more than 2^31 - 1 nodes");
    RC_TRY(check_tri_nodes("dctfp_greedy_tri_mark", t, n_nodes));
    if (range_end > n_nodes) return fail(DCTFP_ERR_INVALID, "dctfp_greedy_tri_mark: the range (every stamp lies below it) ends outside the nodes");
    if (n_rows == 0 || n_cols == 0 || n_nodes == 0) return DCTFP_OK;
    return on_device(ctx, [&] { launch_greedy_tri_mark(t, assign, state, blocked, range_end, next_round, (hipStream_t)stream_v); });
} DCTFP_GUARD("dctfp_greedy_tri_mark")

int dctfp_greedy_pairs_mark(dctfp_ctx* ctx, const int32_t* pi, const int32_t* pj, int64_t n_pairs, int32_t* assign, const int32_t* state,
                            int32_t* blocked, int64_t n_nodes, int64_t range_end, int32_t next_round, void* stream_v) try {
    if (!ctx || !assign || !state || !blocked || ((!pi || !pj) && n_pairs > 0)) return fail(DCTFP_ERR_INVALID, "dctfp_greedy_pairs_mark: NULL argument");
    std::lock_guard<std::mutex> lock(ctx->mu);
    if (n_pairs < 0 || n_nodes < 0 || range_end < 0 || next_round < 1) return fail(DCTFP_ERR_INVALID, "dctfp_greedy_pairs_mark: bad shape or round");
    // (one thread per pair in 256-thread workgroups, as dctfp_link_pairs' limit)
    if (n_nodes > 0x7fffffff || n_pairs > (int64_t)1 << 31)
        return fail(DCTFP_ERR_LIMIT, "dctfp_greedy_pairs_mark: more than 2^31 - 1 nodes or 2^31 pairs per call");
    if (range_end > n_nodes) return fail(DCTFP_ERR_INVALID, "dctfp_greedy_pairs_mark: the range names proteins outside the nodes");
    if (n_pairs == 0 || n_nodes == 0) return DCTFP_OK;
    return on_device(ctx, [&] { launch_greedy_pairs_mark(pi, pj, n_pairs, assign, state, blocked, n_nodes, range_end, next_round, (hipStream_t)stream_v); });
} DCTFP_GUARD("dctfp_greedy_pairs_mark")

int dctfp_l1_knn(dctfp_ctx* ctx, const int8_t* q, int64_t nq, int64_t ldq, const int8_t* b, int64_t nb, int64_t ldb, int32_t d, int32_t k,
                 int64_t col0, int32_t* out_val, int32_t* out_idx, void* stream_v) try {
    if (!ctx || !q || !b || !out_val || !out_idx) return fail(DCTFP_ERR_INVALID, "dctfp_l1_knn: NULL argument");
    std::lock_guard<std::mutex> lock(ctx->mu);
    if (nq < 0 || nb < 0 || d < 1 || ldq < d || ldb < d || k < 1 || col0 < 0) return fail(DCTFP_ERR_INVALID, "dctfp_l1_knn: bad shape");
    if (((reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(b) | (uintptr_t)ldq | (uintptr_t)ldb) & 15u) != 0)
        return fail(DCTFP_ERR_INVALID, "dctfp_l1_knn: fingerprint rows must start on 16-byte boundaries");
    if (nq == 0 || nb == 0) return DCTFP_OK;
    if (k > 1024 || d > 512) return fail(DCTFP_ERR_LIMIT, "dctfp_l1_knn: k above 1024 or rows above 512 bytes (use l1_matrix + row_select)");
    if (nq > 65535 * 128 || !range_within(col0, nb, 0x7fffffff) || ldq >= (1 << 24) || ldb >= (1 << 24))
        return fail(DCTFP_ERR_LIMIT, "dctfp_l1_knn: more than 8M query rows, 2^31 - 1 columns or 2^24-byte rows per call");
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t stream = (hipStream_t)stream_v;
    const int slices = knn_slices(nq, nb, k);
    Hold scratch{ctx->scratch, stream};   // the rows' k-lists (and the slices' candidates): given back after the last kernel
    int rc = scratch.take(knn_scratch_bytes(nq, k, slices), stream);
    if (rc) return rc;
    ctx->last_knn_slices = launch_l1_knn(q, nq, ldq, b, nb, ldb, d, k, slices, scratch.p(), out_val, out_idx, col0, stream);
    ++ctx->knn_calls;
    HIP_TRY(hipGetLastError());
    return scratch.give_back();
} DCTFP_GUARD("dctfp_l1_knn")

int dctfp_query_rank(dctfp_ctx* ctx, const int32_t* val, const int32_t* idx, int64_t n_rows, int32_t k, const int64_t* qoff,
                     const int32_t* prot_of_row, const int64_t* line_base, int32_t khits, int32_t* out_qrow, int32_t* out_drow,
                     int32_t* out_dist, void* stream_v) try {
    if (!ctx || !val || !idx || !qoff || !prot_of_row || !line_base || !out_qrow || !out_drow || !out_dist)
        return fail(DCTFP_ERR_INVALID, "dctfp_query_rank: NULL argument");
    std::lock_guard<std::mutex> lock(ctx->mu);
    if (n_rows < 0 || k < 1 || khits < 1) return fail(DCTFP_ERR_INVALID, "dctfp_query_rank: bad shape");
    // (one thread per hit in 256-thread workgroups)
    if (n_rows > launch_items(256, 256) / k)
        return fail(DCTFP_ERR_LIMIT, "dctfp_query_rank: more than %lld hits (n_rows x k) per call", (long long)launch_items(256, 256));
    if (n_rows == 0) return DCTFP_OK;
    return on_device(ctx, [&] { launch_query_rank(val, idx, n_rows, k, qoff, prot_of_row, line_base, khits, out_qrow, out_drow, out_dist, (hipStream_t)stream_v); });
} DCTFP_GUARD("dctfp_query_rank")

int dctfp_query_lines(dctfp_ctx* ctx, int64_t n_lines, const int32_t* qrow, const int32_t* drow, const int32_t* dist, const int32_t* rank,
                      const uint8_t* q_txt, const int64_t* q_pid_off, const int64_t* q_dom_off, const uint8_t* d_txt, const int64_t* d_pid_off,
                      const int64_t* d_dom_off, const uint8_t* score_txt, const int64_t* score_off, const int64_t* line_off, uint8_t* out,
                      void* stream_v) try {
    if (!ctx || !qrow || !drow || !dist || !rank || !q_txt || !q_pid_off || !q_dom_off || !d_txt || !d_pid_off || !d_dom_off || !score_txt ||
        !score_off || !line_off || !out)
        return fail(DCTFP_ERR_INVALID, "dctfp_query_lines: NULL argument");
    std::lock_guard<std::mutex> lock(ctx->mu);
    if (n_lines < 0) return fail(DCTFP_ERR_INVALID, "dctfp_query_lines: bad shape");
    if (!one_launch(n_lines, 256, 256))
        return fail(DCTFP_ERR_LIMIT, "dctfp_query_lines: more than %lld lines per call", (long long)launch_items(256, 256));
    if (n_lines == 0) return DCTFP_OK;
    return on_device(ctx, [&] {
        launch_query_lines(n_lines, qrow, drow, dist, rank, q_txt, q_pid_off, q_dom_off, d_txt, d_pid_off, d_dom_off, score_txt, score_off, line_off,
                           out, (hipStream_t)stream_v);
    });
} DCTFP_GUARD("dctfp_query_lines")

}  // extern "C"
