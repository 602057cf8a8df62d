// Launchers of the gfx950 kernels, one translation unit per kernel family so that they compile side by side
// (build_ext.py): the stage-A instantiations alone are a third of the device code.  dctfp.hip -- the host side of the C
// ABI -- sees the parameter blocks and the launcher declarations below and no kernel template of these families.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>
#include <cstdint>

#include "dctfp.h"

#ifndef DCTFP_MAX_N_K
#define DCTFP_MAX_N_K DCTFP_MAX_N
#define DCTFP_MAX_M_K DCTFP_MAX_M
#endif
#include "kernels.hip.h"

namespace dctfp {
struct CutJob;   // reccut_kernel.hip.h
struct TriTile;  // tri_tile.hip.h
}

namespace dctfp_host {

using namespace dctfp;

// A failure inside a launcher: the code and the message (at most 255 bytes) it wants dctfp_last_error() to carry.
struct LaunchError {
    int code = 0;
    char msg[256] = "";
};
int launch_fail(LaunchError* err, int code, const char* fmt, ...);

// cos(pi p / q) in long double with exact integer argument reduction (p >= 0, q > 0).
inline long double cospi_ratio_host(int64_t p, int64_t q) {
    p %= 2 * q;
    if (p > q) p = 2 * q - p;
    long double sign = 1.0L;
    if (2 * p > q) {
        p = q - p;
        sign = -1.0L;
    }
    const long double pi = 3.141592653589793238462643383279502884L;
    long double r = (4 * p > q) ? sinl(pi * (long double)(q - 2 * p) / (long double)(2 * q))
                                : cosl(pi * (long double)p / (long double)q);
    return sign * r;
}

template <int N>
inline InvTab<N> make_inv() {
    InvTab<N> t;
    if constexpr (N > 1) {
        for (int j = 0; j < N; ++j)
            for (int k = 1; k < N; ++k)
                t.c[j * (N - 1) + (k - 1)] = (double)cospi_ratio_host((int64_t)k * (2 * j + 1), 2 * (int64_t)N);
    } else {
        t.c[0] = 0.0;
    }
    return t;
}

// What the options "last_stage_a" / "last_stage_b" read (include/dctfp.h has the layout): one byte per field, filled in by
// whoever launches from the template arguments of the instantiation it names -- never from what the dispatcher asked for.
template <typename T> constexpr int64_t storage_code();
template <> constexpr int64_t storage_code<float>() { return DCTFP_F32 + 1; }
template <> constexpr int64_t storage_code<double>() { return DCTFP_F64 + 1; }
template <> constexpr int64_t storage_code<_Float16>() { return DCTFP_F16 + 1; }
template <> constexpr int64_t storage_code<bf16_t>() { return DCTFP_BF16 + 1; }
template <typename T, int N, int VEC, int WAVES, int UNROLL, bool FUSED>
constexpr int64_t stage_a_word(bool packed, bool split) {
    return storage_code<T>() | (int64_t)N << 8 | (int64_t)VEC << 16 | (int64_t)WAVES << 24 | (int64_t)UNROLL << 32 |
           (int64_t)((FUSED ? 1 : 0) | (packed ? 2 : 0) | (split ? 4 : 0)) << 40;
}
constexpr int64_t kStageBMfma = 1, kStageBSlab = 2, kStageBSlabFromSplit = 3;  // "last_stage_b": form ...
constexpr int64_t kStageBPacked = 1 << 16, kStageBCombine = 1 << 17, kStageBCombinePacked = 1 << 18;  // ... and flags
template <int NT, bool PACKED>
constexpr int64_t stage_b_mfma_word() { return kStageBMfma | (int64_t)NT << 8 | (PACKED ? kStageBPacked : 0); }
// ... and "last_walk" / "last_gen", the same for the two one-launch kernels (waves and slots: what the launch was given)
template <typename T, int S, int NT, bool FUSED, bool WIN>
constexpr int64_t walk_word() {
    return storage_code<T>() | (int64_t)S << 8 | (int64_t)NT << 16 | (int64_t)((FUSED ? 1 : 0) | (WIN ? 2 : 0)) << 24;
}
template <typename T, int N, int VEC, bool FUSED, int NTC>
constexpr int64_t gen_word(unsigned waves, int slots) {
    return storage_code<T>() | (int64_t)N << 8 | (int64_t)VEC << 16 | (int64_t)NTC << 24 | (int64_t)(FUSED ? 1 : 0) << 32 |
           (int64_t)(waves & 0xff) << 40 | (int64_t)(slots & 0xff) << 48;
}

struct AParams {
    const JobA* jobs;
    const Walk* walks;
    bool fused;
    const PieceA* pieces;
    unsigned long long* degenerate;
    char* yprime;
    int64_t job_bytes;
    int packed;
    int n_cols;
    int64_t ld;
    int ldy;
    int n_slabs;
    unsigned grid;
    hipStream_t stream;
    int64_t* built;  // the launcher's stage_a_word
};

struct WParams {
    const JobA* jobs;
    const JobB* jobb;
    const Walk* walks;
    const Run* runs;
    const PieceA* pieces;
    const double* stf;
    int8_t* out;
    int n_cols;
    int64_t ld;
    int m;
    unsigned long long* degenerate;
    unsigned grid;
    hipStream_t stream;
    bool two_source = false;  // some piece has PieceA::ptr2 (float32 rows, m <= 80 only)
    int64_t* built = nullptr;  // the launcher's walk_word
};

// walk_gen_kernel: the shapes walk_ab_kernel does not take.
struct GParams {
    const JobA* jobs;
    const JobB* jobb;
    const Walk* walks;   // fused: the walks of the runs (parts + whole protein); else unused
    bool fused;
    const Run* runs;
    const PieceA* pieces;
    const double* stp;
    int8_t* out;
    int n_cols;
    int64_t ld;
    int m;
    int n_slots;
    unsigned long long* degenerate;
    unsigned grid;
    unsigned waves;
    size_t lds_bytes;
    hipStream_t stream;
    int64_t* built = nullptr;  // the launcher's gen_word
};

constexpr size_t kGenLdsBudget = 150 * 1024;  // of the 160 KB of a CU
constexpr int kGenFusedMaxN = 5;              // fused walks of the general kernel: two sets of n - 1 accumulators per channel ...
constexpr int kGenFusedMaxWaves = 10;         // ... in builds bounded to ten waves per workgroup (168 registers)

// LDS of one slot: Y'[N][CH] float64; the partial Z blocks [S][N][cp] reuse it unless a wave's columns are too few
inline size_t gen_slot_bytes(int n, int m, int waves, int vec) {
    const size_t ch = (size_t)waves * 64 * vec, cp = ((size_t)m + 15) / 16 * 16;
    return ((size_t)n * ch + (cp <= (size_t)64 * vec ? 0 : (size_t)waves * n * cp)) * sizeof(double);
}


// stage A (k_stage_a_*.hip: one unit per storage type)
void launch_a_f32(const AParams& p, int vec, int n, int waves);
void launch_a_f64(const AParams& p, int vec, int n, int waves);
void launch_a_f16(const AParams& p, int vec, int n, int waves);
void launch_a_bf16(const AParams& p, int vec, int n, int waves);
// stage B on the matrix pipe (k_stage_b.hip)
// (*built: the stage_b_mfma_word of the instantiation that was launched)
void launch_b_mfma(int nt, bool packed, unsigned grid, hipStream_t s, const char* yp, int64_t job_bytes, int64_t rows,
                   int ldy, const double* st, const JobB* jobs, int n, int m, int8_t* out, int64_t* built);
// the walk kernels (k_walk.hip, k_gen.hip)
int launch_walk(const WParams& p, int dtype, int s, bool fused, LaunchError* err);
int launch_gen(const GParams& p, int dtype, int vec, int n, LaunchError* err);
// the domain cutter's recursion (k_reccut.hip): LDS class of a protein (0 .. 3: 512 / 1024 / 1536 / 2048 residues), launch of one class
constexpr int kCutClasses = 4;
int reccut_class_of(int n_res, int64_t n_contacts);
int launch_reccut(int cls, const dctfp::CutJob* jobs, unsigned n, double cut1, double cut2, hipStream_t stream, LaunchError* err);
// protein-level search (k_search.hip): pair minima from the fingerprints, threshold-aware selection on a last-row distance tile
// (dctfp_pair_min and dctfp_pair_argmin: out_arg_a / out_arg_b = the fingerprint pair the minimum came from, row indices within
// the proteins, -1 = none -- both NULL: dctfp_pair_min's kernel, which keeps no position)
void launch_pair_argmin(const int32_t* pairs, int64_t n_pairs, const int8_t* a, int64_t lda, const int64_t* idx_a, int64_t npa,
                        const int8_t* b, int64_t ldb, const int64_t* idx_b, int64_t npb, int d, int32_t* out_min, int32_t* out_last,
                        int32_t* out_arg_a, int32_t* out_arg_b, hipStream_t stream);
int select_max_cap();   // the largest key the selection's LDS histogram holds
void launch_select_count(const int32_t* dist, int64_t n_rows, int64_t n_cols, int64_t ld, const uint8_t* row_empty, const uint8_t* col_empty,
                         int32_t cap, int32_t bound, int32_t top, int32_t* out_count, int32_t* out_cut, hipStream_t stream);
void launch_select_fill(const int32_t* dist, int64_t n_rows, int64_t n_cols, int64_t ld, const uint8_t* row_empty, const uint8_t* col_empty,
                        int32_t cap, const int32_t* cut, const int64_t* offsets, int32_t max_count, int32_t* out_key, int32_t* out_col,
                        hipStream_t stream);
// all_sim's result lines (k_search.hip): text from a (min, last) tile at offsets computed from the id lengths
void launch_sim_lines(const int32_t* mn, const int32_t* last, int64_t ld, int64_t n_rows, int64_t row0, int64_t col0, int64_t n_cols,
                      const uint8_t* ids, const int64_t* id_off, const char* table, const int64_t* row_base, uint8_t* out, hipStream_t stream);
// all-against-all with score cut-offs (k_filter.hip): the surviving pairs of a tile of the triangle (a TriTile, as for every
// launcher below that takes one) in output order, and result lines for a list of pairs
void launch_tri_filter_count(const TriTile& t, int32_t* out_count, hipStream_t stream);
void launch_tri_filter_fill(const TriTile& t, const int64_t* offsets, int64_t out_len, int32_t* out_i, int32_t* out_j, hipStream_t stream);
// (dctfp_pair_lines and dctfp_pair_domain_lines: labels NULL = the line without the two label fields, la / lb / label_off not read)
void launch_pair_domain_lines(int64_t n_lines, const int32_t* pi, const int32_t* pj, const int32_t* mn, const int32_t* last, const int32_t* la,
                              const int32_t* lb, const uint8_t* ids, const int64_t* id_off, int64_t n_ids, const uint8_t* labels,
                              const int64_t* label_off, int64_t n_labels, const char* table, const int64_t* line_off, uint8_t* out,
                              int64_t out_bytes, hipStream_t stream);

// dct-sim --domain-map (k_map.hip): per pair, every fingerprint row's nearest row of the other protein (dctfp_pair_row_best), and
// dctfp_pair_domain_lines' line with the map of the rows within `bound` behind it (dctfp_pair_map_lines; out_count non-NULL: the
// count pass, every line's byte length and no text)
void launch_pair_row_best(const int32_t* pairs, int64_t n_pairs, const int8_t* a, int64_t lda, const int64_t* idx_a, int64_t npa,
                          const int8_t* b, int64_t ldb, const int64_t* idx_b, int64_t npb, int d, const int64_t* row_off, int64_t out_len,
                          int32_t* out_l1, int32_t* out_arg, hipStream_t stream);
void launch_pair_map_lines(int64_t n_lines, const int32_t* pi, const int32_t* pj, const int32_t* mn, const int32_t* last, const int32_t* la,
                           const int32_t* lb, const uint8_t* ids, const int64_t* id_off, int64_t n_ids, const uint8_t* labels,
                           const int64_t* label_off, int64_t n_labels, const char* table, const int64_t* first_row, const int64_t* row_off,
                           int64_t n_rows, const int32_t* row_l1, const int32_t* row_arg, int32_t bound, const int64_t* line_off, uint8_t* out,
                           int64_t out_bytes, int64_t* out_count, hipStream_t stream);

// single-linkage clusters at a cut-off (k_cluster.hip): unions of a tile's surviving entries / of a list of pairs in a lock-free
// union-find over parent[0 .. n_nodes), and the roots of all nodes afterwards (two launches: flatten, then read)
void launch_tri_link(const TriTile& t, int32_t* parent, hipStream_t stream);
void launch_link_pairs(const int32_t* pi, const int32_t* pj, int64_t n_pairs, int32_t* parent, int64_t n_nodes, hipStream_t stream);
void launch_cluster_labels(int32_t* parent, int64_t n_nodes, int32_t* labels, hipStream_t stream);
// (dctfp_rows_link: the nodes are fingerprint rows -- sad_tile's contraction (sad_tile.hip.h), every pair of rows of different owners
// within the bound joined from the accumulators; the launcher picks the fill by the rows' alignment, sad_tile_align)
void launch_rows_link(const int8_t* a, int64_t na, int64_t lda, int64_t a0, const int8_t* b, int64_t nb, int64_t ldb, int64_t b0, int d,
                      const int32_t* owner, const uint8_t* skip, int32_t cap, int32_t bound, int32_t* parent, hipStream_t stream);

// the single-linkage tree (k_tree.hip): a round of Boruvka's algorithm over the tiles -- tri_link's walk, every surviving entry whose
// ends carry different labels in comp lowers best (packed key << 48 | i << 24 | j) of both labels -- then, once per round, the hook:
// every label appends its best edge at *counter (nothing at or beyond max_edges), joins its ends in parent, and best is refilled
// with "none" behind it on the stream
void launch_tri_nearest(const TriTile& t, const int32_t* comp, uint64_t* best, int64_t n_nodes, hipStream_t stream);
hipError_t launch_tree_hook(const int32_t* comp, uint64_t* best, int32_t* parent, int64_t n_nodes, int32_t* edge_i, int32_t* edge_j,
                            int32_t* edge_key, int32_t* counter, int64_t max_edges, hipStream_t stream);

// complete- and average-linkage clustering (k_linkage.hip; include/dctfp_linkage.h has the state): on a dense n x n matrix of int32
// (wide = 0) or int64 (wide = 1) entries, per live row the nearest live column within the bound (a workgroup per entry of the live
// list, no atomics), and the in-place merge of the pairs of a round (a thread per entry of the rows of keep)
void launch_linkage_nearest(const void* mat, int wide, int64_t n, int64_t ld, const int32_t* size, const int32_t* live, int64_t n_live,
                            int32_t bound, int32_t* nn, hipStream_t stream);
void launch_linkage_merge(void* mat, int wide, int64_t n, int64_t ld, const int32_t* size, const int32_t* partner, const int32_t* keep,
                          int64_t n_keep, hipStream_t stream);

// reciprocal best hits of two files (k_best.hip): one pass over the full rectangle of an int32 L1 tile -- every entry with
// min(L1, cap) <= bound (cap for a flagged protein) lowers best_row[row0 + r] to key << 32 | (col0 + c) and best_col[col0 + c] to
// key << 32 | (row0 + r) with agent-scope atomic minima; rect_best_max_cap = the largest cap the kernel's packed LDS words hold
int rect_best_max_cap();
void launch_rect_best(const TriTile& t, uint64_t* best_row, uint64_t* best_col, hipStream_t stream);

// the summed distances behind a cluster's medoid (k_medoid.hip): the band walk over an int32 L1 tile of one file -- every entry
// with col0 + c > row0 + r whose two proteins carry one label adds min(L1, cap) (cap for a flagged protein) to sums of both, with
// agent-scope 64-bit atomic adds of partial sums kept in 32 bits; label_sums_max_cap = the largest cap for which those cannot overflow
int label_sums_max_cap();
void launch_label_sums(const TriTile& t, const int32_t* labels, uint64_t* sums, hipStream_t stream);

// density clusters (k_density.hip): the band walk over an int32 L1 tile of one file, twice -- every entry tri_filter_count would
// count (col0 + c > row0 + r, min(L1, cap) <= bound, cap for a flagged protein) adds 1 to deg of both ends; then, with core per
// protein, a core-core entry is a union in parent and an entry with one core end lowers nearest of the other end to the core's index.
// Agent-scope atomic adds / minima of parts reduced in the workgroup, and the forest's own atomics
void launch_tri_degree(const TriTile& t, uint32_t* deg, hipStream_t stream);
void launch_tri_link_core(const TriTile& t, const uint8_t* core, int32_t* parent, int32_t* nearest, hipStream_t stream);

// AUC1 of a labelled file (k_auc.hip): the band walk over an int32 L1 tile of one file, twice, with fam (a family per protein)
// beside it -- every entry tri_filter_count would count whose ends are of two families lowers first of both ends to
// key << 32 | the other end (rect_best's packed minima: cap <= rect_best_max_cap()); then, with the finished first, every counted
// entry of one family adds 1 to tp of each end whose own first its word is below.  Agent-scope atomic minima / adds of parts
// reduced in the workgroup
void launch_tri_first_fp(const TriTile& t, const int32_t* fam, uint64_t* first, hipStream_t stream);
void launch_tri_tp_before(const TriTile& t, const int32_t* fam, const uint64_t* first, uint32_t* tp, hipStream_t stream);

// the score distribution of a file (k_hist.hip): a loop of its own over an int32 L1 tile of one file -- every entry tri_degree would
// count adds 1 to hist[cls * (cap + 1) + key], cls = 0 without fam, else fam[i] != fam[j].  32-bit counters private to the workgroup
// in LDS over all its jobs, then one agent-scope 64-bit atomic add per non-zero bin; tri_hist_max_cap = the largest cap whose two
// class rows fit the LDS of a CU.  A tile of more jobs than the counters of a launch can hold goes out as several launches
int tri_hist_max_cap();
int launch_tri_hist(const TriTile& t, const int32_t* fam, uint64_t* hist, hipStream_t stream, LaunchError* err);

// the moments of every protein's background (k_moments.hip): a loop of its own over the full rectangle of an int32 L1 tile -- every
// entry whose row and column are not flagged and whose value x has (uint32_t)x < cap (an exclusion limit; bound is not read) adds
// (1, x, x * x) to row_mom[k * n_a + row0 + r] and to col_mom[k * n_b + col0 + c], k = 0, 1, 2, with agent-scope 64-bit atomic adds
// of parts reduced in the workgroup; either array may be NULL.  rect_moments_max_cap = the largest cap whose 32-bit partial sums
// cannot overflow
int rect_moments_max_cap();
void launch_rect_moments(const TriTile& t, uint64_t* row_mom, int64_t n_a, uint64_t* col_mom, int64_t n_b, hipStream_t stream);

// the sums behind the silhouette of a clustering (k_silhouette.hip; include/dctfp_silhouette.h has the rule): one workgroup per row of
// the full square of an int32 L1 tile of one file -- the key of every column j != i (the tile scans' rule, without a bound) goes to
// the 64-bit LDS sum of j's cluster, pass_clusters cluster ids at a time, a singleton column into a running minimum; per row the sum
// over its own cluster and the other cluster of the smallest mean (sum, size, first member), compared as exact fractions.  No global
// atomics.  silhouette_max_cap = the largest cap whose sums stay below 2^53, silhouette_max_pass = the most sums the LDS of a pass holds
int silhouette_max_cap();
int silhouette_max_pass();
void launch_silhouette_rows(const TriTile& t, const int32_t* cid, const int32_t* size, const int32_t* first, int32_t n_clusters,
                            int32_t pass_clusters, uint64_t* own_sum, uint64_t* near_sum, int32_t* near_size, int32_t* near_first,
                            hipStream_t stream);

// (dctfp_rows_assign, k_assign.hip: the same contraction over a full rectangle -- every pair of rows within the bound lowers
// assign[slot of the b row] to the value of the a row with an atomic minimum; value_a / slot_b NULL: a0 + r / b0 + c)
void launch_rows_assign(const int8_t* a, int64_t na, int64_t lda, const int32_t* value_a, int64_t a0, const int8_t* b, int64_t nb, int64_t ldb,
                        const int32_t* slot_b, int64_t b0, int d, int32_t cap, int32_t bound, int32_t* assign, int64_t n_assign,
                        hipStream_t stream);

// greedy incremental clusters at a cut-off (k_greedy.hip): rounds over a range of nodes [i0, i1) -- decide (one thread per node;
// *undecided grows by the nodes left undecided), then mark from a tile's rows / from a list of pairs (new representatives lower
// assign at their surviving entries, undecided rows stamp blocked inside the range with the next round's number)
void launch_greedy_decide(int32_t* assign, int32_t* state, const int32_t* blocked, int64_t i0, int64_t i1, int32_t round,
                          unsigned long long* undecided, hipStream_t stream);
void launch_greedy_tri_mark(const TriTile& t, int32_t* assign, const int32_t* state, int32_t* blocked, int64_t range_end, int32_t next_round,
                            hipStream_t stream);
void launch_greedy_pairs_mark(const int32_t* pi, const int32_t* pj, int64_t n_pairs, int32_t* assign, const int32_t* state, int32_t* blocked,
                              int64_t n_nodes, int64_t range_end, int32_t next_round, hipStream_t stream);

// DCTdomain of every protein pair from the fingerprints (k_protein.hip): scratch bytes of one side's block plan, and the launches
// (the two plans, then the protein-minimum kernel on a grid of n_workgroups that walks the block pairs); launch_protein_cover: the
// same with the coverage requirement of dct-sim --min-coverage (row weights w_*, per-protein needs need_*, rows matched at L1 <= bound)
size_t protein_plan_bytes(int64_t np);
int launch_protein_min(const int8_t* a, int64_t lda, const int64_t* idx_a, int64_t npa, const int8_t* b, int64_t ldb, const int64_t* idx_b,
                       int64_t npb, int d, int32_t* out, int64_t ldo, void* scratch, int n_workgroups, hipStream_t stream);
int launch_protein_cover(const int8_t* a, int64_t lda, const int64_t* idx_a, int64_t npa, const int32_t* w_a, const int32_t* need_a,
                         const int8_t* b, int64_t ldb, const int64_t* idx_b, int64_t npb, const int32_t* w_b, const int32_t* need_b, int d,
                         int32_t bound, int32_t* out, int64_t ldo, void* scratch, int n_workgroups, hipStream_t stream);

// query_db at database scale (k_query.hip): fused L1 + k nearest, the protein-level ranking, the hit lines as text
int knn_slices(int64_t na, int64_t nb, int k);
size_t knn_scratch_bytes(int64_t na, int k, int n_slices);
// returns the number of slices that own a column (at most n_slices)
int launch_l1_knn(const int8_t* a, int64_t na, int64_t lda, const int8_t* b, int64_t nb, int64_t ldb, int d, int k, int n_slices,
                  void* scratch, int32_t* out_val, int32_t* out_idx, int64_t col0, hipStream_t stream);
void launch_query_rank(const int32_t* val, const int32_t* idx, int64_t n_rows, int k, const int64_t* qoff, const int32_t* prot_of_row,
                       const int64_t* line_base, int khits, int32_t* out_qrow, int32_t* out_drow, int32_t* out_dist, hipStream_t stream);
void launch_query_lines(int64_t n_lines, const int32_t* qrow, const int32_t* drow, const int32_t* dist, const int32_t* rank,
                        const uint8_t* q_txt, const int64_t* q_pid_off, const int64_t* q_dom_off, const uint8_t* d_txt, const int64_t* d_pid_off,
                        const int64_t* d_dom_off, const uint8_t* score_txt, const int64_t* score_off, const int64_t* line_off, uint8_t* out,
                        hipStream_t stream);

}  // namespace dctfp_host
