/* libdctfp: the kernel behind the silhouette of a clustering (python -m dctdomain_amd.cluster_quality).
 *
 * A header of its own beside dctfp.h and dctfp_linkage.h, for the same library, the same dctfp_ctx and the same error codes: the
 * conventions of dctfp.h hold (device pointers, caller-owned buffers, work enqueued on the stream given last, NULL = the default
 * stream).  DCTFP_VERSION does not change with it; this header counts its own version.
 *
 * The rule.  key(i, j) = min(L1(i, j), cap) of two proteins of one file, cap when either has no fingerprint; i == j never counts.
 * A clustering is one label per protein.  For protein i of cluster A, Sa = the sum of key(i, j) over the other members j of A, and
 * for every other cluster B, S(B) = the sum of key(i, j) over its members.  The neighbour cluster of i minimises the fraction
 * S(B) / |B|, compared exactly (cross-multiplied in 128 bits, no floating point), ties to the cluster whose first member comes
 * first in the file.  The silhouette s(i) = (Sb na - Sa nb) / max(Sa nb, Sb na), na = |A| - 1, nb = |B|, is the caller's to form:
 * the library returns integers only.
 */
#ifndef DCTFP_SILHOUETTE_H
#define DCTFP_SILHOUETTE_H

#include "dctfp.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DCTFP_SILHOUETTE_VERSION 1

#define DCTFP_SILHOUETTE_MAX_CAP 4194304        /* 2^22: a sum over fewer than 2^31 proteins stays below 2^53 */
#define DCTFP_SILHOUETTE_MAX_PASS_CLUSTERS 4096 /* 64-bit sums of one pass in the LDS of a workgroup: 32 KiB */

int dctfp_silhouette_version(void);

/* The four sums of the rows of one tile.  Entry (r, c) of the int32 tile, at tile[r * ld + c], is the L1 of proteins row0 + r and
 * col0 + c of ONE file of n_nodes proteins; for the results to be the silhouette's sums the columns are the whole file (col0 = 0,
 * n_cols = n_nodes) -- the export sums over the columns it is given.  row_empty (n_rows bytes) / col_empty (n_cols bytes), either
 * may be NULL, flag the proteins without a fingerprint.  The key of an entry: cap where its row or its column is flagged, cap
 * where the value is negative or >= cap, the value otherwise; the entry with col0 + c == row0 + r is left out whatever it holds.
 *
 * The clustering, written by the caller before the call (device arrays, read with plain loads): cid[n_nodes] (int32) = the dense id
 * 0 .. n_clusters - 1 of the protein's cluster if that has two or more members, ids numbered by first member, or -1 for the one
 * member of a singleton cluster; size[n_clusters] and first[n_clusters] (int32) = the number of members and the lowest member of
 * every such cluster (both may be NULL when n_clusters is 0).  THE CALLER VOUCHES for -1 <= cid[x] < n_clusters, size[c] >= 2 and
 * first[c] being a member of c: the export cannot read device memory and does not validate them (dctdomain_amd.similarity.
 * silhouette_rows does, on the host).  A cid outside that range is an access outside the arrays.
 *
 * Per row, for i = row0 + r (device arrays of n_nodes entries; only the entries of the tile's rows are written, with plain stores):
 *     own_sum[i]    (uint64) = Sa: the sum of the keys of the columns j != i with cid[j] == cid[i] >= 0; 0 for cid[i] == -1
 *     near_sum[i]   (uint64) = S(B), near_size[i] (int32) = |B|, near_first[i] (int32) = the first member of B, for the
 *                   neighbour cluster B of i among the clusters other than i's own, a singleton column j != i being the cluster
 *                   ({j}, key, 1, j); 0, 0 and -1 when there is no other cluster among the columns.
 * A cluster none of whose members is among the columns still is a candidate, with the sum 0 (which is why the columns are the
 * whole file).
 *
 * One workgroup per row; the sums of pass_clusters clusters at a time are kept in the workgroup's LDS (64-bit words), so the row is
 * read ceil(n_clusters / pass_clusters) times, once at least.  The results do not depend on pass_clusters.  No global atomics: a
 * workgroup owns its row.
 *
 * DCTFP_ERR_LIMIT for cap > DCTFP_SILHOUETTE_MAX_CAP, pass_clusters > DCTFP_SILHOUETTE_MAX_PASS_CLUSTERS or n_nodes > 2^31 - 1 (said
 * first, whatever the other arguments are).  DCTFP_ERR_INVALID, with a message, for: a NULL ctx, tile, cid, own_sum, near_sum,
 * near_size or near_first; a NULL size or first with n_clusters > 0; n_rows, n_cols, row0, col0, n_nodes, n_clusters or cap < 0;
 * ld < n_cols; pass_clusters < 1; n_clusters > n_nodes / 2; rows or columns outside n_nodes; tile, cid, size, first, near_size or
 * near_first off a 4-byte boundary, own_sum or near_sum off an 8-byte boundary.  n_rows or n_cols of 0: nothing to do. */
int dctfp_silhouette_rows(dctfp_ctx* ctx, const int32_t* tile, int64_t n_rows, int64_t n_cols, int64_t ld, int64_t row0, int64_t col0,
                          const uint8_t* row_empty, const uint8_t* col_empty, int32_t cap, const int32_t* cid, const int32_t* size,
                          const int32_t* first, int64_t n_clusters, int32_t pass_clusters, uint64_t* own_sum, uint64_t* near_sum,
                          int32_t* near_size, int32_t* near_first, int64_t n_nodes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* DCTFP_SILHOUETTE_H */
