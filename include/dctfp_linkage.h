/* libdctfp: the two kernels of complete- and average-linkage clustering (dct-sim --hac).
 *
 * A header of its own beside dctfp.h, for the same library, the same dctfp_ctx and the same error codes: the conventions of
 * dctfp.h hold (device pointers, caller-owned buffers, work enqueued on the stream given last, NULL = the default stream).
 * DCTFP_VERSION does not change with it; this header counts its own version.
 *
 * State.  A dense symmetric n x n matrix on the device, row stride ld entries, of int32 (wide = 0, complete linkage: entry (a, b)
 * = D(a, b), the largest key = min(L1, 17000) over the member pairs of clusters a and b) or int64 (wide = 1, average linkage:
 * S(a, b), the exact sum of key over the member pairs).  A cluster is named by its lowest member; size[x] (device int32, n
 * entries) is the number of members of cluster x, 0 when x names no cluster (any more).  The diagonal holds the largest value of
 * the type, which passes no bound test.  Rows and columns of a dead cluster keep whatever they held: dctfp_linkage_nearest reads
 * the rows of its live list only and masks every column x with size[x] == 0.
 */
#ifndef DCTFP_LINKAGE_H
#define DCTFP_LINKAGE_H

#include "dctfp.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DCTFP_LINKAGE_VERSION 1

#define DCTFP_LINKAGE_MAX_N 46340     /* floor(sqrt(2^31)); also what keeps S c in 64 bits (below) */
#define DCTFP_LINKAGE_MAX_BOUND 17000 /* the cap of a key */

int dctfp_linkage_version(void);

/* Step 1 of a round: for every a = live[k], k < n_live (device int32; ids in 0 .. n - 1, each at most once),
 *     nn[a] = the x != a with size[x] > 0 and D(a, x) <= bound that minimises (D(a, x), x), or -1 if there is none
 * (device int32, n entries; the entries of ids that are not in the list are left alone).  wide = 0: D is the int32 entry.
 * wide = 1: D(a, x) = S(a, x) / (size[a] size[x]) compared as an exact fraction -- "<= bound" is S <= bound size[a] size[x], and x
 * is before y when S(a, x) size[y] < S(a, y) size[x], ties to the lower id; only entries within the bound are multiplied.  With
 * n <= 46340, bound <= 17000 and size[a] + size[x] + size[y] <= n (three different clusters of n nodes) every product is below
 * 17000 (n / 3)^3 < 2^63.  One workgroup per live row, 16-byte loads from the first 16-byte boundary of a row on (any ld >= n and
 * any base on an entry boundary work; a row on a 16-byte boundary is read with 16-byte loads alone), no atomics.
 * DCTFP_ERR_LIMIT for n > 46340 or bound > 17000 (said first, whatever the other arguments are).  DCTFP_ERR_INVALID, with a
 * message, for: a NULL ctx, mat, size, live or nn; wide outside 0 .. 1; n < 0, ld < n, n_live < 0 or n_live > n; bound < -1; mat off
 * a 4-byte (wide: 8-byte) boundary, size / live / nn off a 4-byte boundary.  n or n_live of 0: nothing to do. */
int dctfp_linkage_nearest(dctfp_ctx* ctx, const void* mat, int32_t wide, int64_t n, int64_t ld, const int32_t* size, const int32_t* live,
                          int64_t n_live, int32_t bound, int32_t* nn, void* stream);

/* Step 2 of a round, in place.  partner[x] (device int32, n entries) = the other cluster of x's pair this round, -1 = none;
 * partner[partner[x]] == x; the lower id of a pair survives and absorbs the higher.  keep[0 .. n_keep) (device int32) lists the
 * survivors of the pairs, each once.  For every x = keep[k] and every y != x with size[y] > 0 that does not die this round, entry
 * (x, y) becomes the maximum (wide = 0) / the sum (wide = 1) of the entries (x, y), (partner[x], y) and, where y survives a pair
 * of its own, (x, partner[y]), (partner[x], partner[y]); the mirror (y, x) is written with it.  No other entry changes: rows and
 * columns of clusters without a pair are byte-identical outside the columns and rows of keep, and rows and columns of the clusters
 * that die keep their old values -- the caller sets their size to 0 (and adds the sizes up) before the next
 * dctfp_linkage_nearest.  size may be the sizes from before or after that update: only size[y] == 0 is read.  Plain loads and
 * stores; every entry a thread reads is either written by that thread alone or not written in the launch, so the result does not
 * depend on the order in which the device ran.
 * DCTFP_ERR_LIMIT for n > 46340.  DCTFP_ERR_INVALID, with a message, for: a NULL ctx, mat, size, partner or keep; wide outside
 * 0 .. 1; n < 0, ld < n, n_keep < 0 or 2 n_keep > n; mat off a 4-byte (wide: 8-byte) boundary, size / partner / keep off a 4-byte
 * boundary.  n or n_keep of 0: nothing to do. */
int dctfp_linkage_merge(dctfp_ctx* ctx, void* mat, int32_t wide, int64_t n, int64_t ld, const int32_t* size, const int32_t* partner,
                        const int32_t* keep, int64_t n_keep, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* DCTFP_LINKAGE_H */
