/*
 * dctfp.h -- C ABI of libdctfp.so: MI355X (gfx950) DCT-fingerprint kernels.
 *
 * Drop-in boundary for ONE path of mgtools/DCTdomain: src/fingerprint.py's
 * Fingerprint.quantize and the helpers it calls.  The reference is pure
 * Python (numpy + scipy.fft) and has no FFI of its own; every entry point
 * below names the reference function (file:line, relative to the reference
 * checkout) whose work it replaces.  The Python host side
 * (dctdomain_amd/fingerprint.py) binds these with ctypes; INTEGRATION.md shows
 * the stub a maintainer of the reference would add.
 *
 * Conventions
 *  - plain C: pointers and sizes only, no C++ or torch types;
 *  - every function returns 0 (DCTFP_OK) or a negative DCTFP_ERR_* code; the
 *    message of the last failure of the calling thread is dctfp_last_error();
 *    nothing throws or longjmps across the boundary;
 *  - "device pointer" = memory of the context's GPU; "host pointer" = ordinary
 *    host memory that is only read during the call;
 *  - the caller owns every buffer.  Work is enqueued on the given hipStream_t
 *    (passed as void*; NULL = the default stream) and is stream-ordered: keep
 *    the device buffers alive until the stream has passed the call;
 *  - one context per (process, device); a context is used by one host thread
 *    at a time;
 *  - arithmetic is float64 end to end like the reference (which promotes to
 *    float64 in get_doms, src/fingerprint.py:160,169); outputs are the
 *    reference's truncated ints 0..127, NaN -> 0 (src/fingerprint.py:194-195).
 */
#ifndef DCTFP_H
#define DCTFP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DCTFP_VERSION 117 /* 0.1.17: dctfp_pair_row_best, dctfp_pair_map_lines */

#define DCTFP_OK 0
#define DCTFP_ERR_INVALID (-1) /* bad argument (null pointer, piece outside its sequence, ...) */
#define DCTFP_ERR_SHAPE (-2)   /* a domain has fewer rows than n, or a layer fewer channels than m:
                                  the reference's "ValueError: cannot reshape array" (src/fingerprint.py:194) */
#define DCTFP_ERR_HIP (-3)     /* a HIP runtime call failed */
#define DCTFP_ERR_NOMEM (-4)   /* workspace allocation failed */
#define DCTFP_ERR_LIMIT (-5)   /* n > DCTFP_MAX_N or m > DCTFP_MAX_M */
#define DCTFP_ERR_UNSUPPORTED (-6) /* dctfp_quantize_windows only: the call is valid but the one-launch kernel that averages two
                                      windows in its row load does not take it; nothing was launched -- materialise the stitched
                                      matrices (dctfp_stitch_sequences) and call dctfp_quantize */

#define DCTFP_MAX_N 8   /* kept points along the sequence axis (reference: 3; PROST: 5) */
#define DCTFP_MAX_M 128 /* kept points along the channel axis  (reference: 80; PROST: 44/85) */

#define DCTFP_F32 0
#define DCTFP_F64 1
#define DCTFP_F16 2  /* IEEE half; dctfp_quantize only (every storage type is promoted exactly, as the */
#define DCTFP_BF16 3 /* bfloat16;   reference's float64 promotion does)                                    */

typedef struct dctfp_ctx dctfp_ctx;

/* One embedding layer of a batch = one value of Fingerprint.embed (src/fingerprint.py:33,184).
 * The rows of sequence s start at seq_data[s]; row r, channel c is seq_data[s][r * ld + c]. */
typedef struct {
    const void* const* seq_data; /* HOST array [n_seq] of DEVICE pointers */
    int64_t ld;                  /* leading dimension in elements (>= n_cols) */
    int32_t n_cols;              /* D */
    int32_t dtype;               /* DCTFP_F32, DCTFP_F64, DCTFP_F16 or DCTFP_BF16 */
    int32_t n_keep;              /* n = qdim[2i]   (src/fingerprint.py:185) */
    int32_t m_keep;              /* m = qdim[2i+1] */
    int32_t out_offset;          /* first column of this layer's n*m block in an output row */
    int32_t reserved;
} dctfp_layer;

/* One contiguous run of rows of a domain = one "b-e" piece of a domain string after
 * get_doms' clean-up (src/fingerprint.py:163-169).  Pieces of one domain are consecutive
 * in the table and in concatenation order. */
typedef struct {
    int64_t row_start; /* 0-based first row inside sequence `seq` */
    int32_t n_rows;    /* > 0 */
    int32_t domain;    /* output row index, 0 .. n_domains-1, non-decreasing over the table */
    int32_t seq;       /* index into seq_data / seq_rows */
    int32_t reserved;
} dctfp_piece;

int dctfp_version(void);
const char* dctfp_last_error(void);

/* The domain-string half of Fingerprint.get_doms (src/fingerprint.py:163-169) for a whole batch, on the host: every
 * domain string ("b-e" or "b-e,b-e,...", 1-based inclusive) becomes its dctfp_piece records, with the reference's
 * behaviour kept exactly: `(int(beg) or int(end)) > L` drops a piece, the list shrinks under its own iterator (the piece
 * after a dropped one is never looked at but stays in the key), remove() takes out the first equal string, `end > L` is
 * clipped, `beg == 0` is the slice [-1:end]; a domain whose cleaned piece list is empty is skipped (:190-191).
 *   text, text_len : all strings in sequence order, separated by '\n';  str_count[s] = strings of sequence s
 *   seq_rows[s]    : rows of sequence s
 *   pieces         : out, room for piece_cap records (number of strings + number of ',' in text is always enough)
 *   str_row[i]     : out, the output row (domain index) of string i, or -1 when it is skipped
 *   str_len[i]     : out, rows of that domain
 *   str_changed[i] : out, 0 = the key under which the reference files the fingerprint is the string itself; 1 = a piece was
 *                    removed, the cleaned key is the next '\n'-terminated entry of key_text; 2 = the string is not of the
 *                    plain form digits-digits[,digits-digits]* -- counted in *n_other and left to the caller's own parser
 *                    (whatever Python's int() / str.split would make of it)
 * Host memory only; needs no GPU and no context. */
int dctfp_build_pieces(const char* text, int64_t text_len, const int32_t* str_count, const int64_t* seq_rows, int32_t n_seq,
                       dctfp_piece* pieces, int64_t piece_cap, int64_t* n_pieces, int32_t* str_row, int64_t* str_len,
                       uint8_t* str_changed, char* key_text, int64_t key_cap, int64_t* key_len, int64_t* n_domains,
                       int64_t* n_other);

/* Context on HIP device `device`: owns the cosine bases, job tables and the float64
 * scratch between the two kernels.  Replaces nothing in the reference (it has no state). */
int dctfp_create(int device, dctfp_ctx** out);
int dctfp_destroy(dctfp_ctx* ctx);

/* Fingerprint.quantize for a ragged batch (src/fingerprint.py:174-201, called by
 * make_db.queue_cpu at src/make_db.py:30):  for every layer i and every domain d
 *     out[d * out_stride + layers[i].out_offset + j * m + c] = trunc(127 * Z_i,d[j][c])
 * where Z is get_doms -> idct_quant(., n) -> idct_quant(.T, m).T of that domain's rows.
 * All layers share the piece table (same sequences, same row numbering).
 *   layers, seq_rows, pieces : host pointers;  out : device pointer, int8.
 *   seq_rows[s] = number of rows of sequence s (bounds check of the pieces).
 * Errors: DCTFP_ERR_SHAPE if some domain has fewer than n rows or n_cols < m (nothing
 * is launched in that case). */
int dctfp_quantize(dctfp_ctx* ctx, const dctfp_layer* layers, int32_t n_layers, int32_t n_seq,
                   const int64_t* seq_rows, const dctfp_piece* pieces, int64_t n_pieces,
                   int64_t n_domains, int8_t* out, int64_t out_stride, void* stream);

/* The same over sequences that exist only as the overlapping WINDOWS the language model embedded -- Embedding.embed_seq
 * (src/embedding.py:153-192) followed by Fingerprint.quantize (src/fingerprint.py:174-201) with the stitched matrix
 *     run[-olp:] = (run[-olp:] + new[:olp]) / 2;  run = cat(run, new[olp:])          (src/embedding.py:185-187)
 * never written: a row two windows share is averaged -- float32 (old + new) / 2, bit for bit what dctfp_stitch_sequences writes --
 * in the row load of the kernel that streams it, so every window row is read once and nothing but the int8 result reaches HBM
 * (stitch, then quantize: the windows read + the stitched matrix written + read again).
 *   layers[l].seq_data : HOST array [seq_win[n_seq]] of DEVICE pointers, one per WINDOW (float32), window w of sequence s at
 *                        index seq_win[s] + w;  seq_win, win_rows, overlap as in dctfp_stitch_sequences (square = 0)
 *   pieces             : rows in STITCHED coordinates (dctfp_stitch_sizes gives each sequence's rows)
 * Results are identical to dctfp_stitch_sequences + dctfp_quantize.  Errors: DCTFP_ERR_SHAPE where the reference's torch expression
 * would fail to broadcast (a window not longer than the overlap) or a domain is shorter than n; DCTFP_ERR_UNSUPPORTED when
 * some row is shared and the call is not one the one-launch kernel takes (see "path": float32 rows 16-byte aligned, n = 3,
 * 64 < m <= 80, 512 <= D <= 2560, 256 jobs or "path" = 2, no domain above 8 192 rows, every window between two others at least
 * 2 x overlap rows) -- nothing has been launched then.  Sequences of one window each are taken in every shape. */
int dctfp_quantize_windows(dctfp_ctx* ctx, const dctfp_layer* layers, int32_t n_layers, int32_t n_seq, const int64_t* seq_win,
                           const int32_t* win_rows, int32_t overlap, const dctfp_piece* pieces, int64_t n_pieces,
                           int64_t n_domains, int8_t* out, int64_t out_stride, void* stream);

/* Fingerprint.quantize for ONE protein -- the reference's own calling pattern (src/make_db.py:29-30 inside a process pool) -- in
 * one call: the protein's domain strings ('\n'-separated, as for dctfp_build_pieces) are cleaned and turned into pieces, the
 * kernels are enqueued, and the call returns when the int8 blocks have arrived in `out` (the device address of a pinned host
 * buffer: dctfp_host_device_pointer; or device memory).  layers[l].seq_data points at ONE device pointer (the layer's matrix of
 * n_rows rows).  str_row / str_changed / key_text / key_len / n_other as in dctfp_build_pieces (n_other > 0: a string this
 * parser leaves to the caller's own -- nothing was launched); *degenerate_seen = 1 when a kernel of THIS call met an exactly
 * constant channel (see "degenerate_seen").  A binding that calls dctfp_build_pieces, dctfp_quantize and
 * dctfp_stream_synchronize itself pays three foreign calls and their argument marshalling per protein. */
int dctfp_quantize_one(dctfp_ctx* ctx, const dctfp_layer* layers, int32_t n_layers, int64_t n_rows, const char* dom_text,
                       int64_t text_len, int32_t n_strings, int8_t* out, int64_t out_rows, int64_t out_stride, int32_t* str_row,
                       uint8_t* str_changed, char* key_text, int64_t key_cap, int64_t* key_len, int64_t* n_domains,
                       int64_t* n_other, int32_t* degenerate_seen, void* stream);

/* Fingerprint.idct_quant(vec, num) for a (n_rows, n_cols) device matrix
 * (src/fingerprint.py:126-142): DCT-II (ortho) along the rows, keep `num`, inverse DCT of
 * length `num`, min-max scale of every column over its `num` values.
 *   scaled_out : device float64 (num, n_cols) = the return value of idct_quant, or NULL
 *   coef_out   : device float64 (n_cols, num) = f[:, :num] of src/fingerprint.py:137
 *                (the "intermediate float coefficients"), or NULL
 * Any num >= 1 (num > n_rows is DCTFP_ERR_SHAPE).  Not a hot path. */
int dctfp_idct_quant(dctfp_ctx* ctx, const void* vec, int32_t dtype, int64_t n_rows, int64_t n_cols,
                     int64_t ld, int32_t num, double* scaled_out, double* coef_out, void* stream);

/* Fingerprint.scale(vec) (src/fingerprint.py:110-123): (v - min) / (max - min) of a
 * device float64 vector of length n; max == min gives NaN like the reference. */
int dctfp_scale(dctfp_ctx* ctx, const double* vec, int64_t n, double* out, void* stream);

/* Row gather + float64 promotion of Fingerprint.get_doms (src/fingerprint.py:160-169) for
 * ONE domain: the pieces (host array, rows relative to `embed`) are concatenated into
 * out (sum n_rows, n_cols) float64, device. */
int dctfp_gather_rows(dctfp_ctx* ctx, const void* embed, int32_t dtype, int64_t n_rows, int64_t n_cols,
                      int64_t ld, const dctfp_piece* pieces, int64_t n_pieces, double* out, void* stream);

/* The contact selection of Fingerprint.writece (src/fingerprint.py:54-67) for a batch of
 * proteins: among the pairs (i, j), j >= i + 5, of each L x L float32 contact map keep the
 * dctfp_contact_count(L, t) = min(int(t * L), number of such pairs) largest values, ties
 * broken by (i, j) ascending as Python's stable reverse sort does.
 *   maps, ld, n_res, out_offs : host arrays (maps[p] = device pointer of protein p's map)
 *   out_i, out_j, out_v       : device arrays; protein p's entries start at out_offs[p], in
 *                               unspecified order (sort by (-v, i, j) for the .ce text)
 *   out_n                     : device int32[n_prot], entries written per protein */
int dctfp_contact_topk(dctfp_ctx* ctx, const void* const* maps, const int64_t* ld, const int32_t* n_res,
                       int32_t n_prot, double t, int32_t* out_i, int32_t* out_j, float* out_v,
                       const int64_t* out_offs, int32_t* out_n, void* stream);
int64_t dctfp_contact_count(int32_t n_res, double t);

/* The ORDER of the selected contacts as the reference's CON line has them (src/fingerprint.py:58-61: sorted by value,
 * reverse=True, Python's stable sort over pairs appended i-major): value descending, ties in (i, j) ascending order.
 * Sorts, in place and on the device, what dctfp_contact_topk wrote for the same arguments (one workgroup per protein, a
 * bitonic network in LDS).  sorted[p] (host, out) = 1 when protein p is in that order afterwards, 0 when it is left as it
 * was (more than 16 384 selected contacts -- L > 6 301 at t = 2.6 -- or L > 65 536: the caller orders those itself). */
int dctfp_contact_sort(dctfp_ctx* ctx, const void* const* maps, const int64_t* ld, const int32_t* n_res, int32_t n_prot,
                       double t, int32_t* out_i, int32_t* out_j, float* out_v, const int64_t* out_offs, uint8_t* sorted,
                       void* stream);

/* The domain cutter itself -- recursiveMaxCut of src/RecCut.cpp (:150-351: single and double max-cut scores over the contact graph,
 * accept / recurse rules, the segment bookkeeping of SplitDomain / SplitDomain_2cuts :16-148), which Fingerprint.reccut reaches
 * through a .ce text file and a subprocess (src/fingerprint.py:92-103) -- for a batch of proteins ON THE GPU, on the contacts
 * dctfp_contact_topk left on the device: one workgroup per protein, sparse adjacency lists, the same integers and the same double
 * expressions as the reference, so the same cuts (include/reccut.h's host library is the definition; both are held to the
 * reference's compiled binary by the tests).
 *   n_res, offs, out_offs : host arrays; protein p's contacts are [offs[p], offs[p+1]) of ci / cj / cv (device; pairs distinct,
 *                           as dctfp_contact_topk writes them), weights as the .ce text carries them
 *   out (device, or the device address of pinned host memory): protein p's result at out + out_offs[p], room out_offs[p+1] -
 *                           out_offs[p] >= dctfp_reccut_room(n_res[p]) ints:
 *                               out[0] = number of domains D, then per domain: n_segs, then n_segs x (first, last), 0-based residues,
 *                           in the order the binary prints them; out[0] = -1: NOT DONE HERE -- more residues / contacts than the
 *                           kernel's tables hold (2 048 residues; contacts + 3 L <= 12 288), a contact outside the protein or a
 *                           non-finite value, or a step at which the reference indexes outside its segment table (undefined
 *                           behaviour there): run reccut_predict (include/reccut.h) on that protein. */
int dctfp_reccut(dctfp_ctx* ctx, const int32_t* n_res, int32_t n_prot, const int32_t* ci, const int32_t* cj, const float* cv,
                 const int64_t* offs, double cut1, double cut2, int32_t* out, const int64_t* out_offs, void* stream);
int64_t dctfp_reccut_room(int32_t n_res);

/* What Fingerprint.reccut appends to `domains` (src/fingerprint.py:103-107) and what Fingerprint.get_doms makes of those strings
 * (:163-169), for a whole flush, straight from dctfp_reccut's encoded results (host copies of them): per protein the strings the
 * binary prints -- "b-e[,b-e]*", 1-based inclusive -- followed by "1-L" where there are several, each terminated by ';' in
 * `text`; str_count[p] = strings of protein p; and the dctfp_piece table of exactly those strings (domain = running index over
 * all strings, seq = p), ready for dctfp_quantize.  A flush of 2 048 proteins used to format the strings in one library, split
 * them per protein, join them again and parse them in dctfp_build_pieces.
 *   enc, enc_off : as dctfp_reccut wrote them (enc_off[n_prot] entries; protein p at enc + enc_off[p]);  seq_rows[p] = residues
 *   text_cap     : 24 bytes per segment + 32 per protein is always enough;  piece_cap : segments + proteins
 *   *n_undone    : proteins left out (str_count[p] = 0, no pieces): status -1, a malformed record, or a segment outside the
 *                  protein (which get_doms' clean-up rules would have to judge): run reccut_predict / dctfp_build_pieces on
 *                  those -- the table then speaks of the other proteins only.
 * Host memory only; needs no GPU and no context. */
int dctfp_reccut_pieces(int32_t n_prot, const int32_t* enc, const int64_t* enc_off, const int64_t* seq_rows, char* text,
                        int64_t text_cap, int64_t* text_len, int32_t* str_count, dctfp_piece* pieces, int64_t piece_cap,
                        int64_t* n_pieces, int64_t* n_domains, int64_t* n_undone);

/* The chunk stitcher of Embedding.embed_seq (src/embedding.py:153-192): a sequence longer than
 * maxlen is embedded in windows; per layer `run[-200:] = (run[-200:] + new[:200]) / 2` then
 * `cat(new[200:])` (:185-187), and for the contact maps combine_contacts (:123-150).  One job =
 * one window of one sequence; `level` = the window's index in its sequence.  Windows are applied
 * level by level (one launch per level for the whole batch), which keeps the reference's
 * sequential semantics.  float32 in, float32 out, (a + b) / 2 as in the reference.
 *   square = 0 : embeddings.  dst rows [0, n_avg) = (dst + src) / 2, rows [n_avg, n_rows) = src.
 *   square = 1 : contact maps (n_cols ignored).  The n_rows x n_rows square at dst: its leading
 *                n_avg x n_avg corner = (dst + src) / 2, the rest = dst + src; the caller zeroes
 *                the output first (new_mat = torch.zeros, :143).
 * jobs: host array; src/dst: device pointers. */
typedef struct {
    const void* src;
    void* dst;
    int64_t ld_src;
    int64_t ld_dst;
    int32_t n_rows;
    int32_t n_avg;
    int32_t level;
    int32_t reserved;
} dctfp_stitch_job;
int dctfp_stitch(dctfp_ctx* ctx, const dctfp_stitch_job* jobs, int64_t n_jobs, int32_t n_cols, int32_t square,
                 void* stream);

/* The same for whole sequences, the window geometry worked out here instead of by the caller (the per-window Python of a
 * batch cost four times its kernels): sequence s owns the windows [seq_win[s], seq_win[s+1]) in order; win_rows / win /
 * win_ld give each window's rows, device pointer and leading dimension.
 *   square = 0, step = the overlap (200 in the reference, src/embedding.py:163): window w > 0 starts `step` rows before
 *                the end of the running embedding, those rows are averaged, the rest appended (:185-187);
 *   square = 1, step = maxlen - overlap: window w's map lands at offset step * w of the running map, the part they share
 *                is averaged (combine_contacts, :123-150).
 * dctfp_stitch_sizes (host only, no context): rows / side of each stitched result, so that the caller can allocate;
 * DCTFP_ERR_SHAPE where the reference's torch expression would fail to broadcast (a window not longer than the overlap,
 * a window offset beyond the running map).  dctfp_stitch_sequences: dst[s] = device pointer of sequence s's result
 * (dst_ld[s] floats per row; contact maps zero-filled by the caller), then the launches of dctfp_stitch -- or, for
 * embeddings whose windows overlap their neighbours only (every window with both a predecessor and a successor has at least
 * 2 * step rows: any maxlen >= 2 * overlap), ONE launch for all windows: the rows two windows share are averaged from the two
 * windows, the same float32 (a + b) / 2, every row read and written once. */
int dctfp_stitch_sizes(const int32_t* win_rows, const int64_t* seq_win, int64_t n_seq, int32_t step, int32_t square,
                       int64_t* out_rows);
int dctfp_stitch_sequences(dctfp_ctx* ctx, const void* const* win, const int32_t* win_rows, const int64_t* win_ld,
                           const int64_t* seq_win, int64_t n_seq, void* const* dst, const int64_t* dst_ld, int32_t n_cols,
                           int32_t step, int32_t square, void* stream);

/* L1 distance matrix between two sets of int8 fingerprints, the quantity under the
 * reference's similarity scores 1 - min(L1 / 17000, 1) (src/dct-sim.py:12-26) and
 * round(1 - L1 / 17000, 4) (src/query_db.py:57; FAISS METRIC_L1, :76):
 *     out[i * ldo + j] = sum_k |a[i * lda + k] - b[j * ldb + k]|,  k < d.   All device pointers.  DCTFP_ERR_LIMIT above 8M
 * (8388480) rows of a or 2147483520 rows of b per call (128 x 128 distances to a 256-thread workgroup, and one launch holds
 * fewer than 2^32 threads along the columns, 65535 workgroups along the rows). */
int dctfp_l1_matrix(dctfp_ctx* ctx, const int8_t* a, int64_t na, int64_t lda, const int8_t* b, int64_t nb, int64_t ldb,
                    int32_t d, int32_t* out, int64_t ldo, void* stream);

/* domain_sim (src/dct-sim.py:28-50) on a distance matrix: protein pa owns rows
 * [idx_a[pa], idx_a[pa+1]), protein pb columns [idx_b[pb], idx_b[pb+1]) (device int64 prefix
 * arrays, the npz "idx"); out_min[pa*npb+pb] = smallest distance of the block (-> DCTdomain),
 * out_last = its last row / last column entry (-> DCTglobal).  DCTFP_ERR_LIMIT above 4294967040 protein pairs (npa x npb) per
 * call: one thread per pair, and one launch holds fewer than 2^32 threads. */
int dctfp_block_min(dctfp_ctx* ctx, const int32_t* dist, int64_t ldo, const int64_t* idx_a, int64_t npa,
                    const int64_t* idx_b, int64_t npb, int32_t* out_min, int32_t* out_last, void* stream);

/* The k nearest database fingerprints of every query fingerprint: the k smallest entries of each row of an
 * int32 distance matrix (dctfp_l1_matrix), ties to the lower column as a flat index scan returns them
 * (index.search at src/query_db.py:87).  out_val / out_idx: device int32 (n_rows, k), unordered within a row.  DCTFP_ERR_LIMIT
 * above 4194303 rows per call (a workgroup of up to 1024 threads per row, and one launch holds fewer than 2^32 threads) or
 * 2^31 - 1 columns (out_idx is int32). */
int dctfp_row_select(dctfp_ctx* ctx, const int32_t* dist, int64_t n_rows, int64_t n_cols, int64_t ld, int32_t k,
                     int32_t* out_val, int32_t* out_idx, void* stream);

/* Orders what dctfp_row_select left, in place and on the device: each row's k (value, column) pairs ascending by value, ties by
 * column -- the order in which a flat L1 index reports its hits (src/query_db.py:87).  k <= 1024 (DCTFP_ERR_LIMIT beyond:
 * order those on the host) and at most 8388607 rows per call (DCTFP_ERR_LIMIT: a workgroup of up to 512 threads per row, and one
 * launch holds fewer than 2^32 threads). */
int dctfp_row_order(dctfp_ctx* ctx, int32_t* val, int32_t* idx, int64_t n_rows, int32_t k, void* stream);

/* domain_sim (src/dct-sim.py:28-50) for a list of protein pairs, straight from the fingerprints -- no distance matrix: pair p
 * = (pairs[2p], pairs[2p+1]) = (protein of a, protein of b), the proteins' rows given by the npz "idx" prefix arrays idx_a
 * (npa + 1 entries) and idx_b (npb + 1) as in dctfp_block_min.  out_min[p] = the smallest L1 over all fingerprint pairs of the
 * two proteins (-> DCTdomain), out_last[p] = the L1 of their last (whole-protein) rows (-> DCTglobal).  Replaces the pair loop
 * of pair_sim (:104-111) and the per-hit domain_sim of db_search (:143-145).  All device pointers; the prefix arrays must be
 * non-decreasing and within their matrices (the caller's guarantee, as for dctfp_block_min).  A protein without fingerprints
 * gives 0x7fffffff in both outputs (dctfp_block_min's fill); a pair index outside [0, npa) x [0, npb) gives -1 in both.
 * DCTFP_ERR_LIMIT above 2^31 - 1 proteins on a side or 67108860 pairs per call (four pairs to a 256-thread workgroup, and one
 * launch holds fewer than 2^32 threads). */
int dctfp_pair_min(dctfp_ctx* ctx, const int32_t* pairs, int64_t n_pairs, const int8_t* a, int64_t lda, const int64_t* idx_a, int64_t npa,
                   const int8_t* b, int64_t ldb, const int64_t* idx_b, int64_t npb, int32_t d, int32_t* out_min, int32_t* out_last,
                   void* stream);

/* dctfp_pair_min that also says WHICH fingerprint pair gave DCTdomain (dct-sim --domains): the same arguments, out_min and
 * out_last exactly as there (0x7fffffff for a protein without fingerprints, -1 for a pair index out of range), and
 * out_arg_a[p] / out_arg_b[p] (device int32) = the rows, counted from 0 within protein pairs[2p] of a and protein pairs[2p+1] of
 * b, of the fingerprint pair with the smallest L1.  The reference's loop (src/dct-sim.py:42-50) runs over the rows of the first
 * protein, then of the second, and replaces its maximum -- started at 0 -- only on `s > maxs`: equal L1 values go to the lowest
 * row of a, then the lowest row of b, and there is NO best pair, -1 in both, when the smallest L1 is 17000 or more (similarity 0
 * is never > 0), when either protein has no fingerprint, or when the pair index is out of range.  Reads the same bytes as
 * dctfp_pair_min.  DCTFP_ERR_LIMIT above 2^31 - 1 proteins on a side or 67108860 pairs per call; a protein must have fewer than
 * 2^31 fingerprints. */
int dctfp_pair_argmin(dctfp_ctx* ctx, const int32_t* pairs, int64_t n_pairs, const int8_t* a, int64_t lda, const int64_t* idx_a, int64_t npa,
                      const int8_t* b, int64_t ldb, const int64_t* idx_b, int64_t npb, int32_t d, int32_t* out_min, int32_t* out_last,
                      int32_t* out_arg_a, int32_t* out_arg_b, void* stream);

/* DCTdomain's L1 for every protein pair of two fingerprint sets, straight from the fingerprints (dct-sim --db --rank domain):
 *     out[pa * ldo + pb] = min over rows r of protein pa (idx_a) and rows s of protein pb (idx_b) of
 *                          sum_k |a[r * lda + k] - b[s * ldb + k]|,  k < d
 * -- dctfp_block_min's out_min on the dctfp_l1_matrix of the two sets, without the distance matrix.  idx_a (npa + 1 entries)
 * and idx_b (npb + 1) are the npz "idx" prefix arrays, as in dctfp_pair_min (non-decreasing and within their matrices: the
 * caller's guarantee).  A protein without fingerprints gives 0x7fffffff (dctfp_block_min's fill).  All device pointers; out is
 * int32 (npa, npb) with row stride ldo >= npb, every entry written, nothing else.  Consecutive proteins are packed into blocks
 * of at most 128 rows on the device; a protein of more rows is a block of its own.  DCTFP_ERR_LIMIT (nothing written) for rows
 * above 512 bytes, rows not on 16-byte boundaries (a, b, lda, ldb) or 2^24 bytes apart, or more than 2^31 - 1 proteins on a
 * side: dctfp_l1_matrix + dctfp_block_min give the same values there.  Uses the context's scratch. */
int dctfp_protein_min(dctfp_ctx* ctx, const int8_t* a, int64_t lda, const int64_t* idx_a, int64_t npa, const int8_t* b, int64_t ldb,
                      const int64_t* idx_b, int64_t npb, int32_t d, int32_t* out, int64_t ldo, void* stream);

/* dctfp_protein_min with a coverage requirement (dct-sim --min-coverage): a protein pair keeps its DCTdomain L1 only when enough
 * of BOTH proteins is matched by the other one.  Row r of protein pa is matched by protein pb when
 *     min over the rows s of pb of sum_k |a[r * lda + k] - b[s * ldb + k]| <= bound
 * (signed: a negative bound matches nothing; bound <= 0x7ffffffe, which matches every row of a pair that has rows on both
 * sides; DCTFP_ERR_INVALID above that), likewise a row of pb by pa.  cov(pa by pb) = the sum of w_a[r] over the matched rows r of
 * pa, cov(pb by pa) = the sum of w_b[s] over the matched rows s of pb (w_a, w_b: device int32, one weight per row of a / of b;
 * summed in 64 bits).  Then, with m = dctfp_protein_min's value of the pair,
 *     out[pa * ldo + pb] = m           when cov(pa by pb) >= need_a[pa] and cov(pb by pa) >= need_b[pb],
 *                          0x7fffffff  otherwise
 * need_a (npa) / need_b (npb): device int32; a value <= 0 asks nothing of that side, so one-sided requirements are a need array of
 * zeros -- and with both arrays all zero the output is dctfp_protein_min's, byte for byte.  A protein without fingerprints gives
 * 0x7fffffff against everything, as there.  Everything else -- idx_a / idx_b, the packing into blocks, out and ldo, every entry
 * written once, the scratch -- is dctfp_protein_min's, and so are the limits: DCTFP_ERR_LIMIT (nothing written) for rows above 512
 * bytes, rows not on 16-byte boundaries (a, b, lda, ldb) or 2^24 bytes apart, or more than 2^31 - 1 proteins on a side.  A block
 * that holds a protein of more than 128 rows costs two passes over its distances instead of one. */
int dctfp_protein_cover(dctfp_ctx* ctx, const int8_t* a, int64_t lda, const int64_t* idx_a, int64_t npa, const int32_t* w_a, const int32_t* need_a,
                        const int8_t* b, int64_t ldb, const int64_t* idx_b, int64_t npb, const int32_t* w_b, const int32_t* need_b, int32_t d,
                        int32_t bound, int32_t* out, int64_t ldo, void* stream);

/* The hits db_search prints (src/dct-sim.py:146-156), selected on the device from an int32 tile of L1 distances between the
 * queries' and the database proteins' last fingerprints (dctfp_l1_matrix).  Key of an entry: min(L1, cap) (cap = 17000: the
 * reference's sorted(..., reverse=True) on 1 - min(L1 / 17000, 1) is "key ascending, ties by column"); row_empty[r] /
 * col_empty[c] (device uint8, either may be NULL) != 0 marks a protein without fingerprints, key cap against everything.
 * `bound` = the largest key whose similarity still reaches the threshold (-1: none, cap: all).  A row's hits are its first
 * m = min(n_cols, max(top, #(key <= bound))) entries in that order.
 * dctfp_select_count: out_count[r] = m (device int32 n_rows), out_cut[2r, 2r+1] (device int32 2 n_rows) = what the fill needs.
 * dctfp_select_fill: offsets (device int64, n_rows + 1) = the exclusive prefix sum of out_count, computed by the caller; the
 * hits of row r go to out_key / out_col [offsets[r], offsets[r+1]) (device int32), ordered by (key, column) when
 * m <= min(max_count, 1024) -- max_count = the largest m of the call -- and in column order when m > 1024 (the caller orders
 * those).  cap <= 17407 (the LDS histogram of the count; DCTFP_ERR_LIMIT beyond), top >= 1, n_cols < 2^31, at most 4194303 rows per
 * call (DCTFP_ERR_LIMIT: one 1024-thread workgroup per row, and one launch holds fewer than 2^32 threads). */
int dctfp_select_count(dctfp_ctx* ctx, const int32_t* dist, int64_t n_rows, int64_t n_cols, int64_t ld, const uint8_t* row_empty,
                       const uint8_t* col_empty, int32_t cap, int32_t bound, int32_t top, int32_t* out_count, int32_t* out_cut,
                       void* stream);
int dctfp_select_fill(dctfp_ctx* ctx, const int32_t* dist, int64_t n_rows, int64_t n_cols, int64_t ld, const uint8_t* row_empty,
                      const uint8_t* col_empty, int32_t cap, const int32_t* cut, const int64_t* offsets, int32_t max_count, int32_t* out_key,
                      int32_t* out_col, void* stream);

/* all_sim's result lines (src/dct-sim.py:158-176) as UTF-8 text, from a tile of (min, last) L1 values (dctfp_block_min's two
 * outputs, device int32, row stride ld): entry (r, c) belongs to proteins i = row0 + r and j = col0 + c, and only j > i is
 * printed.  Line (i, j) = "{id_i} {id_j} {a} {b}\n": ids[id_off[p] .. id_off[p+1]) is protein p's id (device bytes and int64
 * prefix offsets, every protein of the file); a / b = the five bytes of row min(L1, 17001) of the score table (device,
 * 2 x 17002 rows of 5 bytes: DCTdomain text by min, then DCTglobal text by last; row 17001 stands for every L1 above 17000,
 * 0x7fffffff included).  Row i's lines, j = i + 1 .. in order, start at out + row_base[r] (device int64, n_rows); the line of
 * j starts (j - i - 1) (len_i + 14) + (id_off[j] - id_off[i + 1]) bytes after that.  The call writes the lines of columns
 * [col0, col0 + n_cols) only, so a row may be filled by several calls; nothing outside those lines' bytes is written (the
 * caller sizes `out`).  Any id length, any alignment of `out`. */
int dctfp_sim_lines(dctfp_ctx* ctx, const int32_t* mn, const int32_t* last, int64_t ld, int64_t n_rows, int64_t row0, int64_t col0,
                    int64_t n_cols, const uint8_t* ids, const int64_t* id_off, const char* table, const int64_t* row_base, uint8_t* out,
                    void* stream);

/* all_sim with score cut-offs (dct-sim --min-domain / --min-global; the reference parses --threshold but ignores it in this
 * mode, src/dct-sim.py:158-176): the pairs of the upper triangle that pass a cut-off, selected on the device in output order.
 * `tile` = device int32 (n_rows, n_cols), row stride ld, 4-byte aligned, any row alignment: entry (r, c) is an L1 of proteins
 * i = row0 + r and j = col0 + c -- dctfp_protein_min's tile (DCTdomain) or the dctfp_l1_matrix of the proteins' last rows
 * (DCTglobal).  An entry survives when j > i and key <= bound, key = min(L1, cap) as in dctfp_select_count (cap = 17000;
 * row_empty[r] / col_empty[c], device uint8, either may be NULL, != 0: a protein without fingerprints, key cap against
 * everything; a negative value counts as cap).  bound = -1: nothing survives; bound = cap: every j > i does.  Extends
 * dctfp_select_count / dctfp_select_fill (a top-m per row by key order) to "all below a bound, in (i, j) order".
 * dctfp_tri_filter_count: out_count[r] (device int32, n_rows) = the survivors of row r; n_cols may be 0.
 * dctfp_tri_filter_fill: offsets (device int64, n_rows + 1) = the exclusive prefix sum of out_count, computed by the caller;
 * row r's survivors go to out_i / out_j [offsets[r], offsets[r + 1]) (device int32) as the global indices i and j, j ascending.
 * Positions come from that prefix sum and the column order alone, never from the order in which workgroups run.  out_len = the
 * entries of out_i / out_j: nothing is written at or beyond it, nor outside a row's range.
 * DCTFP_ERR_INVALID for a bound outside [-1, cap], ld < n_cols or a tile not on a 4-byte boundary; DCTFP_ERR_LIMIT when
 * row0 + n_rows or col0 + n_cols exceeds 2^31 - 1. */
int dctfp_tri_filter_count(dctfp_ctx* ctx, const int32_t* tile, int64_t n_rows, int64_t n_cols, int64_t ld, int64_t row0, int64_t col0,
                           const uint8_t* row_empty, const uint8_t* col_empty, int32_t cap, int32_t bound, int32_t* out_count,
                           void* stream);
int dctfp_tri_filter_fill(dctfp_ctx* ctx, const int32_t* tile, int64_t n_rows, int64_t n_cols, int64_t ld, int64_t row0, int64_t col0,
                          const uint8_t* row_empty, const uint8_t* col_empty, int32_t cap, int32_t bound, const int64_t* offsets,
                          int64_t out_len, int32_t* out_i, int32_t* out_j, void* stream);

/* all_sim's result lines for a LIST of pairs -- dctfp_sim_lines' text without its dense rows (there a line's place is a closed
 * form of the row; here the caller gives it): line n = "{id_i} {id_j} {a} {b}\n" with i = pi[n], j = pj[n] (device int32),
 * written from byte line_off[n] of out (device int64: the caller's prefix sum of len_i + len_j + 14, as dctfp_query_lines takes
 * it).  ids / id_off (n_ids + 1 offsets) and the score table as in dctfp_sim_lines: a / b = the five bytes of rows
 * min(mn[n], 17001) / min(last[n], 17001) (dctfp_pair_min's two outputs; 0x7fffffff -> row 17001).  Any id length, any
 * alignment of out.  A line whose pair lies outside [0, n_ids) or whose end lies beyond out_bytes is skipped, nothing else is
 * written.  DCTFP_ERR_LIMIT above 268435440 lines per call (sixteen lanes to a line, and one launch holds fewer than 2^32 threads). */
int dctfp_pair_lines(dctfp_ctx* ctx, int64_t n_lines, const int32_t* pi, const int32_t* pj, const int32_t* mn, const int32_t* last,
                     const uint8_t* ids, const int64_t* id_off, int64_t n_ids, const char* table, const int64_t* line_off, uint8_t* out,
                     int64_t out_bytes, void* stream);

/* dctfp_pair_lines with the domain pair behind the scores (dct-sim --domains): line n =
 * "{id_i} {id_j} {a} {b} {label_a} {label_b}\n", everything up to b as in dctfp_pair_lines (and dctfp_sim_lines: ids, id_off,
 * the score table).  labels / label_off (device bytes and n_labels + 1 int64 prefix offsets) = the label table of the file: one
 * UTF-8 entry per fingerprint row and, last, one sentinel entry ("-") for "no domain pair"; la[n] / lb[n] (device int32) pick
 * the two entries -- a global fingerprint row (the protein's first row + dctfp_pair_argmin's argument) or the sentinel.
 * line_off[n] = the caller's prefix sum of len_i + len_j + 14 + len_label_a + len_label_b + 2.  Any id or label length, any
 * alignment of out.  A line with a protein index outside [0, n_ids), a label index outside [0, n_labels) or an end beyond
 * out_bytes is skipped, nothing else is written.  DCTFP_ERR_LIMIT above 268435440 lines per call. */
int dctfp_pair_domain_lines(dctfp_ctx* ctx, int64_t n_lines, const int32_t* pi, const int32_t* pj, const int32_t* mn, const int32_t* last,
                            const int32_t* la, const int32_t* lb, const uint8_t* ids, const int64_t* id_off, int64_t n_ids,
                            const uint8_t* labels, const int64_t* label_off, int64_t n_labels, const char* table, const int64_t* line_off,
                            uint8_t* out, int64_t out_bytes, void* stream);

/* Every fingerprint row's counterpart in the other protein, for a list of protein pairs (dct-sim --domain-map; not in the
 * reference): where dctfp_pair_argmin keeps the one best fingerprint pair, this keeps the best partner of EVERY row, on both
 * sides.  pairs, a, lda, idx_a, npa, b, ldb, idx_b, npb, d: as dctfp_pair_argmin, with its checks and error codes
 * (DCTFP_ERR_LIMIT above 2^31 - 1 proteins on a side or 67108860 pairs per call).  For pair p = (pa, pb) with k and m rows the
 * results lie at [row_off[p], row_off[p + 1]) of out_l1 / out_arg (device int32, out_len entries; row_off = n_pairs + 1 device
 * int64, the caller's prefix sum of k + m): first the k rows of pa, then the m rows of pb.  out_l1 = the smallest L1 between the
 * row and any row of the other protein, raw (not capped at 17000); out_arg = the row of the other protein it was found at,
 * counted from 0 within that protein, ties to the lowest.  Where the other protein has no rows: 0x7fffffff and -1.  A pair with
 * an index outside [0, npa) x [0, npb), a range whose width is not k + m, that starts below 0 or ends beyond out_len writes
 * nothing.  The smallest out_l1 of the first side, ties to the first row, is dctfp_pair_argmin's pair.  Any number of rows per
 * protein; rows above 512 bytes take a slower loop. */
int dctfp_pair_row_best(dctfp_ctx* ctx, const int32_t* pairs, int64_t n_pairs, const int8_t* a, int64_t lda, const int64_t* idx_a, int64_t npa,
                        const int8_t* b, int64_t ldb, const int64_t* idx_b, int64_t npb, int32_t d, const int64_t* row_off, int64_t out_len,
                        int32_t* out_l1, int32_t* out_arg, void* stream);

/* dctfp_pair_domain_lines with one more field, the domain map of the pair (dct-sim --domain-map): line n =
 * "{id_i} {id_j} {a} {b} {label_a} {label_b} {side}/{side}\n".  The first side lists the fingerprint rows of protein pi[n] that
 * are matched by pj[n], the second those of pj[n] matched by pi[n], each in row order as
 * "{label of the row}={label of its counterpart}:{score}" joined by ";", or "-" when no row is matched.  A row is matched when
 * its row_l1 is in [0, bound]; score = the five bytes of the first half of the score table for that L1, so the entry of the best
 * pair repeats the line's own a.  row_off (n_lines + 1), row_l1 and row_arg (n_rows entries): dctfp_pair_row_best's row_off,
 * out_l1 and out_arg for these lines.  first_row (n_ids + 1 device int64): the rows of protein p are the labels
 * first_row[p] .. first_row[p + 1] - 1 (the idx array of the file).  bound below 17000 (DCTFP_ERR_INVALID otherwise).
 * Two passes of one kernel body: with out_count non-NULL (device int64, n_lines) every line's byte length is written there and no
 * text (line_off and out may be NULL); with out_count NULL the text goes to out from line_off[n], the caller's prefix sum of those
 * lengths.  A line with a protein or label index out of range, whose row_off range is not its two proteins' rows within
 * [0, n_rows], whose row_arg names no row of the other protein, or (fill) that ends beyond out_bytes has length 0 and is not
 * written.  Any id or label length, any alignment.  DCTFP_ERR_LIMIT above 268435440 lines per call. */
int dctfp_pair_map_lines(dctfp_ctx* ctx, int64_t n_lines, const int32_t* pi, const int32_t* pj, const int32_t* mn, const int32_t* last,
                         const int32_t* la, const int32_t* lb, const uint8_t* ids, const int64_t* id_off, int64_t n_ids, const uint8_t* labels,
                         const int64_t* label_off, int64_t n_labels, const char* table, const int64_t* line_off, uint8_t* out,
                         int64_t out_bytes, const int64_t* row_off, int64_t n_rows, const int32_t* row_l1, const int32_t* row_arg,
                         const int64_t* first_row, int32_t bound, int64_t* out_count, void* stream);

/* Single-linkage clusters at a cut-off (dct-sim --cluster; not in the reference): the connected components of the graph whose
 * edges are the pairs dctfp_tri_filter_count / dctfp_tri_filter_fill select, joined on the device instead of listed.
 * `parent` = device int32 (n_nodes), a union-find forest the caller starts as parent[x] = x and hands to any number of these
 * calls on one stream: parent[x] <= x always, x is a root when parent[x] == x, a union hooks the larger of two roots under the
 * smaller (compare-and-swap), finds shorten paths (atomic min).  The root of a finished component is therefore its smallest
 * member, whatever the order in which the device ran the unions: the result is a property of the graph.
 * dctfp_tri_link extends dctfp_tri_filter_count's survival rule -- the same tile arguments, j > i and min(L1, cap) <= bound, the
 * same flags -- from counting the surviving entries (i, j) of a tile to joining i and j.  DCTFP_ERR_INVALID as there, and when
 * row0 + n_rows or col0 + n_cols exceeds n_nodes (checked on the host: the device never forms an index outside parent);
 * DCTFP_ERR_LIMIT for n_nodes >= 2^31.  n_rows, n_cols or n_nodes of 0: nothing to do. */
int dctfp_tri_link(dctfp_ctx* ctx, const int32_t* tile, int64_t n_rows, int64_t n_cols, int64_t ld, int64_t row0, int64_t col0,
                   const uint8_t* row_empty, const uint8_t* col_empty, int32_t cap, int32_t bound, int32_t* parent, int64_t n_nodes,
                   void* stream);

/* The union of dctfp_tri_link for a LIST of pairs (pi[n], pj[n]), device int32 -- dctfp_tri_filter_fill's output, or what is left
 * of it after a second cut-off: extends dctfp_tri_filter_count's survival rule to pairs the caller has selected further.  A pair
 * with an index outside [0, n_nodes) is skipped, as dctfp_pair_lines skips it; i == j does nothing.  DCTFP_ERR_LIMIT for
 * n_nodes >= 2^31 or more than 2^31 pairs per call; n_pairs or n_nodes of 0: nothing to do. */
int dctfp_link_pairs(dctfp_ctx* ctx, const int32_t* pi, const int32_t* pj, int64_t n_pairs, int32_t* parent, int64_t n_nodes,
                     void* stream);

/* After the links (dctfp_tri_link, dctfp_link_pairs -- the components of dctfp_tri_filter_count's survival rule): labels[x]
 * (device int32, n_nodes) = the root of x = the smallest member of x's component.  Two launches of its own, ordered after the
 * links by the stream: the first puts every node directly under its root (path halving by all threads at once: the depth of the
 * forest handed in is not the run time), the second reads.  `parent` is left a valid forest of the same components, so linking
 * may go on afterwards.  DCTFP_ERR_LIMIT for n_nodes >= 2^31; n_nodes of 0: nothing to do. */
int dctfp_cluster_labels(dctfp_ctx* ctx, int32_t* parent, int64_t n_nodes, int32_t* labels, void* stream);

/* Domain families (dct-sim --cluster --level domain; not in the reference): the nodes of the forest are fingerprint ROWS, and the
 * distances are never stored.  dctfp_rows_link extends dctfp_tri_link from an int32 tile of protein-pair values to the rows
 * themselves, with dctfp_tri_filter_count's survival rule applied to row pairs: a / b (device int8, na x d at row stride lda,
 * nb x d at ldb; any alignment, dctfp_l1_matrix's three kernels by it) are two ranges of the file's rows, row r of a being node
 * a0 + r and row c of b node b0 + c; owner (device int32, n_nodes) = the protein of every node, skip (device uint8, n_nodes, or
 * NULL) = 1 for a row that is no node.  Every pair with a0 + r < b0 + c, owner[a0 + r] != owner[b0 + c], neither row skipped and
 * min(L1(row r, row c), cap) <= bound is a union in `parent` (as in dctfp_tri_link: agent-scope atomics only, the root of a
 * finished component is its smallest member).  Nothing else is written: the 128 x 128 sums of a workgroup are compared in
 * registers, and a workgroup whose block lies wholly on or left of the diagonal ends before it loads anything.
 * DCTFP_ERR_INVALID for a NULL argument (skip excepted), a negative count or offset, d < 1, lda or ldb < d, cap < 0, bound < 0,
 * a0 + na > n_nodes or b0 + nb > n_nodes (checked on the host: the device never forms an index outside parent, owner or skip);
 * DCTFP_ERR_LIMIT for n_nodes >= 2^31, more than 8M (8388480) rows of a or more than 2147483520 rows of b per call.  na or nb of 0:
 * nothing to do. */
int dctfp_rows_link(dctfp_ctx* ctx, const int8_t* a, int64_t na, int64_t lda, int64_t a0, const int8_t* b, int64_t nb, int64_t ldb,
                    int64_t b0, int32_t d, const int32_t* owner, const uint8_t* skip, int32_t cap, int32_t bound, int32_t* parent,
                    int64_t n_nodes, void* stream);

/* Greedy incremental clusters at a cut-off (dct-sim --cluster --linkage greedy; not in the reference): over the graph whose edges
 * are the pairs dctfp_tri_filter_count / dctfp_tri_filter_fill select, the proteins taken in file order -- one that no earlier
 * representative has an edge to becomes a representative, every other one belongs to the lowest representative it has an edge to.
 * So every member is within the cut-off of its representative and no two representatives are within it of each other, which the
 * components of dctfp_tri_link do not promise.  Device int32 (n_nodes) each, handed to any number of these calls on one stream:
 * `assign` = the lowest representative seen so far (started as 0x7fffffff; a representative's own index), `state` = 0 undecided
 * / 1 member / 2 representative decided by the latest dctfp_greedy_decide over its range / 3 representative done (started as 0),
 * `blocked` = a round number (started as 0).  The caller takes the nodes in ranges [i0, i1) in ascending order -- when a range
 * starts, every representative below i0 has marked all its columns -- and runs rounds over a range until none of it is undecided:
 * a decide, then a mark of the range's rows (dctfp_greedy_tri_mark or dctfp_greedy_pairs_mark).  At the end assign holds the
 * labels; they are a property of the graph, whatever the ranges or the order in which the device ran.
 * dctfp_greedy_decide, one thread per node of [i0, i1): a representative of state 2 becomes 3; an undecided node becomes a member
 * if assign is set, else a representative (assign = its index, state 2) unless blocked holds `round`, else it stays undecided.
 * round 0 makes members only (the pass a range starts with, before its first mark).  *undecided (device int64, the caller's
 * running total) grows by the nodes left undecided.  DCTFP_ERR_INVALID for i0 > i1, i1 > n_nodes or a negative round;
 * DCTFP_ERR_LIMIT for n_nodes >= 2^31.  An empty range: nothing to do. */
int dctfp_greedy_decide(dctfp_ctx* ctx, int32_t* assign, int32_t* state, const int32_t* blocked, int64_t n_nodes, int64_t i0, int64_t i1,
                        int32_t round, int64_t* undecided, void* stream);

/* The mark of a round of dctfp_greedy_decide from a tile: dctfp_tri_link's walk and arguments -- dctfp_tri_filter_count's survival
 * rule, j > i and min(L1, cap) <= bound, the same flags -- over the rows of a range that ends at range_end.  A row of state 2 (a
 * new representative) lowers assign[j] to its index at every surviving entry (atomic min); a row still undecided looks at the
 * columns j < range_end only and stores next_round into blocked[j] there; any other row is skipped.  state is only read.
 * DCTFP_ERR_INVALID as dctfp_tri_link, for range_end > n_nodes and for next_round < 1; DCTFP_ERR_LIMIT for n_nodes >= 2^31.
 * n_rows, n_cols or n_nodes of 0: nothing to do. */
int dctfp_greedy_tri_mark(dctfp_ctx* ctx, const int32_t* tile, int64_t n_rows, int64_t n_cols, int64_t ld, int64_t row0, int64_t col0,
                          const uint8_t* row_empty, const uint8_t* col_empty, int32_t cap, int32_t bound, int32_t* assign, const int32_t* state,
                          int32_t* blocked, int64_t n_nodes, int64_t range_end, int32_t next_round, void* stream);

/* dctfp_greedy_tri_mark for a LIST of pairs (pi[n], pj[n]), device int32, as dctfp_link_pairs is to dctfp_tri_link -- what is left
 * of dctfp_tri_filter_fill's output after a second cut-off: the pairs whose lower end lies in the range.  One thread per pair,
 * the pair taken as (lo, hi) of its ends: lo of state 2 lowers assign[hi] to lo, lo undecided with hi < range_end stores
 * next_round into blocked[hi].  A pair with an index outside [0, n_nodes) or with both ends equal is skipped.  DCTFP_ERR_LIMIT
 * for n_nodes >= 2^31 or more than 2^31 pairs per call; n_pairs or n_nodes of 0: nothing to do. */
int dctfp_greedy_pairs_mark(dctfp_ctx* ctx, const int32_t* pi, const int32_t* pj, int64_t n_pairs, int32_t* assign, const int32_t* state,
                            int32_t* blocked, int64_t n_nodes, int64_t range_end, int32_t next_round, void* stream);

/* Assignment to existing representatives (dct-sim --assign; not in the reference): the cover pass of greedy clustering between
 * two files, with the distances never stored.  dctfp_rows_assign is to dctfp_greedy_tri_mark what dctfp_rows_link is to
 * dctfp_tri_link: dctfp_tri_filter_count's survival rule applied to the row pairs of a FULL rectangle -- no diagonal, no owner.
 * a / b (device int8, na x d at row stride lda, nb x d at ldb; any alignment, dctfp_l1_matrix's three kernels by it) are the
 * representatives' rows and the new proteins' rows.  For every row r of a and row c of b with min(L1(row r, row c), cap) <= bound:
 *     assign[slot] = min(assign[slot], value),  value = value_a ? value_a[r] : a0 + r,  slot = slot_b ? slot_b[c] : b0 + c
 * value_a / slot_b (device int32, one entry per row of a / b, or NULL) map rows to the caller's nodes; assign (device int32,
 * n_assign entries) starts as 0x7fffffff.  Inside the launch assign is touched by agent-scope relaxed atomics only (a load that
 * skips a minimum which would change nothing, then the minimum); the 128 x 128 sums of a workgroup are compared in registers
 * and nothing else is written.  The result is a minimum over a set the inputs alone fix: it does not depend on the order in
 * which the device ran or on how the caller splits the rows into calls.  A slot outside [0, n_assign) or a negative value is
 * skipped on the device (the host cannot see the two arrays).
 * DCTFP_ERR_INVALID for a NULL ctx, a, b or assign, a negative count or offset, d < 1, lda or ldb < d, cap < 0 or bound < 0;
 * DCTFP_ERR_LIMIT for n_assign >= 2^31, more than 8M (8388480) rows of a or more than 2147483520 rows of b per call.  na, nb or
 * n_assign of 0: nothing to do. */
int dctfp_rows_assign(dctfp_ctx* ctx, const int8_t* a, int64_t na, int64_t lda, const int32_t* value_a, int64_t a0, const int8_t* b,
                      int64_t nb, int64_t ldb, const int32_t* slot_b, int64_t b0, int32_t d, int32_t cap, int32_t bound, int32_t* assign,
                      int64_t n_assign, void* stream);

/* The single-linkage tree of a file (dct-sim --tree; not in the reference): the minimum spanning forest of the graph whose edges
 * are the pairs dctfp_tri_filter_count selects, under the strict order (key, i, j) with key = min(L1, cap) -- cut at any bound b it
 * gives the components dctfp_tri_link gives at b.  Boruvka's algorithm in rounds; per round the caller hands every tile of the
 * triangle to dctfp_tri_nearest, then calls dctfp_tree_hook once, then takes the new labels with dctfp_cluster_labels.
 * comp (device int32, n_nodes) = the labels of this round (the smallest member of every component; 0 .. n - 1 at the start);
 * best (device uint64, n_nodes, 8-byte aligned, started as all ones = none) = per label the lightest edge that leaves its
 * component, packed key << 48 | i << 24 | j with i < j: unsigned order is the edge order.
 * dctfp_tri_nearest extends dctfp_tri_filter_count's survival rule -- the same tile arguments, j > i and min(L1, cap) <= bound, the
 * same flags -- from counting the surviving entries (i, j) to ranking them: every survivor with comp[i] != comp[j] lowers
 * best[comp[i]] and best[comp[j]] to its packed edge.  Inside the launch best is touched by agent-scope relaxed atomics only
 * (a load that skips a minimum which would change nothing, then the minimum), after a reduction in the workgroup: at most one
 * global atomic per (row, 1024 columns) and per (column, 64 rows).  The result is a minimum over a set the inputs fix: it does
 * not depend on the order in which the device ran or on how the triangle is cut into tiles.  A label outside [0, n_nodes) is
 * skipped.  DCTFP_ERR_INVALID as dctfp_tri_link (row0 + n_rows or col0 + n_cols above n_nodes: checked on the host) and for best
 * off an 8-byte boundary; DCTFP_ERR_LIMIT for n_nodes > 2^24 or cap > 32767 (the packing).  n_rows, n_cols or n_nodes of 0:
 * nothing to do. */
int dctfp_tri_nearest(dctfp_ctx* ctx, const int32_t* tile, int64_t n_rows, int64_t n_cols, int64_t ld, int64_t row0, int64_t col0,
                      const uint8_t* row_empty, const uint8_t* col_empty, int32_t cap, int32_t bound, const int32_t* comp, uint64_t* best,
                      int64_t n_nodes, void* stream);

/* The end of a round of dctfp_tri_nearest (which extends dctfp_tri_filter_count's survival rule to the lightest surviving edge
 * per component), one thread per node, in launches of its own: every label c (comp[c] == c) whose best[c] names an edge (i, j)
 * leaving its component appends it -- edge_i / edge_j / edge_key [slot] (device int32, max_edges entries each), slot = the old
 * value of *counter (device int32, the caller's running total, started as 0), which grows by one -- and joins i and j in `parent`
 * (dctfp_tri_link's forest).  An edge chosen by both of its components is appended once, by the lower label.  Nothing is written
 * at or beyond max_edges (a forest of n_nodes has at most n_nodes - 1 edges; the counter still counts).  The hooks of a round
 * close no cycle because the edge order is strict.  Afterwards every entry of best is set back to all ones.
 * DCTFP_ERR_INVALID for a NULL argument (the edge arrays may be NULL when max_edges is 0), a negative count or best off an 8-byte
 * boundary; DCTFP_ERR_LIMIT for n_nodes > 2^24.  n_nodes of 0: nothing to do. */
int dctfp_tree_hook(dctfp_ctx* ctx, const int32_t* comp, uint64_t* best, int32_t* parent, int64_t n_nodes, int32_t* edge_i, int32_t* edge_j,
                    int32_t* edge_key, int32_t* counter, int64_t max_edges, void* stream);

/* Reciprocal best hits of two files (dct-sim --db --rbh; not in the reference): per protein of file A its best hit in file B and
 * per protein of B its best hit in A, both kept in one pass over an int32 tile of L1 values (dctfp_protein_min's output, or
 * dctfp_l1_matrix of the last rows).  Entry (r, c), at tile[r * ld + c], is the L1 of protein row0 + r of A and protein col0 + c of
 * B -- a FULL rectangle: no diagonal, no components, no owner.  key = cap when the row is flagged in row_empty, the column in
 * col_empty (device uint8, one per row / column of the tile, either may be NULL) or the value is negative or >= cap, else the
 * value: dctfp_tri_filter_count's rule.  Every entry with key <= bound lowers
 *     best_row[row0 + r] to key << 32 | (col0 + c)   and   best_col[col0 + c] to key << 32 | (row0 + r)
 * (device uint64, n_a / n_b entries, 8-byte aligned).  Unsigned 64-bit order of these words is the order (key, index): ties go
 * to the lower protein.  All ones = none; the caller fills both arrays before the first tile.  Inside the launch the two arrays
 * are touched by agent-scope relaxed atomics only (a load that skips a minimum which would change nothing, then the minimum),
 * after a reduction in the workgroup: at most one global atomic per (row, 1024 columns) and per (column, 64 rows).  The result
 * is a minimum over a set the inputs fix: it does not depend on the order in which the device ran, on how the rectangle is cut
 * into tiles or on the order of the calls.  The tile is read with plain 4-byte loads: any ld >= n_cols, a column view of a wider
 * tensor included.
 * DCTFP_ERR_INVALID, with a message, for: a NULL ctx, tile, best_row or best_col; a negative count or offset; ld < n_cols;
 * cap < 0, bound outside -1 .. cap; a cap above 4194302 (a row's minimum is packed as key << 10 | column in 32 bits); n_a or n_b
 * negative or >= 2^31; row0 + n_rows > n_a or col0 + n_cols > n_b (checked on the host: the kernel bounds no index); a tile off a
 * 4-byte or an array off an 8-byte boundary.  n_rows or n_cols of 0: nothing to do. */
int dctfp_rect_best(dctfp_ctx* ctx, const int32_t* tile, int64_t n_rows, int64_t n_cols, int64_t ld, int64_t row0, int64_t col0,
                    const uint8_t* row_empty, const uint8_t* col_empty, int32_t cap, int32_t bound, uint64_t* best_row, int64_t n_a,
                    uint64_t* best_col, int64_t n_b, void* stream);

/* The summed distances behind a cluster's medoid (dct-sim --cluster --rep medoid; not in the reference): per protein of one file
 * the sum of its distances to the other members of its own cluster, in one pass over an int32 tile of L1 values (dctfp_protein_min's
 * output, or dctfp_l1_matrix of the last rows).  Entry (r, c), at tile[r * ld + c], is the L1 of proteins i = row0 + r and
 * j = col0 + c of the file.  key = cap when the row is flagged in row_empty, the column in col_empty (device uint8, one per row /
 * column of the tile, either may be NULL) or the value is negative or >= cap, else the value: dctfp_tri_filter_count's rule.  Every
 * entry with j > i and labels[i] == labels[j] (device int32, n_nodes entries: dctfp_cluster_labels' output; the values are only
 * compared) adds its key to
 *     sums[i]   and   sums[j]
 * (device uint64, n_nodes entries, 8-byte aligned; the caller zeroes it before the first tile).  The tile may hold entries on
 * both sides of the diagonal: j > i takes every unordered pair once.  `bound` is accepted, so that the ten tile values are those
 * of every export that scans a tile, and ignored: a sum has no cut-off.  Inside the launch sums is touched by agent-scope relaxed
 * 64-bit atomic adds only, after a reduction in the workgroup to 32-bit partial sums: at most one global atomic per (row, 1024
 * columns) and per (column, 64 rows), none for a partial sum of 0.  Integer addition commutes: the result is a sum over a set the
 * inputs fix and does not depend on the order in which the device ran, on how the triangle is cut into tiles or on the order of
 * the calls.  The tile is read with plain 4-byte loads: any ld >= n_cols, a column view of a wider tensor included.
 * DCTFP_ERR_INVALID, with a message, for: a NULL ctx, tile, labels or sums; a negative count or offset; ld < n_cols; cap < 0; a
 * cap above 4194303 (a row's partial sum of 1024 keys, and a column's of 64, stay in 32 bits); n_nodes negative or >= 2^31;
 * row0 + n_rows > n_nodes or col0 + n_cols > n_nodes (checked on the host: the kernel bounds no index); a tile or labels off a
 * 4-byte or sums off an 8-byte boundary.  n_rows or n_cols of 0: nothing to do. */
int dctfp_label_sums(dctfp_ctx* ctx, const int32_t* tile, int64_t n_rows, int64_t n_cols, int64_t ld, int64_t row0, int64_t col0,
                     const uint8_t* row_empty, const uint8_t* col_empty, int32_t cap, int32_t bound, const int32_t* labels, uint64_t* sums,
                     int64_t n_nodes, void* stream);

/* Density clusters of one file (dct-sim --cluster --min-neighbors; not in the reference): DBSCAN whose radius is the cut-off.  The
 * graph's edges are the pairs dctfp_tri_filter_count selects: entry (r, c) of an int32 tile of L1 values, at tile[r * ld + c], is
 * the L1 of proteins i = row0 + r and j = col0 + c, and it COUNTS when j > i and key <= bound, key = cap when the row is flagged in
 * row_empty, the column in col_empty (device uint8, one per row / column of the tile, either may be NULL) or the value is negative
 * or >= cap, else the value.  The tile may hold entries on both sides of the diagonal: j > i takes every unordered pair once.  Two
 * passes over the tiles of the triangle, in dctfp_label_sums' walk (plain 4-byte loads: any ld >= n_cols, a column view of a wider
 * tensor included):
 *   dctfp_tri_degree    -- every counted entry adds 1 to deg[i] and to deg[j] (device uint32, n_nodes entries; the caller zeroes
 *                          it before the first tile).  Afterwards deg[x] = the number of edges at x.
 *   dctfp_tri_link_core -- core (device uint8, n_nodes entries, nonzero = core: the caller's deg[x] >= M, written before the call)
 *                          is only read.  A counted entry with both ends core is a union in `parent` (dctfp_tri_link's forest,
 *                          read with dctfp_cluster_labels); one with exactly one core end lowers nearest[the other end] (device
 *                          int32, n_nodes entries, 0x7fffffff = none: the caller fills it before the first tile) to the core's
 *                          index; one without a core end does nothing.  Afterwards nearest[x] of a non-core x = its lowest core
 *                          neighbour, the core whose cluster a border joins.
 * Inside a launch deg, nearest and parent are touched by agent-scope relaxed atomics only (adds, minima, and the forest's loads
 * and compare-and-swaps), after a reduction in the workgroup: at most one global atomic on deg / nearest per (row, 1024 columns)
 * and per (column, 64 rows), none for a count of 0 or a minimum of none.  A count, a minimum and the components of a graph are
 * fixed by the inputs: the results do not depend on the order in which the device ran, on how the triangle is cut into tiles or on
 * the order of the calls.
 * DCTFP_ERR_INVALID, with a message that starts with the export's name, for: a NULL ctx, tile or array; a negative count or
 * offset; ld < n_cols; cap < 0, bound outside -1 .. cap; n_nodes negative or >= 2^31; row0 + n_rows > n_nodes or
 * col0 + n_cols > n_nodes (checked on the host: the kernels bound no index); a tile, deg, parent or nearest off a 4-byte boundary.
 * n_rows or n_cols of 0: nothing to do. */
int dctfp_tri_degree(dctfp_ctx* ctx, const int32_t* tile, int64_t n_rows, int64_t n_cols, int64_t ld, int64_t row0, int64_t col0,
                     const uint8_t* row_empty, const uint8_t* col_empty, int32_t cap, int32_t bound, uint32_t* deg, int64_t n_nodes,
                     void* stream);
int dctfp_tri_link_core(dctfp_ctx* ctx, const int32_t* tile, int64_t n_rows, int64_t n_cols, int64_t ld, int64_t row0, int64_t col0,
                        const uint8_t* row_empty, const uint8_t* col_empty, int32_t cap, int32_t bound, const uint8_t* core, int32_t* parent,
                        int32_t* nearest, int64_t n_nodes, void* stream);

/* AUC1 of a labelled file (dct-sim --auc1; the reference's bench/cathdb/plot_results.py reads the same number out of ranked text):
 * per protein the hits of its own family ranked before its first hit of another family.  Entry (r, c) of an int32 tile of L1
 * values, at tile[r * ld + c], is the L1 of proteins i = row0 + r and j = col0 + c of ONE file, and it COUNTS when
 * dctfp_tri_degree would count it: j > i and key <= bound, key = cap when the row is flagged in row_empty, the column in col_empty
 * (device uint8, one per row / column of the tile, either may be NULL) or the value is negative or >= cap, else the value.  A
 * counted entry makes j a hit of i and i a hit of j.  fam (device int32, n_nodes entries, written before the call; the values are
 * only compared) names every protein's family, and the hits of one protein are ranked by the word key << 32 | index of the hit:
 * unsigned 64-bit order = (key, index), ties to the lower protein.  Two passes over the tiles of the triangle, in
 * dctfp_tri_degree's walk (plain 4-byte loads: any ld >= n_cols, a column view of a wider tensor included):
 *   dctfp_tri_first_fp  -- a counted entry with fam[i] != fam[j] lowers first[i] to key << 32 | j and first[j] to key << 32 | i
 *                          (device uint64, n_nodes entries, 8-byte aligned, all ones = none: the caller fills it before the
 *                          first tile).  Afterwards first[x] = the first false positive of x.
 *   dctfp_tri_tp_before -- first is finished and only read.  A counted entry with fam[i] == fam[j] adds 1 to tp[i] when
 *                          key << 32 | j < first[i] and, decided on its own, 1 to tp[j] when key << 32 | i < first[j] (device
 *                          uint32, n_nodes entries; the caller zeroes it before the first tile).  Afterwards tp[x] = the true
 *                          positives of x ranked before its first false positive.
 * Inside a launch first (pass 1) and tp (pass 2) are touched by agent-scope relaxed atomics only -- dctfp_rect_best's load and
 * minimum, dctfp_tri_degree's add -- after a reduction in the workgroup: at most one global atomic per (row, 1024 columns) and per
 * (column, 64 rows), none for a minimum of none or a count of 0.  A minimum and a count are fixed by the inputs: the results do
 * not depend on the order in which the device ran, on how the triangle is cut into tiles or on the order of the calls.
 * DCTFP_ERR_INVALID, with a message that starts with the export's name, for: a NULL ctx, tile or array; a negative count or
 * offset; ld < n_cols; cap < 0, bound outside -1 .. cap; n_nodes negative or >= 2^31; row0 + n_rows > n_nodes or
 * col0 + n_cols > n_nodes (checked on the host: the kernels bound no index); a tile, fam or tp off a 4-byte or first off an 8-byte
 * boundary; for dctfp_tri_first_fp a cap above 4194302 (a row's minimum is packed as key << 10 | column in 32 bits).  n_rows or
 * n_cols of 0: nothing to do. */
int dctfp_tri_first_fp(dctfp_ctx* ctx, const int32_t* tile, int64_t n_rows, int64_t n_cols, int64_t ld, int64_t row0, int64_t col0,
                       const uint8_t* row_empty, const uint8_t* col_empty, int32_t cap, int32_t bound, const int32_t* fam, uint64_t* first,
                       int64_t n_nodes, void* stream);
int dctfp_tri_tp_before(dctfp_ctx* ctx, const int32_t* tile, int64_t n_rows, int64_t n_cols, int64_t ld, int64_t row0, int64_t col0,
                        const uint8_t* row_empty, const uint8_t* col_empty, int32_t cap, int32_t bound, const int32_t* fam,
                        const uint64_t* first, uint32_t* tp, int64_t n_nodes, void* stream);

/* The score distribution of one file (dct-sim --hist; the reference draws it from printed pairs, bench/G6PD/hist.py, and takes the
 * ROC AUC of labelled pairs the same way, bench/homo/results/AUC.py): how many pairs have each key.  Entry (r, c) of an int32 tile
 * of L1 values, at tile[r * ld + c], is the L1 of proteins i = row0 + r and j = col0 + c of ONE file, and it COUNTS when
 * dctfp_tri_degree would count it: j > i and key <= bound, key = cap when the row is flagged in row_empty, the column in col_empty
 * (device uint8, one per row / column of the tile, either may be NULL) or the value is negative or >= cap, else the value.  Every
 * counted entry adds 1 to
 *     hist[cls * (cap + 1) + key]
 * (device uint64, 8-byte aligned, cap + 1 entries per class; the caller zeroes it before the first tile).  fam NULL: one class,
 * cls = 0.  Else fam (device int32, n_nodes entries, written before the call; the values are only compared) names every protein's
 * family and cls = (fam[i] != fam[j]): row 0 counts the pairs of one family, row 1 the pairs of two.  The tile may hold entries on
 * both sides of the diagonal: j > i takes every unordered pair once.  A loop of its own over the tile (plain 4-byte loads: any
 * ld >= n_cols, a column view of a wider tensor included); a workgroup counts in 32-bit counters of its own in LDS over all its jobs
 * -- lanes of a wave that share a key add once -- and sends every non-zero bin out once.  Inside the launch hist is touched by
 * agent-scope relaxed 64-bit atomic adds only.  Integer addition commutes: the counts add up over tiles and over calls and do not
 * depend on the order in which the device ran, on how the triangle is cut into tiles or on the order of the calls.
 * DCTFP_ERR_INVALID, with a message that starts with the export's name, for: a NULL ctx, tile or hist; a negative count or offset;
 * ld < n_cols; cap < 0, bound outside -1 .. cap; a cap above 20479 (two classes of cap + 1 counters fill the 160 KiB of LDS of a
 * CU); n_nodes negative or >= 2^31; row0 + n_rows > n_nodes or col0 + n_cols > n_nodes (checked on the host, with or without fam:
 * the kernel bounds no index); a tile or fam off a 4-byte or hist off an 8-byte boundary.  n_rows or n_cols of 0: nothing to do. */
int dctfp_tri_hist(dctfp_ctx* ctx, const int32_t* tile, int64_t n_rows, int64_t n_cols, int64_t ld, int64_t row0, int64_t col0,
                   const uint8_t* row_empty, const uint8_t* col_empty, int32_t cap, int32_t bound, const int32_t* fam, int64_t n_nodes,
                   uint64_t* hist, void* stream);

/* The moments of every protein's background (dct-sim --db --zscore: a z-score beside every hit, the place of its L1 in the L1s of
 * the query against the whole database -- what DALI's Z-score and the E-values of BLAST, MMseqs2 and Foldseek tell their users).
 * Entry (r, c) of an int32 tile of L1 values, at tile[r * ld + c], is the L1 of protein row0 + r of one file and protein col0 + c
 * of another: the full rectangle, no diagonal.  An entry COUNTS unless its row is flagged in row_empty, its column in col_empty
 * (device uint8, one per row / column of the tile, either may be NULL) or its value x has (uint32_t)x >= cap: cap is the EXCLUSION
 * LIMIT here, not a ceiling -- a negative value and dctfp_protein_min's 0x7fffffff are left out, a value below cap counts raw.
 * bound is not read (pass cap).  A counting entry adds (1, x, x * x) to
 *     row_mom[k * n_a + row0 + r]   and   col_mom[k * n_b + col0 + c],   k = 0, 1, 2
 * (device uint64, 8-byte aligned, 3 n_a resp. 3 n_b entries: the planes count, sum and sum of squares; the caller zeroes them
 * before the first tile).  Either array may be NULL: that side is not computed, its n is not compared with the tile, and the
 * other side pays nothing for it.  A loop of its own over the tile (plain 4-byte loads: any ld >= n_cols, a column view of a wider
 * tensor included), jobs of 64 rows x 1024 columns; partial sums are reduced in the workgroup -- 32-bit sums, 64-bit squares --
 * and sent with agent-scope relaxed 64-bit atomic adds, the only way the arrays are touched inside the launch: at most 3 per
 * (row, 1024 columns) and 3 per (column, 64 rows), none for a count of 0.  Integer addition commutes: the words are exact, add up
 * over tiles and over calls and do not depend on the order in which the device ran, on how the rectangle is cut into tiles or on
 * the order of the calls.
 * DCTFP_ERR_INVALID, with a message that starts with the export's name, for: a NULL ctx or tile; row_mom and col_mom both NULL; a
 * negative count or offset or one of 2^31 or more; ld < n_cols; cap < 0 or above 16777216 (a wave's 32-bit sum of one row, 256
 * entries, and a column's over a band must hold); n_a or n_b negative or >= 2^31; row0 + n_rows > n_a with row_mom, col0 + n_cols >
 * n_b with col_mom (checked on the host: the kernel bounds no index); n x (cap - 1)^2 of 2^64 or more, n = max(n_b, col0 + n_cols)
 * for row_mom and max(n_a, row0 + n_rows) for col_mom (a sum of squares must fit its word); a tile off a 4-byte or an array off an
 * 8-byte boundary.  n_rows or n_cols of 0: nothing to do. */
int dctfp_rect_moments(dctfp_ctx* ctx, const int32_t* tile, int64_t n_rows, int64_t n_cols, int64_t ld, int64_t row0, int64_t col0,
                       const uint8_t* row_empty, const uint8_t* col_empty, int32_t cap, int32_t bound, uint64_t* row_mom, int64_t n_a,
                       uint64_t* col_mom, int64_t n_b, void* stream);

/* query_db's search (src/query_db.py:75-87: a flat FAISS index forced to METRIC_L1 at :76, index.search at :87) without a
 * distance matrix: for query rows q (nq x d, row stride ldq) and database rows b (nb x d, stride ldb), int8 on the device, each
 * query row's k_eff = min(k, nb) nearest database rows by L1, ascending, ties to the lower row -- what dctfp_row_select +
 * dctfp_row_order return on the dctfp_l1_matrix of the two.  out_val / out_idx: device int32 (nq, k_eff), contiguous; col0 is
 * added to every index (a caller streaming database blocks).  The distances of a 128-row query tile against a slice of the
 * database and the selection run in one kernel; the slices' lists are merged on the device.  Rows must start on 16-byte
 * boundaries (q, b, ldq, ldb); an empty side returns at once.  DCTFP_ERR_LIMIT for k > 1024 or d > 512 (the caller takes
 * dctfp_l1_matrix + dctfp_row_select then), more than 8M query rows, or col0 + nb >= 2^31.  Uses the context's scratch. */
int dctfp_l1_knn(dctfp_ctx* ctx, const int8_t* q, int64_t nq, int64_t ldq, const int8_t* b, int64_t nb, int64_t ldb, int32_t d, int32_t k,
                 int64_t col0, int32_t* out_val, int32_t* out_idx, void* stream);

/* ranked_hits (src/query_db.py:33-40: the reference's stable sort of a query protein's hits by distance) for many proteins:
 * val / idx = the (n_rows, k) sorted hit lists of dctfp_l1_knn, protein p owning rows [qoff[p], qoff[p + 1]) (prot_of_row[r] =
 * its protein; < 0: a protein the caller ranks itself, skipped).  The protein's hits ordered by (distance, fingerprint within
 * the protein, hit rank); the first min(khits, f k) of them are written from line line_base[p] on: out_qrow = the fingerprint
 * row, out_drow = the database row (idx), out_dist.  All device pointers.  Work per hit grows with the protein's f (one binary
 * search per other fingerprint): callers send proteins of many fingerprints to the host.  DCTFP_ERR_LIMIT above 4294967040 hits
 * (n_rows x k) per call: one thread per hit, and one launch holds fewer than 2^32 threads. */
int dctfp_query_rank(dctfp_ctx* ctx, const int32_t* val, const int32_t* idx, int64_t n_rows, int32_t k, const int64_t* qoff,
                     const int32_t* prot_of_row, const int64_t* line_base, int32_t khits, int32_t* out_qrow, int32_t* out_drow,
                     int32_t* out_dist, void* stream);

/* query_db's result lines (src/query_db.py:57): line n = "Query: {qpid} {qdom}, Result {rank}: {dpid} {ddom}, Similarity: {score}\n"
 * in UTF-8, from byte line_off[n] of out.  qrow / drow index the query / database string tables: the pid of row r is bytes
 * [q_pid_off[r], q_pid_off[r + 1]) of q_txt, its domain [q_dom_off[r], q_dom_off[r + 1]) (likewise d_*); rank = the printed
 * number; the score of distance x is bytes [score_off[x], score_off[x + 1]) of score_txt (a host-built table of the strings the
 * reference prints).  line_off = the prefix sum of the line lengths (the caller's: every line must fit in out).  All device
 * pointers.  DCTFP_ERR_LIMIT above 4294967040 lines per call. */
int dctfp_query_lines(dctfp_ctx* ctx, int64_t n_lines, const int32_t* qrow, const int32_t* drow, const int32_t* dist, const int32_t* rank,
                      const uint8_t* q_txt, const int64_t* q_pid_off, const int64_t* q_dom_off, const uint8_t* d_txt, const int64_t* d_pid_off,
                      const int64_t* d_dom_off, const uint8_t* score_txt, const int64_t* score_off, const int64_t* line_off, uint8_t* out,
                      void* stream);

/* The address under which the GPU sees a pinned (page-locked, mapped) host buffer, e.g. a torch tensor created with
 * pin_memory=True.  A caller that passes this address as `out` of dctfp_quantize gets the int8 result written straight
 * into host memory: no device buffer, no copy -- what a one-protein-per-call user wants (480 bytes per domain). */
int dctfp_host_device_pointer(void* host, void** dev);

/* Blocks until everything enqueued on `stream` (a hipStream_t, NULL = the default stream) is done -- for bindings that
 * have no HIP binding of their own: the synchronous one-protein-per-call user waits here for the bytes that
 * dctfp_quantize writes into its pinned result buffer. */
int dctfp_stream_synchronize(void* stream);

/* Diagnostics (no reference counterpart).
 * dctfp_runtime_info: text into buf -- the HIP version the library was compiled against, the version and file of the HIP
 *   runtime it is bound to in this process, and every libamdhip64 / libhsa-runtime64 / libamd_comgr file mapped.  The
 *   library must run on the runtime that owns the device pointers and streams it is handed (the caller's torch): returns
 *   the number of distinct libamdhip64 files mapped, 1 when healthy.
 * dctfp_crash_handler(1): SIGABRT / SIGSEGV / SIGBUS print the native backtrace of the failing thread to stderr before the
 *   previously installed handler (e.g. Python's faulthandler) runs; also installed at load time when the environment has
 *   DCTFP_CRASH_BACKTRACE=1.  (0) removes it. */
int dctfp_runtime_info(char* buf, int64_t cap);
int dctfp_crash_handler(int enable);

/* Options (no reference counterpart).
 *
 * What a user of the drop-in may want:
 *   "path"         0 (default) = by shape: the walk kernel (stage A + stage B in one launch, nothing but int8 written)
 *                  for n = 3, 64 < m <= 80 (float32 rows: <= 96 -- PROST's [3, 85]; "last_walk_groups" reads 5 or 6),
 *                  float32 / float16 / bfloat16 rows, 512 <= D <= 2560 and calls of 256 jobs
 *                  (layers x domains) or more -- domains above 8 192 rows are cut out of such a call and run on their own;
 *                  stage A -> scratch -> stage B otherwise.
 *                  1 = always the two-kernel path; 2 = the walk kernel wherever its shapes allow (any number of jobs)
 *   "last_path"    read only: which kernels the last dctfp_quantize launched last (1 = two kernels, 2 = walk kernel)
 *   "last_stage_a" read only: the stage-A build the two-kernel path launched last (the last chunk of the last layer group
 *                  of the last dctfp_quantize), written by its launcher from the template arguments of the instantiation;
 *                  0 = that group took another route (walk kernel, general walk kernel, zero fill).  One byte per field:
 *                  byte 0 storage type (DCTFP_F32 .. DCTFP_BF16, plus 1), byte 1 N (kept rows), byte 2 VEC (channels per
 *                  lane), byte 3 WAVES, byte 4 UNROLL (rows in flight), byte 5 flags: 1 = FUSED build, 2 = Y' packed,
 *                  4 = split (stage_a_split_kernel ran instead: float32, N 3, VEC 4, WAVES 8, UNROLL 4, not fused)
 *   "last_stage_b" read only: ... and its stage B.  Byte 0 form: 1 = MFMA kernel, 2 = slab kernel reading Y', 3 = slab
 *                  kernel reading the row-split partial sums; byte 1 NT (16-column tiles of the MFMA build, 1 .. 8; 0 for
 *                  the slab forms); byte 2 flags: 1 = PACKED MFMA build, 2 = stage_a_combine_kernel ran before it,
 *                  4 = ... writing packed Y'.  0 as for "last_stage_a"
 *   "last_walk"    read only: the walk-kernel build launched last (the last layer group of the last dctfp_quantize /
 *                  dctfp_quantize_windows), written by its launcher from the template arguments of the instantiation; 0 = that
 *                  group took another route.  Byte 0 storage type (as "last_stage_a"), byte 1 S (waves per workgroup: 3, 5,
 *                  10), byte 2 NT (16-column groups: 5 or 6, what "last_walk_groups" reads), byte 3 flags: 1 = FUSED build,
 *                  2 = WIN (a two-source build: rows that are the mean of two windows' rows)
 *   "last_gen"     read only: ... and the general walk kernel's.  Byte 0 storage type, byte 1 N (kept rows), byte 2 VEC (channels
 *                  per lane), byte 3 NTC (column groups of fragments per step: 4 for m <= 64, else 8), byte 4 flags: 1 = FUSED
 *                  build (what "last_gen_fused" reads), byte 5 the waves per workgroup it was launched with, byte 6 its Y' slots
 *                  in LDS (1 or 2).  0 as for "last_walk"
 *   "walk_launches" read only: walk-kernel launches of this context so far
 *   "last_knn_slices" read only: database slices that owned a column in the last dctfp_l1_knn launch (1: no merge kernels)
 *   "knn_calls"    read only: dctfp_l1_knn launches of this context so far
 *   "fuse"         1 (default) = proteins given as parts + whole protein are streamed once
 *   "gen_fuse"     1 (default) = ... also by the general walk kernel ("path" = 2, n <= 5, at most ten waves per workgroup);
 *                  0 = it streams every job on its own, as through round 4.  "last_gen_fused" (read only): whether the last
 *                  dctfp_quantize launched the general walk kernel with fused walks
 *   "workspace_mb" two-kernel path: cap of the float64 scratch between the kernels
 *   "profile"      1 = bracket the kernels with hipEvents (see dctfp_profile)
 *   "degenerate_channels"  read: number of (layer, domain, channel) triples seen so far whose resampled values were all
 *                  equal -- an exactly constant channel.  Mathematically that is 0/0 = NaN and the whole (layer, domain)
 *                  block becomes 0, which is what this library writes; the reference (scipy / pocketfft) does the same at
 *                  most domain lengths but scales its own round-off noise at the others (tests/golden/fence_golden.json:
 *                  225 of the lengths 3..2000), so for these blocks -- and only these -- the result is reported instead of
 *                  matched.  Reading synchronises the device; writing 0 resets the counter.
 *   "degenerate_seen"  read: 1 if a kernel has met such a channel since the last read (then cleared).  The kernels set a
 *                  word in pinned host memory, so this costs no synchronisation and no copy: it is meaningful once the
 *                  caller has waited for its call.  The flag belongs to the CONTEXT, not to a call: a caller that wants to
 *                  know about its own call reads (= clears) it before enqueueing and again after waiting.  dctdomain_amd.Fingerprint.quantize and make_db read it after every
 *                  call / flush and log a warning with the protein ids.
 *
 * Engineering knobs -- ONLY in libdctfp_experiments.so, the same sources built with -DDCTFP_EXPERIMENTS (A/B measurements
 * under tools/, kernel-variant parity tests); libdctfp.so answers DCTFP_ERR_INVALID "unknown option" to them.  Their
 * defaults are what is measured and shipped:
 *   "ab_run_jobs"  walk kernel: jobs per workgroup (0 = by the bytes per job and the size of the call)
 *   "ab_align"     walk kernel: walks to look ahead for a workgroup whose job count is a multiple of the flush group, so that
 *                  its last flush is a full one (default 2; 0 = off)
 *   "ab_taper"     walk kernel: the jobs of the last N quarter-rounds of workgroups go out in workgroups of one flush
 *                  group, so that the launch ends evenly (default 4 = one round; 0 = off)
 *   "ab_longest_first" walk kernel: workgroups ordered by the rows they stream, longest first (0 = auto: batches of
 *                  domains at D > 1280, 1 = always, 2 = never)
 *   "small_b_jobs" two-kernel path: calls with fewer jobs (layers x domains) than this run stage B over 64-channel slabs
 *                  instead of the MFMA kernel (default 512)
 *   "a_waves"      two-kernel path: waves per stage-A workgroup: 0 = by average rows per job (default), 2, 4, 8, 16 --
 *                  a forced count goes through the same rules as the automatic one (16 at 4 channels per lane only, at most
 *                  4 at 8 channels per lane, n >= 4 always 4), so it selects one of the builds the automatic choice uses
 *   "overlap"      two-kernel path: sub-chunks of a large batch whose stage B runs on a side stream under the
 *                  next sub-chunk's stage A (1 = off, default 4)
 *   "pack_y"       two-kernel path, 1 (default) = n = 3: the scratch between the kernels holds {0, t, 1} as one
 *                  float64 + 2-bit states per channel (9 bytes instead of 24)
 *
 * Instrumented build only (-DDCTFP_WALK_TIMELINE, tools/build_variant.sh; never shipped): "walk_timeline_0" .. "_10" read the
 * time (10 ns ticks) the waves of the walk kernel spent per phase; "walk_trace" = N records {begin, end, HW_ID, workgroup}
 * of every wave of the next launch, "walk_trace_host" = address of a host copy (tools/walk_timeline.py, tools/walk_trace.py).
 *
 * Test hooks (libdctfp_experiments.so only; tests/test_context_cache.py, tests/asan/driver.cpp):
 *   "basis_cap_kb" size of the cosine-table arena at which it starts over (default 1 GiB); "basis_restarts" /
 *                  "basis_tables" read how often it did / how many tables are cached
 *   "test_fail_once" 1 = the next dctfp_quantize fails with DCTFP_ERR_NOMEM after its table lookups (nothing may stay
 *                  cached that no kernel has filled) */
int dctfp_set_option(dctfp_ctx* ctx, const char* name, int64_t value);
int dctfp_get_option(dctfp_ctx* ctx, const char* name, int64_t* value);

/* With "profile" = 1: synchronises the recorded events and returns the accumulated
 * device time (ms) and launch count of stage A ([0]) and stage B ([1]) since the last
 * call, then resets the accumulators. */
int dctfp_profile(dctfp_ctx* ctx, double ms[2], int64_t launches[2]);

#ifdef __cplusplus
}
#endif
#endif /* DCTFP_H */
