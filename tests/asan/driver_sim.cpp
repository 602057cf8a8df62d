// The second section of the host driver (driver.cpp, hip_stub.cpp): the exports of dct-sim and query_db, from dctfp_pair_min to
// dctfp_query_lines, with dctfp_idct_quant and dctfp_scale.  Three parts, every call through `call` of driver.h (the three caller
// streams in turn, the stream-order check, launch failures injected):
//   (a) random valid calls at small sizes on buffers of exactly the promised size, and malformed ones: NULL for every required
//       pointer, every count below its smallest value, ld < n_cols, bound > cap, rows off their alignment;
//   (b) the limit table: per documented limit of an export its largest accepted value (DCTFP_OK, and not one launch the stub
//       refuses) and its smallest refused value (the code the header names, never DCTFP_ERR_HIP), on pointers that point nowhere;
//   (c) overflow probes: every check that adds or multiplies 64-bit arguments, with one of them at INT64_MAX.
// One function per export states its arguments once; a value is drawn where it is named, together with the range the header accepts,
// and the malformed calls, the limit rows and the probes replace values by name.
#include <algorithm>
#include <climits>
#include <cstdint>
#include <cstdlib>
#include <map>
#include <string>
#include <vector>

#include "driver.h"

extern "C" void __sanitizer_set_death_callback(void (*callback)(void));

namespace {

constexpr int64_t kNoBound = INT64_MIN;
constexpr int64_t kI31 = 0x7fffffff;
// The driver's own arithmetic on values a probe has put at the end of their type: a buffer is sized from clamped counts (c), and a
// value that follows from another (ld from n_cols, n_nodes from the tile) is formed with a saturating sum (plus).
int64_t c(int64_t n) { return std::min<int64_t>(std::max<int64_t>(n, 0), 1 << 22); }
int64_t plus(int64_t a, int64_t b) {
    int64_t r;
    return __builtin_add_overflow(a, b, &r) ? (b < 0 ? INT64_MIN : INT64_MAX) : r;
}

struct Sim {
    dctfp_ctx* ctx = nullptr;
    std::mt19937_64 rng;
    bool fake = false;            // pointers that point nowhere (limit rows, probes): no kernel runs, nothing is dereferenced
    int null_ptr = -1;            // the pointer of this index is NULL / off its alignment
    int misaligned_ptr = -1;
    long fail_after = -1;         // operator new of the library fails after so many allocations (armed around the export only)
    std::map<std::string, int64_t> over;   // values replaced by name
    // what a call tells about itself
    struct Seen { std::string name; int64_t lo, hi; };
    std::vector<Seen> seen;
    int n_ptrs = 0;
    uint64_t required = 0, aligned = 0;
    std::vector<void*> allocs;

    int64_t uni(int64_t lo, int64_t hi) {   // (always one draw, an empty range included)
        const uint64_t r = rng();
        return hi <= lo ? lo : lo + (int64_t)(r % (uint64_t)(hi - lo + 1));
    }
    // the value of argument `name`: `dflt` unless replaced; [lo, hi] = what the export accepts of it, given the values before it
    int64_t v(const char* name, int64_t dflt, int64_t lo = kNoBound, int64_t hi = kNoBound) {
        seen.push_back({name, lo, hi});
        const auto it = over.find(name);
        return it == over.end() ? dflt : it->second;
    }
    // an array of `count` elements; align > 0: the export asks for that alignment; optional: NULL is a valid value (drawn now and then)
    // real: memory even where the call's pointers point nowhere (the library itself writes it: hipMemsetAsync)
    template <typename T> T* buf(int64_t count, int align = 0, bool optional = false, bool real = false) {
        const int i = n_ptrs++;
        if (!optional) required |= 1ull << i;
        if (align) aligned |= 1ull << i;
        const bool drop = optional && uni(0, 3) == 0 && i != misaligned_ptr;
        if (i == null_ptr || drop) return nullptr;
        const size_t off = i == misaligned_ptr ? (size_t)align / 2 : 0;
        if (fake && !real) return (T*)(uintptr_t)(0x100000 + 0x1000 * (uintptr_t)i + off);
        void* p = nullptr;
        const size_t bytes = (size_t)std::max<int64_t>(count, 0) * sizeof(T) + off;
        if (posix_memalign(&p, 64, bytes ? bytes : 1)) abort();
        memset(p, 0, bytes);
        allocs.push_back(p);
        return (T*)((char*)p + off);
    }
    void reset() {
        for (void* p : allocs) free(p);
        allocs.clear(), seen.clear();
        n_ptrs = 0, required = aligned = 0;
    }
    template <typename F> int run(F f) {
        g_fail_after = g_plain ? -1 : fail_after;
        const int rc = f();
        g_fail_after = -1;
        return rc;
    }
};

// ---- the ten values of every export that scans a tile
struct Tile {
    const int32_t* tile;
    int64_t n_rows, n_cols, ld, row0, col0;
    const uint8_t *row_empty, *col_empty;
    int32_t cap, bound;
    int64_t last() const { return std::max(row0 + n_rows, col0 + n_cols); }   // (small values only: a replaced one is not added here)
};
Tile tile_of(Sim& s, bool bound_read = true, int tile_align = 4) {   // bound_read: the export compares bound (two accept and ignore it)
    Tile t;
    t.n_rows = s.v("n_rows", s.uni(1, 200), 0);
    t.n_cols = s.v("n_cols", s.uni(1, 2100), 0);
    t.ld = s.v("ld", plus(t.n_cols, s.uni(0, 2) ? 0 : s.uni(1, 9)), t.n_cols);
    t.row0 = s.v("row0", s.uni(0, 3) ? s.uni(0, 500) : 0, 0);
    t.col0 = s.v("col0", s.uni(0, 3) ? s.uni(0, 500) : 0, 0);
    t.cap = (int32_t)s.v("cap", 17000, 0);
    t.bound = (int32_t)s.v("bound", s.uni(-1, t.cap), bound_read ? -1 : kNoBound, bound_read ? t.cap : kNoBound);
    t.tile = s.buf<int32_t>((c(t.n_rows) - 1) * c(t.ld) + c(t.n_cols), tile_align);
    t.row_empty = s.buf<uint8_t>(c(t.n_rows), 0, true);
    t.col_empty = s.buf<uint8_t>(c(t.n_cols), 0, true);
    return t;
}
// n_nodes of an export whose tile names nodes: at least the last protein of the tile
int64_t nodes_of(Sim& s, const Tile& t, const char* name = "n_nodes") {
    const bool small = t.row0 < (1 << 20) && t.n_rows < (1 << 20) && t.col0 < (1 << 20) && t.n_cols < (1 << 20);
    const int64_t need = small ? t.last() : 0;
    return s.v(name, need + s.uni(0, 5), need);   // (need is small)
}
#define TILE(t) t.tile, t.n_rows, t.n_cols, t.ld, t.row0, t.col0, t.row_empty, t.col_empty, t.cap, t.bound

// ---- the fingerprint arguments of the pair exports: two row sets with their protein prefix arrays
struct Prots {
    const int8_t *a, *b;
    int64_t lda, ldb, npa, npb;
    const int64_t *idx_a, *idx_b;
    int32_t d;
};
Prots prots_of(Sim& s, int align) {
    Prots p;
    p.npa = s.v("npa", s.uni(1, 40), 0);
    p.npb = s.v("npb", s.uni(1, 40), 0);
    p.d = (int32_t)s.v("d", (int64_t[]){480, 470, 16, 3, 129}[s.uni(0, 4)], 1);
    const int64_t pad = align ? 16 : s.uni(0, 7);
    p.lda = s.v("lda", align ? (p.d + 15) / 16 * 16 + (s.uni(0, 1) ? 0 : pad) : p.d + pad, p.d);
    p.ldb = s.v("ldb", align ? (p.d + 15) / 16 * 16 : p.d + (s.uni(0, 1) ? 0 : pad), p.d);
    const int64_t rows_a = std::min<int64_t>(p.npa, 64) * 3, rows_b = std::min<int64_t>(p.npb, 64) * 3;
    p.a = s.buf<int8_t>(rows_a * c(p.lda), align);
    p.idx_a = s.buf<int64_t>(c(p.npa) + 1);
    p.b = s.buf<int8_t>(rows_b * c(p.ldb), align);
    p.idx_b = s.buf<int64_t>(c(p.npb) + 1);
    return p;
}

// ---- one function per export
int x_pair_min(Sim& s) {
    const int64_t n_pairs = s.v("n_pairs", s.uni(1, 300), 0);
    const int32_t* pairs = s.buf<int32_t>(2 * c(n_pairs));
    const Prots p = prots_of(s, 0);
    int32_t* mn = s.buf<int32_t>(c(n_pairs));
    int32_t* last = s.buf<int32_t>(c(n_pairs));
    return s.run([&] { return dctfp_pair_min(s.ctx, pairs, n_pairs, p.a, p.lda, p.idx_a, p.npa, p.b, p.ldb, p.idx_b, p.npb, p.d, mn, last, g_stream); });
}
int x_pair_argmin(Sim& s) {
    const int64_t n_pairs = s.v("n_pairs", s.uni(1, 300), 0);
    const int32_t* pairs = s.buf<int32_t>(2 * c(n_pairs));
    const Prots p = prots_of(s, 0);
    int32_t *mn = s.buf<int32_t>(c(n_pairs)), *last = s.buf<int32_t>(c(n_pairs)), *aa = s.buf<int32_t>(c(n_pairs)), *ab = s.buf<int32_t>(c(n_pairs));
    return s.run([&] { return dctfp_pair_argmin(s.ctx, pairs, n_pairs, p.a, p.lda, p.idx_a, p.npa, p.b, p.ldb, p.idx_b, p.npb, p.d, mn, last, aa, ab, g_stream); });
}
int x_pair_row_best(Sim& s) {
    const int64_t n_pairs = s.v("n_pairs", s.uni(1, 300), 0);
    const int32_t* pairs = s.buf<int32_t>(2 * c(n_pairs));
    const Prots p = prots_of(s, 0);
    const int64_t* row_off = s.buf<int64_t>(c(n_pairs) + 1);
    const int64_t out_len = s.v("out_len", s.uni(0, 2000), 0);
    int32_t *l1 = s.buf<int32_t>(c(out_len)), *arg = s.buf<int32_t>(c(out_len));
    return s.run([&] { return dctfp_pair_row_best(s.ctx, pairs, n_pairs, p.a, p.lda, p.idx_a, p.npa, p.b, p.ldb, p.idx_b, p.npb, p.d, row_off, out_len, l1, arg, g_stream); });
}
int x_protein_min(Sim& s) {
    const Prots p = prots_of(s, 16);
    const int64_t ldo = s.v("ldo", plus(p.npb, s.uni(0, 3)), p.npb);
    int32_t* out = s.buf<int32_t>((c(p.npa) - 1) * c(ldo) + c(p.npb));
    return s.run([&] { return dctfp_protein_min(s.ctx, p.a, p.lda, p.idx_a, p.npa, p.b, p.ldb, p.idx_b, p.npb, p.d, out, ldo, g_stream); });
}
int x_protein_cover(Sim& s) {
    const Prots p = prots_of(s, 16);
    const int32_t *w_a = s.buf<int32_t>(192), *need_a = s.buf<int32_t>(c(p.npa)), *w_b = s.buf<int32_t>(192),
                  *need_b = s.buf<int32_t>(c(p.npb));
    const int32_t bound = (int32_t)s.v("bound", s.uni(-1, 17000), kNoBound, 0x7ffffffe);
    const int64_t ldo = s.v("ldo", plus(p.npb, s.uni(0, 3)), p.npb);
    int32_t* out = s.buf<int32_t>((c(p.npa) - 1) * c(ldo) + c(p.npb));
    return s.run([&] { return dctfp_protein_cover(s.ctx, p.a, p.lda, p.idx_a, p.npa, w_a, need_a, p.b, p.ldb, p.idx_b, p.npb, w_b, need_b, p.d, bound, out, ldo, g_stream); });
}
struct Dist { const int32_t* dist; int64_t n_rows, n_cols, ld; const uint8_t *re, *ce; int32_t cap; };
Dist dist_of(Sim& s) {
    Dist t;
    t.n_rows = s.v("n_rows", s.uni(1, 60), 0);
    t.n_cols = s.v("n_cols", s.uni(1, 3000), 1);
    t.ld = s.v("ld", plus(t.n_cols, s.uni(0, 2) ? 0 : 5), t.n_cols);
    t.dist = s.buf<int32_t>((c(t.n_rows) - 1) * c(t.ld) + c(t.n_cols));
    t.re = s.buf<uint8_t>(c(t.n_rows), 0, true);
    t.ce = s.buf<uint8_t>(c(t.n_cols), 0, true);
    t.cap = (int32_t)s.v("cap", 17000, 0);
    return t;
}
int x_select_count(Sim& s) {
    const Dist t = dist_of(s);
    const int32_t bound = (int32_t)s.v("bound", s.uni(-1, t.cap), -1, t.cap), top = (int32_t)s.v("top", s.uni(1, 20), 1);
    int32_t *count = s.buf<int32_t>(c(t.n_rows)), *cut = s.buf<int32_t>(2 * c(t.n_rows));
    return s.run([&] { return dctfp_select_count(s.ctx, t.dist, t.n_rows, t.n_cols, t.ld, t.re, t.ce, t.cap, bound, top, count, cut, g_stream); });
}
int x_select_fill(Sim& s) {
    const Dist t = dist_of(s);
    const int32_t* cut = s.buf<int32_t>(2 * c(t.n_rows));
    const int64_t* offsets = s.buf<int64_t>(c(t.n_rows) + 1);
    const int32_t max_count = (int32_t)s.v("max_count", (int64_t[]){0, 1, 2, 128, 129, 256, 257, 1024, 3000}[s.uni(0, 8)], 0);   // (every order kernel)
    int32_t *key = s.buf<int32_t>(100), *col = s.buf<int32_t>(100);
    return s.run([&] { return dctfp_select_fill(s.ctx, t.dist, t.n_rows, t.n_cols, t.ld, t.re, t.ce, t.cap, cut, offsets, max_count, key, col, g_stream); });
}
int x_sim_lines(Sim& s) {
    const int64_t n_rows = s.v("n_rows", s.uni(1, 100), 0), n_cols = s.v("n_cols", s.uni(1, 900), 0);
    const int64_t ld = s.v("ld", plus(n_cols, s.uni(0, 3)), n_cols), row0 = s.v("row0", s.uni(0, 50), 0), col0 = s.v("col0", s.uni(0, 50), 0);
    const int32_t *mn = s.buf<int32_t>((c(n_rows) - 1) * c(ld) + c(n_cols)), *last = s.buf<int32_t>((c(n_rows) - 1) * c(ld) + c(n_cols));
    const uint8_t* ids = s.buf<uint8_t>(64);
    const int64_t* id_off = s.buf<int64_t>(1100);
    const char* table = s.buf<char>(2 * 17002 * 5);
    const int64_t* row_base = s.buf<int64_t>(c(n_rows));
    uint8_t* out = s.buf<uint8_t>(64);
    return s.run([&] { return dctfp_sim_lines(s.ctx, mn, last, ld, n_rows, row0, col0, n_cols, ids, id_off, table, row_base, out, g_stream); });
}
int x_tri_filter_count(Sim& s) {
    const Tile t = tile_of(s);
    int32_t* count = s.buf<int32_t>(c(t.n_rows));
    return s.run([&] { return dctfp_tri_filter_count(s.ctx, TILE(t), count, g_stream); });
}
int x_tri_filter_fill(Sim& s) {
    const Tile t = tile_of(s);
    const int64_t* offsets = s.buf<int64_t>(c(t.n_rows) + 1);
    const int64_t out_len = s.v("out_len", s.uni(1, 500), 0);
    int32_t *oi = s.buf<int32_t>(c(out_len)), *oj = s.buf<int32_t>(c(out_len));
    return s.run([&] { return dctfp_tri_filter_fill(s.ctx, TILE(t), offsets, out_len, oi, oj, g_stream); });
}
struct Lines {
    int64_t n_lines, n_ids, n_labels, out_bytes;
    const int32_t *pi, *pj, *mn, *last, *la, *lb;
    const uint8_t *ids, *labels;
    const int64_t *id_off, *label_off, *line_off;
    const char* table;
    uint8_t* out;
};
Lines lines_of(Sim& s, bool with_labels, bool out_optional) {
    Lines l{};
    l.n_lines = s.v("n_lines", s.uni(1, 400), 0);
    const int64_t n = std::min<int64_t>(l.n_lines, 4096);
    l.pi = s.buf<int32_t>(n), l.pj = s.buf<int32_t>(n), l.mn = s.buf<int32_t>(n), l.last = s.buf<int32_t>(n);
    if (with_labels) l.la = s.buf<int32_t>(n), l.lb = s.buf<int32_t>(n);
    l.n_ids = s.v("n_ids", s.uni(0, 50), 0);
    l.ids = s.buf<uint8_t>(200), l.id_off = s.buf<int64_t>(std::min<int64_t>(l.n_ids, 4096) + 1);
    if (with_labels) {
        l.n_labels = s.v("n_labels", s.uni(0, 90), 0);
        l.labels = s.buf<uint8_t>(300), l.label_off = s.buf<int64_t>(std::min<int64_t>(l.n_labels, 4096) + 1);
    }
    l.table = s.buf<char>(2 * 17002 * 5);
    l.line_off = s.buf<int64_t>(n, 0, out_optional);
    l.out_bytes = s.v("out_bytes", s.uni(0, 5000), 0);
    l.out = s.buf<uint8_t>(c(l.out_bytes), 0, out_optional);
    return l;
}
int x_pair_lines(Sim& s) {
    const Lines l = lines_of(s, false, false);
    return s.run([&] { return dctfp_pair_lines(s.ctx, l.n_lines, l.pi, l.pj, l.mn, l.last, l.ids, l.id_off, l.n_ids, l.table, l.line_off, l.out, l.out_bytes, g_stream); });
}
int x_pair_domain_lines(Sim& s) {
    const Lines l = lines_of(s, true, false);
    return s.run([&] {
        return dctfp_pair_domain_lines(s.ctx, l.n_lines, l.pi, l.pj, l.mn, l.last, l.la, l.lb, l.ids, l.id_off, l.n_ids, l.labels, l.label_off, l.n_labels, l.table,
                                       l.line_off, l.out, l.out_bytes, g_stream);
    });
}
int x_pair_map_lines(Sim& s) {
    const bool count_pass = s.uni(0, 1);   // (the count pass: lengths to out_count, line_off and out may be NULL; else the text, out_count NULL)
    const Lines l = lines_of(s, true, count_pass);
    const int64_t n = std::min<int64_t>(l.n_lines, 4096);
    const int64_t* row_off = s.buf<int64_t>(n + 1);
    const int64_t n_rows = s.v("n_rows", s.uni(0, 900), 0);
    const int32_t *row_l1 = s.buf<int32_t>(c(n_rows)), *row_arg = s.buf<int32_t>(c(n_rows));
    const int64_t* first_row = s.buf<int64_t>(std::min<int64_t>(l.n_ids, 4096) + 1);
    const int32_t bound = (int32_t)s.v("bound", s.uni(-1, 16999), kNoBound, 16999);
    int64_t* out_count = count_pass ? s.buf<int64_t>(n, 0, l.line_off && l.out) : nullptr;   // (required where the text has no place to go)
    return s.run([&] {
        return dctfp_pair_map_lines(s.ctx, l.n_lines, l.pi, l.pj, l.mn, l.last, l.la, l.lb, l.ids, l.id_off, l.n_ids, l.labels, l.label_off, l.n_labels, l.table,
                                    l.line_off, l.out, l.out_bytes, row_off, n_rows, row_l1, row_arg, first_row, bound, out_count, g_stream);
    });
}
int x_tri_link(Sim& s) {
    const Tile t = tile_of(s);
    const int64_t n_nodes = nodes_of(s, t);
    int32_t* parent = s.buf<int32_t>(c(n_nodes));
    return s.run([&] { return dctfp_tri_link(s.ctx, TILE(t), parent, n_nodes, g_stream); });
}
int x_link_pairs(Sim& s) {
    const int64_t n_pairs = s.v("n_pairs", s.uni(1, 3000), 0), n_nodes = s.v("n_nodes", s.uni(1, 500), 0);
    const int32_t *pi = s.buf<int32_t>(c(n_pairs)), *pj = s.buf<int32_t>(c(n_pairs));
    int32_t* parent = s.buf<int32_t>(c(n_nodes));
    return s.run([&] { return dctfp_link_pairs(s.ctx, pi, pj, n_pairs, parent, n_nodes, g_stream); });
}
int x_cluster_labels(Sim& s) {
    const int64_t n_nodes = s.v("n_nodes", s.uni(1, 3000), 0);
    int32_t *parent = s.buf<int32_t>(c(n_nodes)), *labels = s.buf<int32_t>(c(n_nodes));
    return s.run([&] { return dctfp_cluster_labels(s.ctx, parent, n_nodes, labels, g_stream); });
}
struct Rows { const int8_t *a, *b; int64_t na, nb, lda, ldb, a0, b0; int32_t d, cap, bound; };
Rows rows_of(Sim& s, bool with_nodes = true) {   // with_nodes: the rows are nodes from a0 / b0 on, compared at cap and bound
    Rows r{};
    r.na = s.v("na", s.uni(1, 300), 0), r.nb = s.v("nb", s.uni(1, 300), 0);
    r.d = (int32_t)s.v("d", (int64_t[]){480, 470, 16, 3, 129}[s.uni(0, 4)], 1);
    r.lda = s.v("lda", r.d + (int64_t[]){0, 0, 10, 16}[s.uni(0, 3)], r.d), r.ldb = s.v("ldb", r.d + (int64_t[]){0, 0, 6, 16}[s.uni(0, 3)], r.d);
    if (with_nodes) {
        r.a0 = s.v("a0", s.uni(0, 100), 0), r.b0 = s.v("b0", s.uni(0, 100), 0);
        r.cap = (int32_t)s.v("cap", 17000, 0), r.bound = (int32_t)s.v("bound", s.uni(0, 17000), 0);
    }
    r.a = s.buf<int8_t>(std::min<int64_t>(c(r.na), 4096) * c(r.lda)), r.b = s.buf<int8_t>(std::min<int64_t>(c(r.nb), 4096) * c(r.ldb));
    return r;
}
int x_rows_link(Sim& s) {
    const Rows r = rows_of(s);
    const bool small = r.a0 < (1 << 20) && r.na < (1 << 24) && r.b0 < (1 << 20) && r.nb < (1 << 24);
    const int64_t need = small ? std::max(r.a0 + r.na, r.b0 + r.nb) : 0, n_nodes = s.v("n_nodes", need + s.uni(0, 5), need);
    const int32_t* owner = s.buf<int32_t>(std::min<int64_t>(n_nodes, 1 << 20));
    const uint8_t* skip = s.buf<uint8_t>(std::min<int64_t>(n_nodes, 1 << 20), 0, true);
    int32_t* parent = s.buf<int32_t>(std::min<int64_t>(n_nodes, 1 << 20));
    return s.run([&] { return dctfp_rows_link(s.ctx, r.a, r.na, r.lda, r.a0, r.b, r.nb, r.ldb, r.b0, r.d, owner, skip, r.cap, r.bound, parent, n_nodes, g_stream); });
}
int x_rows_assign(Sim& s) {
    const Rows r = rows_of(s);
    const int32_t *value_a = s.buf<int32_t>(std::min<int64_t>(r.na, 4096), 0, true), *slot_b = s.buf<int32_t>(std::min<int64_t>(r.nb, 4096), 0, true);
    const int64_t n_assign = s.v("n_assign", s.uni(1, 500), 0);
    int32_t* assign = s.buf<int32_t>(std::min<int64_t>(n_assign, 4096));
    return s.run([&] { return dctfp_rows_assign(s.ctx, r.a, r.na, r.lda, value_a, r.a0, r.b, r.nb, r.ldb, slot_b, r.b0, r.d, r.cap, r.bound, assign, n_assign, g_stream); });
}
int x_greedy_decide(Sim& s) {
    const int64_t i0 = s.v("i0", s.uni(0, 100), 0), i1 = s.v("i1", plus(i0, s.uni(1, 2000)), i0);
    const int64_t n_nodes = s.v("n_nodes", (i1 < (1 << 30) ? i1 : 0) + s.uni(0, 5), i1 < (1 << 30) ? i1 : 0);
    int32_t *assign = s.buf<int32_t>(std::min<int64_t>(n_nodes, 4096)), *state = s.buf<int32_t>(std::min<int64_t>(n_nodes, 4096));
    const int32_t* blocked = s.buf<int32_t>(std::min<int64_t>(n_nodes, 4096));
    const int32_t round = (int32_t)s.v("round", s.uni(0, 9), 0);
    int64_t* undecided = s.buf<int64_t>(1);
    return s.run([&] { return dctfp_greedy_decide(s.ctx, assign, state, blocked, n_nodes, i0, i1, round, undecided, g_stream); });
}
int x_greedy_tri_mark(Sim& s) {
    const Tile t = tile_of(s);
    const int64_t n_nodes = nodes_of(s, t);
    int32_t* assign = s.buf<int32_t>(std::min<int64_t>(n_nodes, 4096));
    const int32_t* state = s.buf<int32_t>(std::min<int64_t>(n_nodes, 4096));
    int32_t* blocked = s.buf<int32_t>(std::min<int64_t>(n_nodes, 4096));
    const int64_t range_end = s.v("range_end", s.uni(0, std::min<int64_t>(n_nodes, 4096)), 0, n_nodes);
    const int32_t next_round = (int32_t)s.v("next_round", s.uni(1, 9), 1);
    return s.run([&] { return dctfp_greedy_tri_mark(s.ctx, TILE(t), assign, state, blocked, n_nodes, range_end, next_round, g_stream); });
}
int x_greedy_pairs_mark(Sim& s) {
    const int64_t n_pairs = s.v("n_pairs", s.uni(1, 3000), 0), n_nodes = s.v("n_nodes", s.uni(1, 500), 0);
    const int32_t *pi = s.buf<int32_t>(std::min<int64_t>(n_pairs, 4096)), *pj = s.buf<int32_t>(std::min<int64_t>(n_pairs, 4096));
    int32_t* assign = s.buf<int32_t>(std::min<int64_t>(n_nodes, 4096));
    const int32_t* state = s.buf<int32_t>(std::min<int64_t>(n_nodes, 4096));
    int32_t* blocked = s.buf<int32_t>(std::min<int64_t>(n_nodes, 4096));
    const int64_t range_end = s.v("range_end", s.uni(0, std::min<int64_t>(n_nodes, 4096)), 0, n_nodes);
    const int32_t next_round = (int32_t)s.v("next_round", s.uni(1, 9), 1);
    return s.run([&] { return dctfp_greedy_pairs_mark(s.ctx, pi, pj, n_pairs, assign, state, blocked, n_nodes, range_end, next_round, g_stream); });
}
int x_tri_nearest(Sim& s) {
    const Tile t = tile_of(s);
    const int64_t n_nodes = nodes_of(s, t);
    const int32_t* comp = s.buf<int32_t>(std::min<int64_t>(n_nodes, 4096));
    uint64_t* best = s.buf<uint64_t>(std::min<int64_t>(n_nodes, 4096), 8);
    return s.run([&] { return dctfp_tri_nearest(s.ctx, TILE(t), comp, best, n_nodes, g_stream); });
}
int x_tree_hook(Sim& s) {
    const int64_t n_nodes = s.v("n_nodes", s.uni(1, 3000), 0), max_edges = s.v("max_edges", s.uni(0, 3000), 0);
    const int64_t n = std::min<int64_t>(n_nodes, 4096);
    const int32_t* comp = s.buf<int32_t>(n);
    uint64_t* best = s.buf<uint64_t>(n_nodes, 8, false, true);   // (the launcher's memset behind the hooks writes all of it: real memory, whole)
    int32_t* parent = s.buf<int32_t>(n);
    int32_t *ei = s.buf<int32_t>(c(max_edges)), *ej = s.buf<int32_t>(c(max_edges)), *ek = s.buf<int32_t>(c(max_edges)), *counter = s.buf<int32_t>(1);
    return s.run([&] { return dctfp_tree_hook(s.ctx, comp, best, parent, n_nodes, ei, ej, ek, counter, max_edges, g_stream); });
}
int x_rect_best(Sim& s) {
    const Tile t = tile_of(s);
    const bool small = t.row0 < (1 << 20) && t.n_rows < (1 << 20) && t.col0 < (1 << 20) && t.n_cols < (1 << 20);
    const int64_t need_a = small ? t.row0 + t.n_rows : 0, need_b = small ? t.col0 + t.n_cols : 0;
    const int64_t n_a = s.v("n_a", need_a + s.uni(0, 5), need_a);
    uint64_t* best_row = s.buf<uint64_t>(std::min<int64_t>(n_a, 4096), 8);
    const int64_t n_b = s.v("n_b", need_b + s.uni(0, 5), need_b);
    uint64_t* best_col = s.buf<uint64_t>(std::min<int64_t>(n_b, 4096), 8);
    return s.run([&] { return dctfp_rect_best(s.ctx, TILE(t), best_row, n_a, best_col, n_b, g_stream); });
}
int x_label_sums(Sim& s) {
    const Tile t = tile_of(s, false);
    const int64_t n_nodes = nodes_of(s, t);
    const int32_t* labels = s.buf<int32_t>(std::min<int64_t>(n_nodes, 4096), 4);
    uint64_t* sums = s.buf<uint64_t>(std::min<int64_t>(n_nodes, 4096), 8);
    return s.run([&] { return dctfp_label_sums(s.ctx, TILE(t), labels, sums, n_nodes, g_stream); });
}
int x_tri_degree(Sim& s) {
    const Tile t = tile_of(s);
    const int64_t n_nodes = nodes_of(s, t);
    uint32_t* deg = s.buf<uint32_t>(std::min<int64_t>(n_nodes, 4096), 4);
    return s.run([&] { return dctfp_tri_degree(s.ctx, TILE(t), deg, n_nodes, g_stream); });
}
int x_tri_link_core(Sim& s) {
    const Tile t = tile_of(s);
    const int64_t n_nodes = nodes_of(s, t);
    const uint8_t* core = s.buf<uint8_t>(std::min<int64_t>(n_nodes, 4096));
    int32_t *parent = s.buf<int32_t>(std::min<int64_t>(n_nodes, 4096), 4), *nearest = s.buf<int32_t>(std::min<int64_t>(n_nodes, 4096), 4);
    return s.run([&] { return dctfp_tri_link_core(s.ctx, TILE(t), core, parent, nearest, n_nodes, g_stream); });
}
int x_tri_first_fp(Sim& s) {
    const Tile t = tile_of(s);
    const int64_t n_nodes = nodes_of(s, t);
    const int32_t* fam = s.buf<int32_t>(std::min<int64_t>(n_nodes, 4096), 4);
    uint64_t* first = s.buf<uint64_t>(std::min<int64_t>(n_nodes, 4096), 8);
    return s.run([&] { return dctfp_tri_first_fp(s.ctx, TILE(t), fam, first, n_nodes, g_stream); });
}
int x_tri_tp_before(Sim& s) {
    const Tile t = tile_of(s);
    const int64_t n_nodes = nodes_of(s, t);
    const int32_t* fam = s.buf<int32_t>(std::min<int64_t>(n_nodes, 4096), 4);
    const uint64_t* first = s.buf<uint64_t>(std::min<int64_t>(n_nodes, 4096), 8);
    uint32_t* tp = s.buf<uint32_t>(std::min<int64_t>(n_nodes, 4096), 4);
    return s.run([&] { return dctfp_tri_tp_before(s.ctx, TILE(t), fam, first, tp, n_nodes, g_stream); });
}
int x_tri_hist(Sim& s) {
    const Tile t = tile_of(s);
    const int64_t n_nodes = nodes_of(s, t);
    const int32_t* fam = s.buf<int32_t>(std::min<int64_t>(n_nodes, 4096), 4, true);
    uint64_t* hist = s.buf<uint64_t>(2 * (c(t.cap) + 1), 8);
    return s.run([&] { return dctfp_tri_hist(s.ctx, TILE(t), fam, n_nodes, hist, g_stream); });
}
int x_rect_moments(Sim& s) {
    const Tile t = tile_of(s, false);
    const bool small = t.row0 < (1 << 20) && t.n_rows < (1 << 20) && t.col0 < (1 << 20) && t.n_cols < (1 << 20);
    const int64_t need_a = small ? t.row0 + t.n_rows : 0, need_b = small ? t.col0 + t.n_cols : 0;
    // (either side may be NULL, not both; the n of a side that is not computed is not compared with the tile)
    uint64_t* row_mom = s.buf<uint64_t>(3 * (need_a + 5), 8, true);
    uint64_t* col_mom = s.buf<uint64_t>(3 * (need_b + 5), 8, row_mom != nullptr);
    const int64_t n_a = s.v("n_a", need_a + s.uni(0, 5), row_mom ? need_a : 0);
    const int64_t n_b = s.v("n_b", need_b + s.uni(0, 5), col_mom ? need_b : 0);
    return s.run([&] { return dctfp_rect_moments(s.ctx, TILE(t), row_mom, n_a, col_mom, n_b, g_stream); });
}
int x_l1_knn(Sim& s) {
    const int64_t nq = s.v("nq", s.uni(1, 300), 0);
    const int64_t nb = s.v("nb", (int64_t[]){1, 50, 300, 9000, 70000}[s.uni(0, 4)], 0);   // (the last: several slices, merge levels)
    const int32_t d = (int32_t)s.v("d", (int64_t[]){480, 470, 16, 3, 129}[s.uni(0, 4)], 1);
    const int64_t ldq = s.v("ldq", (d + 15) / 16 * 16, d), ldb = s.v("ldb", (d + 15) / 16 * 16 + (s.uni(0, 1) ? 16 : 0), d);
    const int32_t k = (int32_t)s.v("k", (int64_t[]){1, 3, 10, 100, 1024}[s.uni(0, 4)], 1);
    const int64_t col0 = s.v("col0", s.uni(0, 1) ? 0 : s.uni(1, 1 << 20), 0);
    const int8_t *q = s.buf<int8_t>(std::min<int64_t>(c(nq), 4096) * c(ldq), 16), *b = s.buf<int8_t>(std::min<int64_t>(c(nb), 1 << 17) * std::min<int64_t>(c(ldb), 1024), 16);
    const int64_t k_eff = c(std::min<int64_t>(k, nb));
    int32_t *val = s.buf<int32_t>(std::min<int64_t>(c(nq), 4096) * k_eff), *idx = s.buf<int32_t>(std::min<int64_t>(c(nq), 4096) * k_eff);
    return s.run([&] { return dctfp_l1_knn(s.ctx, q, nq, ldq, b, nb, ldb, d, k, col0, val, idx, g_stream); });
}
int x_query_rank(Sim& s) {
    const int64_t n_rows = s.v("n_rows", s.uni(1, 300), 0);
    const int32_t k = (int32_t)s.v("k", s.uni(1, 40), 1), khits = (int32_t)s.v("khits", s.uni(1, 40), 1);
    const int64_t n = std::min<int64_t>(c(n_rows), 4096);
    const int32_t *val = s.buf<int32_t>(n * k), *idx = s.buf<int32_t>(n * k);
    const int64_t* qoff = s.buf<int64_t>(n + 1);
    const int32_t* prot = s.buf<int32_t>(n);
    const int64_t* line_base = s.buf<int64_t>(n);
    int32_t *oq = s.buf<int32_t>(n * khits), *od = s.buf<int32_t>(n * khits), *ox = s.buf<int32_t>(n * khits);
    return s.run([&] { return dctfp_query_rank(s.ctx, val, idx, n_rows, k, qoff, prot, line_base, khits, oq, od, ox, g_stream); });
}
int x_query_lines(Sim& s) {
    const int64_t n_lines = s.v("n_lines", s.uni(1, 3000), 0), n = std::min<int64_t>(c(n_lines), 4096);
    const int32_t *qrow = s.buf<int32_t>(n), *drow = s.buf<int32_t>(n), *dist = s.buf<int32_t>(n), *rank = s.buf<int32_t>(n);
    const uint8_t* q_txt = s.buf<uint8_t>(100);
    const int64_t *q_pid = s.buf<int64_t>(20), *q_dom = s.buf<int64_t>(20);
    const uint8_t* d_txt = s.buf<uint8_t>(100);
    const int64_t *d_pid = s.buf<int64_t>(20), *d_dom = s.buf<int64_t>(20);
    const uint8_t* score_txt = s.buf<uint8_t>(100);
    const int64_t *score_off = s.buf<int64_t>(20), *line_off = s.buf<int64_t>(n);
    uint8_t* out = s.buf<uint8_t>(100);
    return s.run([&] { return dctfp_query_lines(s.ctx, n_lines, qrow, drow, dist, rank, q_txt, q_pid, q_dom, d_txt, d_pid, d_dom, score_txt, score_off, line_off, out, g_stream); });
}
int x_idct_quant(Sim& s) {
    const int32_t dtype = (int32_t)s.v("dtype", s.uni(0, 1), 0, 1);
    const int64_t n_rows = s.v("n_rows", s.uni(1, 400), 1), n_cols = s.v("n_cols", s.uni(1, 700), 1);
    const int64_t ld = s.v("ld", plus(n_cols, s.uni(0, 2) ? 0 : 8), n_cols);
    const int32_t num = (int32_t)s.v("num", s.uni(1, std::min<int64_t>(n_rows, 12)), 1, n_rows);
    const void* vec = s.buf<double>(std::min<int64_t>(c(n_rows), 4096) * c(ld));
    double *scaled = s.buf<double>(c(num) * c(n_cols), 0, true), *coef = s.buf<double>(c(n_cols) * c(num), 0, true);
    return s.run([&] { return dctfp_idct_quant(s.ctx, vec, dtype, n_rows, n_cols, ld, num, scaled, coef, g_stream); });
}
int x_scale(Sim& s) {
    const int64_t n = s.v("n", s.uni(1, 5000), 1);
    const double* vec = s.buf<double>(std::min<int64_t>(n, 8192));
    double* out = s.buf<double>(std::min<int64_t>(n, 8192));
    return s.run([&] { return dctfp_scale(s.ctx, vec, n, out, g_stream); });
}
// (four exports of driver.cpp's section whose limits part (b) states: the rows, columns and pairs of a launch)
int x_row_order(Sim& s) {
    const int64_t n_rows = s.v("n_rows", s.uni(1, 50), 0);
    const int32_t k = (int32_t)s.v("k", (int64_t[]){2, 100, 128, 129, 256, 257, 1024}[s.uni(0, 6)], 1);
    int32_t *val = s.buf<int32_t>(std::min<int64_t>(n_rows, 4096) * k), *idx = s.buf<int32_t>(std::min<int64_t>(n_rows, 4096) * k);
    return s.run([&] { return dctfp_row_order(s.ctx, val, idx, n_rows, k, g_stream); });
}
int x_row_select(Sim& s) {
    const int64_t n_rows = s.v("n_rows", s.uni(1, 20), 0), n_cols = s.v("n_cols", (int64_t[]){1, 50, 40960, 40961, 130000}[s.uni(0, 4)], 1);
    const int64_t ld = s.v("ld", n_cols, n_cols);
    const int32_t k = (int32_t)s.v("k", std::min<int64_t>(n_cols, (int64_t[]){1, 100, 1024, 1025, 5000}[s.uni(0, 4)]), 1, n_cols);
    const int32_t* dist = s.buf<int32_t>(std::min<int64_t>(c(n_rows), 64) * c(ld));
    int32_t *val = s.buf<int32_t>(std::min<int64_t>(n_rows, 4096) * k), *idx = s.buf<int32_t>(std::min<int64_t>(n_rows, 4096) * k);
    return s.run([&] { return dctfp_row_select(s.ctx, dist, n_rows, n_cols, ld, k, val, idx, g_stream); });
}

int x_l1_matrix(Sim& s) {
    const Rows r = rows_of(s, false);
    const int64_t ldo = s.v("ldo", plus(r.nb, s.uni(0, 3)), r.nb);
    int32_t* out = s.buf<int32_t>((std::min<int64_t>(c(r.na), 4096) - 1) * c(ldo) + c(r.nb));
    return s.run([&] { return dctfp_l1_matrix(s.ctx, r.a, r.na, r.lda, r.b, r.nb, r.ldb, r.d, out, ldo, g_stream); });
}
int x_block_min(Sim& s) {
    const int64_t npa = s.v("npa", s.uni(1, 60), 0), npb = s.v("npb", s.uni(1, 60), 0), ldo = s.v("ldo", s.uni(200, 300));
    const int32_t* dist = s.buf<int32_t>(200 * c(ldo));
    const int64_t *idx_a = s.buf<int64_t>(c(npa) + 1), *idx_b = s.buf<int64_t>(c(npb) + 1);
    const int64_t total = c(npa) * std::min<int64_t>(c(npb), 1 << 20);
    int32_t *mn = s.buf<int32_t>(total), *last = s.buf<int32_t>(total);
    return s.run([&] { return dctfp_block_min(s.ctx, dist, ldo, idx_a, npa, idx_b, npb, mn, last, g_stream); });
}

struct Export {
    const char* name;
    int (*fn)(Sim&);
    bool uses_scratch;   // takes the context's generic scratch: also run on a fresh context whose scratch is exactly the bytes asked for
};
const Export kExports[] = {
    {"dctfp_pair_min", x_pair_min, false},
    {"dctfp_pair_argmin", x_pair_argmin, false},
    {"dctfp_pair_row_best", x_pair_row_best, false},
    {"dctfp_protein_min", x_protein_min, true},
    {"dctfp_protein_cover", x_protein_cover, true},
    {"dctfp_select_count", x_select_count, false},
    {"dctfp_select_fill", x_select_fill, false},
    {"dctfp_sim_lines", x_sim_lines, false},
    {"dctfp_tri_filter_count", x_tri_filter_count, false},
    {"dctfp_tri_filter_fill", x_tri_filter_fill, false},
    {"dctfp_pair_lines", x_pair_lines, false},
    {"dctfp_pair_domain_lines", x_pair_domain_lines, false},
    {"dctfp_pair_map_lines", x_pair_map_lines, false},
    {"dctfp_tri_link", x_tri_link, false},
    {"dctfp_link_pairs", x_link_pairs, false},
    {"dctfp_cluster_labels", x_cluster_labels, false},
    {"dctfp_rows_link", x_rows_link, false},
    {"dctfp_rows_assign", x_rows_assign, false},
    {"dctfp_greedy_decide", x_greedy_decide, false},
    {"dctfp_greedy_tri_mark", x_greedy_tri_mark, false},
    {"dctfp_greedy_pairs_mark", x_greedy_pairs_mark, false},
    {"dctfp_tri_nearest", x_tri_nearest, false},
    {"dctfp_tree_hook", x_tree_hook, false},
    {"dctfp_rect_best", x_rect_best, false},
    {"dctfp_label_sums", x_label_sums, false},
    {"dctfp_tri_degree", x_tri_degree, false},
    {"dctfp_tri_link_core", x_tri_link_core, false},
    {"dctfp_tri_first_fp", x_tri_first_fp, false},
    {"dctfp_tri_tp_before", x_tri_tp_before, false},
    {"dctfp_tri_hist", x_tri_hist, false},
    {"dctfp_rect_moments", x_rect_moments, false},
    {"dctfp_l1_knn", x_l1_knn, true},
    {"dctfp_query_rank", x_query_rank, false},
    {"dctfp_query_lines", x_query_lines, false},
    {"dctfp_idct_quant", x_idct_quant, true},
    {"dctfp_scale", x_scale, false},
    {"dctfp_row_order", x_row_order, false},
    {"dctfp_row_select", x_row_select, true},
    {"dctfp_l1_matrix", x_l1_matrix, false},
    {"dctfp_block_min", x_block_min, false},
};
const Export* find_export(const char* name) {
    for (const Export& e : kExports)
        if (!strcmp(e.name, name)) return &e;
    fprintf(stderr, "driver_sim: no export %s\n", name);
    abort();
}

// ---- (b) the limit table: include/dctfp.h's comment of the export and the message in dctfp_sim.hip say the same number
constexpr int64_t kPairsMax = (int64_t)(0xffffffffu / 256) * 4;      // four pairs to a 256-thread workgroup, gridDim.x * blockDim.x < 2^32
constexpr int64_t kLinesMax = (int64_t)(0xffffffffu / 256) * 16;     // sixteen lanes to a line: sixteen lines to a 256-thread workgroup
constexpr int64_t kThreadsMax = (int64_t)(0xffffffffu / 256) * 256;  // one thread to an item, 256-thread workgroups
constexpr int64_t kSelRowsMax = 0xffffffffu / 1024;                  // one 1024-thread workgroup to a row
constexpr int64_t kOrderRowsMax = 0xffffffffu / 512;                 // one workgroup of up to 512 threads to a row
constexpr int64_t kRowsAMax = 65535 * 128, kRowsBMax = (int64_t)(0xffffffffu / 256) * 128;   // 128 x 128 rows to a 256-thread workgroup
struct LimitRow {
    const char* name;
    const char* arg;
    int64_t accepted, refused;
    int code;
    std::map<std::string, int64_t> with;   // the other values the row needs
    bool huge_plan = false;                // the accepted value asks for more scratch than the stub grants: DCTFP_ERR_NOMEM instead of DCTFP_OK
};
const LimitRow kLimits[] = {
    {"dctfp_pair_min", "npa", kI31, kI31 + 1, DCTFP_ERR_LIMIT},
    {"dctfp_pair_min", "npb", kI31, kI31 + 1, DCTFP_ERR_LIMIT},
    {"dctfp_pair_min", "n_pairs", kPairsMax, kPairsMax + 1, DCTFP_ERR_LIMIT},
    {"dctfp_pair_argmin", "npa", kI31, kI31 + 1, DCTFP_ERR_LIMIT},
    {"dctfp_pair_argmin", "npb", kI31, kI31 + 1, DCTFP_ERR_LIMIT},
    {"dctfp_pair_argmin", "n_pairs", kPairsMax, kPairsMax + 1, DCTFP_ERR_LIMIT},
    {"dctfp_pair_row_best", "npa", kI31, kI31 + 1, DCTFP_ERR_LIMIT},
    {"dctfp_pair_row_best", "npb", kI31, kI31 + 1, DCTFP_ERR_LIMIT},
    {"dctfp_pair_row_best", "n_pairs", kPairsMax, kPairsMax + 1, DCTFP_ERR_LIMIT},
    {"dctfp_protein_min", "npa", kI31, kI31 + 1, DCTFP_ERR_LIMIT, {}, true},
    {"dctfp_protein_min", "npb", kI31, kI31 + 1, DCTFP_ERR_LIMIT, {}, true},
    {"dctfp_protein_min", "d", 512, 513, DCTFP_ERR_LIMIT, {{"lda", 528}, {"ldb", 528}}},
    {"dctfp_protein_min", "lda", (1 << 24) - 16, 1 << 24, DCTFP_ERR_LIMIT},
    {"dctfp_protein_cover", "npa", kI31, kI31 + 1, DCTFP_ERR_LIMIT, {}, true},
    {"dctfp_protein_cover", "npb", kI31, kI31 + 1, DCTFP_ERR_LIMIT, {}, true},
    {"dctfp_protein_cover", "d", 512, 513, DCTFP_ERR_LIMIT, {{"lda", 528}, {"ldb", 528}}},
    {"dctfp_protein_cover", "bound", 0x7ffffffe, 0x7fffffff, DCTFP_ERR_INVALID},
    {"dctfp_select_count", "cap", 17407, 17408, DCTFP_ERR_LIMIT},
    {"dctfp_select_count", "n_rows", kSelRowsMax, kSelRowsMax + 1, DCTFP_ERR_LIMIT},
    {"dctfp_select_count", "n_cols", kI31, kI31 + 1, DCTFP_ERR_LIMIT},
    {"dctfp_select_fill", "cap", 17407, 17408, DCTFP_ERR_LIMIT},
    {"dctfp_select_fill", "n_rows", kSelRowsMax, kSelRowsMax + 1, DCTFP_ERR_LIMIT, {{"max_count", 1024}}},
    {"dctfp_select_fill", "n_cols", kI31, kI31 + 1, DCTFP_ERR_LIMIT},
    {"dctfp_sim_lines", "n_cols", kThreadsMax, kThreadsMax + 1, DCTFP_ERR_LIMIT, {{"n_rows", 100000}}},
    {"dctfp_tri_filter_count", "row0", kI31 - 7, kI31 - 6, DCTFP_ERR_LIMIT, {{"n_rows", 7}}},
    {"dctfp_tri_filter_count", "col0", kI31 - 7, kI31 - 6, DCTFP_ERR_LIMIT, {{"n_cols", 7}}},
    {"dctfp_tri_filter_count", "n_rows", kI31, kI31 + 1, DCTFP_ERR_LIMIT, {{"row0", 0}}},
    {"dctfp_tri_filter_fill", "row0", kI31 - 7, kI31 - 6, DCTFP_ERR_LIMIT, {{"n_rows", 7}}},
    {"dctfp_tri_filter_fill", "col0", kI31 - 7, kI31 - 6, DCTFP_ERR_LIMIT, {{"n_cols", 7}}},
    {"dctfp_pair_lines", "n_lines", kLinesMax, kLinesMax + 1, DCTFP_ERR_LIMIT},
    {"dctfp_pair_domain_lines", "n_lines", kLinesMax, kLinesMax + 1, DCTFP_ERR_LIMIT},
    {"dctfp_pair_map_lines", "n_lines", kLinesMax, kLinesMax + 1, DCTFP_ERR_LIMIT},
    {"dctfp_pair_map_lines", "bound", 16999, 17000, DCTFP_ERR_INVALID},
    {"dctfp_tri_link", "n_nodes", kI31, kI31 + 1, DCTFP_ERR_LIMIT},
    {"dctfp_link_pairs", "n_nodes", kI31, kI31 + 1, DCTFP_ERR_LIMIT},
    {"dctfp_link_pairs", "n_pairs", (int64_t)1 << 31, ((int64_t)1 << 31) + 1, DCTFP_ERR_LIMIT},
    {"dctfp_cluster_labels", "n_nodes", kI31, kI31 + 1, DCTFP_ERR_LIMIT},
    {"dctfp_rows_link", "n_nodes", kI31, kI31 + 1, DCTFP_ERR_LIMIT},
    {"dctfp_rows_link", "na", kRowsAMax, kRowsAMax + 1, DCTFP_ERR_LIMIT, {{"a0", 0}, {"n_nodes", kI31}}},
    {"dctfp_rows_link", "nb", kRowsBMax, kRowsBMax + 1, DCTFP_ERR_LIMIT, {{"b0", 0}, {"n_nodes", kI31}}},
    {"dctfp_rows_assign", "n_assign", kI31, kI31 + 1, DCTFP_ERR_LIMIT},
    {"dctfp_rows_assign", "na", kRowsAMax, kRowsAMax + 1, DCTFP_ERR_LIMIT},
    {"dctfp_rows_assign", "nb", kRowsBMax, kRowsBMax + 1, DCTFP_ERR_LIMIT},
    {"dctfp_greedy_decide", "n_nodes", kI31, kI31 + 1, DCTFP_ERR_LIMIT, {{"i0", 0}, {"i1", kI31}}},
    {"dctfp_greedy_tri_mark", "n_nodes", kI31, kI31 + 1, DCTFP_ERR_LIMIT},
    {"dctfp_greedy_pairs_mark", "n_nodes", kI31, kI31 + 1, DCTFP_ERR_LIMIT},
    {"dctfp_greedy_pairs_mark", "n_pairs", (int64_t)1 << 31, ((int64_t)1 << 31) + 1, DCTFP_ERR_LIMIT},
    {"dctfp_tri_nearest", "n_nodes", 1 << 24, (1 << 24) + 1, DCTFP_ERR_LIMIT},
    {"dctfp_tri_nearest", "cap", 32767, 32768, DCTFP_ERR_LIMIT},
    {"dctfp_tree_hook", "n_nodes", 1 << 24, (1 << 24) + 1, DCTFP_ERR_LIMIT},
    {"dctfp_rect_best", "cap", 4194302, 4194303, DCTFP_ERR_INVALID},
    {"dctfp_rect_best", "n_a", kI31, kI31 + 1, DCTFP_ERR_INVALID},
    {"dctfp_rect_best", "n_b", kI31, kI31 + 1, DCTFP_ERR_INVALID},
    {"dctfp_label_sums", "cap", 4194303, 4194304, DCTFP_ERR_INVALID},
    {"dctfp_label_sums", "n_nodes", kI31, kI31 + 1, DCTFP_ERR_INVALID},
    {"dctfp_tri_degree", "n_nodes", kI31, kI31 + 1, DCTFP_ERR_INVALID},
    {"dctfp_tri_link_core", "n_nodes", kI31, kI31 + 1, DCTFP_ERR_INVALID},
    {"dctfp_tri_first_fp", "cap", 4194302, 4194303, DCTFP_ERR_INVALID},
    {"dctfp_tri_first_fp", "n_nodes", kI31, kI31 + 1, DCTFP_ERR_INVALID},
    {"dctfp_tri_tp_before", "n_nodes", kI31, kI31 + 1, DCTFP_ERR_INVALID},
    {"dctfp_tri_hist", "cap", 20479, 20480, DCTFP_ERR_INVALID},
    {"dctfp_tri_hist", "n_nodes", kI31, kI31 + 1, DCTFP_ERR_INVALID},
    {"dctfp_rect_moments", "cap", 1 << 24, (1 << 24) + 1, DCTFP_ERR_INVALID},
    {"dctfp_rect_moments", "n_a", kI31, kI31 + 1, DCTFP_ERR_INVALID},
    {"dctfp_rect_moments", "n_rows", kI31, kI31 + 1, DCTFP_ERR_INVALID, {{"row0", 0}, {"n_a", kI31}, {"n_b", kI31}}},
    {"dctfp_l1_knn", "k", 1024, 1025, DCTFP_ERR_LIMIT},
    {"dctfp_l1_knn", "d", 512, 513, DCTFP_ERR_LIMIT, {{"ldq", 528}, {"ldb", 528}}},
    {"dctfp_l1_knn", "nq", kRowsAMax, kRowsAMax + 1, DCTFP_ERR_LIMIT, {{"k", 1}, {"nb", 300}}},
    {"dctfp_l1_knn", "col0", kI31 - 300, kI31 - 299, DCTFP_ERR_LIMIT, {{"nb", 300}}},
    {"dctfp_l1_knn", "ldq", (1 << 24) - 16, 1 << 24, DCTFP_ERR_LIMIT},
    {"dctfp_query_rank", "n_rows", kThreadsMax, kThreadsMax + 1, DCTFP_ERR_LIMIT, {{"k", 1}}},
    {"dctfp_query_lines", "n_lines", kThreadsMax, kThreadsMax + 1, DCTFP_ERR_LIMIT},
    {"dctfp_idct_quant", "num", 65535, 65536, DCTFP_ERR_LIMIT, {{"n_rows", 70000}, {"n_cols", 100}}},
    {"dctfp_row_order", "k", 1024, 1025, DCTFP_ERR_LIMIT},
    {"dctfp_row_order", "n_rows", kOrderRowsMax, kOrderRowsMax + 1, DCTFP_ERR_LIMIT, {{"k", 2}}},
    {"dctfp_row_order", "n_rows", kOrderRowsMax, kOrderRowsMax + 1, DCTFP_ERR_LIMIT, {{"k", 1024}}},
    {"dctfp_row_select", "n_rows", kSelRowsMax, kSelRowsMax + 1, DCTFP_ERR_LIMIT, {{"n_cols", 50}, {"k", 3}}},
    {"dctfp_row_select", "n_rows", kSelRowsMax, kSelRowsMax + 1, DCTFP_ERR_LIMIT, {{"n_cols", 5000}, {"k", 2000}}},   // (the radix select)
    {"dctfp_row_select", "n_rows", kSelRowsMax, kSelRowsMax + 1, DCTFP_ERR_LIMIT, {{"n_cols", 100000}, {"k", 10}}},   // (segments, or the radix select)
    {"dctfp_row_select", "n_cols", kI31, kI31 + 1, DCTFP_ERR_LIMIT, {{"n_rows", 1}, {"k", 3}}},
    {"dctfp_l1_matrix", "na", kRowsAMax, kRowsAMax + 1, DCTFP_ERR_LIMIT},
    {"dctfp_l1_matrix", "nb", kRowsBMax, kRowsBMax + 1, DCTFP_ERR_LIMIT},
    {"dctfp_block_min", "npa", kThreadsMax, kThreadsMax + 1, DCTFP_ERR_LIMIT, {{"npb", 1}}},
    {"dctfp_block_min", "npb", kThreadsMax / 256, kThreadsMax / 256 + 1, DCTFP_ERR_LIMIT, {{"npa", 256}}},
};

// ---- (c) the probes: a check that adds or multiplies 64-bit arguments, one of them at the end of its type
struct Probe {
    const char* name;
    std::map<std::string, int64_t> with;
};
const Probe kProbes[] = {
    {"dctfp_tri_link", {{"row0", INT64_MAX}, {"n_rows", 5}, {"n_nodes", 100}}},
    {"dctfp_tri_link", {{"col0", INT64_MAX - 1}, {"n_cols", 5}, {"ld", 5}, {"n_nodes", 100}}},
    {"dctfp_greedy_tri_mark", {{"row0", INT64_MAX}, {"n_rows", 5}, {"n_nodes", 100}, {"range_end", 10}}},
    {"dctfp_greedy_tri_mark", {{"col0", INT64_MAX}, {"n_cols", 5}, {"ld", 5}, {"n_nodes", 100}, {"range_end", 10}}},
    {"dctfp_tri_nearest", {{"row0", INT64_MAX}, {"n_rows", 5}, {"n_nodes", 100}}},
    {"dctfp_tri_nearest", {{"col0", INT64_MAX - 1}, {"n_cols", 5}, {"ld", 5}, {"n_nodes", 100}}},
    {"dctfp_rows_link", {{"a0", INT64_MAX}, {"na", 5}, {"n_nodes", 100}}},
    {"dctfp_rows_link", {{"b0", INT64_MAX - 1}, {"nb", 5}, {"n_nodes", 100}}},
    {"dctfp_tri_filter_count", {{"row0", INT64_MAX}, {"n_rows", 5}}},
    {"dctfp_tri_filter_count", {{"col0", INT64_MAX}, {"n_cols", 5}, {"ld", 5}}},
    {"dctfp_tri_filter_fill", {{"row0", INT64_MAX - 1}, {"n_rows", 5}}},
    {"dctfp_tri_filter_fill", {{"col0", INT64_MAX}, {"n_cols", 5}, {"ld", 5}}},
    {"dctfp_rect_best", {{"row0", INT64_MAX}, {"n_rows", 5}, {"n_a", 100}}},
    {"dctfp_rect_best", {{"col0", INT64_MAX}, {"n_cols", 5}, {"ld", 5}, {"n_b", 100}}},
    {"dctfp_rect_moments", {{"row0", INT64_MAX}, {"n_rows", 5}, {"n_a", 100}}},
    {"dctfp_rect_moments", {{"col0", INT64_MAX - 1}, {"n_cols", 5}, {"ld", 5}, {"n_b", 100}}},
    {"dctfp_query_rank", {{"n_rows", INT64_MAX}, {"k", 2}}},
    {"dctfp_query_rank", {{"n_rows", INT64_MAX - 1}, {"k", 1024}}},
    // ... and the workgroup counts, (n + per - 1) / per, of the exports that do not bound n before
    {"dctfp_pair_min", {{"n_pairs", INT64_MAX}}},
    {"dctfp_pair_argmin", {{"n_pairs", INT64_MAX}}},
    {"dctfp_pair_row_best", {{"n_pairs", INT64_MAX - 1}}},
    {"dctfp_sim_lines", {{"n_cols", INT64_MAX}, {"ld", INT64_MAX}}},
    {"dctfp_query_lines", {{"n_lines", INT64_MAX}}},
    {"dctfp_rows_assign", {{"na", INT64_MAX}}},
    {"dctfp_rows_assign", {{"nb", INT64_MAX}}},
    {"dctfp_l1_knn", {{"nq", INT64_MAX}}},
    {"dctfp_l1_knn", {{"col0", INT64_MAX}, {"nb", 300}}},
    {"dctfp_l1_matrix", {{"na", INT64_MAX}}},
    {"dctfp_l1_matrix", {{"nb", INT64_MAX}, {"ldo", INT64_MAX}}},
    {"dctfp_block_min", {{"npa", INT64_MAX}, {"npb", 3}}},
    {"dctfp_block_min", {{"npa", (int64_t)1 << 32}, {"npb", (int64_t)1 << 32}}},
    {"dctfp_row_select", {{"n_cols", INT64_MAX}, {"ld", INT64_MAX}, {"k", 3}, {"n_rows", 4194303}}},
};

const char* g_current = "(nothing)";
void on_death() { fprintf(stderr, "driver_sim: the sanitizer stopped the run inside %s\n", g_current); }

bool is_refusal(int rc) { return rc == DCTFP_ERR_INVALID || rc == DCTFP_ERR_LIMIT || rc == DCTFP_ERR_SHAPE; }

// One call of export e with the state of s; what = the kind of call, for the message.
int invoke(Sim& s, const Export& e, bool inject) {
    s.reset();
    g_current = e.name;
    const int rc = call(e.name, [&] { return e.fn(s); }, inject);
    g_current = "(nothing)";
    return rc;
}

int fail_line(const Export& e, const char* what, int rc) {
    fprintf(stderr, "driver_sim: %s, %s -> %d: %s\n", e.name, what, rc, rc ? dctfp_last_error() : "ok");
    return 1;
}

}  // namespace

int sim_entry_points(int rounds, unsigned long long seed) {
    __sanitizer_set_death_callback(on_death);
    Sim s;
    s.rng.seed(seed);
    if (dctfp_create(0, &s.ctx) != DCTFP_OK) return 1;
    long n_calls = 0, n_refused = 0, n_tight = 0;
    // ---- (a) random valid calls and, from each, the malformed ones
    for (int round = 0; round < rounds; ++round) {
        for (const Export& e : kExports) {
            s.fake = false, s.null_ptr = s.misaligned_ptr = -1, s.over.clear();
            s.fail_after = s.uni(0, 4) == 0 ? s.uni(0, 6) : -1;
            const unsigned long regions = dctfp_stub_counter(5);
            dctfp_ctx* const shared = s.ctx;
            const bool tight = e.uses_scratch && !g_plain && s.uni(0, 1);
            if (tight) {   // a context whose scratch is the bytes this call asks for and no more: the stub refuses the padded request
                if (dctfp_create(0, &s.ctx) != DCTFP_OK) return 1;
                s.fail_after = -1;
                stub_fail_malloc(0);
            }
            const std::mt19937_64 pre = s.rng;   // every malformed call draws what the valid one drew: the same shapes but for one value
            int rc = invoke(s, e, true);
            stub_fail_malloc(-1);
            if (tight) {
                n_tight += rc == DCTFP_OK && dctfp_stub_counter(5) != regions;
                if (dctfp_destroy(s.ctx) != DCTFP_OK) return 1;
                s.ctx = shared;
            }
            ++n_calls;
            s.fail_after = -1;
            if (rc != DCTFP_OK && rc != DCTFP_ERR_NOMEM && !(rc == DCTFP_ERR_HIP && g_launch_failed)) return fail_line(e, "a valid call", rc);
            // the arguments as this call named them (a copy: the next call names them again)
            const std::vector<Sim::Seen> seen = s.seen;
            const int n_ptrs = s.n_ptrs;
            const uint64_t required = s.required, aligned = s.aligned;
            const std::mt19937_64 at = s.rng;
            for (int i = 0; i < n_ptrs; ++i) {
                for (int kind = 0; kind < 2; ++kind) {
                    if (!((kind ? aligned : required) >> i & 1)) continue;
                    if (g_aux() % 3) continue;   // (a third of them per round: every one of them over the rounds)
                    s.rng = pre;
                    s.null_ptr = kind ? -1 : i, s.misaligned_ptr = kind ? i : -1;
                    rc = invoke(s, e, false);
                    s.null_ptr = s.misaligned_ptr = -1;
                    ++n_calls, ++n_refused;
                    if (!is_refusal(rc)) {
                        fprintf(stderr, "driver_sim: %s, pointer argument %d of %d\n", e.name, i, n_ptrs);
                        return fail_line(e, kind ? "a pointer off its alignment" : "a NULL pointer", rc);
                    }
                }
            }
            s.fake = true;   // (a value out of range sizes no buffer)
            for (const Sim::Seen& a : seen) {
                for (int side = 0; side < 2; ++side) {
                    const int64_t edge = side ? a.hi : a.lo;
                    if (edge == kNoBound || (side && edge == INT64_MAX) || g_aux() % 3) continue;
                    s.rng = pre;
                    s.over.clear();
                    s.over[a.name] = side ? edge + 1 : edge - 1;
                    rc = invoke(s, e, false);
                    ++n_calls, ++n_refused;
                    if (!is_refusal(rc)) {
                        fprintf(stderr, "driver_sim: %s with %s = %lld (accepted: %s %lld)\n", e.name, a.name.c_str(), (long long)s.over[a.name], side ? "up to" : "from",
                                (long long)edge);
                        return fail_line(e, "a value outside its range", rc);
                    }
                }
            }
            s.over.clear();
            s.fake = false;
            s.rng = at;
        }
    }
    // ---- (b) the limit table
    int rows_failed = 0;
    s.fake = true, s.fail_after = -1;
    for (const LimitRow& row : kLimits) {
        const Export& e = *find_export(row.name);
        Tally& t = tally_of(row.name);
        ++t.limit_rows;
        s.over = row.with;
        s.over[row.arg] = row.accepted;
        const unsigned long refusals = dctfp_stub_counter(4), launches = dctfp_stub_counter(3);
        int rc = invoke(s, e, false);
        bool ok = rc == (row.huge_plan ? DCTFP_ERR_NOMEM : DCTFP_OK) && dctfp_stub_counter(4) == refusals;
        if (!row.huge_plan && dctfp_stub_counter(3) == launches) ok = false;   // (the largest accepted value launches)
        if (!ok)
            fprintf(stderr, "driver_sim: limit row %s, %s = %lld (the largest accepted) -> %d (%s), %lu launches refused by the stub, %lu taken\n", row.name, row.arg,
                    (long long)row.accepted, rc, rc ? dctfp_last_error() : "ok", dctfp_stub_counter(4) - refusals, dctfp_stub_counter(3) - launches);
        s.over[row.arg] = row.refused;
        const unsigned long before = dctfp_stub_counter(3) + dctfp_stub_counter(4);
        rc = invoke(s, e, false);
        if (rc != row.code || dctfp_stub_counter(3) + dctfp_stub_counter(4) != before) {
            fprintf(stderr, "driver_sim: limit row %s, %s = %lld (the smallest refused) -> %d (%s), expected %d and no launch\n", row.name, row.arg,
                    (long long)row.refused, rc, rc ? dctfp_last_error() : "ok", row.code);
            ok = false;
        }
        n_calls += 2;
        if (ok) ++t.limit_rows_passed;
        else ++rows_failed;
    }
    // ---- (c) the probes
    int probes_failed = 0;
    for (const Probe& p : kProbes) {
        const Export& e = *find_export(p.name);
        s.over = p.with;
        const unsigned long before = dctfp_stub_counter(3) + dctfp_stub_counter(4);
        const int rc = invoke(s, e, false);
        ++n_calls;
        if ((rc != DCTFP_ERR_INVALID && rc != DCTFP_ERR_LIMIT) || dctfp_stub_counter(3) + dctfp_stub_counter(4) != before) {
            std::string with;
            for (const auto& kv : p.with) with += " " + kv.first + "=" + std::to_string(kv.second);
            fprintf(stderr, "driver_sim: overflow probe %s with%s -> %d (%s), expected a refusal and no launch\n", p.name, with.c_str(), rc,
                    rc ? dctfp_last_error() : "ok");
            ++probes_failed;
        }
    }
    s.over.clear();
    s.reset();
    // ---- the exports of driver.cpp's section that it never refuses, and the context calls: one refusal each, a NULL context or argument
    {
        int64_t value = 0;
        dctfp_ctx* none = nullptr;
        const struct { const char* name; int rc; } refused[] = {
            {"dctfp_create", dctfp_create(0, nullptr)},
            {"dctfp_set_option", dctfp_set_option(s.ctx, "no such option", 1)},
            {"dctfp_get_option", dctfp_get_option(s.ctx, "no such option", &value)},
            {"dctfp_quantize", dctfp_quantize(none, nullptr, 0, 0, nullptr, nullptr, 0, 0, nullptr, 0, nullptr)},
            {"dctfp_quantize_windows", dctfp_quantize_windows(none, nullptr, 0, 0, nullptr, nullptr, 0, nullptr, 0, 0, nullptr, 0, nullptr)},
            {"dctfp_quantize_one", dctfp_quantize_one(none, nullptr, 0, 0, nullptr, 0, 0, nullptr, 0, 0, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr)},
            {"dctfp_gather_rows", dctfp_gather_rows(none, nullptr, 0, 0, 0, 0, nullptr, 0, nullptr, nullptr)},
            {"dctfp_contact_topk", dctfp_contact_topk(none, nullptr, nullptr, nullptr, 0, 2.6, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr)},
            {"dctfp_contact_sort", dctfp_contact_sort(none, nullptr, nullptr, nullptr, 0, 2.6, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr)},
            {"dctfp_reccut", dctfp_reccut(none, nullptr, 0, nullptr, nullptr, nullptr, nullptr, 0.08, 0.07, nullptr, nullptr, nullptr)},
            {"dctfp_reccut_pieces", dctfp_reccut_pieces(1, nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr)},
            {"dctfp_build_pieces", dctfp_build_pieces(nullptr, 0, nullptr, nullptr, 1, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr)},
            {"dctfp_stitch", dctfp_stitch(none, nullptr, 1, 4, 0, nullptr)},
            {"dctfp_stitch_sizes", dctfp_stitch_sizes(nullptr, nullptr, 1, 200, 0, nullptr)},
            {"dctfp_stitch_sequences", dctfp_stitch_sequences(none, nullptr, nullptr, nullptr, nullptr, 1, nullptr, nullptr, 4, 200, 0, nullptr)},
            {"dctfp_l1_matrix", dctfp_l1_matrix(none, nullptr, 1, 4, nullptr, 1, 4, 4, nullptr, 1, nullptr)},
            {"dctfp_block_min", dctfp_block_min(none, nullptr, 1, nullptr, 1, nullptr, 1, nullptr, nullptr, nullptr)},
        };
        for (const auto& r : refused) {
            tally(r.name, r.rc, 0);
            ++n_calls;
            if (r.rc != DCTFP_ERR_INVALID) {
                fprintf(stderr, "driver_sim: %s with a NULL context or argument -> %d\n", r.name, r.rc);
                return 1;
            }
        }
        // (the context calls that succeed, on a context of their own; dctfp_destroy(NULL) is one: nothing to do, like free(NULL))
        tally("dctfp_destroy", dctfp_destroy(nullptr), 0);
        dctfp_ctx* extra = nullptr;
        int rc = dctfp_create(0, &extra);
        tally("dctfp_create", rc, 0);
        if (rc != DCTFP_OK) return 1;
        rc = dctfp_get_option(extra, "path", &value);
        tally("dctfp_get_option", rc, 0);
        if (rc == DCTFP_OK) rc = dctfp_set_option(extra, "path", value);
        tally("dctfp_set_option", rc, 0);
        if (rc != DCTFP_OK) return 1;
        rc = dctfp_destroy(extra);
        tally("dctfp_destroy", rc, 0);
        if (rc != DCTFP_OK) return 1;
    }
    if (dctfp_destroy(s.ctx) != DCTFP_OK) return 1;
    const int n_rows = (int)(sizeof kLimits / sizeof kLimits[0]), n_probes = (int)(sizeof kProbes / sizeof kProbes[0]);
    printf("the dct-sim and query_db entry points: %ld calls over %d rounds (%ld malformed, all refused), %ld calls on a scratch of exactly the bytes asked for, "
           "%lu scratch regions touched\n", n_calls, rounds, n_refused, n_tight, dctfp_stub_counter(5));
    printf("limit table: %d of %d rows passed\n", n_rows - rows_failed, n_rows);
    printf("overflow probes: %d of %d refused\n", n_probes - probes_failed, n_probes);
    return rows_failed || probes_failed ? 1 : 0;
}
