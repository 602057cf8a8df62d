// Host driver for the export of include/dctfp_silhouette.h (dctfp_silhouette_rows), a program of its own beside driver.cpp /
// driver_sim.cpp / driver_linkage.cpp: the host objects of every unit of the library, compiled with AddressSanitizer and
// UndefinedBehaviorSanitizer, linked against hip_stub.cpp (device memory = host memory, a launch checks its shape and runs nothing)
// and called here directly -- nothing is loaded into an interpreter.
//   (a) seeded valid calls at small sizes on buffers of exactly the promised size, on three caller streams in turn; no call may
//       leave work on a stream its caller's is not ordered after;
//   (b) the malformed ones: NULL for every pointer that must not be (size and first only with clusters to read), every count below
//       its smallest value, ld < n_cols, rows or columns outside n_nodes, more clusters than n_nodes / 2, pass_clusters 0, every
//       pointer off its alignment;
//   (c) the limits the header states, on pointers that point nowhere: cap = 2^22, pass_clusters = 4096 and n_nodes = 2^31 - 1
//       accepted -- and launched, with a shape the runtime takes --, one more of each refused with DCTFP_ERR_LIMIT and no launch;
//       2^20 + 1 rows are one launch of 2^20 workgroups;
//   (d) INT64_MAX, INT64_MIN and the ends of 32 bits in every integer argument: a refusal and no launch (a huge ld is a stride and is
//       accepted), and no overflow for the sanitizer to report;
//   (e) failures injected: a kernel launch that fails comes back as DCTFP_ERR_HIP; with the allocation hooks armed (operator new
//       and hipMalloc) a call comes back as DCTFP_OK or DCTFP_ERR_NOMEM, never anything else -- the export does not allocate, so it is OK.
// Prints one "export ..." line and "no memory error" at the end; returns non-zero after saying what went wrong.
#include <climits>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <random>

#include "dctfp_silhouette.h"

extern "C" unsigned long dctfp_stub_counter(int which);   // 3: launches taken, 4: launches refused for their shape
extern "C" void* stub_new_stream();
extern "C" void stub_call_begin();
extern "C" long stub_call_end(void* stream);
extern "C" unsigned long stub_fail_launch(long n);
extern "C" void stub_fail_malloc(long n);

// ---- the allocation-failure hook of driver.cpp, restated: the N-th operator new from now on throws std::bad_alloc (once)
namespace {
long g_new_fail_after = -1;
void* hooked_alloc(size_t n, size_t align) {
    if (g_new_fail_after >= 0 && g_new_fail_after-- == 0) throw std::bad_alloc();
    void* p = nullptr;
    if (align > sizeof(void*)) {
        if (posix_memalign(&p, align, n ? n : 1)) p = nullptr;
    } else {
        p = malloc(n ? n : 1);
    }
    if (!p) throw std::bad_alloc();
    return p;
}
}  // namespace
void* operator new(size_t n) { return hooked_alloc(n, 0); }
void* operator new[](size_t n) { return hooked_alloc(n, 0); }
void* operator new(size_t n, std::align_val_t a) { return hooked_alloc(n, (size_t)a); }
void* operator new[](size_t n, std::align_val_t a) { return hooked_alloc(n, (size_t)a); }
void* operator new(size_t n, const std::nothrow_t&) noexcept { try { return hooked_alloc(n, 0); } catch (...) { return nullptr; } }
void* operator new[](size_t n, const std::nothrow_t&) noexcept { try { return hooked_alloc(n, 0); } catch (...) { return nullptr; } }
void* operator new(size_t n, std::align_val_t a, const std::nothrow_t&) noexcept { try { return hooked_alloc(n, (size_t)a); } catch (...) { return nullptr; } }
void* operator new[](size_t n, std::align_val_t a, const std::nothrow_t&) noexcept { try { return hooked_alloc(n, (size_t)a); } catch (...) { return nullptr; } }
void operator delete(void* p) noexcept { free(p); }
void operator delete[](void* p) noexcept { free(p); }
void operator delete(void* p, size_t) noexcept { free(p); }
void operator delete[](void* p, size_t) noexcept { free(p); }
void operator delete(void* p, std::align_val_t) noexcept { free(p); }
void operator delete[](void* p, std::align_val_t) noexcept { free(p); }
void operator delete(void* p, size_t, std::align_val_t) noexcept { free(p); }
void operator delete[](void* p, size_t, std::align_val_t) noexcept { free(p); }

namespace {

struct Tally {
    const char* name;
    long calls = 0, ok = 0, ok_launching = 0, code[7] = {0, 0, 0, 0, 0, 0, 0};
    long limit_rows = 0, limit_rows_passed = 0;
};
Tally g_rows{"dctfp_silhouette_rows"};
int g_errors = 0;
void* g_streams[3];
unsigned long g_rotation = 0;
std::mt19937_64 g_rng;

int64_t uni(int64_t lo, int64_t hi) { return hi <= lo ? lo : lo + (int64_t)(g_rng() % (uint64_t)(hi - lo + 1)); }

constexpr int kPointers = 10;   // tile, row_empty, col_empty, cid, size, first, own_sum, near_sum, near_size, near_first

// The arguments of one call; the arrays are real memory of exactly the promised size unless `fake`.
struct Args {
    int64_t n_rows = 0, n_cols = 0, ld = 0, row0 = 0, col0 = 0, n_clusters = 0, n_nodes = 0;
    int32_t cap = 17000, pass = 4096;
    void* p[kPointers] = {};
    void* owned[kPointers] = {};
    void release() {
        for (void*& q : owned) free(q), q = nullptr;
    }
};

void* exact(size_t bytes, int slot, Args& a) {   // a block of exactly `bytes` (at least one): ASan sees a byte beyond it
    void* q = nullptr;
    if (posix_memalign(&q, 64, bytes ? bytes : 1)) abort();
    memset(q, 0, bytes);
    a.owned[slot] = q;
    return q;
}

Args valid(bool fake = false) {
    Args a;
    a.n_nodes = uni(2, 300);
    a.n_cols = uni(1, a.n_nodes);
    a.col0 = uni(0, a.n_nodes - a.n_cols);
    a.n_rows = uni(1, a.n_nodes);
    a.row0 = uni(0, a.n_nodes - a.n_rows);
    a.ld = a.n_cols + (uni(0, 2) ? 0 : uni(1, 9));
    a.n_clusters = uni(0, a.n_nodes / 2);
    a.cap = (int32_t)uni(0, 17000);
    a.pass = (int32_t)uni(1, 4096);
    if (fake) {
        for (int k = 0; k < kPointers; ++k) a.p[k] = (void*)(uintptr_t)(0x100000 * (k + 1));
        return a;
    }
    const bool flags = uni(0, 1) != 0;
    a.p[0] = exact(((size_t)(a.n_rows - 1) * (size_t)a.ld + (size_t)a.n_cols) * 4, 0, a);
    a.p[1] = flags ? exact((size_t)a.n_rows, 1, a) : nullptr;
    a.p[2] = flags ? exact((size_t)a.n_cols, 2, a) : nullptr;
    a.p[3] = exact((size_t)a.n_nodes * 4, 3, a);
    a.p[4] = a.n_clusters ? exact((size_t)a.n_clusters * 4, 4, a) : nullptr;
    a.p[5] = a.n_clusters ? exact((size_t)a.n_clusters * 4, 5, a) : nullptr;
    a.p[6] = exact((size_t)a.n_nodes * 8, 6, a);
    a.p[7] = exact((size_t)a.n_nodes * 8, 7, a);
    a.p[8] = exact((size_t)a.n_nodes * 4, 8, a);
    a.p[9] = exact((size_t)a.n_nodes * 4, 9, a);
    // clusters (2k, 2k + 1) for k < n_clusters, the rest singletons
    int32_t* cid = (int32_t*)a.p[3];
    for (int64_t i = 0; i < a.n_nodes; ++i) cid[i] = i / 2 < a.n_clusters ? (int32_t)(i / 2) : -1;
    for (int64_t k = 0; k < a.n_clusters; ++k) ((int32_t*)a.p[4])[k] = 2, ((int32_t*)a.p[5])[k] = (int32_t)(2 * k);
    return a;
}

// One call on the caller's stream of the moment, with the stream-order check of driver.h's `call`.
int invoke(dctfp_ctx* ctx, const Args& a, bool ctx_null = false) {
    void* stream = g_streams[g_rotation++ % 3];
    Tally& t = g_rows;
    const unsigned long launches = dctfp_stub_counter(3);
    stub_call_begin();
    const int rc = dctfp_silhouette_rows(ctx_null ? nullptr : ctx, (const int32_t*)a.p[0], a.n_rows, a.n_cols, a.ld, a.row0, a.col0,
                                         (const uint8_t*)a.p[1], (const uint8_t*)a.p[2], a.cap, (const int32_t*)a.p[3], (const int32_t*)a.p[4],
                                         (const int32_t*)a.p[5], a.n_clusters, a.pass, (uint64_t*)a.p[6], (uint64_t*)a.p[7], (int32_t*)a.p[8],
                                         (int32_t*)a.p[9], a.n_nodes, stream);
    const long unjoined = stub_call_end(stream);
    ++t.calls;
    if (rc == DCTFP_OK) {
        ++t.ok;
        if (dctfp_stub_counter(3) != launches) ++t.ok_launching;
    } else if (rc < 0 && rc > -7) {
        ++t.code[-rc];
    }
    if (unjoined) {
        fprintf(stderr, "%s (rc %d): %ld operations left on other streams the caller's stream is not ordered after\n", t.name, rc, unjoined);
        ++g_errors;
    }
    return rc;
}

int expect(const char* what, int rc, int want) {
    if (rc == want) return 0;
    fprintf(stderr, "driver_silhouette: dctfp_silhouette_rows, %s -> %d (%s), expected %d\n", what, rc, rc ? dctfp_last_error() : "ok", want);
    ++g_errors;
    return 1;
}

// A refusal: the code, and not one launch attempted.
void refused(dctfp_ctx* ctx, const Args& a, const char* what, int want = DCTFP_ERR_INVALID, bool ctx_null = false) {
    const unsigned long before = dctfp_stub_counter(3) + dctfp_stub_counter(4);
    expect(what, invoke(ctx, a, ctx_null), want);
    if (dctfp_stub_counter(3) + dctfp_stub_counter(4) != before) {
        fprintf(stderr, "driver_silhouette: %s launched although it was refused\n", what);
        ++g_errors;
    }
}

// The largest accepted value launches, with a shape the runtime takes; the smallest refused one does not.
void limit_row(dctfp_ctx* ctx, const Args& accepted, const Args& refused_args, const char* what, int want = DCTFP_ERR_LIMIT) {
    ++g_rows.limit_rows;
    const int errors = g_errors;
    const unsigned long refusals = dctfp_stub_counter(4), launches = dctfp_stub_counter(3);
    expect(what, invoke(ctx, accepted), DCTFP_OK);
    if (dctfp_stub_counter(4) != refusals || dctfp_stub_counter(3) == launches) {
        fprintf(stderr, "driver_silhouette: %s: the largest accepted value must launch, with a shape the runtime takes\n", what);
        ++g_errors;
    }
    refused(ctx, refused_args, what, want);
    if (g_errors == errors) ++g_rows.limit_rows_passed;
}

void print_tally(const Tally& t) {
    printf("export %s: %ld calls, %ld ok, %ld ok with a launch, refused invalid %ld shape %ld limit %ld unsupported %ld, nomem %ld hip %ld, limit rows %ld of %ld\n",
           t.name, t.calls, t.ok, t.ok_launching, t.code[1], t.code[2], t.code[5], t.code[6], t.code[4], t.code[3], t.limit_rows_passed, t.limit_rows);
}

}  // namespace

int main(int argc, char** argv) {
    const int rounds = argc > 1 ? atoi(argv[1]) : 100;
    g_rng.seed(argc > 2 ? strtoull(argv[2], nullptr, 10) : 1);
    g_streams[0] = nullptr, g_streams[1] = stub_new_stream(), g_streams[2] = stub_new_stream();
    dctfp_ctx* ctx = nullptr;
    if (dctfp_create(0, &ctx) != DCTFP_OK || dctfp_silhouette_version() != DCTFP_SILHOUETTE_VERSION) return 1;
    long injected_hip = 0, starved = 0;
    for (int round = 0; round < rounds; ++round) {
        // (a) a valid call
        Args a = valid();
        expect("a valid call", invoke(ctx, a), DCTFP_OK);
        // (e) the same call with its launch failing, then with the allocation hooks armed
        stub_fail_launch(0);
        const int rc = invoke(ctx, a);
        stub_fail_launch(-1);
        injected_hip += !expect("a call whose launch fails", rc, DCTFP_ERR_HIP);
        g_new_fail_after = uni(0, 3);
        stub_fail_malloc(uni(0, 2));
        const int rs = invoke(ctx, a);
        g_new_fail_after = -1;
        stub_fail_malloc(-1);
        if (rs != DCTFP_OK && rs != DCTFP_ERR_NOMEM) expect("a call with allocations failing", rs, DCTFP_ERR_NOMEM);
        ++starved;
        // (b) the malformed ones, each from the valid call
        refused(ctx, a, "a NULL context", DCTFP_ERR_INVALID, true);
        for (int k = 0; k < kPointers; ++k) {
            if (!a.p[k]) continue;                                  // (the flags may be NULL; size and first are with no cluster)
            Args b = a;
            if (k != 1 && k != 2) {
                b.p[k] = nullptr;
                refused(ctx, b, "a NULL pointer");
            }
            if (k == 1 || k == 2) continue;                         // (bytes: no alignment to be off)
            b = a, b.p[k] = (char*)a.p[k] + (k == 6 || k == 7 ? 4 : 2);
            refused(ctx, b, "a pointer off its alignment");
        }
        Args b = a;
        b.n_rows = -1;
        refused(ctx, b, "n_rows = -1");
        b = a, b.n_cols = -1;
        refused(ctx, b, "n_cols = -1");
        b = a, b.ld = a.n_cols - 1;
        refused(ctx, b, "ld < n_cols");
        b = a, b.row0 = -1;
        refused(ctx, b, "row0 = -1");
        b = a, b.col0 = -1;
        refused(ctx, b, "col0 = -1");
        b = a, b.row0 = a.n_nodes - a.n_rows + 1;
        refused(ctx, b, "rows outside n_nodes");
        b = a, b.col0 = a.n_nodes - a.n_cols + 1;
        refused(ctx, b, "columns outside n_nodes");
        b = a, b.n_nodes = -1;
        refused(ctx, b, "n_nodes = -1");
        b = a, b.cap = -1;
        refused(ctx, b, "cap = -1");
        b = a, b.pass = 0;
        refused(ctx, b, "pass_clusters = 0");
        b = a, b.pass = -1;
        refused(ctx, b, "pass_clusters = -1");
        b = a, b.n_clusters = -1;
        refused(ctx, b, "n_clusters = -1");
        b = a, b.n_clusters = a.n_nodes / 2 + 1;
        refused(ctx, b, "more clusters than n_nodes / 2");
        // nothing to do: no launch, DCTFP_OK
        for (int side = 0; side < 2; ++side) {
            b = a, (side ? b.n_cols : b.n_rows) = 0;
            const unsigned long before = dctfp_stub_counter(3);
            expect("an empty tile", invoke(ctx, b), DCTFP_OK);
            if (dctfp_stub_counter(3) != before) fprintf(stderr, "driver_silhouette: an empty tile launched\n"), ++g_errors;
        }
        a.release();
    }
    // (c) the limits, on pointers that point nowhere
    {
        Args a = valid(true);
        a.cap = DCTFP_SILHOUETTE_MAX_CAP;
        Args r = a;
        r.cap = DCTFP_SILHOUETTE_MAX_CAP + 1;
        limit_row(ctx, a, r, "cap at its limit");
        a = valid(true), a.cap = 0;
        r = a, r.cap = -1;
        limit_row(ctx, a, r, "cap at its lower end", DCTFP_ERR_INVALID);
        a = valid(true), a.pass = DCTFP_SILHOUETTE_MAX_PASS_CLUSTERS;
        r = a, r.pass = DCTFP_SILHOUETTE_MAX_PASS_CLUSTERS + 1;
        limit_row(ctx, a, r, "pass_clusters at its limit");
        a = valid(true), a.pass = 1;
        r = a, r.pass = 0;
        limit_row(ctx, a, r, "pass_clusters at its lower end", DCTFP_ERR_INVALID);
        a = valid(true), a.n_nodes = INT32_MAX, a.n_clusters = INT32_MAX / 2, a.pass = DCTFP_SILHOUETTE_MAX_PASS_CLUSTERS;
        r = a, r.n_nodes = (int64_t)INT32_MAX + 1;
        limit_row(ctx, a, r, "n_nodes at its limit");
        r = a, r.n_clusters = INT32_MAX / 2 + 1;
        limit_row(ctx, a, r, "n_clusters at n_nodes / 2", DCTFP_ERR_INVALID);
        // every protein a row and a column: one launch of 2^20 workgroups, the rows beyond taken gridDim.x apart
        a.n_rows = a.n_cols = a.ld = INT32_MAX, a.row0 = a.col0 = 0;
        r = a, r.row0 = 1;
        limit_row(ctx, a, r, "rows up to the end of n_nodes", DCTFP_ERR_INVALID);
        r = a, r.col0 = 1;
        limit_row(ctx, a, r, "columns up to the end of n_nodes", DCTFP_ERR_INVALID);
        r = a, r.ld = a.n_cols - 1;
        limit_row(ctx, a, r, "ld = n_cols", DCTFP_ERR_INVALID);
    }
    // (d) the ends of the types in every integer argument
    for (int64_t big : {INT64_MAX, INT64_MAX - 1, INT64_MIN, (int64_t)1 << 32, (int64_t)1 << 31}) {
        const Args a = valid(true);
        Args b = a;
        b.n_rows = big;
        refused(ctx, b, "n_rows at the end of its type");
        b = a, b.n_cols = big;
        refused(ctx, b, "n_cols at the end of its type");
        b = a, b.row0 = big;
        refused(ctx, b, "row0 at the end of its type");
        b = a, b.col0 = big;
        refused(ctx, b, "col0 at the end of its type");
        b = a, b.n_clusters = big;
        refused(ctx, b, "n_clusters at the end of its type");
        b = a, b.n_nodes = big;
        refused(ctx, b, "n_nodes at the end of its type", big > 0 ? DCTFP_ERR_LIMIT : DCTFP_ERR_INVALID);
        b = a, b.ld = big;
        if (big < 0) refused(ctx, b, "ld at the end of its type");
        else expect("a huge ld on a small tile", invoke(ctx, b), DCTFP_OK);   // (any ld >= n_cols is a stride: one launch, no product of it on the host)
        b = a, b.n_rows = b.n_cols = b.ld = b.row0 = b.col0 = b.n_clusters = b.n_nodes = big;
        refused(ctx, b, "every count at the end of its type", big > 0 ? DCTFP_ERR_LIMIT : DCTFP_ERR_INVALID);
    }
    for (int32_t big : {INT32_MAX, INT32_MIN}) {
        Args b = valid(true);
        b.cap = big;
        refused(ctx, b, "cap at the end of its type", big > 0 ? DCTFP_ERR_LIMIT : DCTFP_ERR_INVALID);
        b = valid(true), b.pass = big;
        refused(ctx, b, "pass_clusters at the end of its type", big > 0 ? DCTFP_ERR_LIMIT : DCTFP_ERR_INVALID);
    }
    if (dctfp_destroy(ctx) != DCTFP_OK) return 1;
    print_tally(g_rows);
    printf("injected launch failures reported as DCTFP_ERR_HIP: %ld; calls with the allocation hooks armed: %ld\n", injected_hip, starved);
    printf("launches the stub refused for their shape: %lu\n", dctfp_stub_counter(4));
    if (g_errors) {
        fprintf(stderr, "driver_silhouette: %d errors\n", g_errors);
        return 1;
    }
    printf("no memory error\n");
    return 0;
}
