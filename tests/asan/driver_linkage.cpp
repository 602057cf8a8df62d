// Host driver for the exports of include/dctfp_linkage.h (dctfp_linkage_nearest, dctfp_linkage_merge), a program of its own beside
// driver.cpp / driver_sim.cpp: the host objects of every unit of the library, compiled with AddressSanitizer and
// UndefinedBehaviorSanitizer, linked against hip_stub.cpp (device memory = host memory, a launch checks its shape and runs nothing)
// and called here directly -- nothing is loaded into an interpreter.  Per export:
//   (a) seeded valid calls at small sizes on buffers of exactly the promised size, on three caller streams in turn; no call may
//       leave work on a stream its caller's is not ordered after;
//   (b) the malformed ones: NULL for every pointer, every count below its smallest value, ld < n, wide outside 0 .. 1, a live list
//       longer than n, more pairs than n / 2, every pointer off its alignment;
//   (c) the limits the header states, on pointers that point nowhere: n = 46340 and bound = 17000 accepted -- and launched, with a
//       shape the runtime takes --, 46341 and 17001 refused with DCTFP_ERR_LIMIT and no launch;
//   (d) INT64_MAX in every 64-bit argument: a refusal and no launch, and no overflow for the sanitizer to report;
//   (e) failures injected: a kernel launch that fails comes back as DCTFP_ERR_HIP; with the allocation hooks armed (operator new
//       and hipMalloc) a call comes back as DCTFP_OK or DCTFP_ERR_NOMEM, never anything else -- neither export allocates, so it is OK.
// Prints one "export ..." line per export and "no memory error" at the end; returns non-zero after saying what went wrong.
#include <climits>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <random>

#include "dctfp_linkage.h"

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
Tally g_nearest{"dctfp_linkage_nearest"}, g_merge{"dctfp_linkage_merge"};
int g_errors = 0;
void* g_streams[3];
unsigned long g_rotation = 0;
std::mt19937_64 g_rng;

int64_t uni(int64_t lo, int64_t hi) { return hi <= lo ? lo : lo + (int64_t)(g_rng() % (uint64_t)(hi - lo + 1)); }

// The arguments of one call of either export; the arrays are real memory of exactly the promised size unless `fake`.
struct Args {
    int32_t wide = 0, bound = 8500;
    int64_t n = 0, ld = 0, count = 0;          // count: n_live / n_keep
    void* mat = nullptr;
    int32_t *size = nullptr, *list = nullptr, *third = nullptr;   // third: nn (nearest) / partner (merge)
    void* owned[4] = {nullptr, nullptr, nullptr, nullptr};
    void release() {
        for (void*& p : owned) free(p), p = nullptr;
    }
};

void* exact(size_t bytes, int slot, Args& a) {   // a block of exactly `bytes` (at least one): ASan sees a byte beyond it
    void* p = nullptr;
    if (posix_memalign(&p, 64, bytes ? bytes : 1)) abort();
    memset(p, 0, bytes);
    a.owned[slot] = p;
    return p;
}

Args valid(bool merge, bool fake = false) {
    Args a;
    a.wide = (int32_t)uni(0, 1);
    a.n = uni(merge ? 2 : 1, 300);
    a.ld = a.n + (uni(0, 2) ? 0 : uni(1, 9));
    a.count = merge ? uni(1, a.n / 2) : uni(1, a.n);
    a.bound = (int32_t)uni(-1, 17000);
    if (fake) {
        a.mat = (void*)(uintptr_t)0x100000, a.size = (int32_t*)(uintptr_t)0x200000, a.list = (int32_t*)(uintptr_t)0x300000;
        a.third = (int32_t*)(uintptr_t)0x400000;
        return a;
    }
    a.mat = exact(((size_t)(a.n - 1) * (size_t)a.ld + (size_t)a.n) * (a.wide ? 8 : 4), 0, a);
    a.size = (int32_t*)exact((size_t)a.n * 4, 1, a);
    a.list = (int32_t*)exact((size_t)a.count * 4, 2, a);
    a.third = (int32_t*)exact((size_t)a.n * 4, 3, a);
    for (int64_t i = 0; i < a.n; ++i) a.size[i] = 1, a.third[i] = -1;
    for (int64_t k = 0; k < a.count; ++k) {                      // nearest: the first ids live; merge: pairs (2k, 2k + 1)
        a.list[k] = (int32_t)(merge ? 2 * k : k);
        if (merge) a.third[2 * k] = (int32_t)(2 * k + 1), a.third[2 * k + 1] = (int32_t)(2 * k);
    }
    return a;
}

// One call on the caller's stream of the moment, with the stream-order check of driver.h's `call`.
int invoke(bool merge, dctfp_ctx* ctx, const Args& a, bool ctx_null = false) {
    void* stream = g_streams[g_rotation++ % 3];
    Tally& t = merge ? g_merge : g_nearest;
    const unsigned long launches = dctfp_stub_counter(3);
    stub_call_begin();
    const int rc = merge ? dctfp_linkage_merge(ctx_null ? nullptr : ctx, a.mat, a.wide, a.n, a.ld, a.size, a.third, a.list, a.count, stream)
                         : dctfp_linkage_nearest(ctx_null ? nullptr : ctx, a.mat, a.wide, a.n, a.ld, a.size, a.list, a.count, a.bound, a.third, stream);
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

int expect(bool merge, const char* what, int rc, int want) {
    if (rc == want) return 0;
    fprintf(stderr, "driver_linkage: %s, %s -> %d (%s), expected %d\n", merge ? "dctfp_linkage_merge" : "dctfp_linkage_nearest", what, rc,
            rc ? dctfp_last_error() : "ok", want);
    ++g_errors;
    return 1;
}

// A refusal: the code, and not one launch attempted.
void refused(bool merge, dctfp_ctx* ctx, const Args& a, const char* what, int want = DCTFP_ERR_INVALID, bool ctx_null = false) {
    const unsigned long before = dctfp_stub_counter(3) + dctfp_stub_counter(4);
    expect(merge, what, invoke(merge, ctx, a, ctx_null), want);
    if (dctfp_stub_counter(3) + dctfp_stub_counter(4) != before) {
        fprintf(stderr, "driver_linkage: %s launched although it was refused\n", what);
        ++g_errors;
    }
}

void limit_row(bool merge, dctfp_ctx* ctx, Args accepted, Args refused_args, const char* what) {
    Tally& t = merge ? g_merge : g_nearest;
    ++t.limit_rows;
    const int errors = g_errors;
    const unsigned long refusals = dctfp_stub_counter(4), launches = dctfp_stub_counter(3);
    expect(merge, what, invoke(merge, ctx, accepted), DCTFP_OK);
    if (dctfp_stub_counter(4) != refusals || dctfp_stub_counter(3) == launches) {
        fprintf(stderr, "driver_linkage: %s: the largest accepted value must launch, with a shape the runtime takes\n", what);
        ++g_errors;
    }
    refused(merge, ctx, refused_args, what, DCTFP_ERR_LIMIT);
    if (g_errors == errors) ++t.limit_rows_passed;
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
    if (dctfp_create(0, &ctx) != DCTFP_OK || dctfp_linkage_version() != DCTFP_LINKAGE_VERSION) return 1;
    long injected_hip = 0, starved = 0;
    for (int round = 0; round < rounds; ++round) {
        for (int m = 0; m < 2; ++m) {
            const bool merge = m == 1;
            // (a) a valid call
            Args a = valid(merge);
            expect(merge, "a valid call", invoke(merge, ctx, a), DCTFP_OK);
            // (e) the same call with its launch failing, then with the allocation hooks armed
            stub_fail_launch(0);
            const int rc = invoke(merge, ctx, a);
            stub_fail_launch(-1);
            injected_hip += !expect(merge, "a call whose launch fails", rc, DCTFP_ERR_HIP);
            g_new_fail_after = uni(0, 3);
            stub_fail_malloc(uni(0, 2));
            const int rs = invoke(merge, ctx, a);
            g_new_fail_after = -1;
            stub_fail_malloc(-1);
            if (rs != DCTFP_OK && rs != DCTFP_ERR_NOMEM) expect(merge, "a call with allocations failing", rs, DCTFP_ERR_NOMEM);
            ++starved;
            // (b) the malformed ones, each from the valid call
            refused(merge, ctx, a, "a NULL context", DCTFP_ERR_INVALID, true);
            for (int p = 0; p < 4; ++p) {
                Args b = a;
                void** field[4] = {&b.mat, (void**)&b.size, (void**)&b.list, (void**)&b.third};
                *field[p] = nullptr;
                refused(merge, ctx, b, "a NULL pointer");
                b = a;
                *field[p] = (char*)*field[p] + (p == 0 && a.wide ? 4 : 2);
                refused(merge, ctx, b, "a pointer off its alignment");
            }
            Args b = a;
            b.n = -1;
            refused(merge, ctx, b, "n = -1");
            b = a, b.ld = a.n - 1;
            refused(merge, ctx, b, "ld < n");
            b = a, b.count = -1;
            refused(merge, ctx, b, "a negative count");
            b = a, b.count = merge ? a.n / 2 + 1 : a.n + 1;
            refused(merge, ctx, b, merge ? "more pairs than n / 2" : "a live list longer than n");
            b = a, b.wide = 2;
            refused(merge, ctx, b, "wide = 2");
            b = a, b.wide = -1;
            refused(merge, ctx, b, "wide = -1");
            if (!merge) {
                b = a, b.bound = -2;
                refused(merge, ctx, b, "bound = -2");
            }
            // nothing to do: no launch, DCTFP_OK
            b = a, b.count = 0;
            const unsigned long before = dctfp_stub_counter(3);
            expect(merge, "an empty list", invoke(merge, ctx, b), DCTFP_OK);
            if (dctfp_stub_counter(3) != before) fprintf(stderr, "driver_linkage: an empty list launched\n"), ++g_errors;
            a.release();
        }
    }
    // (c) the limits, on pointers that point nowhere
    for (int m = 0; m < 2; ++m) {
        const bool merge = m == 1;
        for (int wide = 0; wide < 2; ++wide) {
            Args a = valid(merge, true);
            a.wide = wide, a.n = a.ld = DCTFP_LINKAGE_MAX_N, a.count = merge ? a.n / 2 : a.n, a.bound = DCTFP_LINKAGE_MAX_BOUND;
            Args r = a;
            r.n = r.ld = DCTFP_LINKAGE_MAX_N + 1;
            limit_row(merge, ctx, a, r, "n at its limit");
            if (!merge) {
                r = a, r.bound = DCTFP_LINKAGE_MAX_BOUND + 1;
                limit_row(merge, ctx, a, r, "bound at its limit");
            }
        }
        // (d) INT64_MAX, INT64_MIN and INT32 ends in every integer argument
        for (int64_t big : {INT64_MAX, INT64_MAX - 1, INT64_MIN, (int64_t)1 << 32, (int64_t)1 << 31}) {
            Args a = valid(merge, true);
            Args b = a;
            b.n = big;
            refused(merge, ctx, b, "n at the end of its type", big > 0 ? DCTFP_ERR_LIMIT : DCTFP_ERR_INVALID);
            b = a, b.ld = big;
            if (big < 0) refused(merge, ctx, b, "ld at the end of its type");
            else expect(merge, "a huge ld on a small matrix", invoke(merge, ctx, b), DCTFP_OK);   // (any ld >= n is a stride: one launch, no product of it on the host)
            b = a, b.count = big;
            refused(merge, ctx, b, "the list's length at the end of its type");
            b = a, b.n = big, b.ld = big, b.count = big;
            refused(merge, ctx, b, "every count at the end of its type", big > 0 ? DCTFP_ERR_LIMIT : DCTFP_ERR_INVALID);
        }
        if (!merge) {
            Args b = valid(merge, true);
            b.bound = INT32_MAX;
            refused(merge, ctx, b, "bound = INT32_MAX", DCTFP_ERR_LIMIT);
            b.bound = INT32_MIN;
            refused(merge, ctx, b, "bound = INT32_MIN");
        }
    }
    if (dctfp_destroy(ctx) != DCTFP_OK) return 1;
    print_tally(g_nearest);
    print_tally(g_merge);
    printf("injected launch failures reported as DCTFP_ERR_HIP: %ld; calls with the allocation hooks armed: %ld\n", injected_hip, starved);
    printf("launches the stub refused for their shape: %lu\n", dctfp_stub_counter(4));
    if (g_errors) {
        fprintf(stderr, "driver_linkage: %d errors\n", g_errors);
        return 1;
    }
    printf("no memory error\n");
    return 0;
}
