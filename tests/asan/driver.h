// What the two sections of the driver share (driver.cpp: dctfp_quantize and the entry points either side of it; driver_sim.cpp: the
// exports of dct-sim and query_db): the caller's streams, the call wrapper with its stream-order and launch-failure checks, the
// allocation-failure hook, and one tally per export for the report at the end.  Nothing here allocates through operator new: the
// hook may be armed while it runs.
#pragma once

#include <cstdio>
#include <cstring>
#include <random>

#include "dctfp.h"

extern "C" unsigned long dctfp_stub_counter(int which);   // 3: launches taken, 4: launches refused for their shape, 5: scratch regions
extern "C" void* stub_new_stream();
extern "C" void stub_call_begin();
extern "C" long stub_call_end(void* stream);
extern "C" unsigned long stub_fail_launch(long n);
extern "C" void stub_fail_malloc(long n);

namespace drv {   // (a namespace: hip_stub.cpp has file-local variables of some of these names, and ASan's ODR indicators go by name)
extern long g_fail_after;        // the N-th operator new from now on throws std::bad_alloc (< 0: never)
extern bool g_plain;             // mode "plain": nothing is injected
extern void* g_streams[3];
extern void* g_stream;
extern unsigned long g_rotation;
extern std::mt19937_64 g_aux;
extern bool g_launch_failed;     // the last call's injected launch failure fired
extern int g_stream_errors;
extern long g_launch_failures;
}  // namespace drv
using namespace drv;

// ---- one line of the report per export
struct Tally {
    const char* name;
    long calls, ok, ok_launching, code[7];   // code[-rc]: calls that ended in that DCTFP_ERR_*
    long limit_rows, limit_rows_passed;
};
Tally& tally_of(const char* name);
inline void tally(const char* name, int rc, unsigned long launches) {
    Tally& t = tally_of(name);
    ++t.calls;
    if (rc == DCTFP_OK) {
        ++t.ok;
        if (launches) ++t.ok_launching;
    } else if (rc < 0 && rc > -7) {
        ++t.code[-rc];
    }
}
void print_tallies();

// ---- stream order and launch failures (hip_stub.cpp).  Every call runs on the caller's stream of the moment -- the null stream
// or one of two others, in turn -- and must leave nothing running on another stream that this one is not ordered after: the
// context's own streams are joined back before a call returns, on its error paths too.  Where `inject` is set, one kernel launch
// of the call fails now and then, and the call must come back as DCTFP_ERR_HIP.  (Decisions from a generator of their own: the
// seeded shapes of the batches stay what they were.)
template <typename F>
static int call(const char* name, F f, bool inject = false) {
    g_stream = g_streams[g_rotation++ % 3];
    const long fail_at = inject && g_aux() % 4 == 0 ? (long)(g_aux() % 8) : -1;
    const unsigned long fired = stub_fail_launch(g_plain ? -1 : fail_at);
    const unsigned long launches = dctfp_stub_counter(3);
    stub_call_begin();
    const int rc = f();
    const long unjoined = stub_call_end(g_stream);
    g_launch_failed = stub_fail_launch(-1) != fired;
    g_launch_failures += g_launch_failed ? 1 : 0;
    tally(name, rc, dctfp_stub_counter(3) - launches);
    if (unjoined) {
        fprintf(stderr, "%s (rc %d): %ld operations left on other streams the caller's stream is not ordered after\n", name, rc, unjoined);
        ++g_stream_errors;
    }
    if (g_launch_failed && rc != DCTFP_ERR_HIP) {
        fprintf(stderr, "%s: an injected launch failure came back as %d\n", name, rc);
        ++g_stream_errors;
    }
    return rc;
}

// driver_sim.cpp: the exports driver.cpp does not call.  Returns non-zero after printing what went wrong.
int sim_entry_points(int rounds, unsigned long long seed);
