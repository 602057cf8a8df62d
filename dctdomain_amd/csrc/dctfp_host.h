// Private header of libdctfp's two host units, dctfp.hip and dctfp_sim.hip: the context, its buffers and streams, and the
// helpers with which an export reports a failure.  dctfp_sim.hip is compiled once and linked into both libraries, so nothing
// here may depend on the switch that tells the two builds of dctfp.hip apart: the context has one layout in every object.
#pragma once

#include <algorithm>
#include <map>
#include <mutex>
#include <unordered_map>
#include <vector>

#include "launch.h"   // (kernels.hip.h, the parameter blocks and the launchers of the kernel families built in their own units)
#include "reccut_kernel.hip.h"   // (CutJob, table sizes; the kernel itself is instantiated in k_reccut.hip)

namespace dctfp_host {

// The calling thread's last message (dctfp_last_error): one buffer for the library, defined with these two in dctfp.hip.
void set_err(const char* msg);
int fail(int code, const char* fmt, ...);

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

#define HIP_TRY(expr)                                                                          \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess) return dctfp_host::fail(DCTFP_ERR_HIP, "%s: %s", #expr, hipGetErrorString(e_)); \
    } while (0)
// ... and a step of the library's own that fails ends its caller with the same code
#define RC_TRY(expr) do { const int rc_ = (expr); if (rc_) return rc_; } while (0)

struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    int ensure(size_t bytes) {
        if (bytes <= cap) return DCTFP_OK;
        if (p) {
            // (growth is rare; kernels of ANOTHER stream may still be reading the old block -- a flush's cutter on its side stream --
            //  and hipFree is only known to wait for the blocking streams)
            (void)hipDeviceSynchronize();
            hipError_t e = hipFree(p);  // device-synchronising: earlier launches are done with it
            p = nullptr;
            cap = 0;
            if (e != hipSuccess) return fail(DCTFP_ERR_HIP, "hipFree: %s", hipGetErrorString(e));
        }
        size_t want = bytes + bytes / 4;
        hipError_t e = hipMalloc(&p, want);
        if (e != hipSuccess) {
            want = bytes;
            e = hipMalloc(&p, want);
        }
        if (e != hipSuccess) {
            p = nullptr;
            return fail(DCTFP_ERR_NOMEM, "hipMalloc(%zu bytes): %s", want, hipGetErrorString(e));
        }
        cap = want;
        return DCTFP_OK;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
};

struct Staging {  // pinned host buffer + the event after its last H2D copy (or after its last reader on the GPU)
    void* p = nullptr;
    void* dev = nullptr;  // the same buffer as the GPU addresses it (nullptr: not mapped, copy instead)
    size_t cap = 0;
    hipEvent_t ev = nullptr;
    bool pending = false;
    int ensure(size_t bytes) {
        if (pending) {
            hipError_t e = hipEventSynchronize(ev);
            pending = false;
            if (e != hipSuccess) return fail(DCTFP_ERR_HIP, "hipEventSynchronize: %s", hipGetErrorString(e));
        }
        if (!ev) {
            hipError_t e = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
            if (e != hipSuccess) return fail(DCTFP_ERR_HIP, "hipEventCreate: %s", hipGetErrorString(e));
        }
        if (bytes <= cap) return DCTFP_OK;
        if (p) {
            (void)hipDeviceSynchronize();   // (a kernel reading the tables straight from this buffer, on whatever stream)
            (void)hipHostFree(p);
        }
        p = nullptr;
        dev = nullptr;
        cap = 0;
        size_t want = bytes + bytes / 2 + 4096;
        hipError_t e = hipHostMalloc(&p, want, hipHostMallocDefault);
        if (e != hipSuccess) {
            p = nullptr;
            return fail(DCTFP_ERR_NOMEM, "hipHostMalloc(%zu): %s", want, hipGetErrorString(e));
        }
        cap = want;
        dev = nullptr;
        if (hipHostGetDevicePointer(&dev, p, 0) != hipSuccess) {
            dev = nullptr;
            (void)hipGetLastError();
        }
        return DCTFP_OK;
    }
    void release() {
        if (pending && ev) (void)hipEventSynchronize(ev);
        if (p) (void)hipHostFree(p);
        if (ev) (void)hipEventDestroy(ev);
        p = nullptr;
        ev = nullptr;
        cap = 0;
    }
};

// A device buffer of the context that calls on different streams take in turn (the job tables, the Y' scratch, the cutter's
// adjacency lists, the generic scratch).  The rule -- wait for the last reader before you overwrite, record after your last
// reader -- is applied by Hold and TableLease only.
struct SharedBuf {
    DevBuf buf;
    hipEvent_t ev_free = nullptr;  // after the last reader of the call that used the buffer last (any stream)
    bool busy = false;
    void release() {
        buf.release();
        if (ev_free) (void)hipEventDestroy(ev_free);
    }
};

// A call's hold on a SharedBuf: take() on the stream that first touches it, give_back() on the caller's stream after the last
// reader.  Taken and not given back, it gives the buffer back when it goes out of scope, on every path out of the call;
// keep() instead: the caller waits for its stream before anything else can touch the context.
struct Hold {
    SharedBuf& b;
    hipStream_t caller;
    bool armed = false;
    int take(size_t bytes, hipStream_t s) {
        armed = true;
        const int rc = b.buf.ensure(bytes);
        if (rc == DCTFP_OK && b.busy) HIP_TRY(hipStreamWaitEvent(s, b.ev_free, 0));
        return rc;
    }
    void* p() const { return b.buf.p; }
    int give_back() {
        armed = false;
        if (!b.ev_free) HIP_TRY(hipEventCreateWithFlags(&b.ev_free, hipEventDisableTiming));
        HIP_TRY(hipEventRecord(b.ev_free, caller));
        b.busy = true;
        return DCTFP_OK;
    }
    void keep() { armed = false; }
    ~Hold() {
        if (armed) (void)give_back();
    }
};

// The job tables of the calls: two buffers (pinned staging + device copy) taken in turn, so that the tables of one call go up
// while the kernels of the one before still read theirs.  Only a TableLease reaches them.
class TableRing {
    struct Slot {
        SharedBuf tab;
        Staging stg;
    } slot_[2];
    int next_ = 0;
    friend class TableLease;

  public:
    void release() { for (Slot& s : slot_) s.tab.release(), s.stg.release(); }
};

// A call's lease on the next buffer of the ring.  The host writes the tables into stage(); upload() sends them up on the
// caller's or the copy stream, behind the last reader of the call that had the buffer two calls ago; or the kernels read them
// through zero_copy().  release() marks the point after the last reader on the caller's stream.  A lease that has uploaded
// or handed out its pinned buffer gives the buffer back there when it goes out of scope unreleased (declare the call's Fork
// after the lease: whatever the context's own streams read is joined into the caller's stream by then).
class TableLease {
    TableRing::Slot& s_;
    Hold tab_;
    hipStream_t up_ = nullptr;
    bool uploaded_ = false, zero_copy_ = false;

  public:
    TableLease(TableRing& r, hipStream_t caller) : s_(r.slot_[r.next_]), tab_{s_.tab, caller} { r.next_ ^= 1; }
    int stage(size_t bytes) { return s_.stg.ensure(bytes); }
    char* host() const { return (char*)s_.stg.p; }
    char* dev() const { return (char*)s_.tab.buf.p; }
    bool mapped() const { return s_.stg.dev != nullptr; }
    char* zero_copy() { return zero_copy_ = true, (char*)s_.stg.dev; }
    int upload(size_t bytes, hipStream_t s, size_t dev_bytes = 0) {  // (into a device buffer of at least dev_bytes)
        const int rc = tab_.take(std::max(bytes, dev_bytes), s);
        if (rc) return rc;
        uploaded_ = true;
        up_ = s;
        HIP_TRY(hipMemcpyAsync(dev(), host(), bytes, hipMemcpyHostToDevice, s));
        HIP_TRY(hipEventRecord(s_.stg.ev, s));
        s_.stg.pending = true;
        return DCTFP_OK;
    }
    int release() {
        const bool zc = zero_copy_;
        uploaded_ = zero_copy_ = false;
        const int rc = tab_.give_back();
        if (rc || !zc) return rc;
        HIP_TRY(hipEventRecord(s_.stg.ev, tab_.caller));  // the kernels read the staging buffer itself: free again after them
        s_.stg.pending = true;
        return DCTFP_OK;
    }
    void keep() { tab_.keep(), uploaded_ = zero_copy_ = false; }
    ~TableLease() {
        if (uploaded_ && up_ != tab_.caller) (void)hipStreamWaitEvent(tab_.caller, s_.stg.ev, 0);
        if (uploaded_ || zero_copy_) (void)release();
    }
};

// One of the context's own streams and the event that joins it back into a caller's.
struct Branch {
    hipStream_t s = nullptr;
    hipEvent_t ev = nullptr;
    int create(int priority = 0) {
        if (!s) HIP_TRY(hipStreamCreateWithPriority(&s, hipStreamNonBlocking, priority));
        if (!ev) HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        return DCTFP_OK;
    }
    void destroy() {
        if (s) (void)hipStreamDestroy(s);
        if (ev) (void)hipEventDestroy(ev);
    }
};

// Work a call sends off the caller's stream onto the context's own streams.  branch() hands out a stream, which waits for the
// fork point the first time the call uses it, if the call has set one (fork(); the copy stream, ahead of the caller's, has
// none).  join() -- or the destructor, on every path out of the call -- makes the caller's stream wait for every branch used.
// Declared after the call's TableLease and Holds, it is destroyed first: what they give back on the caller's stream then comes
// after every reader.
class Fork {
    hipStream_t caller_;
    hipEvent_t fork_ = nullptr;
    const Branch* used_[kCutClasses] = {};
    int n_used_ = 0;

  public:
    explicit Fork(hipStream_t caller) : caller_(caller) {}
    int fork(hipEvent_t ev) {
        fork_ = ev;
        HIP_TRY(hipEventRecord(ev, caller_));
        return DCTFP_OK;
    }
    int branch(const Branch& b, hipStream_t* s) {
        *s = b.s;
        if (std::find(used_, used_ + n_used_, &b) != used_ + n_used_) return DCTFP_OK;
        used_[n_used_++] = &b;
        if (fork_) HIP_TRY(hipStreamWaitEvent(b.s, fork_, 0));
        return DCTFP_OK;
    }
    int join() {
        for (; n_used_ > 0; --n_used_) {
            HIP_TRY(hipEventRecord(used_[n_used_ - 1]->ev, used_[n_used_ - 1]->s));
            HIP_TRY(hipStreamWaitEvent(caller_, used_[n_used_ - 1]->ev, 0));
        }
        return DCTFP_OK;
    }
    ~Fork() { (void)join(); }
};

struct StEntry {  // stage-B basis  St[d][c] (ldy x cp), zero padded
    double* dev = nullptr;
    double* frag = nullptr;  // even/odd halves of the basis in MFMA-fragment order (walk_ab_kernel), `frag_groups` 16-pair groups
    int frag_groups = 0;
    double* fragp = nullptr; // the plain basis in MFMA-fragment order (walk_gen_kernel), made when that kernel first wants it
    int ldy = 0, cp = 0;
    uint64_t last_use = 0;
};

struct BasisSlab {  // a piece of the context's cosine-table arena
    double* dev = nullptr;
    size_t cap = 0, used = 0;  // doubles
};

struct EventPair {
    hipEvent_t a = nullptr, b = nullptr;
    int which = 0;
};

constexpr int kMaxSlots = 8;
constexpr size_t kCounterBytes = 24 * sizeof(unsigned long long);  // [0] degenerate channels; [1..11] phase times of an instrumented build; [15] device address of the host flag; [16], [17] trace of an instrumented build

struct Context {   // (what a dctfp_ctx is: below)
    int device = 0;
    int64_t opt_overlap = 4;
    Branch side;                                // stage B of the two-kernel path
    Branch copy;                                // table upload + cosine tables, ahead of the caller's stream
    hipEvent_t ev_basis = nullptr;              // after the last basis_kernel (cosine tables are shared by all later calls)
    hipStream_t basis_stream = nullptr;
    bool basis_valid = false;
    std::mutex mu;                              // one host thread at a time inside a context
    int ensure_copy() {
        if (copy.s) return DCTFP_OK;
        int rc = copy.create();
        if (rc) return rc;
        HIP_TRY(hipEventCreateWithFlags(&ev_basis, hipEventDisableTiming));
        return DCTFP_OK;
    }
    hipEvent_t ev_a[kMaxSlots] = {}, ev_b[kMaxSlots] = {};
    int ensure_side() {
        if (side.s) return DCTFP_OK;
        int rc = side.create();
        if (rc) return rc;
        for (int i = 0; i < kMaxSlots; ++i) {
            if (hipEventCreateWithFlags(&ev_a[i], hipEventDisableTiming) != hipSuccess ||
                hipEventCreateWithFlags(&ev_b[i], hipEventDisableTiming) != hipSuccess) {
                set_err("hipEventCreate failed");
                return DCTFP_ERR_HIP;
            }
        }
        return DCTFP_OK;
    }
    int64_t opt_a_waves = 0, opt_profile = 0, opt_ws_mb = 4096;
    TableRing ring;
    SharedBuf ws;       // yprime
    int64_t opt_fuse = 1, opt_pack_y = 1;
    SharedBuf scratch;  // dctfp_idct_quant's coefficients, dctfp_row_select's candidates
    DevBuf split_ws; // partial sums of the row-split stage A (small calls)
    // stage-A cosine tables, one per (domain length, n - 1): filled once, kept for the life of the context
    std::vector<BasisSlab> basis_slabs;
    std::unordered_map<uint64_t, double*> basis_tabs;
    size_t basis_doubles = 0;
    unsigned long long* degenerate = nullptr;  // device counter: exactly constant channels seen (see dctfp.h)
    uint32_t* flag_host = nullptr;             // pinned + mapped word the kernels set when they see one (option degenerate_seen)
    int n_cu = 256;  // compute units of the device (workgroup slots of the walk kernel = n_cu x workgroups per CU)
    void *trace_dev = nullptr, *trace_host = nullptr;  // instrumented build only (walk_trace)
    int64_t trace_waves = 0;
    SharedBuf cut_ws;   // dctfp_reccut: adjacency lists and node stacks of a batch
    Branch cut[kCutClasses - 1];    // ... its larger size classes run beside the small one (and dctfp_contact_topk's long chain)
    hipEvent_t cut_fork = nullptr;
    int ensure_cut_streams() {
        if (cut[kCutClasses - 2].s) return DCTFP_OK;
        // (the highest priority the device offers: what runs on them -- the long proteins' workgroups, the striped selection -- is
        //  what a flush waits for, and its workgroups should take the CUs the short proteins' ones leave)
        int prio_low = 0, prio_high = 0;
        if (hipDeviceGetStreamPriorityRange(&prio_low, &prio_high) != hipSuccess) {
            (void)hipGetLastError();
            prio_high = 0;
        }
        if (!cut_fork) HIP_TRY(hipEventCreateWithFlags(&cut_fork, hipEventDisableTiming));
        for (Branch& b : cut) {
            const int rc = b.create(prio_high);
            if (rc) return rc;
        }
        return DCTFP_OK;
    }
    int64_t opt_path = 0, opt_ab_run_jobs = 0, opt_small_b_jobs = 512, opt_ab_longest_first = 0, opt_ab_taper = 4, opt_ab_align = 2, opt_l1_kernel = 0, opt_row_select = 0, opt_stitch_once = 0, opt_topk_kernel = 0;
    int64_t last_path = 0;  // which kernels the last dctfp_quantize launched: 1 = stage A + stage B, 2 = walk kernel
    int64_t last_gen_fused = 0;  // ... and whether that was the general walk kernel streaming fused walks (parts + whole protein)
    int64_t last_walk_groups = 0;  // ... or walk_ab_kernel: its build's 16-column groups (5: m <= 80, 6: 80 < m <= 96), 0 = another kernel
    // ... or the two kernels: the builds of the last chunk's stage A and stage B as their launchers named them (launch.h:
    // stage_a_word and the stage-B words), 0 = another route
    int64_t last_stage_a = 0, last_stage_b = 0;
    // ... and the one-launch kernels by name: the build their launcher instantiated (launch.h: walk_word / gen_word), 0 = another route
    int64_t last_walk = 0, last_gen = 0;
    int64_t opt_gen_fuse = 1;    // "gen_fuse": fused walks through the general walk kernel (n <= 5); 0 = the two kernels, as through round 4
    int64_t walk_launches = 0;  // walk-kernel launches so far (a call split at a giant domain ends on the two-kernel path)
    int64_t last_knn_slices = 0;  // database slices that owned a column in the last dctfp_l1_knn launch
    int64_t knn_calls = 0;        // dctfp_l1_knn launches so far
    int64_t test_fail_once = 0;                    // test hook: the next dctfp_quantize fails after its table lookups
    int64_t basis_cap_doubles = (int64_t)1 << 27;  // 1 GiB of cosine tables, then the arena starts over (test hook: basis_cap_kb)
    int64_t basis_restarts = 0;                    // how often it did
    std::map<std::pair<int, int>, StEntry> st_cache;
    uint64_t tick = 0;
    std::vector<EventPair> events;
    size_t events_used = 0;
    double prof_ms[2] = {0, 0};
    int64_t prof_n[2] = {0, 0};
};

}  // namespace dctfp_host

struct dctfp_ctx : dctfp_host::Context {};   // the opaque type of include/dctfp.h

namespace dctfp_host {

// a launcher's failure -> this thread's error message
inline int launcher_rc(int rc, const LaunchError& err) {
    return rc ? fail(err.code ? err.code : rc, "%s", err.msg) : DCTFP_OK;
}

// Nothing may throw across the C ABI: an exception that leaves an extern "C" function ends the process in std::terminate
// (SIGABRT on the calling thread).  Every entry point is a function-try-block that ends here; the vectors of the table
// build are the only things that can throw (std::bad_alloc, std::length_error).
int guard_exception(const char* where) noexcept;
#define DCTFP_GUARD(name) catch (...) { return dctfp_host::guard_exception(name); }

}  // namespace dctfp_host
