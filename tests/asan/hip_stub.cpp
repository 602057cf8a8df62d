// Host-only stand-in for the HIP runtime, for AddressSanitizer runs of libdctfp's host code on a machine WITHOUT a GPU
// (tests/test_host_asan.py; GPU ASan is not available on the pool).  "Device" memory is host memory, so every table the
// host builds, every copy it sizes and every pointer it hands to a kernel is checked by ASan; kernels are not executed --
// instead `hipLaunchKernel` walks the job tables of the main kernels the way their waves do and touches every address they
// would (first / last byte of every row range, cosine table, output block): an index that is wrong on the host side
// shows up here as a heap-buffer-overflow instead of as a GPU fault on the box.
// With DCTFP_STUB_LAUNCH_LOG=<file> in the environment every launch is also written down, one line each: kernel, grid, block,
// dynamic LDS bytes, ordinal of the stream, the scalar arguments decoded below and -- for the kernels whose tables are walked --
// a 64-bit hash over the JobA / PieceA / JobB / Walk / Run records the launch reaches (pointers as null / non-null only).  Two
// builds of the host code that plan the same launches write the same file (driver.cpp, mode "plain").
// Test infrastructure only: never linked into the product.
#include <hip/hip_runtime_api.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>

// The job-table records of dctdomain_amd/csrc/kernels.hip.h, restated (that header is device code: a second translation
// unit including it would define its kernels twice).  tests/test_host_asan.py checks that the two stay in step.
struct JobA {
    uint32_t piece_begin, n_pieces, n_rows, reserved;
    const double* basis;
    const double* w_basis;
    const void* w_ref;
};
struct PieceA {
    const void* ptr;
    uint32_t n_rows, t0, w0, reserved;
    const void* ptr2;
};
struct JobB {
    int64_t out_off;
};
struct Walk {
    uint32_t job_begin, n_parts;
    int32_t whole_job;
    uint32_t reserved;
};
struct Run {
    uint32_t walk_begin, n_walks, job_begin, n_jobs;
};
struct BasisJob {
    double* tab;
    uint32_t len, reserved;
};
static_assert(sizeof(JobA) == 40 && sizeof(PieceA) == 32 && sizeof(JobB) == 8 && sizeof(Walk) == 16 && sizeof(Run) == 16 && sizeof(BasisJob) == 16,
              "job-table records as in kernels.hip.h");

namespace {
std::map<const void*, std::string>& names() {
    static std::map<const void*, std::string> m;
    return m;
}
volatile unsigned char g_sink;
inline void touch(const void* p, size_t bytes) {  // ASan checks both ends of [p, p + bytes)
    if (!bytes) return;
    const volatile unsigned char* c = (const volatile unsigned char*)p;
    g_sink ^= c[0];
    g_sink ^= c[bytes - 1];
}
inline void touch_w(void* p, size_t bytes) {
    if (!bytes) return;
    volatile unsigned char* c = (volatile unsigned char*)p;
    c[0] = c[0];
    c[bytes - 1] = c[bytes - 1];
}
size_t elem_size(const std::string& n, const char* kernel) {
    const size_t at = n.find(kernel);
    const std::string t = n.substr(at + strlen(kernel), 12);
    if (t.rfind("If", 0) == 0) return 4;
    if (t.rfind("Id", 0) == 0) return 8;
    return 2;  // _Float16 / bf16_t
}
int template_int(const std::string& n, const char* kernel, int index) {  // the index-th "Li<k>E" after the kernel name
    size_t at = n.find(kernel);
    for (int i = 0; i <= index; ++i) {
        at = n.find("Li", at + 1);
        if (at == std::string::npos) return -1;
    }
    return atoi(n.c_str() + at + 2);
}
unsigned long g_walk_launches = 0, g_stage_a_launches = 0, g_jobs_walked = 0;
unsigned long g_launches_taken = 0, g_launch_refusals = 0, g_scratch_regions = 0;   // launches that passed the checks of hipLaunchKernel / that it refused; regions the scratch emulators touched

// ---- the launch log (off unless asked for).  Fixed buffers: nothing here may go through operator new (driver.cpp hooks it).
FILE* g_log = nullptr;
uint64_t g_hash = 0;
bool g_hashed = false;
char g_scalars[256];
size_t g_scalars_len = 0;
inline void mix(uint64_t v) {  // FNV-1a over the eight bytes of v
    g_hashed = true;
    for (int i = 0; i < 8; ++i) g_hash = (g_hash ^ ((v >> (8 * i)) & 0xff)) * 0x100000001b3ull;
}
inline void mix(const JobA& j) { mix(j.piece_begin); mix(j.n_pieces); mix(j.n_rows); mix(j.reserved); mix(j.basis != nullptr); mix(j.w_basis != nullptr); mix(j.w_ref != nullptr); }
inline void mix(const PieceA& p) { mix(p.ptr != nullptr); mix(p.n_rows); mix(p.t0); mix(p.w0); mix(p.reserved); mix(p.ptr2 != nullptr); }
inline void mix(const JobB& j) { mix((uint64_t)j.out_off); }
inline void mix(const Walk& w) { mix(w.job_begin); mix(w.n_parts); mix((uint64_t)(int64_t)w.whole_job); mix(w.reserved); }
inline void mix(const Run& r) { mix(r.walk_begin); mix(r.n_walks); mix(r.job_begin); mix(r.n_jobs); }
void scalar(const char* name, long long v) {
    if (g_log && g_scalars_len < sizeof g_scalars) g_scalars_len += (size_t)snprintf(g_scalars + g_scalars_len, sizeof g_scalars - g_scalars_len, " %s=%lld", name, v);
}

void emulate_walk(const std::string& name, dim3 grid, void** a) {
    const JobA* jobs = *(const JobA**)a[0];
    const JobB* jobb = *(const JobB**)a[1];
    const Walk* walks = *(const Walk**)a[2];
    const Run* runs = *(const Run**)a[3];
    const PieceA* pieces = *(const PieceA**)a[4];
    const double* stf = *(const double**)a[5];
    int8_t* out = *(int8_t**)a[6];
    const int n_cols = *(int*)a[7];
    const int64_t ld = *(int64_t*)a[8];
    const int m = *(int*)a[9];
    const size_t esz = elem_size(name, "walk_ab_kernel");
    const int S = template_int(name, "walk_ab_kernel", 0), G = template_int(name, "walk_ab_kernel", 1);
    if (S * 256 < n_cols) { fprintf(stderr, "stub: %d waves cannot cover %d channels\n", S, n_cols); abort(); }
    const int groups = (n_cols / 2 + 15) / 16;
    const int nt_w = template_int(name, "walk_ab_kernel", 2);   // five or six column groups ([E | O] halves of 40 / 48 slots)
    if ((nt_w != 5 && nt_w != 6) || m > nt_w * 16 || (nt_w == 6 && m <= 80)) { fprintf(stderr, "stub: walk_ab_kernel build of %d column groups for m = %d\n", nt_w, m); abort(); }
    touch(stf, (size_t)(groups * 4 + 4) * nt_w * 64 * sizeof(double));  // fragments up to 4 k-steps past the last group
    ++g_walk_launches;
    scalar("n_cols", n_cols), scalar("ld", ld), scalar("m", m);
    for (unsigned b = 0; b < grid.x; ++b) {
        const Run run = runs[b];
        mix(run);
        uint32_t pending = 0, group_job = run.job_begin, jobs_seen = 0;
        for (uint32_t wi = 0; wi < run.n_walks; ++wi) {
            const Walk wk = walks[run.walk_begin + wi];
            mix(wk);
            const bool has_w = wk.whole_job >= 0;
            const uint32_t w_rows = has_w ? jobs[wk.whole_job].n_rows : 0;
            const uint32_t n_walk_jobs = wk.n_parts + (has_w ? 1u : 0u);
            for (uint32_t part = 0; part < n_walk_jobs; ++part) {
                const uint32_t job_id = part < wk.n_parts ? wk.job_begin + part : (uint32_t)wk.whole_job;
                if (job_id != group_job + pending) {  // slot g of a flush <-> job group_job + g (walk_ab_kernel, epilogue)
                    fprintf(stderr, "stub: run %u walk %u part %u is job %u, the flush expects %u\n", b, wi, part, job_id, group_job + pending);
                    abort();
                }
                if (part < wk.n_parts) {
                    const JobA job = jobs[job_id];
                    mix(job);
                    uint32_t rows = 0;
                    for (uint32_t p = 0; p < job.n_pieces; ++p) {
                        const PieceA pc = pieces[job.piece_begin + p];
                        mix(pc);
                        if (pc.n_rows == 0 || pc.t0 != rows) { fprintf(stderr, "stub: piece table of job %u broken\n", job_id); abort(); }
                        touch(pc.ptr, (size_t)n_cols * esz);
                        touch((const char*)pc.ptr + (size_t)(pc.n_rows - 1) * (size_t)ld * esz, (size_t)n_cols * esz);
                        if (pc.ptr2) {  // the mean of two windows' rows: only the builds with the last template flag set read it
                            if (name.find("Lb1EEEvPK") == std::string::npos || esz != 4) { fprintf(stderr, "stub: two-source piece sent to %s\n", name.c_str()); abort(); }
                            touch(pc.ptr2, (size_t)n_cols * esz);
                            touch((const char*)pc.ptr2 + (size_t)(pc.n_rows - 1) * (size_t)ld * esz, (size_t)n_cols * esz);
                        }
                        touch(job.basis + (size_t)pc.t0 * 2, (size_t)pc.n_rows * 2 * sizeof(double));
                        // the compiler merges the cosines of up to four rows into one scalar load: 8 doubles from any row
                        touch(job.basis + (size_t)(pc.t0 + pc.n_rows - 1) * 2, 8 * sizeof(double));
                        if (has_w) {
                            touch(job.w_basis + (size_t)pc.w0 * 2, (size_t)pc.n_rows * 2 * sizeof(double));
                            touch(job.w_basis + (size_t)(pc.w0 + pc.n_rows - 1) * 2, 8 * sizeof(double));
                            touch(job.w_basis + ((size_t)w_rows + pc.w0) * 2, ((size_t)pc.n_rows + 1) * 2 * sizeof(double));  // prefix sums
                        }
                        rows += pc.n_rows;
                    }
                    if (rows != job.n_rows || rows < 3) { fprintf(stderr, "stub: job %u has %u rows, its pieces %u\n", job_id, job.n_rows, rows); abort(); }
                    if (has_w) touch(job.w_ref, (size_t)n_cols * esz);
                }
                ++pending;
                ++jobs_seen;
                ++g_jobs_walked;
                const bool last = wi + 1 == run.n_walks && part + 1 == n_walk_jobs;
                if (pending < (uint32_t)G && !last) continue;
                for (uint32_t g = 0; g < pending; ++g) {
                    mix(jobb[group_job + g]);
                    touch_w(out + jobb[group_job + g].out_off, (size_t)3 * m);
                }
                group_job += pending;
                pending = 0;
            }
        }
        if (jobs_seen != run.n_jobs) { fprintf(stderr, "stub: run %u walks %u jobs, says %u\n", b, jobs_seen, run.n_jobs); abort(); }
    }
}

void emulate_stage_a(const std::string& name, dim3 grid, void** a) {
    const JobA* jobs = *(const JobA**)a[0];
    const Walk* walks = *(const Walk**)a[1];
    const PieceA* pieces = *(const PieceA**)a[2];
    char* yprime = *(char**)a[3];
    const int64_t job_bytes = *(int64_t*)a[4];
    const int n_cols = *(int*)a[6];
    const int64_t ld = *(int64_t*)a[7];
    const int n_slabs = *(int*)a[9];
    const size_t esz = elem_size(name, "stage_a_kernel");
    const int nk = template_int(name, "stage_a_kernel", 0) - 1;
    ++g_stage_a_launches;
    scalar("job_bytes", job_bytes), scalar("n_cols", n_cols), scalar("ld", ld), scalar("n_slabs", n_slabs);
    for (unsigned w = 0; w < grid.x / (unsigned)n_slabs; ++w) {
        const Walk wk = walks[w];
        mix(wk);
        const bool has_w = wk.whole_job >= 0;
        for (uint32_t part = 0; part < wk.n_parts; ++part) {
            const JobA job = jobs[wk.job_begin + part];
            mix(job);
            for (uint32_t p = 0; p < job.n_pieces; ++p) {
                const PieceA pc = pieces[job.piece_begin + p];
                mix(pc);
                if (pc.ptr2) { fprintf(stderr, "stub: two-source piece sent to %s\n", name.c_str()); abort(); }
                touch(pc.ptr, (size_t)n_cols * esz);
                touch((const char*)pc.ptr + (size_t)(pc.n_rows - 1) * (size_t)ld * esz, (size_t)n_cols * esz);
                touch(job.basis + (size_t)pc.t0 * nk, (size_t)pc.n_rows * nk * sizeof(double));
                if (has_w) touch(job.w_basis + (size_t)pc.w0 * nk, (size_t)pc.n_rows * nk * sizeof(double));
            }
            touch_w(yprime + (size_t)(wk.job_begin + part) * job_bytes, (size_t)job_bytes);
            ++g_jobs_walked;
        }
        if (has_w) {
            touch(jobs[wk.job_begin].w_ref, (size_t)n_cols * esz);
            touch_w(yprime + (size_t)wk.whole_job * job_bytes, (size_t)job_bytes);
        }
    }
}

// walk_gen_kernel (the general walk kernel): every job of every run streams its pieces, reads its cosine table, the plain
// fragment table up to the last k-step that holds a channel, and writes its n x m block.
void emulate_walk_gen(const std::string& name, dim3 grid, dim3 block, size_t shmem, void** a) {
    const JobA* jobs = *(const JobA**)a[0];
    const JobB* jobb = *(const JobB**)a[1];
    const Walk* walks = *(const Walk**)a[2];
    const Run* runs = *(const Run**)a[3];
    const PieceA* pieces = *(const PieceA**)a[4];
    const double* stp = *(const double**)a[5];
    int8_t* out = *(int8_t**)a[6];
    const int n_cols = *(int*)a[7];
    const int64_t ld = *(int64_t*)a[8];
    const int m = *(int*)a[9];
    const int n_slots = *(int*)a[10];
    const size_t esz = elem_size(name, "walk_gen_kernel");
    // template <typename T, int N, int VEC, bool FUSED, int NTC>: ... Li<N>E Li<VEC>E Lb<FUSED>E Li<NTC>E
    const int n = template_int(name, "walk_gen_kernel", 0), vec = template_int(name, "walk_gen_kernel", 1), ntc = template_int(name, "walk_gen_kernel", 2);
    const bool fused = name.find("Lb1ELi") != std::string::npos;
    const int waves = (int)(block.x / 64), nt = (m + 15) / 16;
    if (block.x % 64 || waves * 64 * vec < n_cols || n_cols % vec || n_slots < 1 || n_slots > 2 || nt > ntc || (fused && (waves > 10 || n > 5)) ||
        shmem < (size_t)n_slots * ((size_t)n * waves * 64 * vec + (nt * 16 <= 64 * vec ? 0 : (size_t)waves * n * nt * 16)) * 8 + 16 || shmem > 160 * 1024) {
        fprintf(stderr, "stub: walk_gen_kernel launch shape: %d waves x %d channels per lane for D = %d, m = %d (build: %d column groups, fused %d, n %d), %d slots, %zu bytes of LDS\n",
                waves, vec, n_cols, m, ntc, (int)fused, n, n_slots, shmem);
        abort();
    }
    touch(stp, (size_t)((n_cols + 3) / 4) * nt * 64 * sizeof(double));
    ++g_walk_launches;
    scalar("n_cols", n_cols), scalar("ld", ld), scalar("m", m), scalar("n_slots", n_slots);
    const int nk = n - 1;
    for (unsigned b = 0; b < grid.x; ++b) {
        const Run run = runs[b];
        mix(run);
        uint32_t jn = 0;
        const uint32_t n_walks = fused ? run.n_walks : run.n_jobs;
        for (uint32_t wi = 0; wi < n_walks; ++wi) {
            Walk wk{run.job_begin + wi, 1, -1, 0};
            if (fused) mix(wk = walks[run.walk_begin + wi]);
            const bool has_w = fused && wk.whole_job >= 0;
            const uint32_t w_rows = has_w ? jobs[wk.whole_job].n_rows : 0;
            const uint32_t n_walk_jobs = wk.n_parts + (has_w ? 1u : 0u);
            for (uint32_t part = 0; part < n_walk_jobs; ++part, ++jn) {
                const uint32_t job_id = run.job_begin + jn;      // (the kernel takes the jobs of a run in order)
                if (fused && job_id != (part < wk.n_parts ? wk.job_begin + part : (uint32_t)wk.whole_job)) {
                    fprintf(stderr, "stub: run %u walk %u part %u is not job %u\n", b, wi, part, job_id);
                    abort();
                }
                if (part < wk.n_parts) {
                    const JobA job = jobs[job_id];
                    mix(job);
                    uint32_t rows = 0;
                    for (uint32_t p = 0; p < job.n_pieces; ++p) {
                        const PieceA pc = pieces[job.piece_begin + p];
                        mix(pc);
                        if (pc.n_rows == 0 || pc.t0 != rows) { fprintf(stderr, "stub: piece table of job %u broken\n", job_id); abort(); }
                        if (pc.ptr2) { fprintf(stderr, "stub: two-source piece sent to %s\n", name.c_str()); abort(); }
                        touch(pc.ptr, (size_t)n_cols * esz);
                        touch((const char*)pc.ptr + (size_t)(pc.n_rows - 1) * (size_t)ld * esz, (size_t)n_cols * esz);
                        touch(job.basis + (size_t)pc.t0 * nk, (size_t)pc.n_rows * nk * sizeof(double));
                        if (has_w) {
                            touch(job.w_basis + (size_t)pc.w0 * nk, (size_t)pc.n_rows * nk * sizeof(double));
                            touch(job.w_basis + ((size_t)w_rows + pc.w0) * nk, ((size_t)pc.n_rows + 1) * nk * sizeof(double));  // prefix sums
                        }
                        rows += pc.n_rows;
                    }
                    if (rows != job.n_rows || (int)rows < n) { fprintf(stderr, "stub: job %u has %u rows, its pieces %u\n", job_id, job.n_rows, rows); abort(); }
                    if (has_w) touch(job.w_ref, (size_t)n_cols * esz);
                }
                mix(jobb[job_id]);
                touch_w(out + jobb[job_id].out_off, (size_t)n * m);
                ++g_jobs_walked;
            }
        }
        if (jn != run.n_jobs) { fprintf(stderr, "stub: run %u of the general kernel walks %u jobs, says %u\n", b, jn, run.n_jobs); abort(); }
    }
}

void emulate_basis(dim3 grid, void** a) {
    const BasisJob* tabs = *(const BasisJob**)a[0];
    const int nk = *(int*)a[1];
    scalar("nk", nk);
    for (unsigned y = 0; y < grid.y; ++y) mix(tabs[y].len);  // (the lengths of the fresh cosine tables, in the order of the list)
    for (unsigned y = 0; y < grid.y; ++y) touch_w(tabs[y].tab, ((size_t)tabs[y].len * nk + ((size_t)tabs[y].len + 1) * nk) * sizeof(double));
}

// ---- stream order: a vector clock over streams per stream (the null stream included) and per event.  An enqueue ticks its
// stream, hipEventRecord copies the stream's clock into the event, hipStreamWaitEvent merges the event's into the stream, and
// what the host has waited for (stream / event / device synchronisation) every later enqueue inherits.  stub_call_end(s) counts
// the operations a library call enqueued on other streams that stream s is not ordered after: work the call left running
// unowned.  Fixed-size arrays: the driver injects std::bad_alloc through operator new, and nothing here may allocate that way.
constexpr int kMaxStreams = 64;
struct Clock {
    uint32_t t[kMaxStreams];
    void merge(const Clock& o) {
        for (int i = 0; i < kMaxStreams; ++i) t[i] = t[i] > o.t[i] ? t[i] : o.t[i];
    }
};
struct StubStream {
    int id;
    Clock c;
};
struct StubEvent {
    Clock c;
};
StubStream g_null_stream{0, {}};
StubStream* g_streams[kMaxStreams] = {&g_null_stream};
int g_n_streams = 1;
Clock g_host{}, g_call_begin{};
StubStream* of(hipStream_t s) { return s ? (StubStream*)s : &g_null_stream; }
void enqueue(hipStream_t s) {
    StubStream* st = of(s);
    st->c.merge(g_host);
    st->c.t[st->id] += 1;
}
hipStream_t new_stream() {
    if (g_n_streams == kMaxStreams) { fprintf(stderr, "stub: more than %d streams\n", kMaxStreams); abort(); }
    StubStream* st = (StubStream*)calloc(1, sizeof(StubStream));
    st->id = g_n_streams;
    g_streams[g_n_streams++] = st;
    return (hipStream_t)st;
}

// ---- launch-failure injection: the n-th hipLaunchKernel from now on fails (hipErrorLaunchFailure -- the device's error, which
// a later launch on the stream reports -- returned and reported by the next hipGetLastError)
long g_launch_fail_after = -1;
unsigned long g_launch_failures = 0;
hipError_t g_last_error = hipSuccess;

void emulate_stage_b(void** a) {
    const int64_t rows = *(int64_t*)a[2];
    const JobB* jobs = *(const JobB**)a[5];
    const int n = *(int*)a[6], m = *(int*)a[7];
    int8_t* out = *(int8_t**)a[8];
    const char* ypb = *(const char**)a[0];
    const int64_t job_bytes = *(int64_t*)a[1];
    scalar("job_bytes", job_bytes), scalar("rows", rows), scalar("n", n), scalar("m", m);
    for (int64_t j = 0; j < rows / n; ++j) {
        mix(jobs[j]);
        touch(ypb + (size_t)j * job_bytes, (size_t)job_bytes);
        touch_w(out + jobs[j].out_off, (size_t)n * m);
    }
}

// ---- the five users of the context's generic scratch: what the kernel would read or write INSIDE that scratch, from the kernel's
// own arguments, first and last byte of every region.  The scratch is one hipMalloc block (= one malloc block here), so a size
// function that promises less than its launcher carves up is a heap-buffer-overflow.  Caller-owned arrays are not touched: the
// limit probes of driver_sim.cpp pass pointers that point nowhere.
void region(void* p, size_t bytes) { touch_w(p, bytes); ++g_scratch_regions; }
void emulate_plan_count(void** a) {   // protein_plan_count_kernel(idx, np, n_seg, seg_count): one count per segment
    region(*(void**)a[3], (size_t)*(int64_t*)a[2] * sizeof(int64_t));
}
void emulate_plan_scan(void** a) {    // protein_plan_scan_kernel(seg_count, n_seg): the offsets in place + the total behind them
    region(*(void**)a[0], ((size_t)*(int64_t*)a[1] + 1) * sizeof(int64_t));
}
void emulate_plan_write(void** a) {   // protein_plan_write_kernel(idx, np, n_seg, seg_off, starts): at most np blocks + the closing entry
    region(*(void**)a[3], ((size_t)*(int64_t*)a[2] + 1) * sizeof(int64_t));
    region(*(void**)a[4], ((size_t)*(int64_t*)a[1] + 1) * sizeof(int32_t));
}
void emulate_protein_pairs(void** a, bool cover) {   // protein_min_kernel / protein_cover_kernel: the totals and the first block of both plans
    const int sb = cover ? 10 : 8;   // (start_a, nblk_a at 3, 4; start_b, nblk_b behind b, ldb, idx_b)
    region(*(void**)a[4], sizeof(int64_t)), region(*(void**)a[3], 2 * sizeof(int32_t));
    region(*(void**)a[sb + 1], sizeof(int64_t)), region(*(void**)a[sb], 2 * sizeof(int32_t));
}
void emulate_l1_knn(dim3 grid, void** a) {   // l1_knn_kernel(a, na, lda, b, nb, ldb, d, k, slice_cols, n_slices, work, cand, ...)
    const size_t na = (size_t)*(int64_t*)a[1], k = (size_t)*(int*)a[7], S = (size_t)*(int*)a[9];
    if (S != grid.x) { fprintf(stderr, "stub: l1_knn_kernel on %u slices, told %zu\n", grid.x, S); abort(); }
    region(*(void**)a[10], na * S * 2 * k * sizeof(unsigned long long));          // the rows' work lists
    if (S > 1) region(*(void**)a[11], na * S * k * sizeof(unsigned long long));   // the slices' candidates
}
void emulate_knn_merge(dim3 grid, void** a) {   // knn_merge2_kernel(in, n_in, k, out, ...): grid = (rows, lists out)
    const size_t n_in = (size_t)*(int*)a[1], k = (size_t)*(int*)a[2];
    region(*(void**)a[0], (size_t)grid.x * n_in * k * sizeof(unsigned long long));
    if (grid.y > 1) region(*(void**)a[3], (size_t)grid.x * grid.y * k * sizeof(unsigned long long));   // (the last level writes out_val / out_idx)
}
void emulate_row_select_reg(const std::string& name, dim3 grid, void** a) {
    // row_select_reg_kernel<PER, SRC, TH>(src_val, src_col, ld, n_cols, seg_cols, n_seg, k, out_val, out_idx): the first pass over
    // segments writes k candidates per (row, segment), the second (SRC) reads n_cols = ld of them per row
    const size_t n_seg = (size_t)*(int64_t*)a[5], k = (size_t)*(int*)a[6];
    if (name.find("Lb1E") != std::string::npos) {
        const size_t bytes = (size_t)grid.x * (size_t)*(int64_t*)a[2] * sizeof(int32_t);
        region(*(void**)a[0], bytes), region(*(void**)a[1], bytes);
    } else if (n_seg > 1) {
        region(*(void**)a[7], (size_t)grid.x * k * sizeof(int32_t)), region(*(void**)a[8], (size_t)grid.x * k * sizeof(int32_t));
    }
}
void emulate_generic_forward(void** a) {   // generic_forward_kernel(x, n_rows, n_cols, ld, num, fs, coef): num coefficients per column
    region(*(void**)a[5], (size_t)*(int64_t*)a[2] * (size_t)*(int*)a[4] * sizeof(double));
}
void emulate_generic_inverse(void** a) {   // generic_inverse_kernel(fs, n_cols, num, scaled)
    region(*(void**)a[0], (size_t)*(int64_t*)a[1] * (size_t)*(int*)a[2] * sizeof(double));
}

// ---- what the runtime enforces at a launch.  The largest dynamic LDS a kernel was granted (hipFuncSetAttribute), in a fixed table:
// nothing here may go through operator new.
struct FuncLds { const void* fn; int bytes; } g_func_lds[64];
int g_n_func_lds = 0;
constexpr size_t kLdsDefault = 64 * 1024;    // dynamic LDS of a launch that asked for no more through hipFuncSetAttribute
constexpr size_t kLdsPerCu = 160 * 1024;     // the LDS of a gfx950 CU: no attribute raises a workgroup's share above it
constexpr size_t kMallocBudget = (size_t)1 << 30;   // one "device" allocation: a limit probe that plans more gets hipErrorOutOfMemory
long g_malloc_fail_after = -1;
bool launch_shape_ok(const void* fn, dim3 g, dim3 b, size_t shmem) {
    if (!g.x || !g.y || !g.z || !b.x || !b.y || !b.z) return false;
    // hipDeviceProp_t::maxThreadsPerBlock (hip_runtime_api.h) is 1024 on gfx950
    if ((uint64_t)b.x * b.y * b.z > 1024) return false;
    // the second and third grid dimension: 65535, the bound the library's own two-dimensional launches (rows_link, l1_knn) keep to
    if (g.y > 65535 || g.z > 65535) return false;
    // hip_runtime_api.h, hipModuleLaunchKernel: "HIP does not support kernel launch with total work items defined in dimension with
    // size gridDim x blockDim >= 2^32. So gridDim.x * blockDim.x, gridDim.y * blockDim.y and gridDim.z * blockDim.z are always less
    // than 2^32."
    if ((uint64_t)g.x * b.x >= (1ull << 32) || (uint64_t)g.y * b.y >= (1ull << 32) || (uint64_t)g.z * b.z >= (1ull << 32)) return false;
    size_t allowed = kLdsDefault;
    for (int i = 0; i < g_n_func_lds; ++i)
        if (g_func_lds[i].fn == fn) allowed = (size_t)g_func_lds[i].bytes;
    return shmem <= (allowed < kLdsPerCu ? allowed : kLdsPerCu);
}
}  // namespace

extern "C" {
unsigned long dctfp_stub_counter(int which) {
    // 0 .. 2: walk-kernel launches, stage-A launches, jobs walked; 3: launches taken, 4: launches refused for their shape, 5: scratch regions touched
    const unsigned long v[] = {g_walk_launches, g_stage_a_launches, g_jobs_walked, g_launches_taken, g_launch_refusals, g_scratch_regions};
    return which >= 0 && which < 6 ? v[which] : 0;
}
// the n-th hipMalloc from now on fails (n < 0: none)
void stub_fail_malloc(long n) { g_malloc_fail_after = n; }
void* stub_new_stream() { return new_stream(); }
void stub_call_begin() {
    for (int i = 0; i < g_n_streams; ++i)
        if (g_streams[i]) g_call_begin.t[i] = g_streams[i]->c.t[i];
}
long stub_call_end(void* stream) {
    const StubStream* caller = of((hipStream_t)stream);
    long unjoined = 0;
    for (int i = 0; i < g_n_streams; ++i) {
        if (!g_streams[i] || i == caller->id) continue;
        uint32_t done = g_call_begin.t[i];
        if (caller->c.t[i] > done) done = caller->c.t[i];
        if (g_host.t[i] > done) done = g_host.t[i];
        if (g_streams[i]->c.t[i] > done) unjoined += g_streams[i]->c.t[i] - done;
    }
    return unjoined;
}
// the n-th kernel launch from now on fails (n < 0: none); returns how many injected failures have fired so far
unsigned long stub_fail_launch(long n) {
    g_launch_fail_after = n;
    return g_launch_failures;
}

hipError_t hipGetDeviceCount(int* n) { *n = 1; return hipSuccess; }
hipError_t hipSetDevice(int) { return hipSuccess; }
hipError_t hipGetDevicePropertiesR0600(hipDeviceProp_t* p, int) {
    memset(p, 0, sizeof *p);
    strcpy(p->gcnArchName, "gfx950:sramecc+:xnack-");
    p->multiProcessorCount = 256;
    return hipSuccess;
}
hipError_t hipMalloc(void** p, size_t n) {
    *p = nullptr;
    if (n > kMallocBudget || (g_malloc_fail_after >= 0 && g_malloc_fail_after-- == 0)) return hipErrorOutOfMemory;
    *p = malloc(n ? n : 1);
    return *p ? hipSuccess : hipErrorOutOfMemory;
}
hipError_t hipFree(void* p) { free(p); return hipSuccess; }
hipError_t hipHostMalloc(void** p, size_t n, unsigned) { *p = malloc(n ? n : 1); return *p ? hipSuccess : hipErrorOutOfMemory; }
hipError_t hipHostFree(void* p) { free(p); return hipSuccess; }
hipError_t hipHostGetDevicePointer(void** d, void* h, unsigned) { *d = h; return hipSuccess; }
hipError_t hipMemcpy(void* d, const void* s, size_t n, hipMemcpyKind) { memcpy(d, s, n); return hipSuccess; }
hipError_t hipMemcpyAsync(void* d, const void* s, size_t n, hipMemcpyKind, hipStream_t st) { memcpy(d, s, n); enqueue(st); return hipSuccess; }
hipError_t hipMemsetAsync(void* d, int v, size_t n, hipStream_t st) { memset(d, v, n); enqueue(st); return hipSuccess; }
hipError_t hipMemset(void* d, int v, size_t n) { memset(d, v, n); return hipSuccess; }
hipError_t hipDeviceSynchronize() {
    for (int i = 0; i < g_n_streams; ++i)
        if (g_streams[i]) g_host.merge(g_streams[i]->c);
    return hipSuccess;
}
hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned) { *s = new_stream(); return hipSuccess; }
hipError_t hipStreamCreateWithPriority(hipStream_t* s, unsigned, int) { *s = new_stream(); return hipSuccess; }
hipError_t hipDeviceGetStreamPriorityRange(int* lo, int* hi) { *lo = 1; *hi = -1; return hipSuccess; }
hipError_t hipStreamDestroy(hipStream_t s) {
    g_streams[of(s)->id] = nullptr;
    free(s);
    return hipSuccess;
}
hipError_t hipStreamSynchronize(hipStream_t s) { g_host.merge(of(s)->c); return hipSuccess; }
hipError_t hipStreamWaitEvent(hipStream_t s, hipEvent_t e, unsigned) { of(s)->c.merge(((StubEvent*)e)->c); return hipSuccess; }
hipError_t hipEventCreate(hipEvent_t* e) { *e = (hipEvent_t)calloc(1, sizeof(StubEvent)); return hipSuccess; }
hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned) { *e = (hipEvent_t)calloc(1, sizeof(StubEvent)); return hipSuccess; }
hipError_t hipEventDestroy(hipEvent_t e) { free(e); return hipSuccess; }
hipError_t hipEventRecord(hipEvent_t e, hipStream_t s) {
    of(s)->c.merge(g_host);
    ((StubEvent*)e)->c = of(s)->c;
    return hipSuccess;
}
hipError_t hipEventSynchronize(hipEvent_t e) { g_host.merge(((StubEvent*)e)->c); return hipSuccess; }
hipError_t hipEventElapsedTime(float* ms, hipEvent_t, hipEvent_t) { *ms = 1.0f; return hipSuccess; }
hipError_t hipGetLastError() {
    const hipError_t e = g_last_error;
    g_last_error = hipSuccess;
    return e;
}
const char* hipGetErrorString(hipError_t) { return "stub"; }
const char* hipGetErrorName(hipError_t) { return "stub"; }
hipError_t hipRuntimeGetVersion(int* v) { *v = 0; return hipSuccess; }
hipError_t hipDriverGetVersion(int* v) { *v = 0; return hipSuccess; }

void** __hipRegisterFatBinary(const void*) { static void* h; return &h; }
void __hipUnregisterFatBinary(void**) {}
void __hipRegisterFunction(void**, const void* host_fn, char*, const char* device_name, unsigned, void*, void*, void*, void*, int*) {
    names()[host_fn] = device_name;
}
void __hipRegisterVar(void**, void*, char*, const char*, int, size_t, int, int) {}
namespace { dim3 g_grid, g_block; size_t g_shmem; hipStream_t g_stream; }
hipError_t __hipPushCallConfiguration(dim3 grid, dim3 block, size_t shmem, hipStream_t stream) {
    g_grid = grid; g_block = block; g_shmem = shmem; g_stream = stream;
    return hipSuccess;
}
hipError_t __hipPopCallConfiguration(dim3* grid, dim3* block, size_t* shmem, hipStream_t* stream) {
    *grid = g_grid; *block = g_block; *shmem = g_shmem; *stream = g_stream;
    return hipSuccess;
}
hipError_t hipFuncSetAttribute(const void* fn, hipFuncAttribute attr, int value) {
    if (attr != hipFuncAttributeMaxDynamicSharedMemorySize) return hipSuccess;
    if (value < 0 || (size_t)value > kLdsPerCu) return hipErrorInvalidValue;
    for (int i = 0; i < g_n_func_lds; ++i)
        if (g_func_lds[i].fn == fn) { g_func_lds[i].bytes = value; return hipSuccess; }
    if (g_n_func_lds == 64) { fprintf(stderr, "stub: more than 64 kernels with an LDS attribute\n"); abort(); }
    g_func_lds[g_n_func_lds++] = {fn, value};
    return hipSuccess;
}
hipError_t hipLaunchKernel(const void* fn, dim3 grid, dim3 block, void** args, size_t shmem, hipStream_t stream) {
    enqueue(stream);   // (a failed launch too: what the caller cannot know is whether its stream still runs something)
    if (g_launch_fail_after >= 0 && g_launch_fail_after-- == 0) {
        ++g_launch_failures;
        return g_last_error = hipErrorLaunchFailure;
    }
    const auto it = names().find(fn);
    if (it == names().end()) { fprintf(stderr, "stub: launch of an unregistered kernel\n"); abort(); }
    const std::string& n = it->second;
    // a shape the runtime refuses comes back as the runtime's error, so that the library's own error path is what runs
    if (!launch_shape_ok(fn, grid, block, shmem)) {
        ++g_launch_refusals;
        if (getenv("DCTFP_STUB_VERBOSE"))
            fprintf(stderr, "stub: refused %s grid=%u,%u,%u block=%u,%u,%u lds=%zu\n", n.c_str(), grid.x, grid.y, grid.z, block.x, block.y, block.z, shmem);
        return g_last_error = hipErrorInvalidConfiguration;
    }
    ++g_launches_taken;
    static const char* log_path = getenv("DCTFP_STUB_LAUNCH_LOG");
    if (log_path && !g_log && !(g_log = fopen(log_path, "w"))) { fprintf(stderr, "stub: cannot write %s\n", log_path); abort(); }
    g_hash = 0xcbf29ce484222325ull, g_hashed = false, g_scalars_len = 0, g_scalars[0] = 0;
    if (n.find("walk_gen_kernel") != std::string::npos) emulate_walk_gen(n, grid, block, shmem, args);
    else if (n.find("walk_ab_kernel") != std::string::npos) emulate_walk(n, grid, args);
    else if (n.find("stage_a_kernel") != std::string::npos) emulate_stage_a(n, grid, args);
    else if (n.find("basis_kernel") != std::string::npos) emulate_basis(grid, args);
    else if (n.find("stage_b_mfma_kernel") != std::string::npos) emulate_stage_b(args);
    else if (n.find("protein_plan_count_kernel") != std::string::npos) emulate_plan_count(args);
    else if (n.find("protein_plan_scan_kernel") != std::string::npos) emulate_plan_scan(args);
    else if (n.find("protein_plan_write_kernel") != std::string::npos) emulate_plan_write(args);
    else if (n.find("protein_min_kernel") != std::string::npos) emulate_protein_pairs(args, false);
    else if (n.find("protein_cover_kernel") != std::string::npos) emulate_protein_pairs(args, true);
    else if (n.find("l1_knn_kernel") != std::string::npos) emulate_l1_knn(grid, args);
    else if (n.find("knn_merge2_kernel") != std::string::npos) emulate_knn_merge(grid, args);
    else if (n.find("row_select_reg_kernel") != std::string::npos) emulate_row_select_reg(n, grid, args);
    else if (n.find("generic_forward_kernel") != std::string::npos) emulate_generic_forward(args);
    else if (n.find("generic_inverse_kernel") != std::string::npos) emulate_generic_inverse(args);
    if (g_log) {
        fprintf(g_log, "%s grid=%u,%u,%u block=%u,%u,%u lds=%zu stream=%d%s", n.c_str(), grid.x, grid.y, grid.z, block.x, block.y, block.z, shmem,
                of(stream)->id, g_scalars);
        if (g_hashed) fprintf(g_log, " tables=%016llx", (unsigned long long)g_hash);
        fputc('\n', g_log);
        fflush(g_log);
    }
    return hipSuccess;
}
}
