// dct-sim --hac: complete- and average-linkage trees of a file, built in rounds on a dense symmetric n x n matrix that stays on the
// device.  The nodes are the proteins; a cluster is named by its lowest member (its id) and has size[id] > 0 members; size[x] == 0
// says that x names no cluster (any more).  Entry (a, b) of two live clusters holds
//   complete (int32): D(a, b) = the largest key = min(L1, 17000) over their member pairs;
//   average  (int64): S(a, b) = the exact sum of key over their member pairs -- the height S / (c_a c_b) is only ever compared as a
//                     fraction of integers.
// The diagonal holds the sentinel (the largest value of the type), which passes no bound test; whatever a row or column of a dead
// cluster holds is never read as a distance again (below).  A round is two launches with O(n) bookkeeping between them:
//   linkage_nearest_kernel -- per live cluster a: nn[a] = the live b != a with D(a, b) <= bound that minimises (D(a, b), b), -1 = none;
//   linkage_merge_kernel   -- every pair with nn[a] = b and nn[b] = a becomes one cluster under the lower id; every distance between
//                             two clusters of the next round = max (complete) / sum (average) over the pre-round clusters they consist of.
//
// linkage_nearest_kernel<T>.  One workgroup per live row (the live list: no work for a dead row), 256 threads over the n columns:
// the entries up to the first 16-byte boundary of the row one per lane (dword / qword loads: at most 3 / 1 of them), then 16 bytes
// per lane and step -- 1 KiB per wave instruction, consecutive lanes on consecutive addresses -- then the tail one per lane again.
// A row on a 16-byte boundary (ld a multiple of 4 / 2 on an aligned base, as the Python layer allocates it) has no head.  size[] of
// the same columns comes with every step: size[x] == 0 masks a dead column, so a dying row or column needs no sentinel written
// into it (the choice the header of linkage_merge_kernel argues), and average linkage needs c_x anyway.  The lane's best is
// reduced in the wave with shuffles and across the four waves through LDS; lane 0 writes nn[a].  No global atomics.
//   complete: the order is (D, id) -- one 64-bit word D << 32 | id.
//   average:  D(a, x) = S(a, x) / (c_a c_x); c_a is the same along a row and cancels, so x beats y when
//             S(a, x) c_y < S(a, y) c_x, or they are equal and x < y.  The sentinel, size[x] == 0 and the bound test
//             S(a, x) <= bound c_a c_x all come BEFORE that multiply: only entries within the bound are ever multiplied.
//   Overflow.  Such an entry has S(a, x) <= 17000 c_a c_x, so S(a, x) c_y <= 17000 c_a c_x c_y.  a, x and y are three different
//   live clusters: c_a + c_x + c_y <= n <= 46 340 (kLinkageMaxN), and a product of three numbers of a given sum is largest when
//   they are equal: c_a c_x c_y <= (n / 3)^3 < 15 447^3 < 3.686e12, 17000 times that < 6.27e16 < 2^63 = 9.22e18.  The bound test's own
//   right side, bound c_a c_x <= 17000 (n / 2)^2 < 9.2e12, is smaller still.  64 bits suffice, and the host refuses n > 46 340 and
//   bound > 17000 before a launch (dctfp_linkage_nearest).  46 340 is also floor(sqrt(2^31)): n * n fits 31 bits.
//
// linkage_merge_kernel<T>.  partner[x] = the other cluster of x's pair this round, -1 = x merges with nothing; the lower id of a
// pair survives and absorbs the higher, which dies.  keep[0 .. n_keep) lists the survivors of the pairs.  One thread per (x, y),
// x = keep[blockIdx.y], y a column: nothing to do when y == x, size[y] == 0 (dead before this round) or y dies this round.  Else,
// with p_x = partner[x] and p_y = partner[y] if y survives a pair of its own,
//   new (x, y) = combine of (x, y), (p_x, y) and, where p_y exists, (x, p_y), (p_x, p_y)
// -- the up to four pre-round values of the rule -- written to (x, y) and, ONLY where y has no pair of its own, to the mirror
// (y, x) too.  (Where y has one, the thread (y, x) of y's own row computes the same combination and writes (y, x).)
//   Hazards.  Plain loads and stores, no workgroup waits for another; what makes that safe:
//   (1) Every written entry is read by the thread that writes it and by no other.  (x, y) is read as a "(x, y)" by its own thread
//       alone; as a "(x, p_y')" it would need y = p_y' to die, and such y are skipped, never written; as a "(p_x', .)" it would need
//       row x to die, and x survives.  The mirror (y, x) lies in row y of a cluster without a pair: the only rows any thread reads
//       are those of a survivor x' and of its dying partner p_x', so nobody reads row y at all.
//   (2) Every other entry a thread reads -- (p_x, y), (x, p_y), (p_x, p_y) -- lies in a row or column that dies this round, and no
//       entry of a dying row or column is written in this launch.
//   So no read can see a value of this round: the result does not depend on the order in which the threads ran.  Visibility of the
//   new values to the next linkage_nearest_kernel comes from the launch boundary.
//   Dying rows and columns.  They keep their old values.  Rows: the live list leaves them out.  Columns: the scan masks them by
//   size[x] == 0, which the bookkeeping sets (O(n)).  The alternative, a launch that writes the sentinel down every dying column,
//   is n_live x n_dying stores of 4 or 8 bytes a whole row apart -- a third of the matrix in the first rounds, in the pattern the chip
//   handles worst -- where the mask is one more coalesced load of an array that stays in L2 and that average linkage loads anyway.
//   Access.  (x, y) and (p_x, y) are coalesced; (x, p_y), (p_x, p_y) are 4- / 8-byte gathers inside two rows; the mirror store is a
//   column of the matrix, one entry per row.
#define DCTFP_TEMPLATES_ONLY
#include "launch.h"

#include <type_traits>

namespace {

constexpr int kLinkageThreads = 256;

template <typename T> struct Vec16;
template <> struct Vec16<int32_t> { using type = int4; static constexpr int kLanes = 4; };
template <> struct Vec16<int64_t> { using type = longlong2; static constexpr int kLanes = 2; };

template <typename T> __device__ inline T linkage_sentinel();
template <> __device__ inline int32_t linkage_sentinel<int32_t>() { return 0x7fffffff; }
template <> __device__ inline int64_t linkage_sentinel<int64_t>() { return 0x7fffffffffffffffll; }

// The best candidate of a lane: complete keeps (D, id), average (S, c, id).  id < 0 = none.
template <typename T>
struct Cand {
    T v;
    int32_t c;
    int32_t id;
};

// Is (v, c, x) before the candidate b in the order of the header?  b.id < 0: anything is.
template <typename T>
__device__ inline bool cand_before(T v, int32_t c, int32_t x, const Cand<T>& b) {
    if (b.id < 0) return true;
    if constexpr (std::is_same<T, int32_t>::value) {
        return v < b.v || (v == b.v && x < b.id);
    } else {
        const int64_t l = v * (int64_t)b.c, r = b.v * (int64_t)c;   // (both within the bound: the header's overflow argument)
        return l < r || (l == r && x < b.id);
    }
}

// One entry (a, x) of value v: sentinel, dead column, the row's own column and the bound first, then the order.
template <typename T>
__device__ inline void cand_take(Cand<T>& best, T v, int32_t c, int32_t x, int32_t a, int32_t bound, int64_t bound_ca) {
    if (v == linkage_sentinel<T>() || c <= 0 || x == a) return;
    if constexpr (std::is_same<T, int32_t>::value) {
        if (v > bound) return;
    } else {
        if (v > bound_ca * (int64_t)c) return;
    }
    if (cand_before<T>(v, c, x, best)) best = Cand<T>{v, c, x};
}

template <typename T>
__device__ inline Cand<T> cand_shuffle(const Cand<T>& m, int d) {
    Cand<T> o;
    if constexpr (std::is_same<T, int32_t>::value) {
        o.v = __shfl_xor(m.v, d);
    } else {
        o.v = (int64_t)((uint64_t)(uint32_t)__shfl_xor((int)(uint32_t)m.v, d) | (uint64_t)(uint32_t)__shfl_xor((int)(m.v >> 32), d) << 32);
    }
    o.c = __shfl_xor(m.c, d);
    o.id = __shfl_xor(m.id, d);
    return o;
}

template <typename T>
__global__ __launch_bounds__(kLinkageThreads) void linkage_nearest_kernel(const T* __restrict__ mat, int64_t n, int64_t ld,
                                                                          const int32_t* __restrict__ size, const int32_t* __restrict__ live,
                                                                          int64_t n_live, int32_t bound, int32_t* __restrict__ nn) {
    using V = typename Vec16<T>::type;
    constexpr int L = Vec16<T>::kLanes;
    __shared__ Cand<T> s_best[kLinkageThreads / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int64_t k = blockIdx.x; k < n_live; k += gridDim.x) {
        const int32_t a = live[k];
        if ((uint32_t)a >= (uint64_t)n) continue;                 // (an id outside the matrix: the caller's list is no live list)
        const T* row = mat + (int64_t)a * ld;
        const int32_t ca = size[a];
        const int64_t bound_ca = (int64_t)bound * ca;
        Cand<T> best{0, 0, -1};
        // the entries in front of the first 16-byte boundary, the 16-byte body, the tail
        const int64_t head = min(n, (int64_t)((16 - (reinterpret_cast<uintptr_t>(row) & 15)) & 15) / (int64_t)sizeof(T));
        const int64_t n_vec = (n - head) / L;
        if (tid < head) cand_take<T>(best, row[tid], size[tid], (int32_t)tid, a, bound, bound_ca);
        const V* body = reinterpret_cast<const V*>(row + head);
        for (int64_t v = tid; v < n_vec; v += kLinkageThreads) {
            const V q = body[v];
            const int64_t x0 = head + v * L;
            if constexpr (L == 4) {
                cand_take<T>(best, q.x, size[x0], (int32_t)x0, a, bound, bound_ca);
                cand_take<T>(best, q.y, size[x0 + 1], (int32_t)(x0 + 1), a, bound, bound_ca);
                cand_take<T>(best, q.z, size[x0 + 2], (int32_t)(x0 + 2), a, bound, bound_ca);
                cand_take<T>(best, q.w, size[x0 + 3], (int32_t)(x0 + 3), a, bound, bound_ca);
            } else {
                cand_take<T>(best, q.x, size[x0], (int32_t)x0, a, bound, bound_ca);
                cand_take<T>(best, q.y, size[x0 + 1], (int32_t)(x0 + 1), a, bound, bound_ca);
            }
        }
        const int64_t x_tail = head + n_vec * L + tid;
        if (x_tail < n) cand_take<T>(best, row[x_tail], size[x_tail], (int32_t)x_tail, a, bound, bound_ca);
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) {
            const Cand<T> o = cand_shuffle<T>(best, d);
            if (o.id >= 0 && cand_before<T>(o.v, o.c, o.id, best)) best = o;
        }
        __syncthreads();                                            // (the previous row's result has been read)
        if (lane == 0) s_best[wave] = best;
        __syncthreads();
        if (tid == 0) {
            Cand<T> m = s_best[0];
            for (int w = 1; w < kLinkageThreads / 64; ++w)
                if (s_best[w].id >= 0 && cand_before<T>(s_best[w].v, s_best[w].c, s_best[w].id, m)) m = s_best[w];
            nn[a] = m.id;
        }
    }
}

template <typename T>
__device__ inline T linkage_combine(T u, T v) {
    if constexpr (std::is_same<T, int32_t>::value) return max(u, v);
    else return u + v;
}

template <typename T>
__global__ __launch_bounds__(kLinkageThreads) void linkage_merge_kernel(T* mat, int64_t n, int64_t ld, const int32_t* __restrict__ size,
                                                                        const int32_t* __restrict__ partner, const int32_t* __restrict__ keep) {
    const int64_t y = (int64_t)blockIdx.x * kLinkageThreads + threadIdx.x;
    const int32_t x = keep[blockIdx.y];
    if (y >= n || (uint32_t)x >= (uint64_t)n) return;
    const int32_t px = partner[x];
    if (px <= x || px >= n) return;                                // (x survives no pair: the caller's list is no keep list)
    if (y == x || size[y] <= 0) return;
    const int32_t py = partner[y];
    if (py >= 0 && py < y) return;                                 // (y dies this round -- p_x among them)
    T* rx = mat + (int64_t)x * ld;
    const T* rp = mat + (int64_t)px * ld;
    T v = linkage_combine<T>(rx[y], rp[y]);
    const bool paired = py > y && py < n;
    if (paired) v = linkage_combine<T>(v, linkage_combine<T>(rx[py], rp[py]));
    rx[y] = v;
    if (!paired) mat[y * ld + x] = v;
}

template <typename T>
void launch_nearest_t(const T* mat, int64_t n, int64_t ld, const int32_t* size, const int32_t* live, int64_t n_live, int32_t bound,
                      int32_t* nn, hipStream_t stream) {
    hipLaunchKernelGGL(linkage_nearest_kernel<T>, dim3((unsigned)n_live), dim3(kLinkageThreads), 0, stream, mat, n, ld, size, live, n_live,
                       bound, nn);
}

template <typename T>
void launch_merge_t(T* mat, int64_t n, int64_t ld, const int32_t* size, const int32_t* partner, const int32_t* keep, int64_t n_keep,
                    hipStream_t stream) {
    hipLaunchKernelGGL(linkage_merge_kernel<T>, dim3((unsigned)((n + kLinkageThreads - 1) / kLinkageThreads), (unsigned)n_keep),
                       dim3(kLinkageThreads), 0, stream, mat, n, ld, size, partner, keep);
}

}  // namespace

namespace dctfp_host {

void launch_linkage_nearest(const void* mat, int wide, int64_t n, int64_t ld, const int32_t* size, const int32_t* live, int64_t n_live,
                            int32_t bound, int32_t* nn, hipStream_t stream) {
    if (wide) launch_nearest_t<int64_t>(static_cast<const int64_t*>(mat), n, ld, size, live, n_live, bound, nn, stream);
    else launch_nearest_t<int32_t>(static_cast<const int32_t*>(mat), n, ld, size, live, n_live, bound, nn, stream);
}

void launch_linkage_merge(void* mat, int wide, int64_t n, int64_t ld, const int32_t* size, const int32_t* partner, const int32_t* keep,
                          int64_t n_keep, hipStream_t stream) {
    if (wide) launch_merge_t<int64_t>(static_cast<int64_t*>(mat), n, ld, size, partner, keep, n_keep, stream);
    else launch_merge_t<int32_t>(static_cast<int32_t*>(mat), n, ld, size, partner, keep, n_keep, stream);
}

}  // namespace dctfp_host
