// dct-sim --assign: place new proteins on an existing set of representatives.  The cover pass of an assignment compares every
// fingerprint of the representatives (a) with every fingerprint of the new proteins (b) and keeps, per new protein, the lowest
// representative within the cut-off:
//   rows_assign_kernel  -- the 128 x 128 contraction of two sets of rows (a copy of its own of sad_tile.hip.h's sad_tile, see
//                          below: a fix to the tile is made in both places); every pair of rows within the bound lowers assign[slot of the b row] to the value of the a row, straight from the
//                          accumulators: no distance is written anywhere.
// The block is a full rectangle: there is no diagonal and no owner, a and b are different files.  The host maps rows to protein
// nodes through value_a / slot_b (one int32 per row; NULL: a0 + r / b0 + c) -- the DCTdomain route hands in all rows with their
// proteins' nodes, the DCTglobal route the last rows only.
//
// Visibility, as in k_greedy.hip: inside this launch assign is touched by agent-scope relaxed atomics and by nothing else -- a
// load that skips a minimum which would change nothing (a stale view can only show a LARGER value than the one copy the atomics
// of all XCDs reach holds, since values only go down: the minimum is then issued and decided there), and the minimum itself.  No
// plain load or store, nothing through the scalar path, and no wave waits for another workgroup.  The result is the minimum
// over a set of (slot, value) pairs that the inputs alone fix, whatever the order in which waves ran and however the host split
// the rows into calls.
#define DCTFP_TEMPLATES_ONLY
#include "launch.h"

namespace {

using dctfp::kSadKC;
using dctfp::kSadLD;
using dctfp::kSadLds;
using dctfp::kSadTile;
using dctfp::load_bytes4;
using dctfp::sad_b_slot;
using dctfp::v4u32;

// The kernel keeps a copy of its own of sad_tile<ALIGN> and sad_keep_mask (sad_tile.hip.h, which rows_link_kernel calls): through the
// shared function its 16-byte arm compiled to 128 registers instead of 126 and the cover pass of tools/assign_bench.py measured
// 285.8 ms against 285.0 ms (the third runs of five processes each, disjoint ranges; profiles/sad_tile/README.md).  A fix to
// the tile is made there AND here.  The layout numbers (kSadTile, kSadKC, kSadLD, sad_b_slot) are the header's.

// ALIGN = what the rows' addresses are multiples of, dctfp_l1_matrix's three arms: 16 fills the tiles with 16-byte loads (32-bit
// lane offsets: lda, ldb < 2^24), 4 with dword loads, 1 with byte loads -- into the same LDS layout, for the same contraction
// (8 x 8 per thread, 16-byte segments of sign-flipped bytes through v_sad_u8, ds_read_b128 at a row stride of 36 dwords).
// The epilogue: a thread's 64 sums against the bound as a 64-bit mask (bit 8 i + j), rows and columns beyond the sets masked out,
// and a wave-wide ballot, which in the common case shows no survivor anywhere.  Else the lanes with a bit walk theirs.  A slot
// outside [0, n_assign) or a negative value is skipped here: the host cannot see those arrays.
template <int ALIGN>
__global__ __launch_bounds__(256, 4) void rows_assign_kernel(const int8_t* __restrict__ a, int64_t na, int64_t lda,
                                                             const int32_t* __restrict__ value_a, int64_t a0, const int8_t* __restrict__ b,
                                                             int64_t nb, int64_t ldb, const int32_t* __restrict__ slot_b, int64_t b0, int d,
                                                             uint32_t cap, uint32_t bound, int32_t* assign, int64_t n_assign) {
    const int64_t r0 = (int64_t)blockIdx.y * kSadTile, c0 = (int64_t)blockIdx.x * kSadTile;
    const int rows_a = (int)min((int64_t)kSadTile, na - r0), rows_b = (int)min((int64_t)kSadTile, nb - c0);
    __shared__ uint32_t sa[kSadLds];
    __shared__ uint32_t sb[kSadLds];
    const int ty = threadIdx.x >> 4, tx = threadIdx.x & 15;
    const v4u32 flip = {0x80808080u, 0x80808080u, 0x80808080u, 0x80808080u};   // signed -> unsigned order, |x - y| unchanged
    const int8_t* __restrict__ abase = a + r0 * lda;
    const int8_t* __restrict__ bbase = b + c0 * ldb;
    uint32_t acc[8][8] = {};
    auto contract = [&](int kn) {
        for (int k = 0; k < kn; k += 4) {
            v4u32 av[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) av[i] = *reinterpret_cast<const v4u32*>(&sa[(ty * 8 + i) * kSadLD + k]);
#pragma unroll
            for (int h = 0; h < 4; ++h) {
                v4u32 bv[2];
#pragma unroll
                for (int j = 0; j < 2; ++j) bv[j] = *reinterpret_cast<const v4u32*>(&sb[((2 * h + j) * 16 + tx) * kSadLD + k]);
#pragma unroll
                for (int q = 0; q < 4; ++q)
#pragma unroll
                    for (int i = 0; i < 8; ++i)
#pragma unroll
                        for (int j = 0; j < 2; ++j) acc[i][2 * h + j] = __builtin_amdgcn_sad_u8(av[i][q], bv[j][q], acc[i][2 * h + j]);
            }
        }
    };
    // (the b rows sit in LDS in the order the lanes read them: sad_b_slot)
    if constexpr (ALIGN == 16) {
        const int seg = threadIdx.x & 7, frow = threadIdx.x >> 3;
        const uint32_t lda32 = (uint32_t)lda, ldb32 = (uint32_t)ldb;
        const int d16 = d & ~15;
        for (int byte0 = 0; byte0 < d16; byte0 += kSadKC * 4) {
            const int my0 = byte0 + seg * 16;
            const bool have = my0 < d16;
            __syncthreads();
            {
                v4u32 va[kSadTile / 32], vb[kSadTile / 32];
#pragma unroll
                for (int i = 0; i < kSadTile / 32; ++i) {
                    const int r = frow + 32 * i;
                    va[i] = flip;
                    vb[i] = flip;
                    if (have && r < rows_a) va[i] = *reinterpret_cast<const v4u32*>(abase + ((uint32_t)r * lda32 + (uint32_t)my0));
                    if (have && r < rows_b) vb[i] = *reinterpret_cast<const v4u32*>(bbase + ((uint32_t)r * ldb32 + (uint32_t)my0));
                }
#pragma unroll
                for (int i = 0; i < kSadTile / 32; ++i) {
                    const int r = frow + 32 * i;
                    *reinterpret_cast<v4u32*>(&sa[r * kSadLD + seg * 4]) = va[i] ^ flip;
                    *reinterpret_cast<v4u32*>(&sb[sad_b_slot(r) * kSadLD + seg * 4]) = vb[i] ^ flip;
                }
            }
            __syncthreads();
            contract(min(kSadKC, (d16 - byte0) >> 2));
        }
        if (d16 < d) {   // the 1..15 bytes the fingerprints end with
            __syncthreads();
            if (threadIdx.x < kSadTile) {
                const int r = threadIdx.x;
                v4u32 va = flip, vb = flip;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int n = min(4, d - d16 - 4 * q);
                    if (n > 0 && r < rows_a) va[q] = load_bytes4(abase + ((uint32_t)r * lda32 + (uint32_t)(d16 + 4 * q)), n);
                    if (n > 0 && r < rows_b) vb[q] = load_bytes4(bbase + ((uint32_t)r * ldb32 + (uint32_t)(d16 + 4 * q)), n);
                }
                *reinterpret_cast<v4u32*>(&sa[r * kSadLD]) = va ^ flip;
                *reinterpret_cast<v4u32*>(&sb[sad_b_slot(r) * kSadLD]) = vb ^ flip;
            }
            __syncthreads();
            contract(4);
        }
    } else {
        // l1_matrix_kernel's fill: thread -> dword k = tid & 31 of the rows tid >> 5, + 8, + 16, ...; the dwords between the end of
        // the fingerprints and the next multiple of four hold no difference (the contraction takes four at a time)
        const int nd = (d + 3) / 4;
        const int k = threadIdx.x & (kSadKC - 1);
        for (int k0 = 0; k0 < nd; k0 += kSadKC) {
            const int kn4 = (min(kSadKC, nd - k0) + 3) & ~3;
            const int byte0 = (k0 + k) * 4;
            const int valid = min(4, d - byte0);
            __syncthreads();
            if (k < kn4) {
#pragma unroll 4
                for (int r = threadIdx.x >> 5; r < kSadTile; r += 256 / kSadKC) {
                    uint32_t va = 0x80808080u, vb = 0x80808080u;
                    if (valid > 0 && r < rows_a) {
                        const int8_t* p = abase + r * lda + byte0;
                        va = (ALIGN == 4 && valid == 4) ? *reinterpret_cast<const uint32_t*>(p) : load_bytes4(p, valid);
                    }
                    if (valid > 0 && r < rows_b) {
                        const int8_t* p = bbase + r * ldb + byte0;
                        vb = (ALIGN == 4 && valid == 4) ? *reinterpret_cast<const uint32_t*>(p) : load_bytes4(p, valid);
                    }
                    sa[r * kSadLD + k] = va ^ 0x80808080u;
                    sb[sad_b_slot(r) * kSadLD + k] = vb ^ 0x80808080u;
                }
            }
            __syncthreads();
            contract(kn4);
        }
    }
    // row ty * 8 + i, column tx * 8 + j: bit 8 i + j
    uint32_t lo = 0, hi = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            lo |= (uint32_t)(min(acc[i][j], cap) <= bound) << (8 * i + j);
            hi |= (uint32_t)(min(acc[i + 4][j], cap) <= bound) << (8 * i + j);
        }
    const int n_row = max(0, min(8, rows_a - ty * 8)), n_col = max(0, min(8, rows_b - tx * 8));
    uint64_t keep = ((uint64_t)hi << 32 | lo) & (n_row == 8 ? ~(uint64_t)0 : ((uint64_t)1 << (8 * n_row)) - 1) &
                    (0x0101010101010101ull * ((1u << n_col) - 1));
    if (__ballot(keep != 0) == 0) return;
    // (every row the bits name lies inside a and b: the mask above)
    const int64_t row_a = r0 + ty * 8, row_b = c0 + tx * 8;
    while (keep) {
        const int bit = __builtin_ctzll(keep);
        keep &= keep - 1;
        const int64_t r = row_a + (bit >> 3), c = row_b + (bit & 7);
        const int64_t value = value_a ? (int64_t)value_a[r] : a0 + r;
        const int64_t slot = slot_b ? (int64_t)slot_b[c] : b0 + c;
        if (slot < 0 || slot >= n_assign || value < 0 || value > 0x7fffffff) continue;
        if (__hip_atomic_load(assign + slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) <= (int32_t)value) continue;
        __hip_atomic_fetch_min(assign + slot, (int32_t)value, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

}  // namespace

namespace dctfp_host {

void launch_rows_assign(const int8_t* a, int64_t na, int64_t lda, const int32_t* value_a, int64_t a0, const int8_t* b, int64_t nb, int64_t ldb,
                        const int32_t* slot_b, int64_t b0, int d, int32_t cap, int32_t bound, int32_t* assign, int64_t n_assign,
                        hipStream_t stream) {
    const dim3 grid((unsigned)((nb + kSadTile - 1) / kSadTile), (unsigned)((na + kSadTile - 1) / kSadTile));
    const int align = sad_tile_align(a, lda, b, ldb);   // (sad_tile.hip.h)
    auto* const kernel = align == 16 ? rows_assign_kernel<16> : align == 4 ? rows_assign_kernel<4> : rows_assign_kernel<1>;
    hipLaunchKernelGGL(kernel, grid, dim3(256), 0, stream, a, na, lda, value_a, a0, b, nb, ldb, slot_b, b0, d, (uint32_t)cap, (uint32_t)bound,
                       assign, n_assign);
}

}  // namespace dctfp_host
