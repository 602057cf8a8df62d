// The 128 x 128 tile of L1 distances between int8 rows that every kernel of the similarity side is built on: rows_a rows of a
// against rows_b rows of b, 256 threads, 8 x 8 sums per thread through v_sad_u8 (4 byte differences per instruction), both
// operand tiles staged in LDS 32 dwords (128 bytes of the rows) at a time.  Device code only (and the host's choice of a fill),
// defined once for its THREE callers: kernels.hip.h includes it for l1_matrix16_kernel, and k_protein.hip (protein_min_kernel and
// protein_cover_kernel) and k_cluster.hip (rows_link_kernel) call the same function inside their own loops, each with its own launch bounds, LDS
// declarations and epilogue.
//
// TWO COPIES remain, and a fix to the tile (tail round, lane offsets, bank layout, keep mask) goes there too: l1_knn_kernel
// (k_query.hip: sad_tile<16>) and rows_assign_kernel (k_assign.hip: sad_tile<ALIGN> and sad_keep_mask) spell the same loop out in
// the kernel body, because through this function they measured slower than before (profiles/sad_tile/README.md).  They use the
// constants, load_bytes4, sad_b_slot and (k_assign.hip) sad_tile_align from here.  tests/test_sad_tile_gpu.py pins all five to
// one numpy matrix.
//
// Why it looks the way it does (tools/microbench/sad_rate.hip): v_sad_u8 from registers sustains 0.92 of its 157 T/s; fed by
// 16 ds_read_b32 per 64 instructions (l1_matrix_kernel, kernels.hip.h: the older contraction at a row stride of 33 dwords) 0.83, by
// 16 ds_read_b128 per 256 0.91 -- and that kernel reached 0.59: beside the narrow LDS reads it fills its tiles with 64 four-byte
// global loads and as many ds_write_b32 per thread and chunk, through per-byte tail code in the same loop.  Here: 16 bytes per
// lane from HBM / L2 to LDS (8 loads + 8 ds_write_b128 per thread and chunk), row stride 36 dwords (16 lanes reading 16 bytes
// each of 16 different rows hit 64 different banks), 4 k-steps per round of LDS reads.  The b rows sit in LDS in the order the
// lanes read them (row r at slot (r % 8) * 16 + r / 8: the 16 lanes of a row group read 16 consecutive slots; the a rows are
// broadcast reads).  Bytes are sign-flipped on the way in (signed -> unsigned order, |x - y| unchanged); whatever lies beyond a
// set's rows or a row's end holds the same value on both sides and adds no difference.
//
// Barriers.  Every fill of sad_tile starts with __syncthreads(), so a caller may have used sa / sb for something else right up to
// the call.  There is NO barrier after the last contraction: a caller that writes to sa / sb afterwards (protein_min_kernel's
// protein tile; l1_knn_kernel's copy does the same for its below[]) puts one in front of that.  Every thread of the workgroup
// must make the call.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace dctfp {

typedef unsigned v4u32 __attribute__((ext_vector_type(4)));

constexpr int kSadTile = 128;                 // rows of a / of b per workgroup
constexpr int kSadKC = 32;                    // dwords of a row per chunk
constexpr int kSadLD = kSadKC + 4;            // LDS row stride (dwords): ds_read_b128 of 16 consecutive rows without a bank conflict
constexpr int kSadLds = kSadTile * kSadLD;    // dwords of one operand tile in LDS (18 KiB)

__device__ inline uint32_t load_bytes4(const int8_t* p, int n_valid) {  // n_valid in 1..4
    uint32_t v = 0;
    for (int i = 0; i < n_valid; ++i) v |= (uint32_t)(uint8_t)p[i] << (8 * i);
    for (int i = n_valid; i < 4; ++i) v |= 0x80u << (8 * i);  // xor'ed back to 0 by the fill
    return v;
}

// One step of the sum without the tile: s + the four byte differences of two sign-flipped dwords (v_sad_u8), for a kernel that
// contracts one fingerprint pair per wave straight from global memory (k_map.hip's pair_row_best_kernel).
__device__ inline uint32_t sad_dword(uint32_t x, uint32_t y, uint32_t s) { return __builtin_amdgcn_sad_u8(x, y, s); }

// Which fill two sets of rows can take = what all their rows' addresses are multiples of: 16 (and rows less than 2^24 bytes
// apart: that fill addresses a tile's rows with 32-bit lane offsets, 128 * ld < 2^31), 4 or 1.  dctfp_l1_matrix sends 4 and 1 to
// l1_matrix_kernel<true / false>; dctfp_protein_min and dctfp_l1_knn refuse them.
inline int sad_tile_align(const void* a, int64_t lda, const void* b, int64_t ldb) {
    const uintptr_t bits = reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | (uintptr_t)lda | (uintptr_t)ldb;
    return (bits & 15u) == 0 && lda < (1 << 24) && ldb < (1 << 24) ? 16 : (bits & 3u) == 0 ? 4 : 1;
}

__device__ __forceinline__ int sad_b_slot(int r) { return (r & 7) * 16 + (r >> 3); }

// acc[i][j] += L1(row ty * 8 + i of a, row tx * 8 + j of b) over d bytes, ty = tid >> 4, tx = tid & 15; rows at or beyond
// rows_a / rows_b (<= 128) are not read and their sums mean nothing.  abase / bbase = the tiles' first rows (wave-uniform), sa /
// sb = kSadLds dwords of LDS each.  ALIGN = sad_tile_align() of the operands.
template <int ALIGN>
__device__ __forceinline__ void sad_tile(const int8_t* __restrict__ abase, int rows_a, int64_t lda, const int8_t* __restrict__ bbase, int rows_b,
                                         int64_t ldb, int d, uint32_t* sa, uint32_t* sb, uint32_t (&acc)[8][8]) {
    // kn dwords (a multiple of 4) of the staged rows.  4 k-steps: 16 bytes of 8 a rows and, two at a time, of my 8 b rows from
    // LDS -> 256 v_sad_u8 (64 + 32 + 8 registers)
    const int ty = threadIdx.x >> 4, tx = threadIdx.x & 15;
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
    if constexpr (ALIGN == 16) {
        // thread -> 16-byte segment (tid & 7) of the rows tid >> 3, + 32, + 64, + 96.  Addresses = a uniform 64-bit tile base + a
        // 32-bit lane offset: eight 64-bit row pointers held through the k loop would not fit beside the 64 accumulators.
        const int seg = threadIdx.x & 7, frow = threadIdx.x >> 3;
        const v4u32 flip = {0x80808080u, 0x80808080u, 0x80808080u, 0x80808080u};
        const uint32_t lda32 = (uint32_t)lda, ldb32 = (uint32_t)ldb;
        const int d16 = d & ~15;   // whole 16-byte segments; what is left (d % 16 != 0) goes through one more, narrow round below
        for (int byte0 = 0; byte0 < d16; byte0 += kSadKC * 4) {
            const int my0 = byte0 + seg * 16;   // first byte of my segment
            const bool have = my0 < d16;        // (else past the end: both sides equal, no difference)
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
        if (d16 < d) {   // the 1..15 bytes the rows end with: byte loads, one 16-byte segment per row
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
        // l1_matrix_kernel's fill: thread -> dword k = tid & 31 of the rows tid >> 5, + 8, + 16, ... (dword loads at ALIGN 4, byte
        // loads at 1); the dwords between the end of the rows and the next multiple of four hold no difference (the contraction
        // takes four at a time)
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
}

// A thread's 64 sums against a bound: bit 8 i + j is set when min(acc[i][j], cap) <= bound and row ty * 8 + i < rows_a and
// column tx * 8 + j < rows_b (rows_link_kernel's and rows_assign_kernel's survivors; in the common case no lane of a wave has one).
__device__ __forceinline__ uint64_t sad_keep_mask(const uint32_t (&acc)[8][8], uint32_t cap, uint32_t bound, int rows_a, int rows_b) {
    const int ty = threadIdx.x >> 4, tx = threadIdx.x & 15;
    uint32_t lo = 0, hi = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            lo |= (uint32_t)(min(acc[i][j], cap) <= bound) << (8 * i + j);
            hi |= (uint32_t)(min(acc[i + 4][j], cap) <= bound) << (8 * i + j);
        }
    const int n_row = max(0, min(8, rows_a - ty * 8)), n_col = max(0, min(8, rows_b - tx * 8));
    return ((uint64_t)hi << 32 | lo) & (n_row == 8 ? ~(uint64_t)0 : ((uint64_t)1 << (8 * n_row)) - 1) &
           (0x0101010101010101ull * ((1u << n_col) - 1));
}

}  // namespace dctfp
