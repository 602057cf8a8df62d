// The int32 L1 tile that the kernels of the all-against-all cut-offs scan: the description alone.  Users: tri_walk.hip.h (one row at a
// time) and band_walk.hip.h (a band of rows at a time), the units that include either, and dctfp.hip, whose exports build and check it.
#pragma once

#include <cstdint>

namespace dctfp {

// The tile as every kernel, launcher and export of the two families takes it.  Entry (r, c), at tile[r * ld + c], is the L1 of proteins
// row0 + r and col0 + c; row_empty / col_empty (either may be NULL) flag the proteins without a fingerprint, whose key is cap;
// an entry survives when its key = min(L1, cap) <= bound.  A kernel takes the struct by value as its first argument.
struct TriTile {
    const int32_t* tile;
    int64_t n_rows, n_cols, ld, row0, col0;
    const uint8_t* row_empty;
    const uint8_t* col_empty;
    int32_t cap, bound;
};

}  // namespace dctfp
