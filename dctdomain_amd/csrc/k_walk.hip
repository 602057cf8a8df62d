// walk_ab_kernel.
#define DCTFP_TEMPLATES_ONLY
#include "launch.h"

namespace dctfp_host {

template <typename T, int S, int NT>
void launch_walk_impl(const WParams& p, bool fused) {
    static const InvTab<3> inv = make_inv<3>();
    if constexpr (sizeof(T) == 4 && NT == 5) {
        if (p.two_source) {  // pieces that are the mean of two windows' rows (dctfp_quantize_windows): builds of their own
            if (fused) {
                hipLaunchKernelGGL((walk_ab_kernel<T, S, 4, NT, 8, true, true>), dim3(p.grid), dim3(S * 64), 0, p.stream, p.jobs, p.jobb,
                                   p.walks, p.runs, p.pieces, p.stf, p.out, p.n_cols, p.ld, p.m, inv, p.degenerate);
                if (p.built) *p.built = walk_word<T, S, NT, true, true>();
            } else {
                hipLaunchKernelGGL((walk_ab_kernel<T, S, 4, NT, 8, false, true>), dim3(p.grid), dim3(S * 64), 0, p.stream, p.jobs, p.jobb,
                                   p.walks, p.runs, p.pieces, p.stf, p.out, p.n_cols, p.ld, p.m, inv, p.degenerate);
                if (p.built) *p.built = walk_word<T, S, NT, false, true>();
            }
            return;
        }
    }
    if (fused) {
        hipLaunchKernelGGL((walk_ab_kernel<T, S, 4, NT, 8, true>), dim3(p.grid), dim3(S * 64), 0, p.stream, p.jobs, p.jobb, p.walks,
                           p.runs, p.pieces, p.stf, p.out, p.n_cols, p.ld, p.m, inv, p.degenerate);
        if (p.built) *p.built = walk_word<T, S, NT, true, false>();
    } else {
        hipLaunchKernelGGL((walk_ab_kernel<T, S, 4, NT, 8, false>), dim3(p.grid), dim3(S * 64), 0, p.stream, p.jobs, p.jobb, p.walks,
                           p.runs, p.pieces, p.stf, p.out, p.n_cols, p.ld, p.m, inv, p.degenerate);
        if (p.built) *p.built = walk_word<T, S, NT, false, false>();
    }
}

// Instantiated shapes: S waves cover up to 256 S channels; G = 4 jobs per flush, the rows of an MFMA tile (a flush costs the
// same MFMAs for 1..4 jobs; the LDS -- 2304 B per wave and job -- leaves room for 17 waves per CU); 8 rows in flight.  The
// 3 widths x {plain, fused} x {float32, float16, bfloat16} = 18 builds, the six-group builds of 80 < m <= 96 and the
// two-source builds.
int launch_walk(const WParams& p, int dtype, int s, bool fused, LaunchError* err) {
    if (dtype == DCTFP_F16 || dtype == DCTFP_BF16) {
        const bool h = dtype == DCTFP_F16;
        if (s == 3) h ? launch_walk_impl<_Float16, 3, 5>(p, fused) : launch_walk_impl<bf16_t, 3, 5>(p, fused);
        else if (s == 5) h ? launch_walk_impl<_Float16, 5, 5>(p, fused) : launch_walk_impl<bf16_t, 5, 5>(p, fused);
        else h ? launch_walk_impl<_Float16, 10, 5>(p, fused) : launch_walk_impl<bf16_t, 10, 5>(p, fused);
        return DCTFP_OK;
    }
    if (p.m > 80) {   // six column groups (80 < m <= 96: PROST's [3, 85]): float32 rows
        if (p.two_source) return launch_fail(err, DCTFP_ERR_INVALID, "walk kernel: m = %d with two-source pieces", p.m);
        if (s == 3) launch_walk_impl<float, 3, 6>(p, fused);
        else if (s == 5) launch_walk_impl<float, 5, 6>(p, fused);
        else launch_walk_impl<float, 10, 6>(p, fused);
        return DCTFP_OK;
    }
    if (s == 3) launch_walk_impl<float, 3, 5>(p, fused);
    else if (s == 5) launch_walk_impl<float, 5, 5>(p, fused);
    else if (s == 10) launch_walk_impl<float, 10, 5>(p, fused);
    else return launch_fail(err, DCTFP_ERR_INVALID, "walk kernel: no build for %d waves", s);
    return DCTFP_OK;
}


}  // namespace dctfp_host
