// The launch ladder of stage_a_kernel (storage type x n x channels per lane x waves x rows in flight), shared by the four units
// k_stage_a_{f32,f64,f16,bf16}.hip: one unit per storage type only so that their device code compiles side by side (the stage-A
// instantiations are a third of the library's; build_ext.py).  Included inside namespace dctfp_host, after launch.h.
template <typename T, int N, int VEC, int WAVES, int UNROLL, bool FUSED>
void launch_a_build(const AParams& p) {
    static const InvTab<N> inv = make_inv<N>();
    hipLaunchKernelGGL((stage_a_kernel<T, N, VEC, WAVES, UNROLL, FUSED>), dim3(p.grid), dim3(WAVES * 64), 0, p.stream,
                       p.jobs, p.walks, p.pieces, p.yprime, p.job_bytes, p.packed, p.n_cols, p.ld, p.ldy, p.n_slabs,
                       inv, p.degenerate);
    *p.built = stage_a_word<T, N, VEC, WAVES, UNROLL, FUSED>(p.packed != 0, false);
}

// 4 rows in flight, plain and fused
template <typename T, int N, int VEC, int WAVES>
void launch_a_impl(const AParams& p) {
    if (p.fused) launch_a_build<T, N, VEC, WAVES, 4, true>(p);
    else launch_a_build<T, N, VEC, WAVES, 4, false>(p);
}

// n = 2, 3: the builds dctfp_quantize's choice of `waves` can reach -- 2, 4 or 8 waves (at most 4 at 8 channels per lane), and
// at 4 channels per lane 16 waves, with 8 rows in flight unless the walks are fused (a call that cannot fill the chip).
template <typename T, int N, int VEC>
void launch_a_cfg(const AParams& p, int waves) {
    if constexpr (VEC == 4) {
        if (waves == 16) {
            if (p.fused) launch_a_build<T, N, VEC, 16, 4, true>(p);
            else launch_a_build<T, N, VEC, 16, 8, false>(p);
            return;
        }
    }
    if constexpr (VEC != 8) {
        if (waves == 8) return launch_a_impl<T, N, VEC, 8>(p);
    }
    if (waves == 2) launch_a_impl<T, N, VEC, 2>(p);
    else launch_a_impl<T, N, VEC, 4>(p);
}

template <typename T, int VEC>
void launch_a_n(const AParams& p, int n, int waves) {
    switch (n) {
        case 2: launch_a_cfg<T, 2, VEC>(p, waves); break;
        case 3: launch_a_cfg<T, 3, VEC>(p, waves); break;
        case 4: launch_a_impl<T, 4, VEC, 4>(p); break;
        case 5: launch_a_impl<T, 5, VEC, 4>(p); break;
        case 6: launch_a_impl<T, 6, VEC, 4>(p); break;
        case 7: launch_a_impl<T, 7, VEC, 4>(p); break;
        default: launch_a_impl<T, 8, VEC, 4>(p); break;
    }
}
