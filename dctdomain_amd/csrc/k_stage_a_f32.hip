// stage_a_kernel, float32 rows.
#define DCTFP_TEMPLATES_ONLY
#include "launch.h"

namespace dctfp_host {

#include "k_stage_a.inc"

void launch_a_f32(const AParams& p, int vec, int n, int waves) {
    if (vec == 4) launch_a_n<float, 4>(p, n, waves);
    else launch_a_n<float, 1>(p, n, waves);
}

}  // namespace dctfp_host
