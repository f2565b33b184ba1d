// tvprox_device.h -- the per-voxel arithmetic of the TV proximal map (include/naf_hip.h V3): the adjoint
// D^T p at a voxel, the primal point u = P_C(b - lambda D^T p), and one dual update of the fast gradient projection.  It includes
// nothing of HIP, so a host compiler reads it too: tools/tvprox_host_check.cpp runs these very functions on the CPU under
// AddressSanitizer / UBSan and compares them with the float64 oracle of the tests.  Every operation is a single IEEE fp32 add,
// subtract, multiply, divide or square root in the order written (the library and the host check are built with
// -ffp-contract=off).  Selects, not products, apply the masks: whatever lies in a masked slot, a NaN included, has no effect.
#pragma once

#include <cmath>

#include "host_device.h"

namespace naf {

// The dual step 1 / (12 lambda): 12 >= ||D D^T|| in three dimensions.  Formed once on the host and passed to the kernel.
NAF_HD float tvprox_dual_step(float lambda) { return 1.0f / (12.0f * lambda); }

// (D^T p)[v] = sum_a ([v_a > 0] p_a[v] - [v_a < n_a - 1] p_a[v + e_a]), the three terms added in axis order.
// lo[a] = p_a[v], hi[a] = p_a[v + e_a]; has_lo[a] = v_a > 0, has_hi[a] = v_a < n_a - 1.
NAF_HD float tvprox_adjoint(const float lo[3], const float hi[3], const bool has_lo[3], const bool has_hi[3]) {
    float t[3];
    NAF_UNROLL
    for (int a = 0; a < 3; ++a) t[a] = (has_lo[a] ? lo[a] : 0.0f) - (has_hi[a] ? hi[a] : 0.0f);
    return (t[0] + t[1]) + t[2];
}

// u = P_C(b - lambda * dt), dt = (D^T p)[v].  P_C clamps at 0 with a compare, so a NaN stays NaN.
NAF_HD float tvprox_primal(float b, float dt, float lambda, bool nonneg) {
    const float u = b - lambda * dt;
    return (nonneg && u < 0.0f) ? 0.0f : u;
}

// One dual update at voxel v.  u = u[v], u_lo[a] = u[v - e_a], r[a] = r_a[v], p_old[a] = p_{k-1,a}[v], step = tvprox_dual_step:
//   q_a = [v_a > 0] (r_a + step * (u - u_lo[a]))          (a masked component is 0 and does not enter the norm)
//   p_a = q_a / max(1, sqrt(q_0^2 + q_1^2 + q_2^2))       (squares added in axis order)
//   r_next_a = p_a + momentum * (p_a - [v_a > 0] p_old_a)
NAF_HD void tvprox_dual(float u, const float u_lo[3], const float r[3], const float p_old[3], const bool has_lo[3], float step,
                        float momentum, float p[3], float r_next[3]) {
    float q[3];
    NAF_UNROLL
    for (int a = 0; a < 3; ++a) q[a] = has_lo[a] ? r[a] + step * (u - u_lo[a]) : 0.0f;
    float s = q[0] * q[0];
    s = s + q[1] * q[1];
    s = s + q[2] * q[2];
    const float n = sqrtf(s);
    const float d = n > 1.0f ? n : 1.0f;
    NAF_UNROLL
    for (int a = 0; a < 3; ++a) {
        p[a] = q[a] / d;
        r_next[a] = p[a] + momentum * (p[a] - (has_lo[a] ? p_old[a] : 0.0f));
    }
}

}  // namespace naf
