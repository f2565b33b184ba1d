// tv_device.h -- the per-voxel arithmetic of the 3-D total variation and its gradient (include/naf_hip.h V2).
// It includes nothing of HIP, so a host compiler reads it too: tools/tv_host_check.cpp runs these very functions on the CPU under
// AddressSanitizer / UBSan and compares them with the float64 oracle of the tests.  Every operation is a single IEEE fp32 add,
// multiply, divide or square root in the order written (the library and the host check are built with -ffp-contract=off).
#pragma once

#include <cmath>

#include "host_device.h"

namespace naf {

// The 13 values voxel v's gradient depends on.  lo[a] = f[v - e_a], hi[a] = f[v + e_a], diag[a][b] = f[v + e_a - e_b] (a != b).
// has_lo[a] = v_a > 0, has_hi[a] = v_a < n_a - 1; a value whose flag (both flags for a diagonal) is false is never used.
struct TvStencil {
    float c;
    float lo[3], hi[3];
    float diag[3][3];
    bool has_lo[3], has_hi[3];
};

// m = sqrt(eps + d0^2 + d1^2 + d2^2), the squares added in axis order.
NAF_HD float tv_magnitude(float d0, float d1, float d2, float eps) {
    float s = d0 * d0;
    s = s + d1 * d1;
    s = s + d2 * d2;
    return sqrtf(eps + s);
}

// g[v] = (D_0 + D_1 + D_2) f[v] / m[v]  -  sum_a [v_a < n_a - 1] D_a f[v + e_a] / m[v + e_a], the three terms subtracted in axis
// order; *m_out = m[v].  Selects, not products, drop the absent neighbours: whatever lies in their slots has no effect.
NAF_HD float tv_point(const TvStencil &s, float eps, float *m_out) {
    float d[3];
    NAF_UNROLL
    for (int a = 0; a < 3; ++a) d[a] = s.has_lo[a] ? s.c - s.lo[a] : 0.0f;
    const float m = tv_magnitude(d[0], d[1], d[2], eps);
    *m_out = m;
    float g = ((d[0] + d[1]) + d[2]) / m;
    NAF_UNROLL
    for (int a = 0; a < 3; ++a) {
        if (!s.has_hi[a]) continue;
        float e[3];                                  // the backward differences of the neighbour u = v + e_a
        NAF_UNROLL
        for (int b = 0; b < 3; ++b) {
            if (b == a) e[b] = s.hi[a] - s.c;        // u_a = v_a + 1 > 0
            else e[b] = s.has_lo[b] ? s.hi[a] - s.diag[a][b] : 0.0f;
        }
        g = g - e[a] / tv_magnitude(e[0], e[1], e[2], eps);
    }
    return g;
}

// One normalised descent step: scale = step / ||g||_2 with the norm rounded to fp32 from the fp64 sum of squares; a sum that is
// not > 0 (zero, or NaN) gives scale 0 and the volume stays as it is.
NAF_HD float tv_step_scale(double sum_g2, float step) {
    return sum_g2 > 0.0 ? step / (float)sqrt(sum_g2) : 0.0f;
}

NAF_HD float tv_step_apply(float c, float g, float scale) { return c - scale * g; }

}  // namespace naf
