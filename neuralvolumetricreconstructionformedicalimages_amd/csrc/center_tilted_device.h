// center_tilted_device.h -- the per-pixel arithmetic of the tilted-axis (laminographic) centre and tilt search (include/naf_hip.h A5,
// DESIGN.md section 35): one slice z = const back-projected from filtered projections of a tilted parallel beam for several
// candidates (offset of the detector's column axis, tilt) at once.  Read by hipcc for csrc/center_tilted.hip and by a plain host
// compiler for tools/center_tilted_host_check.cpp.  Every float operation is one IEEE fp32 operation in the order written (the
// library and the host check are built with -ffp-contract=off).  Pixel coordinates and limits are those of center_device.h.
//
// Conventions, those of geometry.angle2pose for mode "parallel": at view angle a and tilt tau the detector's column axis is
// (-sin a, cos a, 0), its row axis (sin tau cos a, sin tau sin a, -cos tau), the rays run along (-cos tau cos a, -cos tau sin a,
// -sin tau).  For the point (x, y, z)
//   s = x cos a + y sin a,   t = y cos a - x sin a
//   k* = (t - ou - c) / du - 0.5 + W / 2                      the column coordinate under the candidate offset c
//   v* = sin tau * s - cos tau * z
//   r* = (v* - ov) / dv - 0.5 + H / 2                         the row coordinate under the candidate tilt tau
// Only `- c / du` and (sin tau, cos tau) depend on the candidate, so a view's term is (base, s) with
// base = (t - ou) (1 / du) + (W / 2 - 0.5), and a candidate costs one subtraction, two products and the four taps.
#pragma once

#include "center_device.h"

namespace naf {

struct CenterTiltedTerm {
    float base, s;
};

// The candidate-independent part of pixel (x, y) in the view with (ca, sa) = (cos a, sin a).  half_u = W / 2 - 0.5.
NAF_HD CenterTiltedTerm center_tilted_term(float x, float y, float ca, float sa, float ou, float inv_du, float half_u) {
    const float t = y * ca - x * sa;
    CenterTiltedTerm r;
    r.s = x * ca + y * sa;
    r.base = (t - ou) * inv_du + half_u;
    return r;
}

// The row coordinate of a point at in-plane depth s and height z under the tilt (st, ct) = (sin tau, cos tau).  half_v = H / 2 - 0.5.
NAF_HD float center_tilted_row(float s, float z, float st, float ct, float ov, float inv_dv, float half_v) {
    const float v = st * s - ct * z;
    return (v - ov) * inv_dv + half_v;
}

// The view's value at (row r, column k): linear along the columns in rows floor(r) and floor(r) + 1, then linear between the two;
// zero unless 0 <= floor(k) <= W - 2 and 0 <= floor(r) <= H - 2 (the end-point rule of center_sample on both axes; a NaN compares
// false and gives zero).  Reads view[floor(r) + {0, 1}][floor(k) + {0, 1}] only.
NAF_HD float center_tilted_sample(const float *view, uint32_t H, uint32_t W, float k, float r) {
    const float fk = floorf(k), fr = floorf(r);
    if (!(fk >= 0.0f && fk <= (float)((int32_t)W - 2))) return 0.0f;
    if (!(fr >= 0.0f && fr <= (float)((int32_t)H - 2))) return 0.0f;
    const float *row = view + (size_t)(uint32_t)fr * W + (uint32_t)fk;
    const float wk = k - fk, wr = r - fr;
    const float a0 = row[0], b0 = row[W];
    const float a = a0 + wk * (row[1] - a0);
    const float b = b0 + wk * (row[W + 1u] - b0);
    return a + wr * (b - a);
}

// One view added to the `count` <= kCenterGroup accumulators of a pixel at height z: cand[j] = (c_j / du, sin tau_j, cos tau_j).
NAF_HD void center_tilted_accumulate(float (&acc)[kCenterGroup], const float (&cand)[kCenterGroup][3], uint32_t count, const float *view,
                                     uint32_t H, uint32_t W, CenterTiltedTerm term, float z, float ov, float inv_dv, float half_v) {
    NAF_UNROLL
    for (uint32_t j = 0; j < kCenterGroup; ++j) {
        if (j < count) {
            const float r = center_tilted_row(term.s, z, cand[j][1], cand[j][2], ov, inv_dv, half_v);
            acc[j] = acc[j] + center_tilted_sample(view, H, W, term.base - cand[j][0], r);
        }
    }
}

// What a pixel stores for candidate j: the Jacobian cos tau_j of the laminographic back-projection times the sum over the views.
NAF_HD float center_tilted_result(float acc, float ct) { return ct * acc; }

}  // namespace naf
