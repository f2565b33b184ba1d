// backproject_gather_device.h -- the enumeration of the gather-form transpose (include/naf_hip.h P5): which
// pixels of a view can reach a voxel (its footprint rectangle), which samples of such a pixel's ray can (a k-range), and the weight
// a sample's trilinear cell gives the voxel.  The weights themselves come from project_device.h (ray_span, span_point,
// trilinear_cell), the code the forward projector and the scatter run; this header only decides where to look, so all it has to be
// is a SUPERSET of the (ray, sample) pairs to which the scatter gives the voxel a non-zero weight.
// The grid is voxel_grid.h's VoxelGrid, the one the scatter's ProjVolume holds.  It includes nothing of HIP, so a host compiler reads
// it too: tools/gather_host_check.cpp runs these very functions on the CPU under AddressSanitizer / UBSan against a float64 enumeration.
#pragma once

#include <cmath>
#include <cstdint>

#include "voxel_grid.h"

namespace naf {

struct GatherDetector {              // the fields of RayGeo that place a pixel
    uint32_t W, H;
    float du, dv, ou, ov, DSD;
    int parallel;
};

struct GatherRect {                  // pixels [row0, row1) x [col0, col1); empty when row0 >= row1 or col0 >= col1
    uint32_t row0, row1, col0, col1;
};

// Every margin below is a multiple of kGatherEps = 2^-19 = 32 x 2^-24, i.e. 32 fp32 unit roundoffs u of the largest coordinate that
// enters the quantity.  DESIGN.md section 17 counts the roundings each has to cover: 15 u for the support box, 13 u for a projected
// corner, 4 u for a pixel index.
constexpr float kGatherEps = 1.0f / 524288.0f;

// Support box of voxel i: a sample at p gives the voxel a non-zero weight only if, on every axis, its clamped grid coordinate
// u_a = (p_a + h_a) / d_a - 1/2 lies in (i_a - 1, i_a + 1), that is p_a in (c_a - d_a, c_a + d_a) around the voxel centre c_a.
// Clamp-to-edge gives an edge voxel the whole outer half cell, so the box reaches the volume's face there (an axis of one voxel: both
// faces).  Widened by kGatherEps (h_a + d_a): the fp32 error of c_a, of the kernel's u_a and of the sample position.
NAF_HD void gather_support(const VoxelGrid &g, const uint32_t i[3], float lo[3], float hi[3]) {
    for (int a = 0; a < 3; ++a) {
        const float m = kGatherEps * (g.half[a] + g.d[a]);
        const float below = ((float)i[a] - 0.5f) * g.d[a] - g.half[a], above = ((float)i[a] + 1.5f) * g.d[a] - g.half[a];
        lo[a] = (i[a] == 0u ? -g.half[a] : below) - m;
        hi[a] = (i[a] + 1u >= g.n[a] ? g.half[a] : above) + m;
    }
}

// Smallest / largest pixel index whose centre, at (index + 1/2 - n / 2) * pitch + offset, can lie in [umin, umax] -> [first, last)
// clipped to [0, n).  `margin` is in pixels.
NAF_HD void gather_pixel_range(float umin, float umax, float pitch, float offset, uint32_t n, uint32_t &first, uint32_t &last) {
    const float shift = (float)n / 2.0f - 0.5f;
    const float a = (umin - offset) / pitch + shift, b = (umax - offset) / pitch + shift;
    const float margin = kGatherEps * ((float)n + (fabsf(offset) + fmaxf(fabsf(umin), fabsf(umax))) / fabsf(pitch));
    const float f = ceilf(fminf(a, b) - margin), l = floorf(fmaxf(a, b) + margin);
    first = last = 0u;
    if (!(l >= 0.0f) || !(f <= (float)n - 1.0f) || !(f <= l)) return;          // off the detector, or no centre inside (or NaN)
    first = f > 0.0f ? (uint32_t)f : 0u;
    last = l < (float)n - 1.0f ? (uint32_t)l + 1u : n;
}

// Footprint of the box [lo, hi] on the detector of the view with pose P (3x4 row-major [R | t], fp32): the inverse of make_ray's
// map.  A ray of pixel (u, v) is t + s R (u / DSD, v / DSD, 1) (cone) or t + R (u, v, s) (parallel); with q = R^T (p - t) a point p
// lies on the ray of u = q_x / q_z DSD, v = q_y / q_z DSD (cone) or u = q_x, v = q_y (parallel).  The rays that meet a convex box
// project inside the convex hull of its eight projected corners, so the bounding rectangle of those serves.  Each corner's u, v is
// widened by its fp32 error bound (section 17): kGatherEps S / q_z (DSD + |u|) for a cone, kGatherEps S for a parallel beam,
// S = sum_a |p_a - t_a|.  A corner at or behind the source plane (q_z <= 0: no bound exists) gives the whole detector.
NAF_HD GatherRect gather_footprint(const float lo[3], const float hi[3], const float *P, const GatherDetector &det) {
    float umin = INFINITY, umax = -INFINITY, vmin = INFINITY, vmax = -INFINITY;
    bool whole = false;
    for (int c = 0; c < 8; ++c) {
        const float e[3] = {((c & 4) ? hi[0] : lo[0]) - P[3], ((c & 2) ? hi[1] : lo[1]) - P[7], ((c & 1) ? hi[2] : lo[2]) - P[11]};
        const float S = fabsf(e[0]) + fabsf(e[1]) + fabsf(e[2]);
        const float qx = (P[0] * e[0] + P[4] * e[1]) + P[8] * e[2];
        const float qy = (P[1] * e[0] + P[5] * e[1]) + P[9] * e[2];
        float u = qx, v = qy, ru = kGatherEps * S, rv = ru;
        if (!det.parallel) {
            const float qz = (P[2] * e[0] + P[6] * e[1]) + P[10] * e[2];
            if (!(qz > kGatherEps * S)) whole = true;
            u = qx / qz * det.DSD;
            v = qy / qz * det.DSD;
            ru = kGatherEps * S / qz * (det.DSD + fabsf(u));
            rv = kGatherEps * S / qz * (det.DSD + fabsf(v));
        }
        umin = fminf(umin, u - ru);
        umax = fmaxf(umax, u + ru);
        vmin = fminf(vmin, v - rv);
        vmax = fmaxf(vmax, v + rv);
    }
    GatherRect r;
    if (whole || !(umin <= umax) || !(vmin <= vmax)) {                         // (the negations also catch a NaN)
        r.row0 = r.col0 = 0u;
        r.row1 = det.H;
        r.col1 = det.W;
        return r;
    }
    gather_pixel_range(umin, umax, det.du, det.ou, det.W, r.col0, r.col1);
    gather_pixel_range(vmin, vmax, det.dv, det.ov, det.H, r.row0, r.row1);
    return r;
}

// Samples of a span (p0, d, seg, n of RaySpan: sample k at p0 + (k + 1/2) seg d) that can lie in the box [lo, hi] -> k in
// [k_lo, k_hi], false when there is none.  The slab test of ray_span on the box, with d[a] == 0 handled the same way; the interval
// of t / seg - 1/2 is widened by one sample to either side, which covers the rounding of the two divisions and of span_point's
// (k + 1/2) seg (relative 2^-23 of a value below n < 2^24; the box already carries the margin for positions).
NAF_HD bool gather_k_range(const float lo[3], const float hi[3], const float p0[3], const float d[3], float seg, uint32_t n,
                           uint32_t &k_lo, uint32_t &k_hi) {
    float t0 = 0.0f, t1 = INFINITY;
    for (int a = 0; a < 3; ++a) {
        if (d[a] == 0.0f) {
            if (p0[a] < lo[a] || p0[a] > hi[a]) return false;
            continue;
        }
        const float ta = (lo[a] - p0[a]) / d[a], tb = (hi[a] - p0[a]) / d[a];
        const float first = ta < tb ? ta : tb, last = ta < tb ? tb : ta;
        t0 = first > t0 ? first : t0;
        t1 = last < t1 ? last : t1;
    }
    if (!(t1 >= t0)) return false;
    const float top = (float)(n - 1u);
    const float a = floorf(t0 / seg - 0.5f) - 1.0f, b = ceilf(t1 / seg - 0.5f) + 1.0f;
    if (!(a <= top) || !(b >= 0.0f)) return false;
    k_lo = a > 0.0f ? (uint32_t)a : 0u;
    k_hi = b < top ? (uint32_t)b : n - 1u;
    return true;
}

// Weight the cell at `cell` (offset of its lower corner, trilinear_cell's) with upper-corner weights w gives the voxel at offset
// `voxel`: the scatter's (x[cx] * y[cy]) * z[cz] for the corner c whose offset cx next[0] + cy next[1] + cz next[2] is
// voxel - cell, 0 if there is none.  An upper corner on a constant axis (next[a] == 0) does not exist.  The offsets of the existing
// corners are distinct and no voxel other than a corner has one of them (section 17), so at most one term is taken.
NAF_HD float gather_corner_weight(uint64_t voxel, uint64_t cell, const uint64_t next[3], const float w[3]) {
    const uint64_t diff = voxel - cell;                                        // wraps for a voxel below the cell: matches nothing
    const float x[2] = {1.0f - w[0], w[0]}, y[2] = {1.0f - w[1], w[1]}, z[2] = {1.0f - w[2], w[2]};
    float out = 0.0f;
    for (int c = 0; c < 8; ++c) {
        const int cx = c >> 2, cy = (c >> 1) & 1, cz = c & 1;
        if ((cx && !next[0]) || (cy && !next[1]) || (cz && !next[2])) continue;
        if (diff == (uint64_t)cx * next[0] + (uint64_t)cy * next[1] + (uint64_t)cz * next[2]) out = (x[cx] * y[cy]) * z[cz];
    }
    return out;
}

}  // namespace naf
