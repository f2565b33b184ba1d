// center_device.h -- the per-pixel arithmetic of the centre-of-rotation search (include/naf_hip.h A5): one slice
// back-projected from filtered detector rows for several candidate offsets of the detector's column axis, and the two terms a slice
// is scored with.  Read by hipcc for csrc/center.hip and by a plain host compiler for tools/center_host_check.cpp.  Every float
// operation is one IEEE fp32 operation in the order written (the library and the host check are built with -ffp-contract=off).
//
// Conventions, those of filter.fan_angles: the detector's column axis is Rz(a) e_y, the source stands at DSO (cos a, sin a) and looks
// along -Rz(a) e_x.  For the pixel (x, y) and the view at angle a
//   s = x cos a + y sin a,   t = y cos a - x sin a
//   cone:      U = DSO - s,  u* = DSD t / U,  weight (DSO / U)^2
//   parallel:  u* = t,  weight 1
//   k* = (u* - ou - c) / du - 0.5 + W / 2            the column coordinate under the candidate offset c
// Only `- c / du` depends on the candidate, so a view's term is (base, weight) with base = (u* - ou) (1 / du) + (W / 2 - 0.5), and a
// candidate's column is base - c / du: one subtraction.
#pragma once

#include <cmath>
#include <cstdint>

#include "host_device.h"

namespace naf {

constexpr uint32_t kCenterMaxW = 16384u;                            // NAF_CENTER_MAX_W
constexpr uint32_t kCenterMaxK = 64u;                               // NAF_CENTER_MAX_K
constexpr uint32_t kCenterMaxN = 4096u;                             // NAF_CENTER_MAX_SIZE: pixels along one side of a slice
constexpr uint32_t kCenterGroup = 8u;                               // NAF_CENTER_GROUP: candidates a lane accumulates at once
constexpr uint32_t kCenterTile = 16u;                               // a workgroup's pixel tile is kCenterTile squared
constexpr uint32_t kCenterLdsFloats = 8192u;                        // filtered rows staged at once: 32 KB, or one row if wider

// Views staged together: as many whole rows as fit kCenterLdsFloats, at least one (a row has at most kCenterMaxW floats, 64 KB).
NAF_HD uint32_t center_chunk_views(uint32_t N, uint32_t W) {
    const uint32_t fit = kCenterLdsFloats / W;
    return fit < 1u ? 1u : (fit < N ? fit : N);
}

// The coordinate of pixel i of n along an axis of pitch d about the origin o.  0.5 (n - 1) is exact for n <= 2^24.
NAF_HD float center_coord(uint32_t i, uint32_t n, float d, float o) {
    const float steps = (float)i - 0.5f * (float)(n - 1u);
    return steps * d + o;
}

struct CenterTerm {
    float base, weight;
};

// The candidate-independent part of pixel (x, y) in the view with (ca, sa) = (cos a, sin a).  half = W / 2 - 0.5.
NAF_HD CenterTerm center_term(int parallel, float x, float y, float ca, float sa, float DSO, float DSD, float ou, float inv_du, float half) {
    const float t = y * ca - x * sa;
    CenterTerm r;
    float ustar;
    if (parallel) {
        ustar = t;
        r.weight = 1.0f;
    } else {
        const float s = x * ca + y * sa;
        const float U = DSO - s;
        ustar = DSD * t / U;
        const float m = DSO / U;
        r.weight = m * m;
    }
    r.base = (ustar - ou) * inv_du + half;
    return r;
}

// The row's value at column coordinate k: linear between floor(k) and floor(k) + 1, zero unless 0 <= floor(k) <= W - 2 (a NaN
// compares false and gives zero).  Reads row[floor(k)] and row[floor(k) + 1] only.
NAF_HD float center_sample(const float *row, uint32_t W, float k) {
    const float fl = floorf(k);
    if (!(fl >= 0.0f && fl <= (float)((int32_t)W - 2))) return 0.0f;
    const uint32_t i = (uint32_t)fl;
    const float w = k - fl;
    const float lo = row[i];
    const float d = row[i + 1u] - lo;
    return lo + w * d;
}

// One view added to the `count` <= kCenterGroup accumulators of a pixel: shift[j] = c_j / du.
NAF_HD void center_accumulate(float (&acc)[kCenterGroup], const float (&shift)[kCenterGroup], uint32_t count, const float *row, uint32_t W,
                              CenterTerm term) {
    NAF_UNROLL
    for (uint32_t j = 0; j < kCenterGroup; ++j) {
        if (j < count) {
            const float v = center_sample(row, W, term.base - shift[j]);
            acc[j] = acc[j] + term.weight * v;
        }
    }
}

// True when pixel (ix, iy) of an n x n slice of pitch (dx, dy) lies within r of the slice's centre; fp64, so that the numpy
// restatement decides the boundary alike.
NAF_HD bool center_in_mask(uint32_t ix, uint32_t iy, uint32_t n, double dx, double dy, double r) {
    const double mid = 0.5 * (double)(n - 1u);
    const double X = ((double)ix - mid) * dx, Y = ((double)iy - mid) * dy;
    return X * X + Y * Y <= r * r;
}

// A pixel's negativity term, -min(f, 0); a NaN stays one.
NAF_HD double center_negativity(float f) { return f < 0.0f ? -(double)f : (f != f ? (double)f : 0.0); }

// A forward difference's sharpness term.
NAF_HD double center_step(float a, float b) { return fabs((double)b - (double)a); }

}  // namespace naf
