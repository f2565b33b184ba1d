// volume_sample_device.h -- the per-point arithmetic of the volume sampler (include/naf_hip.h V4): the
// trilinear cell of a world point, the value there, and the counter-based draw of a point in a box.  It includes nothing of HIP, so a
// host compiler reads it too: tools/volume_sample_host_check.cpp runs these very functions on the CPU under AddressSanitizer / UBSan
// over heap volumes of exactly n1 n2 n3 floats and compares them with a float64 evaluation.  Every operation is a single IEEE fp32
// operation in the order written (the library and the host check are built with -ffp-contract=off); every fused multiply-add is
// asked for by name.
//
// The cell and its weights are voxel_grid.h's (voxel_cell: u = (p_a + h_a) r_a - 1/2, clamped on the float before any conversion,
// so no index can leave the volume whatever p holds); a NaN u gives w = NaN instead.  The eight corners c_xyz = f[i_0 + x, i_1 + y,
// i_2 + z] (an axis of one voxel has no upper corner: its x is dropped and its w is 0) are loaded before the first of them is used,
// then seven interpolations lerp(a, b, w) = fma(w, b, fma(-w, a, a)), two fmas each
// (a - w a, then + w b: w = 0 returns a's bits and w = 1 returns b's, which a + w (b - a) does not):
//   along axis 2:  c_00 = lerp(c_000, c_001, w_2), c_01 = lerp(c_010, c_011, w_2), c_10 = lerp(c_100, c_101, w_2), c_11 = lerp(c_110, c_111, w_2)
//   along axis 1:  c_0 = lerp(c_00, c_01, w_1), c_1 = lerp(c_10, c_11, w_1)
//   along axis 0:  result = lerp(c_0, c_1, w_0)
// A point whose three u are whole numbers therefore returns that voxel's bits, the last voxel of an axis (i = n_a - 2, w = 1) included.
#pragma once

#include <cmath>
#include <cstdint>

#include "mix32.h"
#include "voxel_grid.h"

namespace naf {

// voxel_cell of p with V4's contract for a NaN: a coordinate whose u is NaN gets that NaN as its weight.  It never chose an index:
// voxel_cell clamped it to 0 first.
NAF_HD uint64_t sample_cell(const VoxelGrid &g, const float p[3], float w[3]) {
    float u[3];
    const uint64_t base = voxel_cell(g, p, w, u);
    NAF_UNROLL
    for (int a = 0; a < 3; ++a) w[a] = u[a] != u[a] ? u[a] : w[a];
    return base;
}

NAF_HD float sample_lerp(float a, float b, float w) { return fmaf(w, b, fmaf(-w, a, a)); }

// The eight corners of the cell at `base`, all loaded before the first is used (c[4 x + 2 y + z]).
NAF_HD void sample_corners(const float *f, const VoxelGrid &g, uint64_t base, float c[8]) {
    const float *q = f + base;
    const uint64_t sx = g.next[0], sy = g.next[1], sz = g.next[2];
    c[0] = q[0];
    c[1] = q[sz];
    c[2] = q[sy];
    c[3] = q[sy + sz];
    c[4] = q[sx];
    c[5] = q[sx + sz];
    c[6] = q[sx + sy];
    c[7] = q[sx + sy + sz];
}

NAF_HD float sample_blend(const float c[8], const float w[3]) {
    const float c00 = sample_lerp(c[0], c[1], w[2]), c01 = sample_lerp(c[2], c[3], w[2]);
    const float c10 = sample_lerp(c[4], c[5], w[2]), c11 = sample_lerp(c[6], c[7], w[2]);
    const float c0 = sample_lerp(c00, c01, w[1]), c1 = sample_lerp(c10, c11, w[1]);
    return sample_lerp(c0, c1, w[0]);
}

// Value of the volume at p: trilinear, clamp-to-edge; NaN when a coordinate of p is NaN.
NAF_HD float sample_point(const float *f, const VoxelGrid &g, const float p[3]) {
    float w[3], c[8];
    const uint64_t base = sample_cell(g, p, w);
    sample_corners(f, g, base, c);
    return sample_blend(c, w);
}

// ---- the draw: point i of step `step` under `seed`, uniform in the box [lo, hi] -----------------------------------------------------
// 32 random bits of (seed, step, i, axis): three rounds of the finaliser, each keyed by the next word.  No state: equal arguments
// give equal bits.  All arithmetic is uint32 with wrap-around.
NAF_HD uint32_t sample_hash(uint64_t seed, uint32_t step, uint32_t i, uint32_t axis) {
    uint32_t h = mix32((uint32_t)seed ^ (i * 0x9e3779b1u));
    h = mix32(h ^ (uint32_t)(seed >> 32) ^ (step * 0x85ebca77u) ^ 0x27d4eb2fu);
    return mix32(h ^ ((axis + 1u) * 0xc2b2ae3du));
}

// 32 bits -> [0, 1): the top 24 bits times 2^-24 (both exact in fp32).
NAF_HD float sample_unit(uint32_t bits) { return (float)(bits >> 8) * (1.0f / 16777216.0f); }

// p_a = min(lo_a + r_a * (hi_a - lo_a), hi_a): one subtract, one multiply, one add, one minimum; lo <= p <= hi for lo <= hi.
NAF_HD void sample_draw(uint64_t seed, uint32_t step, uint32_t i, const float lo[3], const float hi[3], float p[3]) {
    NAF_UNROLL
    for (uint32_t a = 0; a < 3u; ++a) {
        const float r = sample_unit(sample_hash(seed, step, i, a));
        const float e = hi[a] - lo[a];
        const float s = r * e;
        p[a] = fminf(lo[a] + s, hi[a]);
    }
}

}  // namespace naf
