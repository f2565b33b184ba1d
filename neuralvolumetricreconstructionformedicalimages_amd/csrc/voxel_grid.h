// voxel_grid.h -- the three definitions every operator that walks or samples a voxel volume shares to the bit (include/naf_hip.h
// P1, P2, P4-P8 and V4): the grid of a [n1, n2, n3] volume, the clip of a ray against its box, and the
// clamp-to-edge trilinear cell of a point.  It includes nothing of HIP, so the stand-alone checks of tools/*_host_check.cpp run
// these very functions on the CPU.  Everything is built with -ffp-contract=off: every fused multiply-add here is asked for by name,
// everything else is one IEEE fp32 operation in the order written.
#pragma once

#include <cmath>
#include <cstdint>

#include "host_device.h"

namespace naf {

// A kernel reads its grid from the argument segment with scalar loads that the compiler merges by adjacency, so the order of the
// fields decides a few scalar instructions of every prologue.  n ... inv_d is the run the trilinear kernels
// read; d, which of them only the gather's support reads, stands in front of it.
struct VoxelGrid {
    float d[3];                        // dvoxel_a
    uint32_t n[3];
    uint32_t imax[3];                  // max(n_a - 2, 0): the largest lower corner of a trilinear cell
    uint64_t stride[3];                // n2 * n3, n3, 1: axis 0 = x, C-contiguous
    uint64_t next[3];                  // stride of the upper corner: 0 when n_a == 1 (constant axis)
    float half[3];                     // h_a = fp32(n_a * dvoxel_a / 2), the product and the halving in double: one rounding
    float inv_d[3];                    // fp32(1 / dvoxel_a)
};

// imax and next from n and stride: the builder's, and of a kernel that was handed only the fields it reads (SiddonPair::Grid).
NAF_HD void voxel_grid_corners(VoxelGrid &g) {
    NAF_UNROLL
    for (int a = 0; a < 3; ++a) {
        g.imax[a] = g.n[a] >= 2u ? g.n[a] - 2u : 0u;
        g.next[a] = g.n[a] > 1u ? g.stride[a] : 0u;
    }
}

// Host: the grid of a [n1, n2, n3] volume with voxel size dvoxel (HOST f32 [3]).  Arguments are checked by the caller.
inline VoxelGrid voxel_grid(uint32_t n1, uint32_t n2, uint32_t n3, const float *dvoxel) {
    VoxelGrid g;
    const uint32_t n[3] = {n1, n2, n3};
    g.stride[0] = (uint64_t)n2 * n3;
    g.stride[1] = n3;
    g.stride[2] = 1;
    for (int a = 0; a < 3; ++a) {
        g.n[a] = n[a];
        g.half[a] = (float)((double)n[a] * (double)dvoxel[a] / 2.0);
        g.inv_d[a] = 1.0f / dvoxel[a];
        g.d[a] = dvoxel[a];
    }
    voxel_grid_corners(g);
    return g;
}

// The part [t0, t1] of the ray o + t d (d un-normalised) inside the box and [near, far], by slabs: IEEE subtract, divide and
// compare, axis by axis.  False when there is none (a NaN lands here too).
NAF_HD bool clip_ray(const VoxelGrid &g, const float o[3], const float d[3], float near, float far, float &t0, float &t1) {
    t0 = near;
    t1 = far;
    NAF_UNROLL
    for (int k = 0; k < 3; ++k) {
        if (d[k] == 0.0f) {
            if (o[k] < -g.half[k] || o[k] > g.half[k]) t1 = -INFINITY;    // parallel to the slab and outside it
            continue;
        }
        const float ta = (-g.half[k] - o[k]) / d[k], tb = (g.half[k] - o[k]) / d[k];
        const float lo = ta < tb ? ta : tb, hi = ta < tb ? tb : ta;
        t0 = lo > t0 ? lo : t0;
        t1 = hi < t1 ? hi : t1;
    }
    return t1 > t0;
}

// Where the clipped segment begins: p0 = o + t0 d, each coordinate a single-rounding fma.  A cone ray's origin is ~1 m from the
// volume, and o + t d with an fp32 t ~ 1 would place every point ~6e-8 m off its spot.  Callers form it after their early returns.
NAF_HD void clip_entry(float t0, const float o[3], const float d[3], float p0[3]) {
    NAF_UNROLL
    for (int k = 0; k < 3; ++k) p0[k] = fmaf(t0, d[k], o[k]);
}

// The trilinear cell of p, clamp-to-edge: the element offset of its lower corner (64-bit: a 1024^3 volume is 4 GiB) and the weights
// w_a of the upper corners.  Per axis, u_a = (p_a + h_a) * r_a - 1/2 (one add, one multiply, one subtract) is handed back as it is
// and then clamped to [0, n_a - 1] on the float, before any conversion: fmaxf / fminf return the other operand for a NaN, so a NaN
// becomes 0 and +-inf the nearer edge, and no index can leave the volume whatever p holds.  i_a = min((uint32)u_a, imax_a) (u >= 0:
// the truncation is the floor) and w_a = u_a - (float)i_a, exact: the two are less than 2 apart and below 2^24.
NAF_HD uint64_t voxel_cell(const VoxelGrid &g, const float p[3], float w[3], float u[3]) {
    uint64_t base = 0;
    NAF_UNROLL
    for (int a = 0; a < 3; ++a) {
        u[a] = (p[a] + g.half[a]) * g.inv_d[a] - 0.5f;
        const float c = fminf(fmaxf(u[a], 0.0f), (float)(g.n[a] - 1u));
        const uint32_t t = (uint32_t)c;
        const uint32_t i = t < g.imax[a] ? t : g.imax[a];
        w[a] = c - (float)i;
        base += (uint64_t)i * g.stride[a];
    }
    return base;
}

}  // namespace naf
