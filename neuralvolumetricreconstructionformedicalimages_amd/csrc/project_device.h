// project_device.h -- the pieces of the projection definition (include/naf_hip.h P1) that the forward
// projector, its transpose (both projector.hip) and the OS-SART subset kernels (sart.hip) must share to the bit: the
// volume, the clipped segment of a ray with its sample count, the sample positions, and the forward's sum over the samples.  The
// grid, the clip itself and the trilinear cell are voxel_grid.h's, which the Siddon pair and the volume sampler read too.
#pragma once

#include <cmath>
#include <cstdio>

#include "naf_host.h"
#include "voxel_grid.h"

namespace naf {

struct ProjVolume {
    const float *__restrict__ data;  // [n1, n2, n3] fp32, axis 0 = x, C-contiguous (the forward's input; unused by the transpose)
    VoxelGrid grid;
    float step;                      // target sample spacing in metres (accuracy * min dVoxel)
};

// voxel_cell of p.  Only called for points inside the box (midpoints of the clipped segment); the clamp keeps every p in bounds.
__device__ __forceinline__ uint64_t trilinear_cell(const ProjVolume &v, const float p[3], float w[3]) {
    float u[3];                      // dropped on purpose (the sampler's NaN hand-on needs it); gone once inlined
    return voxel_cell(v.grid, p, w, u);
}

// The part of a ray inside the box and [near, far], cut into n midpoint-rule samples.  t0, t1 and n are the quantities a float32
// restatement reproduces exactly (IEEE add / multiply / divide / sqrt, no contraction: build.py passes -ffp-contract=off).
struct RaySpan {
    float p0[3], d[3];               // p0 = o + t0 d
    float seg;                       // (t1 - t0) / n
    float len;                       // (t1 - t0) * |d|: the length of the segment in metres
    float weight;                    // len / n: what one sample contributes per unit of the volume's value
    uint32_t n;
};

enum SpanKind { kSpanEmpty = 0, kSpanOk = 1, kSpanUnbounded = 2 };   // unbounded: NaN / infinite ray, no loop of 2^24+ steps

__device__ __forceinline__ SpanKind ray_span(const ProjVolume &v, float4 a, float4 b, RaySpan &s) {
    const float o[3] = {a.x, a.y, a.z}, d[3] = {a.w, b.x, b.y};
    float t0, t1;
    if (!clip_ray(v.grid, o, d, b.z, b.w, t0, t1)) return kSpanEmpty;
    const float dn = sqrtf(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
    const float len = (t1 - t0) * dn;
    const float nf = fmaxf(1.0f, ceilf(len / v.step));
    if (!(nf < 16777216.0f)) return kSpanUnbounded;
    s.n = (uint32_t)nf;
    s.seg = (t1 - t0) / nf;
    s.len = len;
    s.weight = len / nf;
#pragma unroll
    for (int k = 0; k < 3; ++k) s.d[k] = d[k];
    clip_entry(t0, o, d, s.p0);
    return kSpanOk;
}

// Position of sample k, from k and not by increments: p0 + s_k d with s_k = (k + 1/2) seg, a single-rounding fma like p0 itself.
__device__ __forceinline__ void span_point(const RaySpan &s, uint32_t k, float p[3]) {
    const float t = ((float)k + 0.5f) * s.seg;
#pragma unroll
    for (int a = 0; a < 3; ++a) p[a] = fmaf(t, s.d[a], s.p0[a]);
}

// Value of the volume at p: trilinear, clamp-to-edge.  Only called for points inside the box (midpoints of the clipped segment).
__device__ __forceinline__ float sample_volume(const ProjVolume &v, const float p[3]) {
    float w[3];
    const float *__restrict__ q = v.data + trilinear_cell(v, p, w);
    const uint64_t sx = v.grid.next[0], sy = v.grid.next[1], sz = v.grid.next[2];
    const float c000 = q[0], c001 = q[sz], c010 = q[sy], c011 = q[sy + sz];
    const float c100 = q[sx], c101 = q[sx + sz], c110 = q[sx + sy], c111 = q[sx + sy + sz];
    const float c00 = c000 + w[2] * (c001 - c000), c01 = c010 + w[2] * (c011 - c010);
    const float c10 = c100 + w[2] * (c101 - c100), c11 = c110 + w[2] * (c111 - c110);
    const float c0 = c00 + w[1] * (c01 - c00), c1 = c10 + w[1] * (c11 - c10);
    return c0 + w[0] * (c1 - c0);
}

// Sum of the volume's value at the n samples of a span: position from k, not by increments; fp32 sum in k order.  The line
// integral is this sum times s.weight.
__device__ __forceinline__ float span_sum(const ProjVolume &v, const RaySpan &s) {
    float acc = 0.0f;
#pragma unroll 4
    for (uint32_t k = 0; k < s.n; ++k) {
        float p[3];
        span_point(s, k, p);
        acc += sample_volume(v, p);
    }
    return acc;
}

// Host: argument checks shared by the entry points, and the grid of a [n1, n2, n3] volume with voxel size dvoxel (HOST f32 [3]).
inline int make_volume(const char *who, const float *volume, uint32_t n1, uint32_t n2, uint32_t n3, const float *dvoxel, float step,
                       ProjVolume *v) {
    if (!volume || !dvoxel) return fail_who(who, "null pointer");
    if (n1 == 0 || n2 == 0 || n3 == 0) return fail_who(who, "zero volume dimension");
    if (!(step > 0.0f) || !std::isfinite(step)) return fail_who(who, "step must be > 0");
    for (int a = 0; a < 3; ++a) {
        if (!(dvoxel[a] > 0.0f) || !std::isfinite(dvoxel[a])) return fail_who(who, "voxel size must be > 0");
    }
    v->data = volume;
    v->grid = voxel_grid(n1, n2, n3, dvoxel);
    v->step = step;
    return NAF_OK;
}

constexpr uint32_t kProjTile = 16;   // scan kernels: 16 x 16 pixels per workgroup, 8 x 8 per wave

// Pixel of lane `t` (of 256) in tile (tx, ty) of the 2-D layout.
__device__ __forceinline__ void tile_pixel(uint32_t tx, uint32_t ty, uint32_t t, uint32_t &row, uint32_t &col) {
    const uint32_t wave = t >> 6, lane = t & 63u;
    row = ty * kProjTile + (wave >> 1) * 8u + (lane >> 3);
    col = tx * kProjTile + (wave & 1u) * 8u + (lane & 7u);
}

}  // namespace naf
