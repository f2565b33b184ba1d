// siddon_device.h -- the per-ray traversal of the ray-voxel intersection ("Siddon") projector (include/naf_hip.h P6, DESIGN.md
// section 20): the volume is constant inside a voxel, and a ray's integral is the sum over voxels of value x chord length.  It
// includes nothing of HIP, so a host compiler reads it too: tools/siddon_host_check.cpp walks these very functions on the CPU under
// AddressSanitizer / UBSan over heap volumes of exactly n1 n2 n3 floats.  The library and the host check are built with
// -ffp-contract=off: every fused multiply-add here is asked for by name, everything else is one IEEE operation in the order written.
//
// INVARIANT.  Before the loop the entry and the exit voxel of the clipped segment are fixed per axis as integers i0_a, i1_a, each
// clamped to [0, n_a - 1].  Axis a then has rem_a = |i1_a - i0_a| plane crossings left, its index moves by sign(i1_a - i0_a) per
// crossing, and the loop makes exactly rem_x + rem_y + rem_z + 1 steps (rounded up to whole groups of kSiddonGroup; the walk's state
// after the last step is a fixed point that yields zero-length segments of the exit voxel).  Float comparisons only choose WHICH axis
// with rem_a > 0 crosses next; an axis with rem_a == 0 is never chosen, whatever the floats hold (NaN included), so every index
// stays between i0_a and i1_a, every load is inside the volume, and the trip count is an integer known before the first step.
// A rounding error can only reorder crossings that nearly coincide or shorten a segment; it cannot move an index out of range or
// extend the loop.
#pragma once

#include <cmath>
#include <cstdint>

#include "voxel_grid.h"

namespace naf {

constexpr uint32_t kSiddonGroup = 4;   // steps whose loads are issued together, before the first of them is used

// The clipped segment of a ray: clip_ray's and clip_entry's, and what the walk needs of it.
struct SiddonSpan {
    float p0[3], d[3];                 // p0 = clip_entry(t0, o, d)
    float s_end;                       // t1 - t0
    float dn;                          // |d|
};

enum SiddonKind { kSiddonEmpty = 0, kSiddonOk = 1, kSiddonNotFinite = 2 };

NAF_HD bool siddon_finite(float x) { return (x - x) == 0.0f; }   // false for NaN and +-infinity

NAF_HD SiddonKind siddon_span(const VoxelGrid &g, const float o[3], const float d[3], float near, float far, SiddonSpan &s) {
    float t0, t1;
    if (!clip_ray(g, o, d, near, far, t0, t1)) return kSiddonEmpty;
    s.dn = sqrtf(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
    s.s_end = t1 - t0;
    bool finite = siddon_finite(s.s_end);
    clip_entry(t0, o, d, s.p0);
    NAF_UNROLL
    for (int k = 0; k < 3; ++k) {
        s.d[k] = d[k];
        finite = finite && siddon_finite(s.p0[k]);
    }
    return finite ? kSiddonOk : kSiddonNotFinite;
}

// Voxel index of coordinate p on axis a, clamped to [0, n_a - 1].  The clamp is made on the float (fmaxf / fminf drop a NaN), so the
// conversion to an integer is defined for every input.
NAF_HD int32_t siddon_index(const VoxelGrid &g, int a, float p) {
    float u = floorf((p + g.half[a]) * g.inv_d[a]);
    u = fminf(fmaxf(u, 0.0f), (float)(g.n[a] - 1u));
    return (int32_t)u;
}

// Parameter s (from p0) at which the ray crosses plane m of axis a: from m itself, never by increments.
NAF_HD float siddon_crossing(const VoxelGrid &g, const SiddonSpan &r, int a, int32_t m) {
    return (fmaf((float)m, g.d[a], -g.half[a]) - r.p0[a]) / r.d[a];
}

// State of a walk: the current voxel (as a 64-bit element offset), the crossings left per axis and each axis' next crossing.
struct SiddonWalk {
    int32_t idx[3], dir[3];            // current index; +1 / -1 / 0 per crossing
    uint32_t rem[3];                   // crossings left
    int64_t jump[3];                   // dir_a * stride_a
    float next[3];                     // parameter of the next crossing (unused once rem_a == 0)
    uint64_t offset;
    float s_prev;
};

// Returns the number of steps: rem_x + rem_y + rem_z + 1.
NAF_HD uint32_t siddon_begin(const VoxelGrid &g, const SiddonSpan &r, SiddonWalk &w) {
    uint32_t steps = 1;
    w.offset = 0;
    w.s_prev = 0.0f;
    NAF_UNROLL
    for (int a = 0; a < 3; ++a) {
        const int32_t i0 = siddon_index(g, a, r.p0[a]);
        const int32_t i1 = siddon_index(g, a, fmaf(r.s_end, r.d[a], r.p0[a]));
        w.idx[a] = i0;
        w.dir[a] = i1 > i0 ? 1 : (i1 < i0 ? -1 : 0);       // 0 for d_a == 0 and for n_a == 1: both ends clamp to one index
        w.rem[a] = (uint32_t)(i1 > i0 ? i1 - i0 : i0 - i1);
        w.jump[a] = (int64_t)w.dir[a] * (int64_t)g.stride[a];
        w.next[a] = siddon_crossing(g, r, a, i0 + (w.dir[a] > 0 ? 1 : 0));
        w.offset += (uint64_t)i0 * g.stride[a];
        steps += w.rem[a];
    }
    return steps;
}

// One step: the offset of the current voxel and the length (in s) of the segment inside it, then the move across the nearest plane.
// With no crossing left the segment runs to s_end, and every later step is a zero-length segment of the same voxel.
NAF_HD void siddon_step(const VoxelGrid &g, const SiddonSpan &r, SiddonWalk &w, uint64_t &offset, float &ds) {
    const float dx = r.d[0], dy = r.d[1], dz = r.d[2];
    const bool ax = w.rem[0] > 0u, ay = w.rem[1] > 0u, az = w.rem[2] > 0u;
    // the smallest of the next crossings; an exhausted axis counts as +infinity: it is never chosen (integer tests gate every choice)
    const bool px = ax && (!ay || w.next[0] <= w.next[1]) && (!az || w.next[0] <= w.next[2]);
    const bool py = !px && ay && (!az || w.next[1] <= w.next[2]);
    const bool pz = !px && !py && az;
    const bool pick[3] = {px, py, pz};
    float s = px ? w.next[0] : (py ? w.next[1] : (pz ? w.next[2] : r.s_end));
    s = fminf(fmaxf(s, w.s_prev), r.s_end);                // simultaneous crossings follow as zero-length segments
    offset = w.offset;
    ds = s - w.s_prev;
    w.s_prev = s;
    // the move, without a branch: the picked axis steps, and its next crossing comes from its new plane by one division
    NAF_UNROLL
    for (int a = 0; a < 3; ++a) {
        w.idx[a] += pick[a] ? w.dir[a] : 0;
        w.rem[a] -= pick[a] ? 1u : 0u;
        w.offset = (uint64_t)((int64_t)w.offset + (pick[a] ? w.jump[a] : (int64_t)0));
    }
    float num[3];
    NAF_UNROLL
    for (int a = 0; a < 3; ++a) num[a] = fmaf((float)(w.idx[a] + (w.dir[a] > 0 ? 1 : 0)), g.d[a], -g.half[a]) - r.p0[a];
    const float c = (px ? num[0] : (py ? num[1] : num[2])) / (px ? dx : (py ? dy : dz));   // siddon_crossing of the picked axis
    NAF_UNROLL
    for (int a = 0; a < 3; ++a) w.next[a] = pick[a] ? c : w.next[a];
}

// One ray as the walks take it; d is un-normalised.
struct SiddonRay {
    float o[3], d[3], near, far;
};

// What a forward walk keeps of a ray: add(f, len) is called once per step, padding included, in traversal order.  SiddonIntegral is
// P6's sum.  SiddonIntegralAndRow (P8) keeps the ray's row sum beside it: the bits the plain sum has on a
// volume of ones (1.0f * len == len), so 1 / row is the weight R of the fp32 matrix P7 defines and no A 1 is ever stored.
struct SiddonIntegral {
    float acc = 0.0f;
    NAF_HD void add(float f, float len) { acc += f * len; }
};
struct SiddonIntegralAndRow {
    float acc = 0.0f, row = 0.0f;
    NAF_HD void add(float f, float len) {
        acc += f * len;
        row += len;
    }
};

// The forward walk of one ray through the piecewise-constant volume `load` reads (load(offset) -> float, one call per step): into
// `sum`, in traversal order, every step's value and length (s_next - s_prev) * |d|.  The loads of a group of steps are issued before
// the first of them is used: the indices depend on one another, the loads do not.  Returns the span's kind; `sum` is left as it was
// unless that is kSiddonOk, and what an empty or a non-finite span yields is the caller's to say.
template <class Load, class Sum>
NAF_HD SiddonKind siddon_forward(const VoxelGrid &g, const SiddonRay &ray, Load load, Sum &sum) {
    SiddonSpan r;
    const SiddonKind kind = siddon_span(g, ray.o, ray.d, ray.near, ray.far, r);
    if (kind != kSiddonOk) return kind;
    SiddonWalk w;
    const uint32_t steps = siddon_begin(g, r, w);
    // group n + 1 is stepped and its loads are issued before group n's values are used, so the loads of two groups are in flight
    // while the next indices are computed
    float len[kSiddonGroup], f[kSiddonGroup];
    uint64_t offset[kSiddonGroup];
    NAF_UNROLL
    for (uint32_t j = 0; j < kSiddonGroup; ++j) {
        float ds;
        siddon_step(g, r, w, offset[j], ds);
        len[j] = ds * r.dn;
    }
    NAF_UNROLL
    for (uint32_t j = 0; j < kSiddonGroup; ++j) f[j] = load(offset[j]);
    for (uint32_t k = kSiddonGroup; k < steps; k += kSiddonGroup) {
        float len_next[kSiddonGroup], f_next[kSiddonGroup];
        NAF_UNROLL
        for (uint32_t j = 0; j < kSiddonGroup; ++j) {
            float ds;
            siddon_step(g, r, w, offset[j], ds);
            len_next[j] = ds * r.dn;
        }
        NAF_UNROLL
        for (uint32_t j = 0; j < kSiddonGroup; ++j) f_next[j] = load(offset[j]);
        NAF_UNROLL
        for (uint32_t j = 0; j < kSiddonGroup; ++j) {
            sum.add(f[j], len[j]);
            f[j] = f_next[j];
            len[j] = len_next[j];
        }
    }
    NAF_UNROLL
    for (uint32_t j = 0; j < kSiddonGroup; ++j) sum.add(f[j], len[j]);
    return kSiddonOk;                                      // the constant: a caller's tests of the kind then fold into the early return
}

// The transpose of that map for one ray (include/naf_hip.h P7 and P8, DESIGN.md sections 21 and 22): the same span, end-point
// indices, trip count, crossings and tie order, and for every step of positive length one call deposit(offset, len), len being the
// very float the forward walk hands to `sum` beside the voxel.  Steps of length 0 (ties, the padding of the last group, the exit
// voxel's fixed point) send nothing, and neither does an empty span, a non-finite one, or a deposit that says up front
// (deposit.wanted()) that it has nothing to add.  A group is stepped first and sent after: nothing here waits for what `deposit` does.
template <class Deposit>
NAF_HD void siddon_transpose(const VoxelGrid &g, const SiddonRay &ray, const Deposit &deposit) {
    if (!deposit.wanted()) return;
    SiddonSpan r;
    if (siddon_span(g, ray.o, ray.d, ray.near, ray.far, r) != kSiddonOk) return;
    SiddonWalk w;
    const uint32_t steps = siddon_begin(g, r, w);
    for (uint32_t k = 0; k < steps; k += kSiddonGroup) {
        float len[kSiddonGroup];
        uint64_t offset[kSiddonGroup];
        NAF_UNROLL
        for (uint32_t j = 0; j < kSiddonGroup; ++j) {
            float ds;
            siddon_step(g, r, w, offset[j], ds);
            len[j] = ds * r.dn;
        }
        NAF_UNROLL
        for (uint32_t j = 0; j < kSiddonGroup; ++j)
            if (len[j] > 0.0f) deposit(offset[j], len[j]);
    }
}

}  // namespace naf
