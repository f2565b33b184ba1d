// backproject_device.h -- the ray scatter of the transpose (include/naf_hip.h P2), shared by projector.hip
// and sart.hip: the march over a ray's samples with the merge of consecutive samples that share a cell.  What a finished cell adds
// to memory is the caller's `Deposit`: one volume for P2, the numerator / column-sum pair of the OS-SART subset step for P4.
#pragma once

#include "project_device.h"

namespace naf {

// Adds scale * acc[c] to the eight corners of the cell at `q`; corners that got no weight (a constant axis, a sample on a voxel
// centre) are skipped.  Corner c = 4 cx + 2 cy + cz.
__device__ __forceinline__ void flush_cell(float *__restrict__ q, const ProjVolume &v, float scale, const float acc[8]) {
    const uint64_t sx = v.grid.next[0], sy = v.grid.next[1], sz = v.grid.next[2];
    const uint64_t off[8] = {0, sz, sy, sy + sz, sx, sx + sz, sx + sy, sx + sy + sz};
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const float add = scale * acc[c];
        if (add != 0.0f) atomicAdd(q + off[c], add);          // no-return global_atomic_add_f32
    }
}

// P2's deposit: value * (len / n) * w_c into one volume.
struct DepositValue {
    float *__restrict__ volume;
    float value;
    __device__ __forceinline__ void operator()(const ProjVolume &v, uint64_t cell, float weight, const float acc[8]) const {
        flush_cell(volume + cell, v, value * weight, acc);
    }
};

// P4's deposit: value * (len / n) * w_c into `num` and, where `den` is given, (len / n) * w_c into `den`, from the same eight sums.
struct DepositPair {
    float *__restrict__ num;
    float *__restrict__ den;                                  // may be null
    float value;
    __device__ __forceinline__ void operator()(const ProjVolume &v, uint64_t cell, float weight, const float acc[8]) const {
        flush_cell(num + cell, v, value * weight, acc);
        if (den) flush_cell(den + cell, v, weight, acc);
    }
};

// Runs `deposit(v, cell, len / n, acc)` for every run of consecutive samples of the ray that share a cell, acc[c] the sum of the
// run's corner weights w_c.  An empty segment and a NaN / infinite ray deposit nothing.
template <class Deposit>
__device__ __forceinline__ void scatter_ray(const ProjVolume &v, float4 a, float4 b, const Deposit &deposit) {
    RaySpan s;
    if (ray_span(v, a, b, s) != kSpanOk) return;
    constexpr uint64_t kNoCell = ~0ull;
    uint64_t cell = kNoCell;
    float acc[8];
    for (uint32_t k = 0; k < s.n; ++k) {
        float p[3], w[3];
        span_point(s, k, p);
        const uint64_t base = trilinear_cell(v, p, w);
#ifdef NAF_BACKPROJECT_PER_SAMPLE
        const bool moved = true;
#else
        const bool moved = base != cell;
#endif
        if (moved) {
            if (cell != kNoCell) deposit(v, cell, s.weight, acc);
            cell = base;
#pragma unroll
            for (int c = 0; c < 8; ++c) acc[c] = 0.0f;
        }
        const float x[2] = {1.0f - w[0], w[0]}, y[2] = {1.0f - w[1], w[1]}, z[2] = {1.0f - w[2], w[2]};
#pragma unroll
        for (int c = 0; c < 8; ++c) acc[c] += (x[c >> 2] * y[(c >> 1) & 1]) * z[c & 1];
    }
    if (cell != kNoCell) deposit(v, cell, s.weight, acc);
}

}  // namespace naf
