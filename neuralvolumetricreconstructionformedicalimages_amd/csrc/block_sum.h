// block_sum.h -- the fixed-order fp64 sums that make the reducing operators (tv.hip, ssim.hip, cgls.hip) bit-reproducible: no
// atomics, an order of additions that depends on the shapes alone, and nothing skipped, so that a NaN propagates.  A kernel of
// kThreads lanes leaves one partial per workgroup (block_sum); a second kernel of one workgroup adds the partials (strided_sum, then
// block_sum again) and keeps its own epilogue.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace naf {

// Tree over the workgroup's kThreads sums, the upper half onto the lower at every level; the result is in red[0] for thread 0.
template <uint32_t kThreads>
__device__ __forceinline__ void block_sum(double (&red)[kThreads], double mine, uint32_t tid) {
    red[tid] = mine;
    __syncthreads();
    for (uint32_t h = kThreads / 2; h > 0; h >>= 1) {
        if (tid < h) red[tid] += red[tid + h];
        __syncthreads();
    }
}

// The same for two sums at once, with one barrier per level: the results are in red[0][0] and red[1][0].
template <uint32_t kThreads>
__device__ __forceinline__ void block_sum(double (*red)[kThreads], double mine0, double mine1, uint32_t tid) {
    red[0][tid] = mine0;
    red[1][tid] = mine1;
    __syncthreads();
    for (uint32_t h = kThreads / 2; h > 0; h >>= 1) {
        if (tid < h) {
            red[0][tid] += red[0][tid + h];
            red[1][tid] += red[1][tid + h];
        }
        __syncthreads();
    }
}

// Lane tid's share of n partials: the elements tid, tid + kThreads, .. in ascending order.  Count is the type the kernel counts its
// partials in.
template <uint32_t kThreads, typename Count>
__device__ __forceinline__ double strided_sum(const double *__restrict__ partials, Count n, uint32_t tid) {
    double t = 0.0;
    for (Count i = tid; i < n; i += kThreads) t += partials[i];
    return t;
}

}  // namespace naf
