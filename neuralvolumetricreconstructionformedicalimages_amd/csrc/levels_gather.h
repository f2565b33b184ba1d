// levels_gather.h -- level-parallel training (naf_levels_scatter): the pass that moves the all-to-all's gradient blocks into the
// scatter's [level][point][C] order and takes the maximum |gradient| on its way.  Included from render_fused.hip only (through
// render_step.h).
#pragma once

#include "naf_device.h"

namespace naf {

// ---- level-parallel training (naf_levels_*, naf_hip.h): each rank owns a range of levels ----------------------------------
// Feature gradients arrive from the all-to-all as one block per source rank, [rank][owned level][that rank's points][C]; the
// scatter wants [level][all points][C].  One pass moves them there (16 bytes per lane where the block length allows it), takes
// the maximum |gradient| the fixed-point reducer scales by (the MLP backward of a single-GPU step hands that over; here it ran on
// other GPUs) -- as the bit pattern of the fp32 value, so that NaN / Inf poison the step as they do there.
template <typename T> __device__ __forceinline__ uint32_t abs_bits(T raw);
template <> __device__ __forceinline__ uint32_t abs_bits<uint16_t>(uint16_t raw) { return ((uint32_t)raw << 16) & 0x7fffffffu; }      // bf16
template <> __device__ __forceinline__ uint32_t abs_bits<uint32_t>(uint32_t raw) { return raw & 0x7fffffffu; }                        // fp32

template <typename T, bool kVec>
__global__ void __launch_bounds__(256)
levels_gather_kernel(const unsigned char *__restrict__ blocks, size_t block_stride, T *__restrict__ dst, uint32_t n_ranks, uint32_t nl, uint32_t run,
                     uint32_t lv_begin, uint32_t *__restrict__ gmax_bits) {
    // run = elements of one (rank, level): points of a rank x C.  dst[((lv_begin + l) * n_ranks + r) * run + i] = block_r[l * run + i];
    // blockIdx.y = r * nl + l, the x dimension strides over the run
    constexpr uint32_t kPer = kVec ? 16u / sizeof(T) : 1u;
    const uint32_t r = blockIdx.y / nl, l = blockIdx.y - r * nl, units = run / kPer;
    const T *src = reinterpret_cast<const T *>(blocks + (size_t)r * block_stride) + (size_t)l * run;
    T *out = dst + ((size_t)(lv_begin + l) * n_ranks + r) * run;
    uint32_t m = 0u;
    const uint32_t stride = gridDim.x * blockDim.x;
    if constexpr (kVec) {
        constexpr uint32_t kFlight = 4u;                            // 16-byte loads in flight per lane
        for (uint32_t u0 = blockIdx.x * blockDim.x + threadIdx.x; u0 < units; u0 += kFlight * stride) {
            uint4 q[kFlight];
#pragma unroll
            for (uint32_t j = 0; j < kFlight; ++j) q[j] = reinterpret_cast<const uint4 *>(src)[min(u0 + j * stride, units - 1u)];
#pragma unroll
            for (uint32_t j = 0; j < kFlight; ++j) {
                if (u0 + j * stride < units) reinterpret_cast<uint4 *>(out)[u0 + j * stride] = q[j];
                const uint32_t w[4] = {q[j].x, q[j].y, q[j].z, q[j].w};
#pragma unroll
                for (uint32_t k = 0; k < 4; ++k) {
                    if constexpr (sizeof(T) == 2) m = max(m, max(abs_bits<uint16_t>((uint16_t)(w[k] & 0xffffu)), abs_bits<uint16_t>((uint16_t)(w[k] >> 16))));
                    else m = max(m, abs_bits<uint32_t>(w[k]));
                }
            }
        }
    } else {
        for (uint32_t u = blockIdx.x * blockDim.x + threadIdx.x; u < units; u += stride) {
            const T v = src[u];
            out[u] = v;
            m = max(m, abs_bits<T>(v));
        }
    }
#pragma unroll
    for (uint32_t off = 32u; off != 0u; off >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, (int)off));
    __shared__ uint32_t part[4];
    if ((threadIdx.x & 63u) == 0u) part[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0u) {
        m = max(max(part[0], part[1]), max(part[2], part[3]));
        if (m != 0u) atomicMax(gmax_bits, m);                    // one per workgroup
    }
}

}  // namespace naf
