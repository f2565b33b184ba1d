// mlp_tile_io.h -- what the MLP kernels of the step share around a tile: the feature-tile loads and stores (split so that the next
// tile's loads are in flight during this one's arithmetic), the per-wave depth buffer, the per-sample outputs (emit_samples) and
// OutMap.  Device code only; included by mlp_kernels.h and fused_forward.h, i.e. from render_fused.hip only.
#pragma once

#include "field_mlp.h"
#include "hash_kernels.h"
#include "mlp_step_plan.h"

namespace naf {

// ---- feature tile I/O ------------------------------------------------------------------------------------
// Lane (n,h) owns features f = 8q + 4h + i (q,i = 0..3) of point p; feature f is channel f % C of level f / C.
// The load is split in two so that a kernel can issue the (raw) loads of its NEXT tile before it starts the arithmetic of
// the current one and convert them an iteration later: the MLP kernels run at one or two waves per SIMD, nothing else
// hides the ~2 us HBM round trip.
template <uint32_t kBytes> struct RawWord;
template <> struct RawWord<2> { typedef uint16_t type; };
template <> struct RawWord<4> { typedef uint32_t type; };
template <> struct RawWord<8> { typedef uint2 type; };
template <> struct RawWord<16> { typedef uint4 type; };

template <typename FT, uint32_t C>
struct FeatRaw {
    static constexpr uint32_t V = C < 4 ? C : 4;     // contiguous channels per access
    using word_t = typename RawWord<V * sizeof(typename FT::store_t)>::type;
    word_t w[16 / V];
};
template <typename FT, uint32_t C>
__device__ __forceinline__ void load_feat_raw(const typename FT::store_t *__restrict__ feat, uint32_t B, uint32_t p,
                                              uint32_t h, FeatRaw<FT, C> &raw) {
    constexpr uint32_t V = FeatRaw<FT, C>::V;
#pragma unroll
    for (uint32_t q = 0; q < 4; ++q)
#pragma unroll
        for (uint32_t i = 0; i < 4; i += V) {
            const uint32_t f = 8u * q + 4u * h + i;
            raw.w[(4 * q + i) / V] =
                *reinterpret_cast<const typename FeatRaw<FT, C>::word_t *>(feat + ((size_t)(f / C) * B + p) * C + (f % C));
        }
}
template <typename FT, uint32_t C>
__device__ __forceinline__ void unpack_feat_raw(const FeatRaw<FT, C> &raw, float (&x)[16]) {
    constexpr uint32_t V = FeatRaw<FT, C>::V;
    using S = typename FT::store_t;
#pragma unroll
    for (uint32_t j = 0; j < 16 / V; ++j) {
        S e[V];
        __builtin_memcpy(e, &raw.w[j], sizeof(e));
#pragma unroll
        for (uint32_t k = 0; k < V; ++k) x[V * j + k] = Conv<FT>::load(&e[k]);
    }
}
// Hands out the tile whose features are in flight and requests the next one: `next()` is the point whose features come next.
template <typename FT, uint32_t C, typename Next>
__device__ __forceinline__ FeatRaw<FT, C> take_tile(const typename FT::store_t *__restrict__ feat, uint32_t B, uint32_t h, FeatRaw<FT, C> &ahead, Next next) {
    const FeatRaw<FT, C> now = ahead;
    load_feat_raw<FT, C>(feat, B, next(), h, ahead);
    return now;
}
template <typename FT, uint32_t C>
__device__ __forceinline__ void load_feat_slots(const typename FT::store_t *__restrict__ feat, uint32_t B, uint32_t p,
                                                uint32_t h, float (&x)[16]) {
    FeatRaw<FT, C> raw;
    load_feat_raw<FT, C>(feat, B, p, h, raw);
    unpack_feat_raw<FT, C>(raw, x);
}
template <typename FT, uint32_t C>
__device__ __forceinline__ void store_feat_slots(typename FT::store_t *__restrict__ feat, uint32_t B, uint32_t p,
                                                 uint32_t h, const float (&x)[16]) {
    constexpr uint32_t V = C < 4 ? C : 4;
#pragma unroll
    for (uint32_t q = 0; q < 4; ++q)
#pragma unroll
        for (uint32_t i = 0; i < 4; i += V) {
            const uint32_t f = 8u * q + 4u * h + i;
            float v[V];
#pragma unroll
            for (uint32_t k = 0; k < V; ++k) v[k] = x[4 * q + i + k];
            store_vec<FT, V>(feat + ((size_t)(f / C) * B + p) * C + (f % C), v);
        }
}

__device__ __forceinline__ float wave_sum32(float v) {   // sum over the 32 lanes that share a lane half
#pragma unroll
    for (int off = 16; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// The ray header: the depth range and |d| of ray r (32-byte record: origin, direction, near, far).
struct RayHead { float near, far, dnorm; };
__device__ __forceinline__ RayHead ray_head(const SrcRays &src, uint32_t r) {
    const float *ray = src.rays + (size_t)r * 8;
    return RayHead{ray[6], ray[7], sqrtf(ray[3] * ray[3] + ray[4] * ray[4] + ray[5] * ray[5])};
}

// Per-wave depth buffer: the S depths of the current ray are evaluated once (lanes stride the samples) and kept in LDS,
// so the sample distances of all tiles of the ray are two LDS reads instead of two jitter/depth evaluations per point.
// (kMaxSamplesLds: mlp_step_plan.h)
__device__ __forceinline__ void fill_depths(const SrcRays &src, uint32_t r, float near, float far, float *zbuf, uint32_t lane) {
    for (uint32_t s = lane; s < src.S; s += 64u) zbuf[s] = src.depth(r, s, near, far);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
__device__ __forceinline__ float buffered_dist(const float *zbuf, uint32_t s, uint32_t S, float dnorm) {
    if (s + 1u >= S) return 1e-10f * dnorm;
    return (zbuf[s + 1u] - zbuf[s]) * dnorm;
}

// dist of sample s on ray r (render.py:192-194): (z[s+1]-z[s]) * |d|, last sample 1e-10 * |d|
__device__ __forceinline__ float sample_dist(const SrcRays &src, uint32_t r, uint32_t s, float near, float far, float dnorm) {
    if (s + 1u >= src.S) return 1e-10f * dnorm;
    return (src.depth(r, s + 1u, near, far) - src.depth(r, s, near, far)) * dnorm;
}

// Per-sample outputs of the forward pass (what the fine pass consumes, render.py:113-126,203-211): the network output
// sigma[r,s] and the RUNNING optical depth tau[r,s] = sum_{s' <= s} sigma * dist.  The W samples of a tile sit in W
// consecutive lanes; the running sum is an inclusive wave prefix sum over them (log2 W shuffle steps) plus the carry
// of the ray's earlier tiles.  Every lane of the wave takes part in the shuffles; `writer` lanes store.  Returns the new carry.
template <uint32_t W>
__device__ __forceinline__ float emit_samples(float term, float sigma, float carry, bool writer, uint32_t pos,
                                              float *__restrict__ sigma_out, float *__restrict__ depth_out, size_t idx) {
    float scan = term;
#pragma unroll
    for (uint32_t d = 1; d < W; d <<= 1) {
        const float up = __shfl_up(scan, d, W);
        if (pos >= d) scan += up;
    }
    scan += carry;
    if (writer) {
        if (sigma_out != nullptr) sigma_out[idx] = sigma;
        if (depth_out != nullptr) depth_out[idx] = scan;
    }
    return __shfl(scan, W - 1u, W);          // the tile's last sample carries the total so far (lanes past S add 0)
}

// Where point p of a point-list launch writes its output: identity, or (grid queries, SrcGrid traversal) the position of
// grid point p in the caller's [n0, n1, n2] array.
struct OutMap {
    uint32_t n0, n1, n2;          // n0 == 0: identity
    uint32_t first;               // grid queries in chunks: point p of the launch is point first + p of the traversal
    __device__ __forceinline__ size_t at(uint32_t p) const {
        if (n0 == 0u) return p;
        p += first;
        const uint32_t i0 = p % n0, rest = p / n0, i2 = rest % n2, i1 = rest / n2;
        return ((size_t)i0 * n1 + i1) * n2 + i2;
    }
};

}  // namespace naf
