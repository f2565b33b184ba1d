// mlp_kernels.h -- the sigma-MLP of the step on 32-point tiles (field_mlp.h; fp32 parity mode and every shape with C != 2):
// mlp_forward_kernel, mlp_backward_kernel, and what both tile sizes share of the backward (LossInputs, kClearWords, wave_lds_fence).
// Included by mlp16_kernels.h, i.e. from render_fused.hip only.
#pragma once

#include "field_mlp.h"
#include "mlp_slabs.h"
#include "mlp_tile_io.h"

namespace naf {

// ---- 2: MLP forward + line integral ----------------------------------------------------------------------
// kRays: one wave per ray, acc[r] = sum_s sigma*dist.   !kRays: plain point list, out[p] = sigma(p).
template <typename P, uint32_t C, bool kRays>
__global__ void __launch_bounds__(256, 2)        // 3 waves per SIMD cost the fp32 kernel 91 spilled registers per lane
mlp_forward_kernel(const typename P::feat_t::store_t *__restrict__ feat, const float *__restrict__ mlp, SrcRays src,
                   float *__restrict__ out, float *__restrict__ sigma_out, float *__restrict__ depth_out, uint32_t n_items,
                   uint32_t B, int act, OutMap omap) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    MlpShared<P>::build(smem, mlp, 4);
    const uint32_t lane = threadIdx.x & 63u, n = lane & 31u, h = lane >> 5;
    const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = (gridDim.x * blockDim.x) >> 6;
    typename P::Frag x0f;
    float x0[16], h1[16], h2[16], h3[16];

    if constexpr (kRays) {
        const uint32_t S = src.S, tiles = (S + 31u) / 32u;
        const bool use_zbuf = S <= kMaxSamplesLds;
        float *zbuf = reinterpret_cast<float *>(smem + ((MlpShared<P>::kBytes + 15u) & ~15u)) + (threadIdx.x >> 6) * kMaxSamplesLds;
        FeatRaw<typename P::feat_t, C> ahead;                 // features of the next tile, in flight during this one
        if (wave < n_items) load_feat_raw<typename P::feat_t, C>(feat, B, wave * S + min(n, S - 1u), h, ahead);
        for (uint32_t r = wave; r < n_items; r += n_waves) {
            const RayHead rh = ray_head(src, r);
            const float near = rh.near, far = rh.far, dnorm = rh.dnorm;
            if (use_zbuf) fill_depths(src, r, near, far, zbuf, lane);
            float part = 0.0f, carry = 0.0f;
            for (uint32_t k = 0; k < tiles; ++k) {
                const uint32_t s = 32u * k + n;
                const bool valid = s < S;
                const FeatRaw<typename P::feat_t, C> now = take_tile<typename P::feat_t, C>(feat, B, h, ahead, [&] {
                    // next tile of this ray, else first tile of this wave's next ray, else (nothing left) this tile again
                    const bool more = k + 1u < tiles;
                    const uint32_t rn = more ? r : (r + n_waves < n_items ? r + n_waves : r);
                    return rn * S + min(more ? s + 32u : n, S - 1u);
                });
                unpack_feat_raw<typename P::feat_t, C>(now, x0);
                const float z4 = mlp_tile_forward<P>(smem, lane, x0, x0f, h1, h2, h3);
                const float sigma = last_act(act, z4);
                const float term = !valid ? 0.0f
                                 : sigma * (use_zbuf ? buffered_dist(zbuf, s, S, dnorm) : sample_dist(src, r, s, near, far, dnorm));
                if (sigma_out != nullptr || depth_out != nullptr)          // per-sample outputs (wave-uniform test)
                    carry = emit_samples<32>(term, sigma, carry, valid && h == 0, n, sigma_out, depth_out, (size_t)r * S + s);
                if (h == 0) part += term;
            }
            part = wave_sum32(part);
            if (lane == 0) out[r] = part;
        }
    } else {
        const uint32_t tiles = (n_items + 31u) / 32u;
        for (uint32_t k = wave; k < tiles; k += n_waves) {
            const uint32_t p0 = 32u * k + n;
            const bool valid = p0 < n_items;
            const uint32_t p = valid ? p0 : n_items - 1u;
            load_feat_slots<typename P::feat_t, C>(feat, B, p, h, x0);
            const float z4 = mlp_tile_forward<P>(smem, lane, x0, x0f, h1, h2, h3);
            if (valid && h == 0) out[omap.at(p)] = last_act(act, z4);
        }
    }
}

// ---- 3: MLP backward --------------------------------------------------------------------------------------
// slab layout == parameter block layout (kW0 .. kB3), one slab of kSlabStride floats per workgroup.
// Training steps hand the backward kernels what the loss needs instead of a precomputed d loss / d acc: the masked squared error
// of train.py:127 / loss.py:37 in weighted form, loss = sum_r w_r (acc_r - y_r)^2, d loss / d acc_r = 2 w_r (acc_r - y_r), is two
// flops per ray -- a kernel launch of its own (loss_grad_kernel) cost a fortieth of the reference-size step.
struct LossInputs { const float *acc, *target, *weight; };
constexpr uint32_t kClearWords = 33;               // overflow counters of the binned scatter: total + one per level (Workspace::overflow)

template <typename P>
__device__ __forceinline__ void wave_lds_fence() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <typename P, uint32_t C>
__global__ void __launch_bounds__(256)
mlp_backward_kernel(const typename P::feat_t::store_t *__restrict__ feat, const float *__restrict__ mlp, SrcRays src,
                    const float *__restrict__ grad_acc, LossInputs loss, typename P::feat_t::store_t *__restrict__ dfeat,
                    float *__restrict__ slabs, uint32_t n_rays, uint32_t B, int act, uint32_t *__restrict__ clear_words) {
    using Sh = MlpShared<P>;
    if (clear_words != nullptr && blockIdx.x == 0u && threadIdx.x < kClearWords) clear_words[threadIdx.x] = 0u;      // see StepExtras
    using TR = typename P::tr_t;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    Sh::build(smem, mlp, 8);
    const uint32_t lane = threadIdx.x & 63u, n = lane & 31u, h = lane >> 5, wib = threadIdx.x >> 6;
    const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = (gridDim.x * blockDim.x) >> 6;
    constexpr uint32_t kImg = 32u * P::kTrPitch;                                  // elements per transpose image
    constexpr uint32_t kShAligned = (Sh::kBytes + 15u) & ~15u;
    TR *imgA = reinterpret_cast<TR *>(smem + kShAligned) + (size_t)wib * 3u * kImg;   // gradient tile  G
    TR *imgB = imgA + kImg;                                                        // input tile     X0
    TR *imgC = imgB + kImg;                                                        // hidden tile    H2 / H1
    constexpr uint32_t kImgBytes = ((4u * 3u * kImg * (uint32_t)sizeof(TR)) + 15u) & ~15u;
    float *zbuf = reinterpret_cast<float *>(smem + kShAligned + kImgBytes) + wib * kMaxSamplesLds;
    const bool use_zbuf = src.S <= kMaxSamplesLds;

    // weight-gradient accumulators: lane (c,h), register t  <->  dW[out = slot_row(t,h)][in = c]
    f32x16 dW0 = {0}, dW1 = {0}, dW2a = {0}, dW2b = {0};
    float db0 = 0.0f, db1 = 0.0f, db2 = 0.0f, db3 = 0.0f;
    uint32_t dmax = 0u;                                      // bit pattern of max |feature gradient| (scale of the binned scatter);
                                                             // compared as integers so that Inf / NaN win and stay visible
    float loss_part = 0.0f;                                  // this wave's rays: sum w (acc - y)^2
    float dw3[16];
#pragma unroll
    for (int t = 0; t < 16; ++t) dw3[t] = 0.0f;
    float w3s[16];
    Sh::slot_vector(smem, 3, h, w3s);

    const uint32_t S = src.S, tiles = (S + 31u) / 32u;
    FeatRaw<typename P::feat_t, C> ahead;                     // features of the next tile, in flight during this one
    if (wave < n_rays) load_feat_raw<typename P::feat_t, C>(feat, B, wave * S + min(n, S - 1u), h, ahead);
    for (uint32_t r = wave; r < n_rays; r += n_waves) {
        const RayHead rh = ray_head(src, r);
        const float near = rh.near, far = rh.far, dnorm = rh.dnorm;
        float dacc;
        if (loss.target != nullptr) {                        // training step: the loss lives here (wave-uniform arithmetic)
            const float err = loss.acc[r] - loss.target[r], w = loss.weight[r];
            dacc = 2.0f * w * err;
            loss_part += w * err * err;
        } else dacc = grad_acc[r];
        if (use_zbuf) fill_depths(src, r, near, far, zbuf, lane);

        for (uint32_t k = 0; k < tiles; ++k) {
            const uint32_t s = 32u * k + n;
            const bool valid = s < S;
            const uint32_t p = r * S + (valid ? s : S - 1u);
            float x0[16], h1[16], h2[16], h3[16];
            typename P::Frag x0f;
            const FeatRaw<typename P::feat_t, C> now = take_tile<typename P::feat_t, C>(feat, B, h, ahead, [&] {
                // next tile of this ray, else first tile of this wave's next ray, else (nothing left) this tile again
                const bool more = k + 1u < tiles;
                const uint32_t rn = more ? r : (r + n_waves < n_rays ? r + n_waves : r);
                return rn * S + min(more ? s + 32u : n, S - 1u);
            });
            unpack_feat_raw<typename P::feat_t, C>(now, x0);
            const float z4 = mlp_tile_forward<P>(smem, lane, x0, x0f, h1, h2, h3);
            const float sigma = last_act(act, z4);
            const float gsig = !valid ? 0.0f
                             : dacc * (use_zbuf ? buffered_dist(zbuf, s, S, dnorm) : sample_dist(src, r, s, near, far, dnorm));
            const float g4 = gsig * last_act_grad(act, z4, sigma);

            // output layer: dw3 += g4 * h3, db3 += g4 ; G3 = (w3 g4) * lrelu'(z3)
            float g[16];
#pragma unroll
            for (int t = 0; t < 16; ++t) {
                dw3[t] = __fmaf_rn(g4, h3[t], dw3[t]);
                g[t] = w3s[t] * g4 * (h3[t] > 0.0f ? 1.0f : kLeaky);
            }
            if (h == 0) db3 += g4;

            // transpose G3, X0, H2 through LDS (P::tr_put / P::tr_load): the weight gradients contract over points
            const typename P::Frag g3f = P::pack(g);
            P::tr_put(imgA, n, h, g, g3f);
            P::tr_put(imgB, n, h, x0, x0f);
            P::tr_put(imgC, n, h, h2, P::pack(h2));
            wave_lds_fence<P>();
            typename P::Frag gA = P::tr_load(imgA, n, h);             // A[m = out][k = point]
            const typename P::Frag xB = P::tr_load(imgB, n, h);        // B[k = point][n = in]
            typename P::Frag hB = P::tr_load(imgC, n, h);
            dW2a = P::mma(gA, xB, dW2a);
            dW2b = P::mma(gA, hB, dW2b);
            db2 += P::frag_sum(gA);
            wave_lds_fence<P>();

            // back through layer 2 (skip layer): d[input] and d[h2]
            f32x16 zero = {0};
            f32x16 dx0 = P::mma(P::load_wfrag(smem, kFW2aT, lane), g3f, zero);
            f32x16 dh = P::mma(P::load_wfrag(smem, kFW2bT, lane), g3f, zero);
#pragma unroll
            for (int t = 0; t < 16; ++t) g[t] = dh[t] * (h2[t] > 0.0f ? 1.0f : kLeaky);      // G2

            const typename P::Frag g2f = P::pack(g);
            P::tr_put(imgA, n, h, g, g2f);
            P::tr_put(imgC, n, h, h1, P::pack(h1));
            wave_lds_fence<P>();
            gA = P::tr_load(imgA, n, h);
            hB = P::tr_load(imgC, n, h);
            dW1 = P::mma(gA, hB, dW1);
            db1 += P::frag_sum(gA);
            wave_lds_fence<P>();

            dh = P::mma(P::load_wfrag(smem, kFW1T, lane), g2f, zero);
#pragma unroll
            for (int t = 0; t < 16; ++t) g[t] = dh[t] * (h1[t] > 0.0f ? 1.0f : kLeaky);      // G1
            const typename P::Frag g1f = P::pack(g);
            P::tr_put(imgA, n, h, g, g1f);
            wave_lds_fence<P>();
            gA = P::tr_load(imgA, n, h);
            dW0 = P::mma(gA, xB, dW0);
            db0 += P::frag_sum(gA);
            wave_lds_fence<P>();

            dx0 = P::mma(P::load_wfrag(smem, kFW0T, lane), g1f, dx0);
            if (valid) {
                float o[16];
#pragma unroll
                for (int t = 0; t < 16; ++t) { o[t] = dx0[t]; dmax = max(dmax, __float_as_uint(o[t]) & 0x7fffffffu); }
                store_feat_slots<typename P::feat_t, C>(dfeat, B, p, h, o);
            }
        }
    }

#pragma unroll
    for (int off = 32; off > 0; off >>= 1) dmax = max(dmax, (uint32_t)__shfl_xor((int)dmax, off, 64));     // non-negative floats order like uints

    // ---- fold the 4 waves of the workgroup into one slab (fixed order -> deterministic), then one store ------
    __syncthreads();                                        // everyone is done with the transpose images
    float *red = reinterpret_cast<float *>(smem + kShAligned);          // kSlabStride floats, reuses the images
    // per-lane partial sums that still need a cross-lane reduction
#pragma unroll
    for (int t = 0; t < 16; ++t) dw3[t] = wave_sum32(dw3[t]);          // over the 32 points of a lane half
    db0 += __shfl_xor(db0, 32, 64);                                     // the two lane halves hold 16 points each
    db1 += __shfl_xor(db1, 32, 64);
    db2 += __shfl_xor(db2, 32, 64);
    db3 = wave_sum32(db3) ;
    db3 += __shfl_xor(db3, 32, 64);
    for (uint32_t w = 0; w < (blockDim.x >> 6); ++w) {
        if (wib == w) {
            const bool first = w == 0;
#pragma unroll
            for (uint32_t t = 0; t < 16; ++t) {
                const uint32_t o = slot_row(t, h);
                const uint32_t i0 = kW0 + o * 32u + n, i1 = kW1 + o * 32u + n, i2 = kW2 + o * 64u + n;
                red[i0] = (first ? 0.0f : red[i0]) + dW0[t];
                red[i1] = (first ? 0.0f : red[i1]) + dW1[t];
                red[i2] = (first ? 0.0f : red[i2]) + dW2a[t];
                red[i2 + 32u] = (first ? 0.0f : red[i2 + 32u]) + dW2b[t];
                if (n == 0) red[kW3 + o] = (first ? 0.0f : red[kW3 + o]) + dw3[t];
            }
            if (h == 0) {                                    // db*: lane n holds the sum for feature n
                red[kB0 + n] = (first ? 0.0f : red[kB0 + n]) + db0;
                red[kB1 + n] = (first ? 0.0f : red[kB1 + n]) + db1;
                red[kB2 + n] = (first ? 0.0f : red[kB2 + n]) + db2;
            }
            if (lane == 0) {
                red[kB3] = (first ? 0.0f : red[kB3]) + db3;
                red[kSlabLoss] = (first ? 0.0f : red[kSlabLoss]) + loss_part;
                red[kSlabGmax] = __uint_as_float(first ? dmax : max(dmax, __float_as_uint(red[kSlabGmax])));
            }
        }
        __syncthreads();
    }
    float *slab = slabs + (size_t)blockIdx.x * kSlabStride;
    for (uint32_t i = threadIdx.x; i <= kSlabGmax; i += blockDim.x) slab[i] = red[i];
}

}  // namespace naf
