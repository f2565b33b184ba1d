// mlp16_kernels.h -- the sigma-MLP of the step on 16-point tiles (field_mlp16.h; bf16 mode, C = 2): mlp16_forward_kernel,
// mlp16_forward_split_kernel, the backward's shared pieces (Mlp16Sums, mlp16_backward_tile, mlp16_fold_slab), mlp16_backward_kernel,
// the one-launch mlp16_train_kernel, and mlp_grad_reduce_kernel.  Included from render_fused.hip only (through render_step.h).
#pragma once

#include "field_mlp16.h"
#include "mlp_kernels.h"

namespace naf {

// ---- 2b: the same on 16-point tiles (bf16 mode, C = 2; field_mlp16.h) -------------------------------------------
template <bool kRays>
__global__ void __launch_bounds__(256, 4)
mlp16_forward_kernel(const uint16_t *__restrict__ feat, const float *__restrict__ mlp, SrcRays src, float *__restrict__ out,
                     float *__restrict__ sigma_out, float *__restrict__ depth_out, uint32_t n_items, uint32_t B, int act,
                     OutMap omap) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const uint32_t lane = threadIdx.x & 63u, c = lane & 15u, g = lane >> 4;
    const uint32_t wave = __builtin_amdgcn_readfirstlane((blockIdx.x * blockDim.x + threadIdx.x) >> 6), n_waves = (gridDim.x * blockDim.x) >> 6;
    Act16 a;
    if constexpr (kRays) {
        const uint32_t S = src.S, tiles = (S + 15u) / 16u;
        const bool use_zbuf = S <= kMaxSamplesLds;
        float *zbuf = reinterpret_cast<float *>(smem + ((Mlp16Shared::kBytes + 15u) & ~15u)) + (threadIdx.x >> 6) * kMaxSamplesLds;
        Feat16Raw ahead;                                     // features of the next tile, in flight during this one
        if (wave < n_items) load_feat16(feat, B, wave * S + min(c, S - 1u), g, ahead);
        // (after the first feature request: the two round trips overlap; the depth buffers are filled later: they stage the weights)
        Mlp16Shared::build_staged<4>(smem, mlp, reinterpret_cast<float *>(smem + ((Mlp16Shared::kBytes + 15u) & ~15u)));
        Mlp16InRegs wt;
        wt.load(smem, lane);
        for (uint32_t r = wave; r < n_items; r += n_waves) {
            const RayHead rh = ray_head(src, r);
            const float near = rh.near, far = rh.far, dnorm = rh.dnorm;
            if (use_zbuf) fill_depths(src, r, near, far, zbuf, lane);
            float part = 0.0f, carry = 0.0f;
            if (sigma_out == nullptr && depth_out == nullptr) {            // (wave-uniform) line integrals only: training, projections
                // All four lane groups of a tile hold the same z4, so the activation and the sample distance -- 40 of a tile's ~125
                // vector instructions -- would be evaluated four times over.  Four tiles share one evaluation instead: lane group j
                // keeps the z4 of tile k0 + j, i.e. lane (c, g) ends up with sample 16 (k0 + g) + c.  The terms then return to lane
                // group 0 row by row (v_permlane*_swap) and are added in tile order -- the order of the loop below: same bits.
                for (uint32_t k0 = 0; k0 < tiles; k0 += 4u) {
                    float zsel = 0.0f;
#pragma unroll
                    for (uint32_t j = 0; j < 4u; ++j) {
                        const uint32_t k = k0 + j;
                        if (k >= tiles) break;                               // uniform
                        const uint32_t sk = 16u * k + c;
                        const Feat16Raw now = ahead;
                        {   // next tile of this ray, else first tile of this wave's next ray, else (nothing left) this tile again
                            const bool more = k + 1u < tiles;
                            const uint32_t rn = more ? r : (r + n_waves < n_items ? r + n_waves : r);
                            const uint32_t sn = more ? sk + 16u : c;
                            load_feat16(feat, B, rn * S + min(sn, S - 1u), g, ahead);
                        }
                        const float z4 = mlp16_tile_forward(wt, feat16_operand(now), a);
                        zsel = g == j ? z4 : zsel;
                    }
                    const uint32_t s = 16u * (k0 + g) + c;
                    const float sigma = last_act16(act, zsel);
                    const float term = s >= S ? 0.0f
                                     : sigma * (use_zbuf ? buffered_dist(zbuf, s, S, dnorm) : sample_dist(src, r, s, near, far, dnorm));
                    const uint32_t tb = __float_as_uint(term);
                    const auto r16 = __builtin_amdgcn_permlane16_swap(tb, tb, false, false);          // [1]: rows 1 1 3 3
                    const auto r32 = __builtin_amdgcn_permlane32_swap(tb, tb, false, false);          // [1]: rows 2 3 2 3
                    const auto r48 = __builtin_amdgcn_permlane16_swap(r32[1], r32[1], false, false);  // [1]: rows 3 3 3 3
                    if (g == 0u) {
                        part += term;
                        if (k0 + 1u < tiles) part += __uint_as_float(r16[1]);
                        if (k0 + 2u < tiles) part += __uint_as_float(r32[1]);
                        if (k0 + 3u < tiles) part += __uint_as_float(r48[1]);
                    }
                }
            } else
            for (uint32_t k = 0; k < tiles; ++k) {
                const uint32_t s = 16u * k + c;
                const bool valid = s < S;
                const Feat16Raw now = ahead;
                {   // next tile of this ray, else first tile of this wave's next ray, else (nothing left) this tile again
                    const bool more = k + 1u < tiles;
                    const uint32_t rn = more ? r : (r + n_waves < n_items ? r + n_waves : r);
                    const uint32_t sn = more ? s + 16u : c;
                    load_feat16(feat, B, rn * S + min(sn, S - 1u), g, ahead);
                }
                const float z4 = mlp16_tile_forward(wt, feat16_operand(now), a);
                const float sigma = last_act16(act, z4);
                const float term = !valid ? 0.0f
                                 : sigma * (use_zbuf ? buffered_dist(zbuf, s, S, dnorm) : sample_dist(src, r, s, near, far, dnorm));
                if (sigma_out != nullptr || depth_out != nullptr)          // per-sample outputs (wave-uniform test)
                    carry = emit_samples<16>(term, sigma, carry, valid && g == 0u, c, sigma_out, depth_out, (size_t)r * S + s);
                if (g == 0u) part += term;
            }
#pragma unroll
            for (int off = 8; off > 0; off >>= 1) part += __shfl_xor(part, off, 64);     // the 16 points of lane group 0
            if (lane == 0) out[r] = part;
        }
    } else {
        Mlp16Shared::build_staged<4>(smem, mlp, reinterpret_cast<float *>(smem + ((Mlp16Shared::kBytes + 15u) & ~15u)));
        Mlp16InRegs wt;
        wt.load(smem, lane);
        const uint32_t tiles = (n_items + 15u) / 16u;
        for (uint32_t k = wave; k < tiles; k += n_waves) {
            const uint32_t p0 = 16u * k + c;
            const bool valid = p0 < n_items;
            const uint32_t p = valid ? p0 : n_items - 1u;
            Feat16Raw raw;
            load_feat16(feat, B, p, g, raw);
            const float z4 = mlp16_tile_forward(wt, feat16_operand(raw), a);
            if (valid && g == 0u) out[omap.at(p)] = last_act16(act, z4);
        }
    }
}

// ---- 2b': the same line integrals with FOUR waves per ray (steps with fewer rays than two waves per SIMD: the reference's 1 024) ---
// One wave per ray walks a ray's tiles one after the other, and with one wave per SIMD nothing hides the dependent MFMA / epilogue
// chain of a tile: the forward of a 1 024-ray step is a single ray's latency (12 tiles, ~18 000 cycles) whatever the chip could do
// beside it.  Here a workgroup takes a ray at a time and its four waves a quarter of the tiles each; the terms sigma * dist meet in
// LDS and wave 0 adds them in tile order, then across the 16 lanes like mlp16_forward_kernel does: the same sums in the same order,
// bit-identical line integrals.  Each wave fills the depths of its own tiles (+ 1) in its depth buffer; the term buffers (double-
// buffered: one barrier per ray) live in the upper halves of the first two depth buffers, which is why S <= kMaxSamplesLds / 2.
__global__ void __launch_bounds__(256, 4)
mlp16_forward_split_kernel(const uint16_t *__restrict__ feat, const float *__restrict__ mlp, SrcRays src, float *__restrict__ out,
                           uint32_t n_rays, uint32_t B, int act) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const uint32_t lane = threadIdx.x & 63u, c = lane & 15u, g = lane >> 4, wib = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t S = src.S, tiles = (S + 15u) / 16u;
    const uint32_t k_begin = wib * tiles / 4u, k_end = (wib + 1u) * tiles / 4u;
    float *zall = reinterpret_cast<float *>(smem + ((Mlp16Shared::kBytes + 15u) & ~15u));
    float *zbuf = zall + wib * kMaxSamplesLds;
    float *terms[2] = {zall + kMaxSamplesLds / 2u, zall + kMaxSamplesLds + kMaxSamplesLds / 2u};
    Act16 a;
    Feat16Raw ahead;
    if (blockIdx.x < n_rays) load_feat16(feat, B, blockIdx.x * S + min(16u * k_begin + c, S - 1u), g, ahead);
    Mlp16Shared::build_staged<4>(smem, mlp, zall);
    Mlp16InRegs wt;
    wt.load(smem, lane);
    uint32_t turn = 0u;
    for (uint32_t r = blockIdx.x; r < n_rays; r += gridDim.x, turn ^= 1u) {
        const RayHead rh = ray_head(src, r);
        const float near = rh.near, far = rh.far, dnorm = rh.dnorm;
        for (uint32_t s = 16u * k_begin + lane; s < min(S, 16u * k_end + 1u); s += 64u) zbuf[s] = src.depth(r, s, near, far);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        float *T = terms[turn];
        for (uint32_t k0 = k_begin; k0 < k_end; k0 += 4u) {
            float zsel = 0.0f;
#pragma unroll
            for (uint32_t j = 0; j < 4u; ++j) {
                const uint32_t k = k0 + j;
                if (k >= k_end) break;                                   // uniform
                const Feat16Raw now = ahead;
                {   // next tile of this wave's range, else the first one of the workgroup's next ray, else (nothing left) this tile again
                    const bool more = k + 1u < k_end;
                    const uint32_t rn = more ? r : (r + gridDim.x < n_rays ? r + gridDim.x : r);
                    const uint32_t sn = 16u * (more ? k + 1u : k_begin) + c;
                    load_feat16(feat, B, rn * S + min(sn, S - 1u), g, ahead);
                }
                const float z4 = mlp16_tile_forward(wt, feat16_operand(now), a);
                zsel = g == j ? z4 : zsel;
            }
            const uint32_t s = 16u * (k0 + g) + c;
            const float sigma = last_act16(act, zsel);
            const float term = s >= S ? 0.0f : sigma * buffered_dist(zbuf, s, S, dnorm);
            if (k0 + g < k_end) T[s] = term;
        }
        __syncthreads();
        if (wib == 0u) {
            float part = 0.0f;
            if (g == 0u)
                for (uint32_t k = 0; k < tiles; ++k) part += T[16u * k + c];
#pragma unroll
            for (int off = 8; off > 0; off >>= 1) part += __shfl_xor(part, off, 64);     // the 16 points of lane group 0
            if (lane == 0) out[r] = part;
        }
        // (no second barrier: the next ray's terms go to the other buffer, and this buffer is written again only behind the next
        // ray's barrier, which wave 0 reaches after it has read it)
    }
}

// ---- 3b: MLP backward on 16-point tiles (bf16 mode, C = 2; field_mlp16.h) ----------------------------------------
// Same outputs as mlp_backward_kernel (dfeat, one dW slab per workgroup, max |dfeat|) at two or more waves per SIMD.  The sums of a
// wave, the backward of one tile and the fold of four waves into a slab are shared with mlp16_train_kernel (3c).
struct Mlp16Sums {
    // weight-gradient accumulators: tile (o, q) covers outputs 16o.. and inputs 16q..; lane (col, grp), register i
    // <-> dW[out = 16 o + 4 grp + i][in = 16 q + col]
    f32x4v dW0[2][2], dW1[2][2], dW2[2][4];
    float db[3][2];                                          // per lane: output 16o + (lane & 15), its 4 points
    float db3, loss_part;
    uint32_t dmax;                                           // see mlp_backward_kernel
    f32x4v dw3lo, dw3hi;
    __device__ __forceinline__ void clear() {
        const f32x4v zero4 = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int o = 0; o < 2; ++o) {
#pragma unroll
            for (int q = 0; q < 2; ++q) { dW0[o][q] = zero4; dW1[o][q] = zero4; }
#pragma unroll
            for (int q = 0; q < 4; ++q) dW2[o][q] = zero4;
        }
#pragma unroll
        for (int l = 0; l < 3; ++l) db[l][0] = db[l][1] = 0.0f;
        db3 = 0.0f; loss_part = 0.0f;
        dmax = 0u;
        dw3lo = zero4; dw3hi = zero4;
    }
};
constexpr uint32_t kImg16 = 16u * 64u;                       // bytes per transpose image; a wave owns three (G, X0, H) in a row

// Backward of one tile: forward recomputed from the features `now`, gsig = d loss / d sigma of the lane's point (0 past the ray's
// end), feature gradients of point p stored when `valid`.  `imgs`: the wave's three transpose images.
__device__ __forceinline__ void mlp16_backward_tile(Mlp16Sums &sm, const unsigned char *smem, unsigned char *imgs, uint32_t lane, const Feat16Raw &now,
                                                    float gsig, int act, bool valid, uint16_t *__restrict__ dfeat, uint32_t B, uint32_t p) {
    const uint32_t c = lane & 15u, g = lane >> 4;
    const f32x4v zero4 = {0.0f, 0.0f, 0.0f, 0.0f};
    unsigned char *imgG = imgs, *imgX = imgs + kImg16, *imgH = imgs + 2u * kImg16;      // gradient tile G3 / G2 / G1, input tile X0, hidden tile H2 / H1
    const bf16x8 x0f = feat16_operand(now);
    // Weight fragments and biases are re-read from LDS for every tile: hoisted out of the loop (which the compiler
    // does when it can prove the addresses loop-invariant) they would pin ~90 registers and halve the occupancy.
    uint32_t tile_tag = 0;
    asm volatile("" : "+v"(tile_tag));
    const unsigned char *wsh = smem + tile_tag;
    Act16 a;
    const float z4 = mlp16_tile_forward(wsh, lane, x0f, a);
    const float sigma = last_act16(act, z4);
    const float g4 = gsig * last_act_grad(act, z4, sigma);

    // output layer: dw3 += g4 * h3, db3 += g4 ; G3 = (w3 g4) * lrelu'(z3)
    f32x4v glo, ghi;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        sm.dw3lo[j] = __fmaf_rn(g4, a.h3lo[j], sm.dw3lo[j]);
        sm.dw3hi[j] = __fmaf_rn(g4, a.h3hi[j], sm.dw3hi[j]);
        glo[j] = a.w3lo[j] * g4 * (a.h3lo[j] > 0.0f ? 1.0f : kLeaky);
        ghi[j] = a.w3hi[j] * g4 * (a.h3hi[j] > 0.0f ? 1.0f : kLeaky);
    }
    if (g == 0u) sm.db3 += g4;

    // layer 2: dW2 = G3 . [X0; H2]^T over the 16 points of the tile
    bf16x8 gf = pack16(glo, ghi);
    tr16_put(imgG, c, g, gf);
    tr16_put(imgX, c, g, x0f);
    tr16_put(imgH, c, g, a.h2f);
    wave_lds_fence<PrecBF16>();
    i16x4v gA[2], xB[2], hB[2];
#pragma unroll
    for (uint32_t o = 0; o < 2; ++o) { gA[o] = tr16_get(imgG, lane, o); xB[o] = tr16_get(imgX, lane, o); hB[o] = tr16_get(imgH, lane, o); }
#pragma unroll
    for (int o = 0; o < 2; ++o) {
        sm.dW2[o][0] = mma16k16(gA[o], xB[0], sm.dW2[o][0]);
        sm.dW2[o][1] = mma16k16(gA[o], xB[1], sm.dW2[o][1]);
        sm.dW2[o][2] = mma16k16(gA[o], hB[0], sm.dW2[o][2]);
        sm.dW2[o][3] = mma16k16(gA[o], hB[1], sm.dW2[o][3]);
        sm.db[2][o] = add_bf16x4(sm.db[2][o], gA[o]);
    }
    wave_lds_fence<PrecBF16>();

    // back through layer 2 (skip layer): d[input] and d[h2]
    f32x4v dxlo = mma16(Mlp16Shared::frag(wsh, kFW2aT, 0, lane), gf, zero4);
    f32x4v dxhi = mma16(Mlp16Shared::frag(wsh, kFW2aT, 1, lane), gf, zero4);
    f32x4v dhlo = mma16(Mlp16Shared::frag(wsh, kFW2bT, 0, lane), gf, zero4);
    f32x4v dhhi = mma16(Mlp16Shared::frag(wsh, kFW2bT, 1, lane), gf, zero4);
    glo = leaky_grad4_packed(dhlo, a.h2f, 0);                              // G2
    ghi = leaky_grad4_packed(dhhi, a.h2f, 1);
    gf = pack16(glo, ghi);
    tr16_put(imgG, c, g, gf);
    tr16_put(imgH, c, g, a.h1f);
    wave_lds_fence<PrecBF16>();
#pragma unroll
    for (uint32_t o = 0; o < 2; ++o) { gA[o] = tr16_get(imgG, lane, o); hB[o] = tr16_get(imgH, lane, o); }
#pragma unroll
    for (int o = 0; o < 2; ++o) {
        sm.dW1[o][0] = mma16k16(gA[o], hB[0], sm.dW1[o][0]);
        sm.dW1[o][1] = mma16k16(gA[o], hB[1], sm.dW1[o][1]);
        sm.db[1][o] = add_bf16x4(sm.db[1][o], gA[o]);
    }
    wave_lds_fence<PrecBF16>();

    dhlo = mma16(Mlp16Shared::frag(wsh, kFW1T, 0, lane), gf, zero4);
    dhhi = mma16(Mlp16Shared::frag(wsh, kFW1T, 1, lane), gf, zero4);
    glo = leaky_grad4_packed(dhlo, a.h1f, 0);                              // G1
    ghi = leaky_grad4_packed(dhhi, a.h1f, 1);
    gf = pack16(glo, ghi);
    tr16_put(imgG, c, g, gf);
    wave_lds_fence<PrecBF16>();
#pragma unroll
    for (uint32_t o = 0; o < 2; ++o) { gA[o] = tr16_get(imgG, lane, o); xB[o] = tr16_get(imgX, lane, o); }   // X0 again: cheaper than keeping it
#pragma unroll
    for (int o = 0; o < 2; ++o) {
        sm.dW0[o][0] = mma16k16(gA[o], xB[0], sm.dW0[o][0]);
        sm.dW0[o][1] = mma16k16(gA[o], xB[1], sm.dW0[o][1]);
        sm.db[0][o] = add_bf16x4(sm.db[0][o], gA[o]);
    }
    wave_lds_fence<PrecBF16>();

    dxlo = mma16(Mlp16Shared::frag(wsh, kFW0T, 0, lane), gf, dxlo);
    dxhi = mma16(Mlp16Shared::frag(wsh, kFW0T, 1, lane), gf, dxhi);
    if (valid) {
#pragma unroll
        for (int j = 0; j < 4; ++j) sm.dmax = max(sm.dmax, max(__float_as_uint(dxlo[j]) & 0x7fffffffu, __float_as_uint(dxhi[j]) & 0x7fffffffu));
        store_feat16(dfeat, B, p, g, __builtin_bit_cast(uint4, pack16(dxlo, dxhi)));
    }
}

// ---- fold four waves into one slab (wave order -> deterministic), then one store ---------------------------------------------
// Called by every wave of the workgroup (it holds workgroup barriers): wave `wig` of a group of four, `tid` = thread of the group,
// imgA / imgB = the group's two slab images, `slab` = where the group's sums go (nullptr: nowhere).  The first barrier ends every
// other use of the LDS.
__device__ __forceinline__ void mlp16_fold_slab(Mlp16Sums &sm, float *imgA, float *imgB, uint32_t tid, uint32_t wig, float *__restrict__ slab) {
    const uint32_t lane = tid & 63u, c = lane & 15u, g = lane >> 4;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) sm.dmax = max(sm.dmax, (uint32_t)__shfl_xor((int)sm.dmax, off, 64));     // non-negative floats order like uints
#pragma unroll
    for (int l = 0; l < 3; ++l)
#pragma unroll
        for (int o = 0; o < 2; ++o) {                                               // over the four point groups of an output
            sm.db[l][o] += __shfl_xor(sm.db[l][o], 16, 64);
            sm.db[l][o] += __shfl_xor(sm.db[l][o], 32, 64);
        }
#pragma unroll
    for (int off = 8; off > 0; off >>= 1) {                                         // over the 16 points of a lane group
#pragma unroll
        for (int j = 0; j < 4; ++j) { sm.dw3lo[j] += __shfl_xor(sm.dw3lo[j], off, 64); sm.dw3hi[j] += __shfl_xor(sm.dw3hi[j], off, 64); }
        sm.db3 += __shfl_xor(sm.db3, off, 64);
    }
    __syncthreads();                                                                // images / depth buffers are dead
    // ---- in wave order: ((0 + a0) + a1) + a2) + a3 per entry, as ever --------------
    // tools/mlp_stamps.py put the fold of rounds 2-4 -- the waves took turns adding their 64 + 17 values to one LDS image, `red[i] += x`,
    // a dependent read-add-write round trip each -- at 14 000 of the kernel's 52 900 cycles at the reference's batch (with the pass
    // that cleared the image); batching a turn's reads did not help (the turns stay dependent and three workgroups per CU take them at
    // once), an XOR swizzle against the 4-way bank conflict of the lane groups neither.  Now nobody reads what it has just written: a wave
    // STORES its values into an image of its own (no waits), and all 256 threads add two images entry by entry, coalesced.  There is
    // room for two images -- A over the weight fragments, which are dead too, B over the transpose images -- so waves 0 and 1 write
    // together and waves 2 and 3 follow one by one.  Same operands in the same order: the slab has the same bits.
    auto put = [&](float *img) {
#pragma unroll
        for (uint32_t o = 0; o < 2; ++o)
#pragma unroll
            for (uint32_t i = 0; i < 4; ++i) {
                const uint32_t out = 16u * o + 4u * g + i;
#pragma unroll
                for (uint32_t q = 0; q < 2; ++q) {
                    img[kW0 + out * 32u + 16u * q + c] = sm.dW0[o][q][i];
                    img[kW1 + out * 32u + 16u * q + c] = sm.dW1[o][q][i];
                }
#pragma unroll
                for (uint32_t q = 0; q < 4; ++q) img[kW2 + out * 64u + 16u * q + c] = sm.dW2[o][q][i];
            }
        if (g == 0u) {
#pragma unroll
            for (uint32_t o = 0; o < 2; ++o) {
                img[kB0 + 16u * o + c] = sm.db[0][o];
                img[kB1 + 16u * o + c] = sm.db[1][o];
                img[kB2 + 16u * o + c] = sm.db[2][o];
            }
        }
        if (c == 0u) {
#pragma unroll
            for (uint32_t j = 0; j < 4; ++j) {
                img[kW3 + 4u * g + j] = sm.dw3lo[j];
                img[kW3 + 16u + 4u * g + j] = sm.dw3hi[j];
            }
        }
        if (lane == 0u) {
            img[kB3] = sm.db3;
            img[kSlabLoss] = sm.loss_part;
            img[kSlabGmax] = __uint_as_float(sm.dmax);
        }
    };
    // A (+)= B, entry by entry; the first time A's entries are a wave's raw values and stand for 0 + a0 (the cleared image of old: -0.0
    // becomes +0.0), the last time the sums go to the slab instead.  The maximum of the gradient bit patterns rides along.
    auto combine = [&](bool first_pair, bool last_pair) {
        constexpr uint32_t kPer = (kSlabGmax + 1u + 255u) / 256u;
        float x[kPer], y[kPer];
#pragma unroll
        for (uint32_t u = 0; u < kPer; ++u) {
            const uint32_t i = min(tid + 256u * u, kSlabGmax);
            x[u] = imgA[i];
            y[u] = imgB[i];
        }
#pragma unroll
        for (uint32_t u = 0; u < kPer; ++u) {
            const uint32_t i = tid + 256u * u;
            if (i > kSlabGmax) break;
            const float lhs = first_pair ? 0.0f + x[u] : x[u];
            const float v = i == kSlabGmax ? __uint_as_float(max(__float_as_uint(x[u]), __float_as_uint(y[u]))) : lhs + y[u];
            if (!last_pair) imgA[i] = v; else if (slab != nullptr) slab[i] = v;
        }
    };
    if (wig == 0u) put(imgA);
    if (wig == 1u) put(imgB);
    __syncthreads();
    combine(true, false);
    __syncthreads();
    if (wig == 2u) put(imgB);
    __syncthreads();
    combine(false, false);
    __syncthreads();
    if (wig == 3u) put(imgB);
    __syncthreads();
    combine(false, true);
}

__global__ void __launch_bounds__(256, 3)                     // three waves per SIMD
mlp16_backward_kernel(const uint16_t *__restrict__ feat, const float *__restrict__ mlp, SrcRays src,
                      const float *__restrict__ grad_acc, LossInputs loss, uint16_t *__restrict__ dfeat, float *__restrict__ slabs,
                      uint32_t n_rays, uint32_t B, int act, uint32_t parts, uint32_t *__restrict__ clear_words) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
#ifdef NAF_MLP_STAMPS        // diagnostic builds (tools/mlp_stamps.py): shader-clock stamps of the kernel's phases, written behind the slab's payload
    long long stamp_[6];
    const long long wall0_ = wall_clock64();
#define NAF_STAMP(i) stamp_[i] = clock64()
#else
#define NAF_STAMP(i)
#endif
    NAF_STAMP(0);
    if (clear_words != nullptr && blockIdx.x == 0u && threadIdx.x < kClearWords) clear_words[threadIdx.x] = 0u;      // see StepExtras
    const uint32_t lane = threadIdx.x & 63u, c = lane & 15u, g = lane >> 4, wib = threadIdx.x >> 6;
    // wave-uniform values are made scalar explicitly: the ray record, its depths range and d acc then live in SGPRs
    const uint32_t wave = __builtin_amdgcn_readfirstlane((blockIdx.x * blockDim.x + threadIdx.x) >> 6), n_waves = (gridDim.x * blockDim.x) >> 6;
    constexpr uint32_t kShAligned = (Mlp16Shared::kBytes + 15u) & ~15u;
    unsigned char *imgs = smem + kShAligned + wib * 3u * kImg16;
    float *zbuf = reinterpret_cast<float *>(smem + kShAligned + 4u * 3u * kImg16) + wib * kMaxSamplesLds;
    const bool use_zbuf = src.S <= kMaxSamplesLds;
    Mlp16Sums sums;
    sums.clear();

    // A work item is one ray, or one of `parts` consecutive tile ranges of a ray when there are fewer rays than resident waves
    // (1 024-ray steps: three waves per ray, four tiles each; the backward of a sample needs nothing of its ray but d acc, so
    // the ranges are independent): more waves per SIMD to hide the latency of the dependent MFMA chain behind.
    const uint32_t S = src.S, tiles = (S + 15u) / 16u;
    const uint32_t n_items = n_rays * parts;
    auto ray_of = [&](uint32_t item) { return item / parts; };
    auto first_tile = [&](uint32_t part) { return part * tiles / parts; };
    Feat16Raw ahead;
    if (wave < n_items) load_feat16(feat, B, ray_of(wave) * S + min(16u * first_tile(wave - ray_of(wave) * parts) + c, S - 1u), g, ahead);
    // the weight fragments are built AFTER the first tile's features have been requested: the two round trips overlap (the build
    // ends with the workgroup barrier that makes the fragments visible)
    Mlp16Shared::build_staged<8>(smem, mlp, reinterpret_cast<float *>(smem + kShAligned));      // (the transpose images and depth buffers lend the space)
    NAF_STAMP(1);
    for (uint32_t item = wave; item < n_items; item += n_waves) {
        const uint32_t r = ray_of(item), part = item - r * parts, k_begin = first_tile(part), k_end = first_tile(part + 1u);
        const RayHead rh = ray_head(src, r);
        const float near = rh.near, far = rh.far, dnorm = rh.dnorm;
        float dacc;
        if (loss.target != nullptr) {                        // training step: the loss lives here (wave-uniform arithmetic)
            const float err = loss.acc[r] - loss.target[r], w = loss.weight[r];
            dacc = 2.0f * w * err;
            if (part == 0u) sums.loss_part += w * err * err;               // once per ray, not once per tile range
        } else dacc = grad_acc[r];
        if (use_zbuf) fill_depths(src, r, near, far, zbuf, lane);

        for (uint32_t k = k_begin; k < k_end; ++k) {
            const uint32_t s = 16u * k + c;
            const bool valid = s < S;
            const uint32_t p = r * S + (valid ? s : S - 1u);
            const Feat16Raw now = ahead;
            {   // the next tile of this item, or the first tile of the wave's next item (a harmless reload at the very end)
                const bool more = k + 1u < k_end;
                const uint32_t next = item + n_waves < n_items ? item + n_waves : item;
                const uint32_t rn = more ? r : ray_of(next);
                const uint32_t sn = more ? s + 16u : 16u * first_tile(next - ray_of(next) * parts) + c;
                load_feat16(feat, B, rn * S + min(sn, S - 1u), g, ahead);
            }
            const float gsig = !valid ? 0.0f
                             : dacc * (use_zbuf ? buffered_dist(zbuf, s, S, dnorm) : sample_dist(src, r, s, near, far, dnorm));
            mlp16_backward_tile(sums, smem, imgs, lane, now, gsig, act, valid, dfeat, B, p);
        }
    }

    NAF_STAMP(2);
    float *slab = slabs + (size_t)blockIdx.x * kSlabStride;
    static_assert(kShAligned >= (kSlabGmax + 1u) * 4u, "the fragment area holds one slab image");
    mlp16_fold_slab(sums, reinterpret_cast<float *>(smem), reinterpret_cast<float *>(smem + kShAligned), threadIdx.x, wib, slab);
#ifdef NAF_MLP_STAMPS
    NAF_STAMP(5);
    if (threadIdx.x == 0u) {
        uint32_t *dbg = reinterpret_cast<uint32_t *>(slab) + 4300u;
        stamp_[3] = stamp_[4] = stamp_[5];                   // (the fold's inner phases are no longer stamped apart)
        for (int i = 0; i < 6; ++i) dbg[i] = (uint32_t)(stamp_[i] - stamp_[0]);
        dbg[6] = (uint32_t)wall0_; dbg[7] = (uint32_t)wall_clock64();
    }
#endif
#undef NAF_STAMP
}

// ---- 3c: MLP forward, loss and backward of a small training step in ONE launch (bf16 mode, C = 2, loss formed in the kernel) -----
// Below ~3 000 rays the pair mlp16_forward_split_kernel / mlp16_backward_kernel is bound by latency, not throughput: each stages
// the weights, each waits for its first features, the line integrals travel to HBM and back, and a launch boundary sits between.
// Here a workgroup of kWaves waves (4 or 12) owns kWaves / parts whole rays and writes kWaves / 4 slabs.  Wave `w` of workgroup
// `b` takes work item kWaves b + w of mlp16_backward_kernel's item list.  At these ray counts that kernel gives every wave one item
// and folds items 4 i .. 4 i + 3 into slab i; so does this one (group of four waves by group), hence every slab is the fold of the
// same four tile ranges in the same order and has the same bits as the pair's -- and so has everything downstream.
//   phase A  forward of the wave's tiles (weights in registers, as in the split kernel); the terms sigma * dist meet in LDS;
//            one workgroup barrier
//   loss     EVERY wave of a ray adds the ray's terms in tile order, then across the 16 lanes -- the order of both forward
//            kernels: same bits, and no second barrier; the wave of the ray's first range stores acc[r] and owns the loss share
//   phase B  mlp16_backward_tile on the same tiles (features re-read: they are L2 hits), then the slab fold per group of four waves
// The depths of the wave's tile range are evaluated once for both phases.  S <= kMaxSamplesLds / 2: the upper half of a wave's
// depth buffer holds its terms.
template <uint32_t kWaves>
__global__ void __launch_bounds__(kWaves * 64u, 3)
mlp16_train_kernel(const uint16_t *__restrict__ feat, const float *__restrict__ mlp, SrcRays src, LossInputs loss, float *__restrict__ acc_out,
                   uint16_t *__restrict__ dfeat, float *__restrict__ slabs, uint32_t n_rays, uint32_t B, int act, uint32_t parts, uint32_t n_slabs,
                   uint32_t *__restrict__ clear_words) {
    static_assert(kWaves % 4u == 0u, "whole slabs per workgroup");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    if (clear_words != nullptr && blockIdx.x == 0u && threadIdx.x < kClearWords) clear_words[threadIdx.x] = 0u;      // see StepExtras
    const uint32_t lane = threadIdx.x & 63u, c = lane & 15u, g = lane >> 4, wib = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    constexpr uint32_t kShAligned = (Mlp16Shared::kBytes + 15u) & ~15u;
    constexpr uint32_t kTermOff = kMaxSamplesLds / 2u;
    unsigned char *imgs = smem + kShAligned + wib * 3u * kImg16;
    float *zall = reinterpret_cast<float *>(smem + kShAligned + kWaves * 3u * kImg16);
    float *zbuf = zall + wib * kMaxSamplesLds;
    static_assert(kWaves * 3u * kImg16 + kWaves * kMaxSamplesLds * 4u >= Mlp16Shared::kStageFloats * 4u, "images and depth buffers stage the weights");
    static_assert(kShAligned + kWaves * (3u * kImg16 + kMaxSamplesLds * 4u) >= (kWaves / 2u) * kShAligned, "two slab images per group of four waves");

    // (kWaves is a multiple of parts: the waves of a ray share a workgroup, and the ray's first range sits `part` waves below)
    const uint32_t S = src.S, tiles = (S + 15u) / 16u;
    auto first_tile = [&](uint32_t part) { return part * tiles / parts; };
    const uint32_t item = blockIdx.x * kWaves + wib;
    const bool has = item < n_rays * parts;                  // (a wave without an item still folds: zeros, like the pair's idle waves)
    const uint32_t r = has ? item / parts : 0u, part = has ? item - r * parts : 0u;
    const uint32_t k_begin = has ? first_tile(part) : 0u, k_end = has ? first_tile(part + 1u) : 0u;
    Mlp16Sums sums;
    sums.clear();

    Feat16Raw ahead;
    if (has) load_feat16(feat, B, r * S + min(16u * k_begin + c, S - 1u), g, ahead);
    Mlp16Shared::build_staged<8, kWaves>(smem, mlp, reinterpret_cast<float *>(smem + kShAligned));
    const float *ray = src.rays + (size_t)r * 8;
    const float dnorm = sqrtf(ray[3] * ray[3] + ray[4] * ray[4] + ray[5] * ray[5]);
    if (has) {
        const float near = ray[6], far = ray[7];
        for (uint32_t s = 16u * k_begin + lane; s < min(S, 16u * k_end + 1u); s += 64u) zbuf[s] = src.depth(r, s, near, far);
    }
    wave_lds_fence<PrecBF16>();
    {   // ---- phase A (the tile loop of mlp16_forward_split_kernel) ----
        Mlp16InRegs wt;
        wt.load(smem, lane);
        Act16 a;
        float *T = zbuf + kTermOff;
        for (uint32_t k0 = k_begin; k0 < k_end; k0 += 4u) {
            float zsel = 0.0f;
#pragma unroll
            for (uint32_t j = 0; j < 4u; ++j) {
                const uint32_t k = k0 + j;
                if (k >= k_end) break;                                   // uniform
                const Feat16Raw now = ahead;
                // next tile of this wave's range, else its first one again: phase B starts there
                load_feat16(feat, B, r * S + min(16u * (k + 1u < k_end ? k + 1u : k_begin) + c, S - 1u), g, ahead);
                const float z4 = mlp16_tile_forward(wt, feat16_operand(now), a);
                zsel = g == j ? z4 : zsel;
            }
            const uint32_t s = 16u * (k0 + g) + c;
            const float sigma = last_act16(act, zsel);
            const float term = s >= S ? 0.0f : sigma * buffered_dist(zbuf, s, S, dnorm);
            if (k0 + g < k_end) T[s] = term;
        }
    }
    __syncthreads();
    float dacc = 0.0f;
    if (has) {
        const float *T0 = zall + (wib - part) * kMaxSamplesLds + kTermOff;      // terms of the ray's first range; range q: + q depth buffers
        float line = 0.0f;
        if (g == 0u)
            for (uint32_t q = 0; q < parts; ++q)
                for (uint32_t k = first_tile(q); k < first_tile(q + 1u); ++k) line += T0[q * kMaxSamplesLds + 16u * k + c];
#pragma unroll
        for (int off = 8; off > 0; off >>= 1) line += __shfl_xor(line, off, 64);     // the 16 points of lane group 0
        if (part == 0u && lane == 0u) acc_out[r] = line;
        const float acc = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, line)));
        const float err = acc - loss.target[r], w = loss.weight[r];
        dacc = 2.0f * w * err;
        if (part == 0u) sums.loss_part += w * err * err;                   // once per ray, not once per tile range
    }
    // ---- phase B ----
    for (uint32_t k = k_begin; k < k_end; ++k) {
        const uint32_t s = 16u * k + c;
        const bool valid = s < S;
        const uint32_t p = r * S + (valid ? s : S - 1u);
        const Feat16Raw now = ahead;
        load_feat16(feat, B, r * S + min(k + 1u < k_end ? s + 16u : s, S - 1u), g, ahead);      // (a harmless reload at the very end)
        const float gsig = !valid ? 0.0f : dacc * buffered_dist(zbuf, s, S, dnorm);
        mlp16_backward_tile(sums, smem, imgs, lane, now, gsig, act, valid, dfeat, B, p);
    }
    const uint32_t grp = wib >> 2, slab_i = blockIdx.x * (kWaves / 4u) + grp;
    mlp16_fold_slab(sums, reinterpret_cast<float *>(smem + 2u * grp * kShAligned), reinterpret_cast<float *>(smem + (2u * grp + 1u) * kShAligned),
                    threadIdx.x & 255u, wib & 3u, slab_i < n_slabs ? slabs + (size_t)slab_i * kSlabStride : nullptr);
}

// ---- 5: slabs -> grad_mlp (+=), loss, gradient maximum: slab_reduce_block (mlp_slabs.h), as a launch of its own ----------------
// (training steps on the binned scatter let spare workgroups of scatter_bin_kernel do it instead: launch_binned_scatter)
__global__ void __launch_bounds__(1024)
mlp_grad_reduce_kernel(SlabReduce sr) {
    __shared__ float part[kReduceGroups][kReduceParams];
    slab_reduce_block<kReduceGroups>(part, sr, blockIdx.x, threadIdx.x);
}

}  // namespace naf
