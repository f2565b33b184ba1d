// tvprox.hip -- the proximal map of the isotropic total variation for gfx950 (naf_tv_prox_step, naf_tv_prox_primal): the hot path
// of the FISTA-TV baseline.  Defined in include/naf_hip.h (V3) and DESIGN.md section 18; the per-voxel arithmetic is
// csrc/tvprox_device.h.
//
// tvprox_step_kernel, one dual iteration in one launch (seven arrays read, six written).  Layout: the slab grid of csrc/slab_grid.h
// (one lane per column of an 8 x 32 tile, a workgroup per tile and chunk of axis 0).  Per slice x it
//   1. stages r_0[x], r_1[x], r_2[x] of the tile plus a halo of one voxel in LDS.  r_0[x] is what the lane fetched as r_0[x + 1]
//      one slice earlier and kept in a register; the r_1 and r_2 planes serve a voxel and its v - e_1 / v - e_2 neighbours from
//      one load;
//   2. computes u = P_C(b - lambda D^T r) on the tile and its low halo (the voxels v, v - e_1, v - e_2 of every lane) into LDS;
//   3. forms q, p_k and r_next of its own voxel from u[x] (LDS), u[x - 1] (its register) and r (LDS), and stores them.
// Two barriers per slice; the LDS planes are double buffered, so slice x + 1 is staged while slower waves still read slice x, and
// the global loads of slice x + 1 fly during steps 2 and 3 of slice x.  A chunk that does not start at slice 0 first runs steps 1
// and 2 on slice a_begin - 1 to have u[x - 1].
// tvprox_primal_kernel is a plain map with neighbour reads, run once per prox.
#include <cmath>

#include "naf_host.h"
#include "slab_grid.h"
#include "tvprox_device.h"

namespace naf {

namespace {

constexpr uint32_t kTileY = kSlabTileY, kTileZ = kSlabTileZ;              // voxels per workgroup along axes 1 and 2 (256 lanes)
constexpr uint32_t kInY = kTileY + 2, kInZ = kTileZ + 2;                  // 10 x 34 staged values per plane
constexpr uint32_t kIn = kInY * kInZ;              // 340
constexpr uint32_t kLoads = (kIn + 255u) / 256u;   // staged elements per lane (2)
constexpr uint32_t kMinChunk = 8;                  // no chunk shorter than this (each recomputes one slice of u)
constexpr uint32_t kPrimalThreads = 256;

// r and r_next are different buffers and p is only touched at the lane's own voxel, so every pointer may be __restrict__.
__global__ void __launch_bounds__(256)
tvprox_step_kernel(const float *__restrict__ b, const float *__restrict__ r, float *__restrict__ p, float *__restrict__ r_next,
                   uint32_t n1, uint32_t n2, uint32_t n3, uint32_t tiles_y, uint32_t tiles_z, uint32_t chunk, float lambda,
                   float step, float momentum, int nonneg) {
    __shared__ float rs[2][3][kIn];                // r_a[x] of the tile and its halo, slice x in buffer x & 1
    __shared__ float us[2][kIn];                   // u[x] on the rows 0 .. kTileY and columns 0 .. kTileZ of the same layout

    const uint32_t tid = threadIdx.x;
    const SlabLane l = slab_lane(tiles_y, tiles_z, chunk);
    const uint32_t y0 = l.y0, z0 = l.z0, ly = l.ly, lz = l.lz;
    const uint32_t y = y0 + ly, z = z0 + lz;
    const bool valid = y < n2 && z < n3;
    const uint32_t a_begin = l.a_begin, a_end = min(a_begin + chunk, n1);
    const uint32_t x_first = a_begin > 0 ? a_begin - 1u : 0u;             // the slice before the chunk gives u[x - 1]
    const uint64_t slice = (uint64_t)n2 * n3, volume = slice * n1;        // 64-bit: a 1024^3 fp32 volume is 4 GiB

    // staged element e = row * kInZ + col holds voxel (y0 + row - 1, z0 + col - 1).  Positions outside the volume are staged as
    // 0 and never used (their flag is false).  r_1 needs the rows up to y0 + kTileY and r_2 the columns up to z0 + kTileZ (the
    // v + e_a terms of D^T at the tile's last row and column); u, b and r_0 live on the rows and columns below those (`inner`).
    uint64_t off[kLoads];
    bool in[kLoads], inner[kLoads], lo1[kLoads], hi1[kLoads], lo2[kLoads], hi2[kLoads];
#pragma unroll
    for (uint32_t k = 0; k < kLoads; ++k) {
        const uint32_t e = tid + 256u * k, row = e / kInZ, col = e - row * kInZ;
        const uint32_t gy = y0 + row - 1u, gz = z0 + col - 1u;            // wraps to >= n for row / col 0 of the first tile
        in[k] = e < kIn && gy < n2 && gz < n3;
        inner[k] = e < kIn && row < kInY - 1u && col < kInZ - 1u;
        off[k] = in[k] ? (uint64_t)gy * n3 + gz : 0;
        lo1[k] = gy > 0;
        hi1[k] = gy + 1u < n2;
        lo2[k] = gz > 0;
        hi2[k] = gz + 1u < n3;
    }
    const uint64_t column = (uint64_t)y * n3 + z;

    // what the lane holds of the slice being fetched: r_0 of the slice after it, r_1, r_2 and b at its staged elements, and
    // p_{k-1} at its own voxel
    float f_r0n[kLoads], f_r1[kLoads], f_r2[kLoads], f_b[kLoads], f_p[3];
    auto fetch = [&](uint32_t s) {
        const uint64_t base = (uint64_t)s * slice;
#pragma unroll
        for (uint32_t k = 0; k < kLoads; ++k) {
            const bool own = in[k] && inner[k];
            f_r0n[k] = own && s + 1u < n1 ? r[base + slice + off[k]] : 0.0f;
            f_r1[k] = in[k] ? r[volume + base + off[k]] : 0.0f;
            f_r2[k] = in[k] ? r[2u * volume + base + off[k]] : 0.0f;
            f_b[k] = own ? b[base + off[k]] : 0.0f;
        }
        const bool mine = valid && s >= a_begin;
#pragma unroll
        for (uint32_t a = 0; a < 3; ++a) f_p[a] = mine ? p[a * volume + base + column] : 0.0f;
    };

    float r0[kLoads];                              // r_0[x] at the lane's staged elements
#pragma unroll
    for (uint32_t k = 0; k < kLoads; ++k) r0[k] = in[k] && inner[k] ? r[(uint64_t)x_first * slice + off[k]] : 0.0f;
    fetch(x_first);

    bool has_lo[3];
    has_lo[1] = y > 0;
    has_lo[2] = z > 0;
    const uint32_t ci = (ly + 1u) * kInZ + (lz + 1u);
    float u_prev = 0.0f;
    for (uint32_t x = x_first; x < a_end; ++x) {
        const uint32_t buf = x & 1u;
        float c_r0n[kLoads], c_b[kLoads], p_old[3];
#pragma unroll
        for (uint32_t k = 0; k < kLoads; ++k) {
            const uint32_t e = tid + 256u * k;
            if (e < kIn) {
                rs[buf][0][e] = r0[k];
                rs[buf][1][e] = f_r1[k];
                rs[buf][2][e] = f_r2[k];
            }
            c_r0n[k] = f_r0n[k];
            c_b[k] = f_b[k];
        }
#pragma unroll
        for (uint32_t a = 0; a < 3; ++a) p_old[a] = f_p[a];
        __syncthreads();                           // slice x is staged; also orders the readers of this buffer (slice x - 2)
        if (x + 1u < a_end) fetch(x + 1u);         // the next slice's loads fly during the arithmetic

#pragma unroll
        for (uint32_t k = 0; k < kLoads; ++k) {
            const uint32_t e = tid + 256u * k;
            if (inner[k]) {
                const float lo[3] = {r0[k], rs[buf][1][e], rs[buf][2][e]};
                const float hi[3] = {c_r0n[k], rs[buf][1][e + kInZ], rs[buf][2][e + 1u]};
                const bool e_lo[3] = {x > 0, lo1[k], lo2[k]}, e_hi[3] = {x + 1u < n1, hi1[k], hi2[k]};
                us[buf][e] = tvprox_primal(c_b[k], tvprox_adjoint(lo, hi, e_lo, e_hi), lambda, nonneg != 0);
            }
            r0[k] = c_r0n[k];
        }
        __syncthreads();                           // u[x] of the tile and its low halo is in LDS

        const float u = us[buf][ci];
        if (valid && x >= a_begin) {
            const float u_lo[3] = {u_prev, us[buf][ci - kInZ], us[buf][ci - 1u]};
            const float rr[3] = {rs[buf][0][ci], rs[buf][1][ci], rs[buf][2][ci]};
            has_lo[0] = x > 0;
            float p_new[3], rn[3];
            tvprox_dual(u, u_lo, rr, p_old, has_lo, step, momentum, p_new, rn);
            const uint64_t at = (uint64_t)x * slice + column;
#pragma unroll
            for (uint32_t a = 0; a < 3; ++a) {
                p[a * volume + at] = p_new[a];
                if (r_next) r_next[a * volume + at] = rn[a];
            }
        }
        u_prev = u;
    }
}

// One lane per voxel, lanes along axis 2: block = (slice x, row y, 256 columns).  x may be b: a voxel reads b only at itself.
__global__ void __launch_bounds__(kPrimalThreads)
tvprox_primal_kernel(const float *b, const float *__restrict__ p, float *x, uint32_t n1, uint32_t n2, uint32_t n3, uint32_t tiles_z,
                     float lambda, int nonneg) {
    const uint32_t tile = blockIdx.x % tiles_z, rest = blockIdx.x / tiles_z;
    const uint32_t vy = rest % n2, vx = rest / n2;
    const uint32_t vz = tile * kPrimalThreads + threadIdx.x;
    if (vz >= n3) return;
    const uint64_t slice = (uint64_t)n2 * n3, volume = slice * n1;
    const uint64_t at = (uint64_t)vx * slice + (uint64_t)vy * n3 + vz;
    const bool has_lo[3] = {vx > 0, vy > 0, vz > 0}, has_hi[3] = {vx + 1u < n1, vy + 1u < n2, vz + 1u < n3};
    const uint64_t stride[3] = {slice, n3, 1};
    float lo[3], hi[3];
#pragma unroll
    for (uint32_t a = 0; a < 3; ++a) {
        lo[a] = has_lo[a] ? p[a * volume + at] : 0.0f;
        hi[a] = has_hi[a] ? p[a * volume + at + stride[a]] : 0.0f;
    }
    x[at] = tvprox_primal(b[at], tvprox_adjoint(lo, hi, has_lo, has_hi), lambda, nonneg != 0);
}

}  // namespace

}  // namespace naf

using namespace naf;

extern "C" int naf_tv_prox_step(const float *b, const float *r, float *p, float *r_next, uint32_t n1, uint32_t n2, uint32_t n3,
                                float lambda, float momentum, int nonneg, void *stream) {
    if (!b || !r || !p) return fail(NAF_ERR_INVALID_ARGUMENT, "tv_prox_step: null pointer");
    if (r_next == r) return fail(NAF_ERR_INVALID_ARGUMENT, "tv_prox_step: r_next must not be r (a voxel's neighbours read r)");
    if (n1 == 0 || n2 == 0 || n3 == 0) return fail_who("tv_prox_step", "zero volume dimension", NAF_ERR_UNSUPPORTED);
    if (!std::isfinite(lambda) || !(lambda > 0.0f))
        return fail(NAF_ERR_INVALID_ARGUMENT, "tv_prox_step: lambda must be > 0 and finite");
    if (!std::isfinite(momentum) || momentum < 0.0f)
        return fail(NAF_ERR_INVALID_ARGUMENT, "tv_prox_step: momentum must be >= 0 and finite");
    const SlabGrid g = slab_grid(n1, n2, n3, kMinChunk);
    if (g.blocks > 0x7fffffffull) return fail_who("tv_prox_step", "volume too large for one call");
    return launch("tvprox_step_kernel", tvprox_step_kernel, dim3((uint32_t)g.blocks), dim3(256), 0, (hipStream_t)stream, b, r, p, r_next,
                  n1, n2, n3, g.tiles_y, g.tiles_z, g.chunk, lambda, tvprox_dual_step(lambda), momentum, nonneg);
}

extern "C" int naf_tv_prox_primal(const float *b, const float *p, float *x, uint32_t n1, uint32_t n2, uint32_t n3, float lambda,
                                  int nonneg, void *stream) {
    if (!b || !p || !x) return fail(NAF_ERR_INVALID_ARGUMENT, "tv_prox_primal: null pointer");
    if (n1 == 0 || n2 == 0 || n3 == 0) return fail_who("tv_prox_primal", "zero volume dimension", NAF_ERR_UNSUPPORTED);
    if (!std::isfinite(lambda) || lambda < 0.0f)
        return fail(NAF_ERR_INVALID_ARGUMENT, "tv_prox_primal: lambda must be >= 0 and finite");
    const uint32_t tiles_z = (n3 + kPrimalThreads - 1u) / kPrimalThreads;
    const uint64_t blocks = (uint64_t)n1 * n2 * tiles_z;
    if (blocks > 0x7fffffffull) return fail_who("tv_prox_primal", "volume too large for one call");
    return launch("tvprox_primal_kernel", tvprox_primal_kernel, dim3((uint32_t)blocks), dim3(kPrimalThreads), 0, (hipStream_t)stream, b, p,
                  x, n1, n2, n3, tiles_z, lambda, nonneg);
}
