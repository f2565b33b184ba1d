// tv.hip -- 3-D total variation of an fp32 volume, its gradient and normalised steepest descent on it for gfx950
// (naf_tv_gradient, naf_tv_descent): the regulariser of the ASD-POCS baseline.  Defined in include/naf_hip.h (V2) and DESIGN.md
// section 14; the per-voxel arithmetic is csrc/tv_device.h.
//
// Layout: the slab grid of csrc/slab_grid.h (one lane per column of an 8 x 32 tile, a workgroup per tile and chunk of axis 0).  Every
// slice's tile plus a halo of one voxel is staged in LDS once, four slots deep, so that the slices x - 1, x and x + 1 of the 13-point
// stencil are there with one barrier per slice while slice x + 2 is in flight.
//   tv_kernel<kGradient>  writes g and one fp64 partial of sum m and of sum g^2 per workgroup
//   tv_kernel<kPartials>  the same without the store of g (descent, first pass)
//   tv_reduce_kernel      adds the partials in a fixed order into stats[0..1] (csrc/block_sum.h: two calls return the same bits)
//   tv_kernel<kUpdate>    recomputes g and writes f - (step / ||g||) g to the other buffer (descent, second pass)
// A descent step therefore reads the volume twice and writes it once; g is never materialised.
#include <cmath>

#include "block_sum.h"
#include "naf_host.h"
#include "slab_grid.h"
#include "tv_device.h"

namespace naf {

namespace {

constexpr uint32_t kTileY = kSlabTileY, kTileZ = kSlabTileZ;              // voxels per workgroup along axes 1 and 2 (256 lanes)
constexpr uint32_t kInY = kTileY + 2, kInZ = kTileZ + 2;                  // 10 x 34 staged values per slice
constexpr uint32_t kIn = kInY * kInZ;              // 340
constexpr uint32_t kLoads = (kIn + 255u) / 256u;   // staged elements per lane (2)
constexpr uint32_t kSlots = 4;                     // slices kept in LDS
constexpr uint32_t kMinChunk = 8;                  // no chunk shorter than this (each reads 2 halo slices)
constexpr uint32_t kReduceThreads = 256;

enum TvMode { kGradient = 0, kPartials = 1, kUpdate = 2 };

uint64_t tv_workspace_bytes(const SlabGrid &g) { return (g.blocks * 2u * sizeof(double) + 255u) & ~(uint64_t)255u; }

template <int kMode>
__global__ void __launch_bounds__(256)
tv_kernel(const float *__restrict__ f, uint32_t n1, uint32_t n2, uint32_t n3, uint32_t tiles_y, uint32_t tiles_z, uint32_t chunk,
          float eps, float step, float *__restrict__ out, double *__restrict__ partials, const double *__restrict__ stats) {
    __shared__ float tile[kSlots][kIn];            // slice s lives in slot (s + 1) & 3
    __shared__ double red[2][256];

    const uint32_t tid = threadIdx.x;
    const SlabLane l = slab_lane(tiles_y, tiles_z, chunk);
    const uint32_t y0 = l.y0, z0 = l.z0, ly = l.ly, lz = l.lz;
    const uint32_t y = y0 + ly, z = z0 + lz;
    const bool valid = y < n2 && z < n3;
    const uint32_t a_begin = l.a_begin, a_end = min(a_begin + chunk, n1);

    // staged element e = row * kInZ + col holds voxel (y0 + row - 1, z0 + col - 1); positions outside the volume are staged as 0
    // and never used (their has_lo / has_hi flag is false)
    uint64_t off[kLoads];
    bool in[kLoads];
#pragma unroll
    for (uint32_t k = 0; k < kLoads; ++k) {
        const uint32_t e = tid + 256u * k, r = e / kInZ, col = e - r * kInZ;
        const uint32_t gy = y0 + r - 1u, gz = z0 + col - 1u;              // wraps to >= n for row / col 0 of the first tile
        in[k] = e < kIn && gy < n2 && gz < n3;
        off[k] = in[k] ? (uint64_t)gy * n3 + gz : 0;                      // 64-bit: a 1024^3 fp32 volume is 4 GiB
    }
    const uint64_t slice = (uint64_t)n2 * n3;
    float pf[kLoads];
    auto fetch = [&](uint32_t s) {
        const uint64_t base = (uint64_t)s * slice;
#pragma unroll
        for (uint32_t k = 0; k < kLoads; ++k) pf[k] = in[k] ? f[base + off[k]] : 0.0f;
    };
    auto put = [&](uint32_t s) {
        float *slot = tile[(s + 1u) & (kSlots - 1u)];
#pragma unroll
        for (uint32_t k = 0; k < kLoads; ++k) {
            const uint32_t e = tid + 256u * k;
            if (e < kIn) slot[e] = pf[k];
        }
    };

    float scale = 0.0f;
    if (kMode == kUpdate) scale = tv_step_scale(stats[1], step);

    if (a_begin > 0) {
        fetch(a_begin - 1);
        put(a_begin - 1);
    }
    fetch(a_begin);
    put(a_begin);
    if (a_begin + 1 < n1) fetch(a_begin + 1);

    TvStencil st;
    st.has_lo[1] = y > 0;
    st.has_lo[2] = z > 0;
    st.has_hi[1] = y + 1 < n2;
    st.has_hi[2] = z + 1 < n3;
    const uint32_t ci = (ly + 1u) * kInZ + (lz + 1u);
    const uint64_t column = (uint64_t)y * n3 + z;
    double sum_m = 0.0, sum_g2 = 0.0;
    for (uint32_t x = a_begin; x < a_end; ++x) {
        if (x + 1 < n1) put(x + 1);
        __syncthreads();                           // also orders this slot's last readers (iteration x - 2) before its writers
        if (x + 2 < n1 && x + 2 <= a_end) fetch(x + 2);                   // the next slice's loads fly during the arithmetic
        const float *prev = tile[x & (kSlots - 1u)], *cur = tile[(x + 1u) & (kSlots - 1u)], *next = tile[(x + 2u) & (kSlots - 1u)];
        st.has_lo[0] = x > 0;
        st.has_hi[0] = x + 1 < n1;
        st.c = cur[ci];
        st.lo[0] = prev[ci];
        st.lo[1] = cur[ci - kInZ];
        st.lo[2] = cur[ci - 1u];
        st.hi[0] = next[ci];
        st.hi[1] = cur[ci + kInZ];
        st.hi[2] = cur[ci + 1u];
        st.diag[0][0] = st.diag[1][1] = st.diag[2][2] = 0.0f;
        st.diag[0][1] = next[ci - kInZ];
        st.diag[0][2] = next[ci - 1u];
        st.diag[1][0] = prev[ci + kInZ];
        st.diag[1][2] = cur[ci + kInZ - 1u];
        st.diag[2][0] = prev[ci + 1u];
        st.diag[2][1] = cur[ci + 1u - kInZ];
        float m;
        const float g = tv_point(st, eps, &m);
        if (valid) {
            if (kMode == kUpdate) {
                out[(uint64_t)x * slice + column] = tv_step_apply(st.c, g, scale);
            } else {
                if (kMode == kGradient) out[(uint64_t)x * slice + column] = g;
                sum_m += (double)m;
                sum_g2 += (double)g * (double)g;
            }
        }
    }
    if (kMode == kUpdate) return;

    block_sum<256>(red, sum_m, sum_g2, tid);
    if (tid == 0) {
        partials[2u * (uint64_t)blockIdx.x] = red[0][0];
        partials[2u * (uint64_t)blockIdx.x + 1u] = red[1][0];
    }
}

__global__ void __launch_bounds__(kReduceThreads)
tv_reduce_kernel(const double *__restrict__ partials, uint64_t n_partials, double *__restrict__ stats) {
    __shared__ double red[2][kReduceThreads];
    const uint32_t tid = threadIdx.x;
    double t = 0.0, u = 0.0;
    for (uint64_t i = tid; i < n_partials; i += kReduceThreads) {      // the two interleaved sums, each in ascending order
        t += partials[2u * i];
        u += partials[2u * i + 1u];
    }
    block_sum<kReduceThreads>(red, t, u, tid);
    if (tid == 0) {
        stats[0] = red[0][0];
        stats[1] = red[1][0];
    }
}

// Argument checks shared by the two entry points; fills the grid.
int tv_check(const char *who, uint32_t n1, uint32_t n2, uint32_t n3, float eps, const void *workspace, size_t workspace_bytes,
             SlabGrid *g) {
    if (n1 == 0 || n2 == 0 || n3 == 0) return fail_who(who, "zero volume dimension");
    if (!(eps > 0.0f) || !std::isfinite(eps)) return fail_who(who, "eps must be > 0 and finite");
    *g = slab_grid(n1, n2, n3, kMinChunk);
    if (g->blocks > 0x7fffffffull) return fail_who(who, "volume too large for one call");
    const uint64_t need = tv_workspace_bytes(*g);
    if (workspace_bytes < need) return workspace_too_small(who, workspace_bytes, need);
    if (!aligned(workspace, 7u)) return misaligned(who, "workspace", 8);
    return NAF_OK;
}

template <int kMode>
int tv_launch(const char *name, const SlabGrid &g, const float *f, uint32_t n1, uint32_t n2, uint32_t n3, float eps, float step,
              float *out, double *partials, const double *stats, hipStream_t stream) {
    return launch(name, tv_kernel<kMode>, dim3((uint32_t)g.blocks), dim3(256), 0, stream, f, n1, n2, n3, g.tiles_y, g.tiles_z, g.chunk,
                  eps, step, out, partials, stats);
}

int tv_reduce(const SlabGrid &g, const double *partials, double *stats, hipStream_t stream) {
    return launch("tv_reduce_kernel", tv_reduce_kernel, dim3(1), dim3(kReduceThreads), 0, stream, partials, g.blocks, stats);
}

}  // namespace

}  // namespace naf

using namespace naf;

extern "C" size_t naf_tv_workspace_bytes(uint32_t n1, uint32_t n2, uint32_t n3) {
    if (n1 == 0 || n2 == 0 || n3 == 0) return 0;
    return (size_t)tv_workspace_bytes(slab_grid(n1, n2, n3, kMinChunk));
}

extern "C" int naf_tv_gradient(const float *x, uint32_t n1, uint32_t n2, uint32_t n3, float eps, float *grad, double *stats,
                               void *workspace, size_t workspace_bytes, void *stream) {
    if (!x || !grad || !stats || !workspace) return fail(NAF_ERR_INVALID_ARGUMENT, "tv_gradient: null pointer");
    if (x == grad) return fail(NAF_ERR_INVALID_ARGUMENT, "tv_gradient: grad must not be x (a voxel's neighbours read x)");
    SlabGrid g;
    int rc = tv_check("tv_gradient", n1, n2, n3, eps, workspace, workspace_bytes, &g);
    if (rc != NAF_OK) return rc;
    double *partials = static_cast<double *>(workspace);
    rc = tv_launch<kGradient>("tv_gradient_kernel", g, x, n1, n2, n3, eps, 0.0f, grad, partials, nullptr, (hipStream_t)stream);
    if (rc != NAF_OK) return rc;
    return tv_reduce(g, partials, stats, (hipStream_t)stream);
}

extern "C" int naf_tv_descent(float *x, float *scratch, uint32_t n1, uint32_t n2, uint32_t n3, float step, uint32_t n_steps,
                              float eps, double *stats, void *workspace, size_t workspace_bytes, void *stream) {
    if (!x || !scratch || !stats || !workspace) return fail(NAF_ERR_INVALID_ARGUMENT, "tv_descent: null pointer");
    SlabGrid g;
    int rc = tv_check("tv_descent", n1, n2, n3, eps, workspace, workspace_bytes, &g);
    if (rc != NAF_OK) return rc;
    if (!std::isfinite(step) || step < 0.0f) return fail(NAF_ERR_INVALID_ARGUMENT, "tv_descent: step must be >= 0 and finite");
    if (x == scratch) return fail(NAF_ERR_INVALID_ARGUMENT, "tv_descent: scratch must not be x");
    if (n_steps == 0) return NAF_OK;
    double *partials = static_cast<double *>(workspace);
    hipStream_t s = (hipStream_t)stream;
    float *src = x, *dst = scratch;
    if (n_steps & 1u) {
        // an odd count would end in `scratch`: start from a copy there, so that the last step writes x
        const size_t bytes = (size_t)n1 * n2 * n3 * sizeof(float);
        if (hipMemcpyAsync(scratch, x, bytes, hipMemcpyDeviceToDevice, s) != hipSuccess) {
            (void)hipGetLastError();
            return fail(NAF_ERR_LAUNCH, "tv_descent: device copy failed");
        }
        src = scratch;
        dst = x;
    }
    for (uint32_t i = 0; i < n_steps; ++i) {
        rc = tv_launch<kPartials>("tv_partials_kernel", g, src, n1, n2, n3, eps, 0.0f, nullptr, partials, nullptr, s);
        if (rc != NAF_OK) return rc;
        rc = tv_reduce(g, partials, stats, s);
        if (rc != NAF_OK) return rc;
        rc = tv_launch<kUpdate>("tv_update_kernel", g, src, n1, n2, n3, eps, step, dst, nullptr, stats, s);
        if (rc != NAF_OK) return rc;
        std::swap(src, dst);
    }
    return NAF_OK;
}
