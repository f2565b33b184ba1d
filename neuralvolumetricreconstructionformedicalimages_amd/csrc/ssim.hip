// ssim.hip -- 3-D SSIM of two fp32 volumes for gfx950 (naf_ssim_3d): the reference's `ssim_3d` evaluation metric
// (src/utils/util.py:87-139 with scikit-image 0.19.3 defaults), defined in include/naf_hip.h (M1) and DESIGN.md section 11.
//
// Layout: the slab grid of csrc/slab_grid.h over the window starts (one lane per column of an 8 x 32 tile of them, a workgroup per
// tile and chunk of axis 0).  For each x slice it stages the (kTileY + 6) x (kTileZ + 6) fp32 input tile of both volumes in LDS, forms
// the 7-tap sums of the five moments along axis 2 (row pass, fp64 into LDS) and then along axis 1 (column pass, per lane), and keeps
// the last seven slice sums of each lane in registers: their sum is the 7 x 7 x 7 window.  A chunk starts with 6 warm-up slices.
// Nothing full-size is written; every workgroup writes one fp64 partial sum of S and a second one-workgroup kernel adds the
// partials in the fixed order of csrc/block_sum.h (no atomics: two calls return the same bits).
#include <cstdio>

#include "block_sum.h"
#include "naf_host.h"
#include "slab_grid.h"

namespace naf {

namespace {

constexpr uint32_t kWin = 7;                       // window edge; N_P = 343
constexpr uint32_t kTileY = kSlabTileY, kTileZ = kSlabTileZ;              // window starts per workgroup along axes 1 and 2 (256 lanes)
constexpr uint32_t kInY = kTileY + kWin - 1, kInZ = kTileZ + kWin - 1;    // 14 x 38 staged inputs
constexpr uint32_t kIn = kInY * kInZ;              // 532
constexpr uint32_t kLoads = (kIn + 255u) / 256u;   // staged elements per lane and volume (3)
constexpr uint32_t kRows = kInY * kTileZ;          // row-pass outputs (448)
constexpr uint32_t kMinChunk = 16;                 // no chunk shorter than this (each has 6 warm-up slices)
constexpr uint32_t kReduceThreads = 256;

uint64_t ssim_workspace_bytes(const SlabGrid &g) { return (g.blocks * sizeof(double) + 255u) & ~(uint64_t)255u; }

// S of one window from its five moment sums (skimage.metrics.structural_similarity, gaussian_weights=False, data_range=2).
__device__ __forceinline__ double ssim_of(double sx, double sy, double sxx, double syy, double sxy) {
    const double inv_np = 1.0 / 343.0, cov_norm = 343.0 / 342.0;
    const double C1 = (0.01 * 2.0) * (0.01 * 2.0), C2 = (0.03 * 2.0) * (0.03 * 2.0);
    const double ux = sx * inv_np, uy = sy * inv_np, uxx = sxx * inv_np, uyy = syy * inv_np, uxy = sxy * inv_np;
    const double vx = cov_norm * (uxx - ux * ux), vy = cov_norm * (uyy - uy * uy), vxy = cov_norm * (uxy - ux * uy);
    const double A1 = 2.0 * ux * uy + C1, A2 = 2.0 * vxy + C2;
    const double B1 = ux * ux + uy * uy + C1, B2 = vx + vy + C2;
    return (A1 * A2) / (B1 * B2);
}

__global__ void __launch_bounds__(256)
ssim_partial_kernel(const float *__restrict__ x, const float *__restrict__ y, uint32_t n1, uint32_t n2, uint32_t n3,
                    uint32_t tiles_y, uint32_t tiles_z, uint32_t chunk, double *__restrict__ partials) {
    __shared__ float xs[kIn], ys[kIn];
    __shared__ double rows[5][kRows];              // 7-tap sums along axis 2 of x, y, xx, yy, xy
    __shared__ double red[256];

    const uint32_t tid = threadIdx.x;
    const SlabLane l = slab_lane(tiles_y, tiles_z, chunk);
    const uint32_t y0 = l.y0, z0 = l.z0, ly = l.ly, lz = l.lz;
    const bool valid = y0 + ly < n2 - 6 && z0 + lz < n3 - 6;     // this lane's window start is interior
    const uint32_t a_begin = l.a_begin, a_end = min(a_begin + chunk, n1 - 6);
    const uint32_t s_end = a_end + 6;                              // input slices [a_begin, s_end), s_end <= n1

    // staged element e = row * kInZ + col of the tile; elements outside the volume feed no valid window and are staged as 0
    uint64_t off[kLoads];
    bool in[kLoads];
#pragma unroll
    for (uint32_t k = 0; k < kLoads; ++k) {
        const uint32_t e = tid + 256u * k, r = e / kInZ, col = e - r * kInZ;
        in[k] = e < kIn && y0 + r < n2 && z0 + col < n3;
        off[k] = in[k] ? (uint64_t)(y0 + r) * n3 + (z0 + col) : 0;   // 64-bit: a 1024^3 fp32 volume is 4 GiB
    }
    const uint64_t slice = (uint64_t)n2 * n3;
    float px[kLoads], py[kLoads];
    auto fetch = [&](uint32_t s) {
        const uint64_t base = (uint64_t)s * slice;
#pragma unroll
        for (uint32_t k = 0; k < kLoads; ++k) {
            px[k] = in[k] ? x[base + off[k]] : 0.0f;
            py[k] = in[k] ? y[base + off[k]] : 0.0f;
        }
    };
    fetch(a_begin);

    double ring[kWin][5];                          // slice sums of the last seven slices (slot = (s - a_begin) mod 7)
    double acc = 0.0;
    for (uint32_t s0 = a_begin; s0 < s_end; s0 += kWin) {
#pragma unroll
        for (uint32_t u = 0; u < kWin; ++u) {      // unrolled: every ring slot has a static index
            const uint32_t s = s0 + u;
            if (s >= s_end) break;                 // workgroup-uniform
#pragma unroll
            for (uint32_t k = 0; k < kLoads; ++k) {
                const uint32_t e = tid + 256u * k;
                if (e < kIn) {
                    xs[e] = px[k];
                    ys[e] = py[k];
                }
            }
            __syncthreads();
            if (s + 1 < s_end) fetch(s + 1);       // the next slice's loads fly during both passes
            for (uint32_t i = tid; i < kRows; i += 256u) {
                const uint32_t r = i / kTileZ, col = i % kTileZ;
                double sx = 0.0, sy = 0.0, sxx = 0.0, syy = 0.0, sxy = 0.0;
#pragma unroll
                for (uint32_t d = 0; d < kWin; ++d) {
                    const double a = (double)xs[r * kInZ + col + d], b = (double)ys[r * kInZ + col + d];
                    sx += a;
                    sy += b;
                    sxx += a * a;
                    syy += b * b;
                    sxy += a * b;
                }
                rows[0][i] = sx;
                rows[1][i] = sy;
                rows[2][i] = sxx;
                rows[3][i] = syy;
                rows[4][i] = sxy;
            }
            __syncthreads();
#pragma unroll
            for (uint32_t m = 0; m < 5; ++m) {
                double t = 0.0;
#pragma unroll
                for (uint32_t d = 0; d < kWin; ++d) t += rows[m][(ly + d) * kTileZ + lz];
                ring[u][m] = t;
            }
            if (valid && s >= a_begin + kWin - 1) {                 // the window [s - 6, s] along axis 0 is complete
                double w[5];
#pragma unroll
                for (uint32_t m = 0; m < 5; ++m) {
                    w[m] = ring[0][m];
#pragma unroll
                    for (uint32_t v = 1; v < kWin; ++v) w[m] += ring[v][m];
                }
                acc += ssim_of(w[0], w[1], w[2], w[3], w[4]);
            }
        }
    }

    // The tree of block_sum.h, written out: inlined from there, the compiler schedules this kernel's last level differently, and the
    // kernels here keep the machine code they were measured with.  The order of the additions is the same.
    red[tid] = acc;
    __syncthreads();
    for (uint32_t h = 128; h > 0; h >>= 1) {
        if (tid < h) red[tid] += red[tid + h];
        __syncthreads();
    }
    if (tid == 0) partials[blockIdx.x] = red[0];
}

__global__ void __launch_bounds__(kReduceThreads)
ssim_reduce_kernel(const double *__restrict__ partials, uint64_t n_partials, double count, double *__restrict__ out) {
    __shared__ double red[kReduceThreads];
    const uint32_t tid = threadIdx.x;
    red[tid] = strided_sum<kReduceThreads>(partials, n_partials, tid);
    __syncthreads();
    for (uint32_t h = kReduceThreads / 2; h > 0; h >>= 1) {                // as above
        if (tid < h) red[tid] += red[tid + h];
        __syncthreads();
    }
    if (tid == 0) out[0] = red[0] / count;
}

}  // namespace

}  // namespace naf

using namespace naf;

extern "C" size_t naf_ssim_3d_workspace_bytes(uint32_t n1, uint32_t n2, uint32_t n3) {
    if (n1 < kWin || n2 < kWin || n3 < kWin) return 0;
    return (size_t)ssim_workspace_bytes(slab_grid(n1 - 6, n2 - 6, n3 - 6, kMinChunk));
}

extern "C" int naf_ssim_3d(const float *x, const float *y, uint32_t n1, uint32_t n2, uint32_t n3, double *out, void *workspace,
                           size_t workspace_bytes, void *stream) {
    if (!x || !y || !out || !workspace) return fail(NAF_ERR_INVALID_ARGUMENT, "ssim_3d: null pointer");
    char msg[160];
    if (n1 < kWin || n2 < kWin || n3 < kWin) {
        std::snprintf(msg, sizeof(msg), "ssim_3d: win_size exceeds image extent (every extent must be >= 7, got %u x %u x %u)",
                      n1, n2, n3);
        return fail(NAF_ERR_INVALID_ARGUMENT, msg);
    }
    const SlabGrid g = slab_grid(n1 - 6, n2 - 6, n3 - 6, kMinChunk);           // over the window starts
    if (g.blocks > 0x7fffffffull) return fail(NAF_ERR_INVALID_ARGUMENT, "ssim_3d: volume too large for one call");
    const uint64_t need = ssim_workspace_bytes(g);
    if (workspace_bytes < need) return workspace_too_small("ssim_3d", workspace_bytes, need);
    if (!aligned(workspace, 7u)) return misaligned("ssim_3d", "workspace", 8);
    double *partials = static_cast<double *>(workspace);
    const double count = (double)(n1 - 6) * (double)(n2 - 6) * (double)(n3 - 6);
    const int rc = launch("ssim_partial_kernel", ssim_partial_kernel, dim3((uint32_t)g.blocks), dim3(256), 0, (hipStream_t)stream, x, y,
                          n1, n2, n3, g.tiles_y, g.tiles_z, g.chunk, partials);
    if (rc != NAF_OK) return rc;
    return launch("ssim_reduce_kernel", ssim_reduce_kernel, dim3(1), dim3(kReduceThreads), 0, (hipStream_t)stream, partials, g.blocks,
                  count, out);
}
