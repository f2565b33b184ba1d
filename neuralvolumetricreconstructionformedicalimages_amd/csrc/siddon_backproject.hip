// siddon_backproject.hip -- the exact transpose of the ray-voxel intersection ("Siddon") projector for gfx950:
// naf_backproject_rays_siddon scatters one value per ray into a voxel volume, naf_backproject_scan_siddon does it for every pixel
// ray of a scan.  With A = naf_project_scan_siddon this is A^T to rounding and summation order: the span, the end-point indices, the
// crossings, the tie order and the chord length of every step come from siddon_device.h, the code the forward kernel runs.  Defined
// in include/naf_hip.h (P7) and DESIGN.md section 21.
//
// Layout of the scan kernel: scan_launch.h's, rays made in registers, so the 64 lanes of a wave (8 x 8 pixels) at equal step add
// into a small neighbourhood of the volume.  One no-return fp32 hardware atomic per voxel of positive chord length; a group of
// kSiddonGroup steps is walked before its atomics are issued, and nothing waits for them.
#include "siddon_launch.h"

namespace naf {

namespace {

__global__ void __launch_bounds__(256)
siddon_backproject_rays_kernel(SiddonGrid grid, float *__restrict__ volume, const float *__restrict__ values,
                               const float *__restrict__ rays, uint64_t n_rays) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_rays) return;
    const float4 *r = reinterpret_cast<const float4 *>(rays + i * 8);
    siddon_transpose(grid, siddon_ray(r[0], r[1]), SiddonDepositValue{volume, values[i]});
}

// The launch's poses and projections come pre-offset to its first view.
__global__ void __launch_bounds__(256)
siddon_backproject_scan_kernel(SiddonGrid grid, float *__restrict__ volume, const float *__restrict__ projections,
                               const float *__restrict__ poses, RayGeo g, uint32_t tiles_x, uint32_t tiles_per_view) {
    ScanPixel p;
    if (!scan_pixel(tiles_x, tiles_per_view, g, p)) return;
    float4 r[2];
    make_pixel_ray(poses + (size_t)p.j * 12, p.row, p.col, g, r);
    siddon_transpose(grid, siddon_ray(r[0], r[1]), SiddonDepositValue{volume, projections[(uint64_t)p.j * g.W * g.H + p.pixel]});
}

}  // namespace

}  // namespace naf

using namespace naf;

extern "C" int naf_backproject_rays_siddon(const float *values, const float *rays, uint64_t n_rays, uint32_t n1, uint32_t n2,
                                           uint32_t n3, const float *dvoxel, float *volume, void *stream) {
    if (n_rays == 0) return NAF_OK;
    SiddonGrid grid;
    uint32_t blocks;
    int rc = make_siddon_grid("backproject_rays_siddon", volume, n1, n2, n3, dvoxel, &grid);
    if (rc == NAF_OK) rc = make_ray_launch("backproject_rays_siddon", rays, values, n_rays, &blocks);
    if (rc != NAF_OK) return rc;
    { ProfScope prof_("siddon_backproject_rays_kernel", (hipStream_t)stream);
      hipLaunchKernelGGL(siddon_backproject_rays_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, grid, volume,
                         values, rays, n_rays); }
    return check_launch("siddon_backproject_rays_kernel");
}

extern "C" int naf_backproject_scan_siddon(const float *projections, const uint32_t *dims, const float *dvoxel, const float *poses,
                                           uint32_t n_projections, const naf_detector *det, float *volume, void *stream) {
    if (n_projections == 0) return NAF_OK;
    ScanLaunch s;
    SiddonGrid grid;
    const int rc = make_siddon_scan_launch("backproject_scan_siddon", volume, {projections}, dims, dvoxel, poses, n_projections, det, &s,
                                           &grid);
    if (rc != NAF_OK) return rc;
    { ProfScope prof_("siddon_backproject_scan_kernel", (hipStream_t)stream);
      hipLaunchKernelGGL(siddon_backproject_scan_kernel, dim3(s.tiles_per_view * n_projections), dim3(256), 0, (hipStream_t)stream,
                         grid, volume, projections, poses, s.g, s.tiles_x, s.tiles_per_view); }
    return check_launch("siddon_backproject_scan_kernel");
}
