// siddon.hip -- ray-voxel intersection ("Siddon") forward projector for gfx950: line integrals of a piecewise-constant voxel volume
// along rays (naf_project_rays_siddon) and along every pixel ray of a scan (naf_project_scan_siddon).  It is the second forward
// model beside project.hip's interpolated one: exact chord lengths per voxel, no sampling step.  The projection is defined in
// include/naf_hip.h (P6) and DESIGN.md section 20; the traversal is csrc/siddon_device.h.
//
// Layout of the scan kernel: scan_launch.h's, rays made in registers: neighbouring lanes walk neighbouring voxels.
#include "siddon_launch.h"

namespace naf {

namespace {

// P6's line integral of one ray: 0 on an empty span, NaN on a non-finite one.
__device__ __forceinline__ float siddon_line_integral(const SiddonGrid &grid, const float *__restrict__ volume, float4 a, float4 b) {
    SiddonIntegral sum;
    const SiddonKind kind = siddon_forward(grid, siddon_ray(a, b), [volume](uint64_t offset) { return volume[offset]; }, sum);
    if (kind == kSiddonEmpty) return 0.0f;
    if (kind == kSiddonNotFinite) return __builtin_nanf("");
    return sum.acc;
}

__global__ void __launch_bounds__(256)
siddon_rays_kernel(SiddonGrid grid, const float *__restrict__ volume, const float *__restrict__ rays, float *__restrict__ out,
                   uint64_t n_rays) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_rays) return;
    const float4 *r = reinterpret_cast<const float4 *>(rays + i * 8);
    out[i] = siddon_line_integral(grid, volume, r[0], r[1]);
}

// The launch's poses and output come pre-offset to its first view.
__global__ void __launch_bounds__(256)
siddon_scan_kernel(SiddonGrid grid, const float *__restrict__ volume, const float *__restrict__ poses, RayGeo g,
                   float *__restrict__ out, uint32_t tiles_x, uint32_t tiles_per_view) {
    ScanPixel p;
    if (!scan_pixel(tiles_x, tiles_per_view, g, p)) return;
    float4 r[2];
    make_pixel_ray(poses + (size_t)p.j * 12, p.row, p.col, g, r);
    out[(uint64_t)p.j * g.W * g.H + p.pixel] = siddon_line_integral(grid, volume, r[0], r[1]);
}

}  // namespace

}  // namespace naf

using namespace naf;

extern "C" int naf_project_rays_siddon(const float *volume, uint32_t n1, uint32_t n2, uint32_t n3, const float *dvoxel,
                                       const float *rays, uint64_t n_rays, float *out, void *stream) {
    if (n_rays == 0) return NAF_OK;
    SiddonGrid grid;
    uint32_t blocks;
    int rc = make_siddon_grid("project_rays_siddon", volume, n1, n2, n3, dvoxel, &grid);
    if (rc == NAF_OK) rc = make_ray_launch("project_rays_siddon", rays, out, n_rays, &blocks);
    if (rc != NAF_OK) return rc;
    { ProfScope prof_("siddon_rays_kernel", (hipStream_t)stream);
      hipLaunchKernelGGL(siddon_rays_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, grid, volume, rays, out, n_rays); }
    return check_launch("siddon_rays_kernel");
}

extern "C" int naf_project_scan_siddon(const float *volume, const uint32_t *dims, const float *dvoxel, const float *poses,
                                       uint32_t n_projections, const naf_detector *det, float *out, void *stream) {
    if (n_projections == 0) return NAF_OK;
    ScanLaunch s;
    SiddonGrid grid;
    const int rc = make_siddon_scan_launch("project_scan_siddon", volume, {out}, dims, dvoxel, poses, n_projections, det, &s, &grid);
    if (rc != NAF_OK) return rc;
    { ProfScope prof_("siddon_scan_kernel", (hipStream_t)stream);
      hipLaunchKernelGGL(siddon_scan_kernel, dim3(s.tiles_per_view * n_projections), dim3(256), 0, (hipStream_t)stream, grid, volume,
                         poses, s.g, out, s.tiles_x, s.tiles_per_view); }
    return check_launch("siddon_scan_kernel");
}
