// backproject.hip -- the transpose of the forward projector for gfx950: naf_backproject_rays scatters one value per ray into a voxel
// volume, naf_backproject_scan does it for every pixel ray of a scan.  With A = naf_project_scan this is A^T to rounding and
// summation order: the segment, the samples and the trilinear cell of every sample come from project_device.h, the code the forward
// kernel runs.  Defined in include/naf_hip.h (P2) and DESIGN.md section 13.
//
// Layout of the scan kernel: scan_launch.h's, the forward's, so the 64 lanes of a wave at equal k add into a small neighbourhood of
// the volume.  The sample spacing is half a voxel, so consecutive samples of a ray often
// share their cell: the eight corner weights are summed in registers while the cell stays the same and go out as eight fp32 hardware
// atomics when it changes (backproject_device.h, shared with sart.hip).  Built with -DNAF_BACKPROJECT_PER_SAMPLE every sample sends
// its own eight atomics (the A/B of section 13).
#include "backproject_device.h"
#include "scan_launch.h"

namespace naf {

namespace {

__global__ void __launch_bounds__(256)
backproject_rays_kernel(ProjVolume v, float *__restrict__ volume, const float *__restrict__ values, const float *__restrict__ rays,
                        uint64_t n_rays) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_rays) return;
    const float4 *r = reinterpret_cast<const float4 *>(rays + i * 8);
    scatter_ray(v, r[0], r[1], DepositValue{volume, values[i]});
}

__global__ void __launch_bounds__(256)
backproject_scan_kernel(ProjVolume v, float *__restrict__ volume, const float *__restrict__ projections, const float *__restrict__ poses,
                        RayGeo g, uint32_t tiles_x, uint32_t tiles_per_view) {
    ScanPixel p;
    if (!scan_pixel(tiles_x, tiles_per_view, g, p)) return;
    float4 r[2];
    make_pixel_ray(poses + (size_t)p.j * 12, p.row, p.col, g, r);
    scatter_ray(v, r[0], r[1], DepositValue{volume, projections[(uint64_t)p.j * g.W * g.H + p.pixel]});
}

}  // namespace

}  // namespace naf

using namespace naf;

extern "C" int naf_backproject_rays(const float *values, const float *rays, uint64_t n_rays, uint32_t n1, uint32_t n2, uint32_t n3,
                                    const float *dvoxel, float step, float *volume, void *stream) {
    if (n_rays == 0) return NAF_OK;
    ProjVolume v;
    uint32_t blocks;
    int rc = make_volume("backproject_rays", volume, n1, n2, n3, dvoxel, step, &v);
    if (rc == NAF_OK) rc = make_ray_launch("backproject_rays", rays, values, n_rays, &blocks);
    if (rc != NAF_OK) return rc;
    { ProfScope prof_("backproject_rays_kernel", (hipStream_t)stream);
      hipLaunchKernelGGL(backproject_rays_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, v, volume, values, rays,
                         n_rays); }
    return check_launch("backproject_rays_kernel");
}

extern "C" int naf_backproject_scan(const float *projections, const uint32_t *dims, const float *dvoxel, const float *poses,
                                    uint32_t n_projections, const naf_detector *det, float step, float *volume, void *stream) {
    if (n_projections == 0) return NAF_OK;
    ScanLaunch s;
    const int rc = make_scan_launch("backproject_scan", volume, {projections}, dims, dvoxel, poses, n_projections, det, step, &s);
    if (rc != NAF_OK) return rc;
    { ProfScope prof_("backproject_scan_kernel", (hipStream_t)stream);
      hipLaunchKernelGGL(backproject_scan_kernel, dim3(s.tiles_per_view * n_projections), dim3(256), 0, (hipStream_t)stream, s.v, volume,
                         projections, poses, s.g, s.tiles_x, s.tiles_per_view); }
    return check_launch("backproject_scan_kernel");
}
