// project.hip -- forward projector for gfx950: line integrals of a voxel volume along rays (naf_project_rays) and along every
// pixel ray of a scan (naf_project_scan).  It makes training scans from CT volumes, the job TIGRE's `Ax` does for the reference's
// dataGenerator/generateData.py.  The projection it computes is defined in include/naf_hip.h and DESIGN.md section 10.
//
// Layout of the scan kernel: scan_launch.h's.  Built with -DNAF_PROJECT_ROW_STRIP it takes 256 consecutive pixels of a detector row
// per workgroup instead (the layout A/B of DESIGN.md section 10).
#include "scan_launch.h"

namespace naf {

namespace {

// Midpoint-rule line integral of one ray (o, d, near, far); d is un-normalised.  Segment, sample count, sample positions and the
// sum over the samples come from project_device.h, shared with the transpose and the OS-SART residual.
__device__ __forceinline__ float line_integral(const ProjVolume &v, float4 a, float4 b) {
    RaySpan s;
    const SpanKind kind = ray_span(v, a, b, s);
    if (kind == kSpanEmpty) return 0.0f;
    if (kind == kSpanUnbounded) return __builtin_nanf("");
    return span_sum(v, s) * s.weight;
}

__global__ void __launch_bounds__(256)
project_rays_kernel(ProjVolume v, const float *__restrict__ rays, float *__restrict__ out, uint64_t n_rays) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_rays) return;
    const float4 *r = reinterpret_cast<const float4 *>(rays + i * 8);
    out[i] = line_integral(v, r[0], r[1]);
}

#ifdef NAF_PROJECT_ROW_STRIP
constexpr ScanLayout kLayout = kScanRowStrip;
#else
constexpr ScanLayout kLayout = kScanTiles;
#endif

// The launch's poses and output come pre-offset to its first view.
__global__ void __launch_bounds__(256)
project_scan_kernel(ProjVolume v, const float *__restrict__ poses, RayGeo g, float *__restrict__ out, uint32_t tiles_x,
                    uint32_t tiles_per_view) {
    ScanPixel p;
    if (!scan_pixel<kLayout>(tiles_x, tiles_per_view, g, p)) return;
    float4 r[2];
    make_pixel_ray(poses + (size_t)p.j * 12, p.row, p.col, g, r);
    out[(uint64_t)p.j * g.W * g.H + p.pixel] = line_integral(v, r[0], r[1]);
}

}  // namespace

}  // namespace naf

using namespace naf;

extern "C" int naf_project_rays(const float *volume, uint32_t n1, uint32_t n2, uint32_t n3, const float *dvoxel, const float *rays,
                                uint64_t n_rays, float step, float *out, void *stream) {
    if (n_rays == 0) return NAF_OK;
    ProjVolume v;
    uint32_t blocks;
    int rc = make_volume("project_rays", volume, n1, n2, n3, dvoxel, step, &v);
    if (rc == NAF_OK) rc = make_ray_launch("project_rays", rays, out, n_rays, &blocks);
    if (rc != NAF_OK) return rc;
    { ProfScope prof_("project_rays_kernel", (hipStream_t)stream);
      hipLaunchKernelGGL(project_rays_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, v, rays, out, n_rays); }
    return check_launch("project_rays_kernel");
}

extern "C" int naf_project_scan(const float *volume, const uint32_t *dims, const float *dvoxel, const float *poses,
                                uint32_t n_projections, const naf_detector *det, float step, float *out, void *stream) {
    if (n_projections == 0) return NAF_OK;
    ScanLaunch s;
    const int rc = make_scan_launch("project_scan", volume, {out}, dims, dvoxel, poses, n_projections, det, step, &s, kLayout);
    if (rc != NAF_OK) return rc;
    { ProfScope prof_("project_scan_kernel", (hipStream_t)stream);
      hipLaunchKernelGGL(project_scan_kernel, dim3(s.tiles_per_view * n_projections), dim3(256), 0, (hipStream_t)stream, s.v, poses,
                         s.g, out, s.tiles_x, s.tiles_per_view); }
    return check_launch("project_scan_kernel");
}
