// projector.hip -- the forward projectors and their transposes for gfx950, one template per kernel and per entry point over the
// projector pairs of projector_pair.h:
//   rays forward    line integrals of a voxel volume along a list of rays           naf_project_rays (P1), naf_project_rays_siddon (P6)
//   scan forward    the same along every pixel ray of a scan                         naf_project_scan, naf_project_scan_siddon
//   rays transpose  one value per ray scattered into a voxel volume                  naf_backproject_rays (P2), naf_backproject_rays_siddon (P7)
//   scan transpose  the same for every pixel ray of a scan                           naf_backproject_scan, naf_backproject_scan_siddon
// The forward makes training scans from CT volumes, the job TIGRE's `Ax` does for the reference's dataGenerator/generateData.py;
// each transpose is its forward's A^T to rounding and summation order, because both halves of a pair run the same per-ray code.
// Defined in include/naf_hip.h and DESIGN.md sections 10, 13, 20 and 21; section 28 maps the kernel names used there, by the
// profiler and by check_launch to the instantiations here.
//
// Layout of the scan kernels: scan_launch.h's, rays made in registers, so the 64 lanes of a wave (8 x 8 pixels) at equal step touch
// a small neighbourhood of the volume.  Built with -DNAF_PROJECT_ROW_STRIP the interpolated forward takes 256 consecutive pixels of
// a detector row per workgroup instead (the layout A/B of section 10).  The interpolated transpose sums the corner weights of
// consecutive samples that share a cell and sends eight fp32 hardware atomics when the cell changes; built with
// -DNAF_BACKPROJECT_PER_SAMPLE every sample sends its own (the A/B of section 13).  The Siddon transpose sends one no-return
// atomic per voxel of positive chord length, a group of kSiddonGroup steps at a time, and nothing waits for them.
#include "projector_pair.h"

namespace naf {

namespace {

template <class P>
__global__ void __launch_bounds__(256)
rays_forward_kernel(typename P::Field field, const float *__restrict__ rays, float *__restrict__ out, uint64_t n_rays) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_rays) return;
    const float4 *r = reinterpret_cast<const float4 *>(rays + i * 8);
    out[i] = P::integral(field, r[0], r[1]);
}

// The launch's poses and output come pre-offset to its first view.
template <class P>
__global__ void __launch_bounds__(256)
scan_forward_kernel(typename P::Field field, const float *__restrict__ poses, RayGeo g, float *__restrict__ out, uint32_t tiles_x,
                    uint32_t tiles_per_view) {
    ScanPixel p;
    if (!scan_pixel<P::kForwardLayout>(tiles_x, tiles_per_view, g, p)) return;
    float4 r[2];
    make_pixel_ray(poses + (size_t)p.j * 12, p.row, p.col, g, r);
    out[(uint64_t)p.j * g.W * g.H + p.pixel] = P::integral(field, r[0], r[1]);
}

template <class P>
__global__ void __launch_bounds__(256)
rays_transpose_kernel(typename P::Grid grid, float *__restrict__ volume, const float *__restrict__ values,
                      const float *__restrict__ rays, uint64_t n_rays) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_rays) return;
    const float4 *r = reinterpret_cast<const float4 *>(rays + i * 8);
    P::transpose(grid, P::ray(r[0], r[1]), typename P::ValueDeposit{volume, values[i]});
}

// The launch's poses and projections come pre-offset to its first view.
template <class P>
__global__ void __launch_bounds__(256)
scan_transpose_kernel(typename P::Grid grid, float *__restrict__ volume, const float *__restrict__ projections,
                      const float *__restrict__ poses, RayGeo g, uint32_t tiles_x, uint32_t tiles_per_view) {
    ScanPixel p;
    if (!scan_pixel(tiles_x, tiles_per_view, g, p)) return;
    float4 r[2];
    make_pixel_ray(poses + (size_t)p.j * 12, p.row, p.col, g, r);
    P::transpose(grid, P::ray(r[0], r[1]), typename P::ValueDeposit{volume, projections[(uint64_t)p.j * g.W * g.H + p.pixel]});
}

// The entry points: `who` names the call in a refusal, `kernel` the launch to the profiler and in a launch error.

template <class P>
int project_rays(const char *who, const char *kernel, const float *volume, uint32_t n1, uint32_t n2, uint32_t n3, const float *dvoxel,
                 const float *rays, uint64_t n_rays, float step, float *out, void *stream) {
    if (n_rays == 0) return NAF_OK;
    ProjVolume v;
    uint32_t blocks;
    int rc = make_volume(who, volume, n1, n2, n3, dvoxel, step, &v);
    if (rc == NAF_OK) rc = make_ray_launch(who, rays, out, n_rays, &blocks);
    if (rc != NAF_OK) return rc;
    return launch(kernel, rays_forward_kernel<P>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, P::field(v), rays, out, n_rays);
}

template <class P>
int project_scan(const char *who, const char *kernel, const float *volume, const uint32_t *dims, const float *dvoxel,
                 const float *poses, uint32_t n_projections, const naf_detector *det, float step, float *out, void *stream) {
    if (n_projections == 0) return NAF_OK;
    ScanLaunch s;
    const int rc = make_scan_launch(who, volume, {out}, dims, dvoxel, poses, n_projections, det, step, &s, P::kForwardLayout);
    if (rc != NAF_OK) return rc;
    return launch(kernel, scan_forward_kernel<P>, dim3(s.tiles_per_view * n_projections), dim3(256), 0, (hipStream_t)stream,
                  P::field(s.v), poses, s.g, out, s.tiles_x, s.tiles_per_view);
}

template <class P>
int backproject_rays(const char *who, const char *kernel, const float *values, const float *rays, uint64_t n_rays, uint32_t n1,
                     uint32_t n2, uint32_t n3, const float *dvoxel, float step, float *volume, void *stream) {
    if (n_rays == 0) return NAF_OK;
    ProjVolume v;
    uint32_t blocks;
    int rc = make_volume(who, volume, n1, n2, n3, dvoxel, step, &v);
    if (rc == NAF_OK) rc = make_ray_launch(who, rays, values, n_rays, &blocks);
    if (rc != NAF_OK) return rc;
    return launch(kernel, rays_transpose_kernel<P>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, P::grid(P::field(v)), volume,
                  values, rays, n_rays);
}

template <class P>
int backproject_scan(const char *who, const char *kernel, const float *projections, const uint32_t *dims, const float *dvoxel,
                     const float *poses, uint32_t n_projections, const naf_detector *det, float step, float *volume, void *stream) {
    if (n_projections == 0) return NAF_OK;
    ScanLaunch s;
    const int rc = make_scan_launch(who, volume, {projections}, dims, dvoxel, poses, n_projections, det, step, &s);
    if (rc != NAF_OK) return rc;
    return launch(kernel, scan_transpose_kernel<P>, dim3(s.tiles_per_view * n_projections), dim3(256), 0, (hipStream_t)stream,
                  P::grid(P::field(s.v)), volume, projections, poses, s.g, s.tiles_x, s.tiles_per_view);
}

}  // namespace

}  // namespace naf

using namespace naf;

extern "C" int naf_project_rays(const float *volume, uint32_t n1, uint32_t n2, uint32_t n3, const float *dvoxel, const float *rays,
                                uint64_t n_rays, float step, float *out, void *stream) {
    return project_rays<InterpolatedPair>("project_rays", "project_rays_kernel", volume, n1, n2, n3, dvoxel, rays, n_rays, step, out,
                                          stream);
}

extern "C" int naf_project_rays_siddon(const float *volume, uint32_t n1, uint32_t n2, uint32_t n3, const float *dvoxel,
                                       const float *rays, uint64_t n_rays, float *out, void *stream) {
    return project_rays<SiddonPair>("project_rays_siddon", "siddon_rays_kernel", volume, n1, n2, n3, dvoxel, rays, n_rays, 1.0f, out,
                                    stream);
}

extern "C" int naf_project_scan(const float *volume, const uint32_t *dims, const float *dvoxel, const float *poses,
                                uint32_t n_projections, const naf_detector *det, float step, float *out, void *stream) {
    return project_scan<InterpolatedPair>("project_scan", "project_scan_kernel", volume, dims, dvoxel, poses, n_projections, det, step,
                                          out, stream);
}

extern "C" int naf_project_scan_siddon(const float *volume, const uint32_t *dims, const float *dvoxel, const float *poses,
                                       uint32_t n_projections, const naf_detector *det, float *out, void *stream) {
    return project_scan<SiddonPair>("project_scan_siddon", "siddon_scan_kernel", volume, dims, dvoxel, poses, n_projections, det, 1.0f,
                                    out, stream);
}

extern "C" int naf_backproject_rays(const float *values, const float *rays, uint64_t n_rays, uint32_t n1, uint32_t n2, uint32_t n3,
                                    const float *dvoxel, float step, float *volume, void *stream) {
    return backproject_rays<InterpolatedPair>("backproject_rays", "backproject_rays_kernel", values, rays, n_rays, n1, n2, n3, dvoxel,
                                              step, volume, stream);
}

extern "C" int naf_backproject_rays_siddon(const float *values, const float *rays, uint64_t n_rays, uint32_t n1, uint32_t n2,
                                           uint32_t n3, const float *dvoxel, float *volume, void *stream) {
    return backproject_rays<SiddonPair>("backproject_rays_siddon", "siddon_backproject_rays_kernel", values, rays, n_rays, n1, n2, n3,
                                        dvoxel, 1.0f, volume, stream);
}

extern "C" int naf_backproject_scan(const float *projections, const uint32_t *dims, const float *dvoxel, const float *poses,
                                    uint32_t n_projections, const naf_detector *det, float step, float *volume, void *stream) {
    return backproject_scan<InterpolatedPair>("backproject_scan", "backproject_scan_kernel", projections, dims, dvoxel, poses,
                                              n_projections, det, step, volume, stream);
}

extern "C" int naf_backproject_scan_siddon(const float *projections, const uint32_t *dims, const float *dvoxel, const float *poses,
                                           uint32_t n_projections, const naf_detector *det, float *volume, void *stream) {
    return backproject_scan<SiddonPair>("backproject_scan_siddon", "siddon_backproject_scan_kernel", projections, dims, dvoxel, poses,
                                        n_projections, det, 1.0f, volume, stream);
}
