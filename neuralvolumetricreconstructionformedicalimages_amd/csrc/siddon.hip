// siddon.hip -- ray-voxel intersection ("Siddon") forward projector for gfx950: line integrals of a piecewise-constant voxel volume
// along rays (naf_project_rays_siddon) and along every pixel ray of a scan (naf_project_scan_siddon).  It is the second forward
// model beside project.hip's interpolated one: exact chord lengths per voxel, no sampling step.  The projection is defined in
// include/naf_hip.h (P6) and DESIGN.md section 20; the traversal is csrc/siddon_device.h.
//
// Layout of the scan kernel: scan_launch.h's, rays made in registers: neighbouring lanes walk neighbouring voxels.
#include "scan_launch.h"
#include "siddon_device.h"

namespace naf {

namespace {

struct SiddonVolume {
    const float *__restrict__ data;  // [n1, n2, n3] fp32, axis 0 = x, C-contiguous
    SiddonGrid grid;
};

__device__ __forceinline__ float siddon_ray(const SiddonVolume &v, float4 a, float4 b) {
    const float o[3] = {a.x, a.y, a.z}, d[3] = {a.w, b.x, b.y};
    const float *__restrict__ data = v.data;
    return siddon_line_integral(v.grid, o, d, b.z, b.w, [data](uint64_t offset) { return data[offset]; });
}

__global__ void __launch_bounds__(256)
siddon_rays_kernel(SiddonVolume v, const float *__restrict__ rays, float *__restrict__ out, uint64_t n_rays) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_rays) return;
    const float4 *r = reinterpret_cast<const float4 *>(rays + i * 8);
    out[i] = siddon_ray(v, r[0], r[1]);
}

// The launch's poses and output come pre-offset to its first view.
__global__ void __launch_bounds__(256)
siddon_scan_kernel(SiddonVolume v, const float *__restrict__ poses, RayGeo g, float *__restrict__ out, uint32_t tiles_x,
                   uint32_t tiles_per_view) {
    ScanPixel p;
    if (!scan_pixel(tiles_x, tiles_per_view, g, p)) return;
    float4 r[2];
    make_pixel_ray(poses + (size_t)p.j * 12, p.row, p.col, g, r);
    out[(uint64_t)p.j * g.W * g.H + p.pixel] = siddon_ray(v, r[0], r[1]);
}

// The argument checks of P1's make_volume (there is no sample step here).
int make_siddon_volume(const char *who, const float *volume, uint32_t n1, uint32_t n2, uint32_t n3, const float *dvoxel,
                       SiddonVolume *v) {
    ProjVolume checked;
    const int rc = make_volume(who, volume, n1, n2, n3, dvoxel, 1.0f, &checked);
    if (rc != NAF_OK) return rc;
    v->data = volume;
    siddon_grid(n1, n2, n3, dvoxel, &v->grid);
    return NAF_OK;
}

}  // namespace

}  // namespace naf

using namespace naf;

extern "C" int naf_project_rays_siddon(const float *volume, uint32_t n1, uint32_t n2, uint32_t n3, const float *dvoxel,
                                       const float *rays, uint64_t n_rays, float *out, void *stream) {
    if (n_rays == 0) return NAF_OK;
    SiddonVolume v;
    const int rc = make_siddon_volume("project_rays_siddon", volume, n1, n2, n3, dvoxel, &v);
    if (rc != NAF_OK) return rc;
    if (!rays || !out) return fail(NAF_ERR_INVALID_ARGUMENT, "project_rays_siddon: null pointer");
    if (((uintptr_t)rays) & 15u) return fail(NAF_ERR_INVALID_ARGUMENT, "project_rays_siddon: rays must be 16-byte aligned");
    const uint64_t blocks = (n_rays + 255u) / 256u;
    if (blocks > 0x7fffffffull) return fail(NAF_ERR_INVALID_ARGUMENT, "project_rays_siddon: too many rays for one call");
    { ProfScope prof_("siddon_rays_kernel", (hipStream_t)stream);
      hipLaunchKernelGGL(siddon_rays_kernel, dim3((uint32_t)blocks), dim3(256), 0, (hipStream_t)stream, v, rays, out, n_rays); }
    return check_launch("siddon_rays_kernel");
}

extern "C" int naf_project_scan_siddon(const float *volume, const uint32_t *dims, const float *dvoxel, const float *poses,
                                       uint32_t n_projections, uint32_t det_w, uint32_t det_h, float du, float dv, float ou, float ov,
                                       float DSD, float near, float far, int parallel, float *out, void *stream) {
    if (n_projections == 0) return NAF_OK;
    ScanLaunch s;                                               // there is no sample step here: any valid one passes the checks
    const int rc = make_scan_launch("project_scan_siddon", volume, {out}, dims, dvoxel, poses, n_projections, det_w, det_h, du, dv, ou,
                                    ov, DSD, near, far, parallel, 1.0f, &s);
    if (rc != NAF_OK) return rc;
    SiddonVolume v{volume};
    siddon_grid(dims[0], dims[1], dims[2], dvoxel, &v.grid);
    { ProfScope prof_("siddon_scan_kernel", (hipStream_t)stream);
      hipLaunchKernelGGL(siddon_scan_kernel, dim3(s.tiles_per_view * n_projections), dim3(256), 0, (hipStream_t)stream, v, poses, s.g,
                         out, s.tiles_x, s.tiles_per_view); }
    return check_launch("siddon_scan_kernel");
}
