// siddon_sart.hip -- the two scan kernels of one OS-SART subset step on the ray-voxel intersection ("Siddon") pair for gfx950
// (include/naf_hip.h P8):
//   naf_sart_residual_scan_siddon     r = b - A x and y = r / (A 1) for a list of views of a scan, in one forward walk
//   naf_sart_backproject_scan_siddon  num += A_s^T y and den += A_s^T 1 for the same list, in one transpose walk
// A is P6's map and A^T P7's, restricted to the list: both walks are csrc/siddon_device.h's, the functions siddon.hip and
// siddon_backproject.hip run.  The third launch of the step, naf_sart_update (sart.hip), knows nothing of the projector.
//
// Layout of both kernels: scan_launch.h's.  Launch view j is scan view view_index[j] (j itself without a list), whose pose, pixel
// rays and measured values are read in place from the whole scan, so no subset is ever gathered.  No LDS, no scratch.
#include "siddon_launch.h"

namespace naf {

namespace {

__global__ void __launch_bounds__(256)
siddon_sart_residual_scan_kernel(SiddonGrid grid, const float *__restrict__ volume, const float *__restrict__ poses, RayGeo g,
                                 ViewList list, const float *__restrict__ projections, float *__restrict__ y, float *__restrict__ r,
                                 uint32_t tiles_x, uint32_t tiles_per_view) {
    ScanPixel p;
    if (!scan_pixel(tiles_x, tiles_per_view, g, p)) return;
    const uint64_t per_view = (uint64_t)g.W * g.H;
    const uint32_t view = scan_view(list, p.j);
    const float nan = __builtin_nanf("");
    float res = nan, weighted = nan;                          // a view outside the scan: nothing is read through it
    if (view < list.n_scan_views) {
        const float b = projections[(uint64_t)view * per_view + p.pixel];
        float4 ray[2];
        make_pixel_ray(poses + (size_t)view * 12, p.row, p.col, g, ray);
        SiddonIntegralAndRow sum;
        const SiddonKind kind =
            siddon_forward(grid, siddon_ray(ray[0], ray[1]), [volume](uint64_t offset) { return volume[offset]; }, sum);
        if (kind == kSiddonEmpty) {
            res = b;
            weighted = 0.0f;
        } else if (kind == kSiddonOk) {
            res = b - sum.acc;                                // b - (A x): P6's own sum
            weighted = sum.row > 0.0f ? res / sum.row : 0.0f; // R = 1 / (A 1), the row sum of the same walk
        }
    }
    const uint64_t out = (uint64_t)p.j * per_view + p.pixel;
    y[out] = weighted;
    if (r) r[out] = res;
}

__global__ void __launch_bounds__(256)
siddon_sart_backproject_scan_kernel(SiddonGrid grid, float *__restrict__ num, float *__restrict__ den, const float *__restrict__ y,
                                    const float *__restrict__ poses, RayGeo g, ViewList list, uint32_t tiles_x,
                                    uint32_t tiles_per_view) {
    ScanPixel p;
    if (!scan_pixel(tiles_x, tiles_per_view, g, p)) return;
    const uint32_t view = scan_view(list, p.j);
    if (view >= list.n_scan_views) return;
    float4 ray[2];
    make_pixel_ray(poses + (size_t)view * 12, p.row, p.col, g, ray);
    siddon_transpose(grid, siddon_ray(ray[0], ray[1]), SiddonDepositPair{num, den, y[(uint64_t)p.j * g.W * g.H + p.pixel]});
}

}  // namespace

}  // namespace naf

using namespace naf;

extern "C" int naf_sart_residual_scan_siddon(const float *volume, const uint32_t *dims, const float *dvoxel, const float *poses,
                                             uint32_t n_sub, const naf_detector *det, const uint32_t *view_index,
                                             uint32_t n_scan_views, const float *projections, float *y, float *r, void *stream) {
    if (n_sub == 0) return NAF_OK;
    ScanLaunch s;
    SiddonGrid grid;
    const int rc = make_siddon_scan_launch("sart_residual_scan_siddon", volume, {projections, y}, dims, dvoxel, poses, n_sub, det, &s, &grid,
                                           view_index, n_scan_views);
    if (rc != NAF_OK) return rc;
    { ProfScope prof_("siddon_sart_residual_scan_kernel", (hipStream_t)stream);
      hipLaunchKernelGGL(siddon_sart_residual_scan_kernel, dim3(s.tiles_per_view * n_sub), dim3(256), 0, (hipStream_t)stream, grid,
                         volume, poses, s.g, ViewList{view_index, n_scan_views}, projections, y, r, s.tiles_x, s.tiles_per_view); }
    return check_launch("siddon_sart_residual_scan_kernel");
}

extern "C" int naf_sart_backproject_scan_siddon(const float *y, const uint32_t *view_index, uint32_t n_sub, uint32_t n_scan_views,
                                                const uint32_t *dims, const float *dvoxel, const float *poses, const naf_detector *det,
                                                float *num, float *den, void *stream) {
    if (n_sub == 0) return NAF_OK;
    ScanLaunch s;
    SiddonGrid grid;
    const int rc = make_siddon_scan_launch("sart_backproject_scan_siddon", num, {y}, dims, dvoxel, poses, n_sub, det, &s, &grid, view_index,
                                           n_scan_views);
    if (rc != NAF_OK) return rc;
    if (den == num) return fail(NAF_ERR_INVALID_ARGUMENT, "sart_backproject_scan_siddon: num and den must be two volumes");
    { ProfScope prof_("siddon_sart_backproject_scan_kernel", (hipStream_t)stream);
      hipLaunchKernelGGL(siddon_sart_backproject_scan_kernel, dim3(s.tiles_per_view * n_sub), dim3(256), 0, (hipStream_t)stream, grid,
                         num, den, y, poses, s.g, ViewList{view_index, n_scan_views}, s.tiles_x, s.tiles_per_view); }
    return check_launch("siddon_sart_backproject_scan_kernel");
}
