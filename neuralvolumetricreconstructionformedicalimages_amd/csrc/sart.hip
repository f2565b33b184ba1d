// sart.hip -- the three kernels of one OS-SART subset step for gfx950 (include/naf_hip.h P4 and P8, DESIGN.md sections 16 and 22),
// the two that know the projector as one template each over the projector pairs of projector_pair.h:
//   subset residual   r = b - A x and y = r / len (interpolated) or r / (A 1) (Siddon) for a list of views of a scan, in one
//                     forward march                              naf_sart_residual_scan, naf_sart_residual_scan_siddon
//   subset transpose  num += A_s^T y and den += A_s^T 1 for the same list, in one transpose march
//                                                                naf_sart_backproject_scan, naf_sart_backproject_scan_siddon
//   naf_sart_update   x += relax * num / den (clamped at 0), num = 0, den = 0, in one pass over the volume; it knows nothing of
//                     the projector
// Both halves are the pair's own per-ray code, the functions projector.hip runs, so a subset step is A and A^T of P1 / P2 or of
// P6 / P7 restricted to the list.  Section 28 maps the kernel names used in DESIGN.md, by the profiler and by check_launch to the
// instantiations here.
//
// Layout of the two scan kernels: scan_launch.h's.  Launch view j is scan view view_index[j] (j itself without a list), whose pose,
// pixel rays and measured values are read in place from the whole scan, so no subset is ever gathered.  No LDS, no scratch.
#include "projector_pair.h"

namespace naf {

namespace {

template <class P>
__global__ void __launch_bounds__(256)
subset_residual_kernel(typename P::Field field, const float *__restrict__ poses, RayGeo g, ViewList list,
                       const float *__restrict__ projections, float *__restrict__ y, float *__restrict__ r, uint32_t tiles_x,
                       uint32_t tiles_per_view) {
    ScanPixel p;
    if (!scan_pixel(tiles_x, tiles_per_view, g, p)) return;
    const uint64_t per_view = (uint64_t)g.W * g.H;
    const uint32_t view = scan_view(list, p.j);
    const float nan = __builtin_nanf("");
    Residual res{nan, nan};                                   // a view outside the scan: nothing is read through it
    if (view < list.n_scan_views) {
        const float b = projections[(uint64_t)view * per_view + p.pixel];
        float4 ray[2];
        make_pixel_ray(poses + (size_t)view * 12, p.row, p.col, g, ray);
        res = P::residual(field, P::ray(ray[0], ray[1]), b);
    }
    const uint64_t out = (uint64_t)p.j * per_view + p.pixel;
    y[out] = res.y;
    if (r) r[out] = res.res;
}

// The Siddon pair's residual kernel stays written out: with its rule behind a function of the pair, as the interpolated one's is,
// the walk is optimised once more before it reaches the kernel and comes out with 75 VGPRs for 72.
template <>
__global__ void __launch_bounds__(256)
subset_residual_kernel<SiddonPair>(SiddonPair::Field field, const float *__restrict__ poses, RayGeo g, ViewList list,
                                   const float *__restrict__ projections, float *__restrict__ y, float *__restrict__ r,
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
        const float *volume = field.volume;
        SiddonIntegralAndRow sum;
        const SiddonKind kind =
            siddon_forward(field.grid.grid(), SiddonPair::ray(ray[0], ray[1]), [volume](uint64_t offset) { return volume[offset]; }, sum);
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

template <class P>
__global__ void __launch_bounds__(256)
subset_transpose_kernel(typename P::Grid grid, float *__restrict__ num, float *__restrict__ den, const float *__restrict__ y,
                        const float *__restrict__ poses, RayGeo g, ViewList list, uint32_t tiles_x, uint32_t tiles_per_view) {
    ScanPixel p;
    if (!scan_pixel(tiles_x, tiles_per_view, g, p)) return;
    const uint32_t view = scan_view(list, p.j);
    if (view >= list.n_scan_views) return;
    float4 ray[2];
    make_pixel_ray(poses + (size_t)view * 12, p.row, p.col, g, ray);
    P::transpose(grid, P::ray(ray[0], ray[1]), typename P::PairDeposit{num, den, y[(uint64_t)p.j * g.W * g.H + p.pixel]});
}

struct UpdateArgs {
    float relax;
    int nonneg, den_is_reciprocal, zero_den;
};

__device__ __forceinline__ void update_voxel(float &x, float &num, float &den, const UpdateArgs &a) {
    float c = den;
    if (!a.den_is_reciprocal) {
        c = den > 0.0f ? 1.0f / den : 0.0f;
        if (a.zero_den) den = 0.0f;
    }
    float next = x + a.relax * (c * num);
    if (a.nonneg) next = next < 0.0f ? 0.0f : next;           // a NaN stays a NaN
    x = next;
    num = 0.0f;
}

// Elements [head, head + 4 n_vec) as float4 (x + head, num + head and den + head are 16-byte aligned), the `head` elements before
// and the fewer than four after them one by one.  Grid-stride.
__global__ void __launch_bounds__(256)
sart_update_kernel(float *__restrict__ x, float *__restrict__ num, float *__restrict__ den, uint64_t n, uint64_t head, uint64_t n_vec,
                   UpdateArgs a) {
    const uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (uint64_t)gridDim.x * blockDim.x;
    float4 *__restrict__ xv = reinterpret_cast<float4 *>(x + head);
    float4 *__restrict__ nv = reinterpret_cast<float4 *>(num + head);
    float4 *__restrict__ dv = reinterpret_cast<float4 *>(den + head);
    const bool store_den = !a.den_is_reciprocal && a.zero_den;
    for (uint64_t i = tid; i < n_vec; i += stride) {
        float4 xs = xv[i], ns = nv[i], ds = dv[i];
        update_voxel(xs.x, ns.x, ds.x, a);
        update_voxel(xs.y, ns.y, ds.y, a);
        update_voxel(xs.z, ns.z, ds.z, a);
        update_voxel(xs.w, ns.w, ds.w, a);
        xv[i] = xs;
        nv[i] = ns;
        if (store_den) dv[i] = ds;
    }
    const uint64_t tail = head + 4u * n_vec, n_single = head + (n - tail);
    for (uint64_t i = tid; i < n_single; i += stride) {
        const uint64_t e = i < head ? i : tail + (i - head);
        float xs = x[e], ns = num[e], ds = den[e];
        update_voxel(xs, ns, ds, a);
        x[e] = xs;
        num[e] = ns;
        if (store_den) den[e] = ds;
    }
}

// The entry points: `who` names the call in a refusal, `kernel` the launch to the profiler and in a launch error.

template <class P>
int sart_residual_scan(const char *who, const char *kernel, const float *volume, const uint32_t *dims, const float *dvoxel,
                       const float *poses, uint32_t n_sub, const naf_detector *det, float step, const uint32_t *view_index,
                       uint32_t n_scan_views, const float *projections, float *y, float *r, void *stream) {
    if (n_sub == 0) return NAF_OK;
    ScanLaunch s;
    const int rc = make_scan_launch(who, volume, {projections, y}, dims, dvoxel, poses, n_sub, det, step, &s, kScanTiles, view_index,
                                    n_scan_views);
    if (rc != NAF_OK) return rc;
    return launch(kernel, subset_residual_kernel<P>, dim3(s.tiles_per_view * n_sub), dim3(256), 0, (hipStream_t)stream,
                  P::field(s.v), poses, s.g, ViewList{view_index, n_scan_views}, projections, y, r, s.tiles_x, s.tiles_per_view);
}

template <class P>
int sart_backproject_scan(const char *who, const char *kernel, const float *y, const uint32_t *view_index, uint32_t n_sub,
                          uint32_t n_scan_views, const uint32_t *dims, const float *dvoxel, const float *poses,
                          const naf_detector *det, float step, float *num, float *den, void *stream) {
    if (n_sub == 0) return NAF_OK;
    ScanLaunch s;
    const int rc = make_scan_launch(who, num, {y}, dims, dvoxel, poses, n_sub, det, step, &s, kScanTiles, view_index, n_scan_views);
    if (rc != NAF_OK) return rc;
    if (den == num) return fail_who(who, "num and den must be two volumes");
    return launch(kernel, subset_transpose_kernel<P>, dim3(s.tiles_per_view * n_sub), dim3(256), 0, (hipStream_t)stream,
                  P::grid(P::field(s.v)), num, den, y, poses, s.g, ViewList{view_index, n_scan_views}, s.tiles_x,
                  s.tiles_per_view);
}

}  // namespace

}  // namespace naf

using namespace naf;

extern "C" int naf_sart_residual_scan(const float *volume, const uint32_t *dims, const float *dvoxel, const float *poses, uint32_t n_sub,
                                      const naf_detector *det, float step, const uint32_t *view_index, uint32_t n_scan_views,
                                      const float *projections, float *y, float *r, void *stream) {
    return sart_residual_scan<InterpolatedPair>("sart_residual_scan", "sart_residual_scan_kernel", volume, dims, dvoxel, poses, n_sub,
                                                det, step, view_index, n_scan_views, projections, y, r, stream);
}

extern "C" int naf_sart_residual_scan_siddon(const float *volume, const uint32_t *dims, const float *dvoxel, const float *poses,
                                             uint32_t n_sub, const naf_detector *det, const uint32_t *view_index,
                                             uint32_t n_scan_views, const float *projections, float *y, float *r, void *stream) {
    return sart_residual_scan<SiddonPair>("sart_residual_scan_siddon", "siddon_sart_residual_scan_kernel", volume, dims, dvoxel, poses,
                                          n_sub, det, 1.0f, view_index, n_scan_views, projections, y, r, stream);
}

extern "C" int naf_sart_backproject_scan(const float *y, const uint32_t *view_index, uint32_t n_sub, uint32_t n_scan_views,
                                         const uint32_t *dims, const float *dvoxel, const float *poses, const naf_detector *det,
                                         float step, float *num, float *den, void *stream) {
    return sart_backproject_scan<InterpolatedPair>("sart_backproject_scan", "sart_backproject_scan_kernel", y, view_index, n_sub,
                                                   n_scan_views, dims, dvoxel, poses, det, step, num, den, stream);
}

extern "C" int naf_sart_backproject_scan_siddon(const float *y, const uint32_t *view_index, uint32_t n_sub, uint32_t n_scan_views,
                                                const uint32_t *dims, const float *dvoxel, const float *poses, const naf_detector *det,
                                                float *num, float *den, void *stream) {
    return sart_backproject_scan<SiddonPair>("sart_backproject_scan_siddon", "siddon_sart_backproject_scan_kernel", y, view_index,
                                             n_sub, n_scan_views, dims, dvoxel, poses, det, 1.0f, num, den, stream);
}

extern "C" int naf_sart_update(float *x, float *num, float *den, uint64_t n, float relax, int nonneg, int den_is_reciprocal,
                               int zero_den, void *stream) {
    if (n == 0) return NAF_OK;
    if (!x || !num || !den) return fail(NAF_ERR_INVALID_ARGUMENT, "sart_update: null pointer");
    if (!std::isfinite(relax)) return fail(NAF_ERR_INVALID_ARGUMENT, "sart_update: relax must be finite");
    if (den_is_reciprocal && zero_den)
        return fail(NAF_ERR_INVALID_ARGUMENT, "sart_update: a reciprocal den is read only, zero_den cannot be set with it");
    const uintptr_t ax = (uintptr_t)x, an = (uintptr_t)num, ad = (uintptr_t)den;
    if ((ax | an | ad) & 3u) return fail(NAF_ERR_INVALID_ARGUMENT, "sart_update: pointers must be 4-byte aligned");
    // The float4 body needs the three arrays to reach a 16-byte boundary after the same number of elements; otherwise every
    // element goes one by one (head = n).
    uint64_t head = n;
    if ((ax & 15u) == (an & 15u) && (ax & 15u) == (ad & 15u)) head = std::min<uint64_t>(n, ((16u - (ax & 15u)) & 15u) / 4u);
    const uint64_t n_vec = (n - head) / 4u;
    const uint64_t work = std::max<uint64_t>(n_vec, n - 4u * n_vec);
    const uint32_t blocks = (uint32_t)std::min<uint64_t>((work + 255u) / 256u, 2048u);
    UpdateArgs a{relax, nonneg != 0, den_is_reciprocal != 0, zero_den != 0};
    return launch("sart_update_kernel", sart_update_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, x, num, den, n, head, n_vec,
                  a);
}
