// backproject_gather.hip -- the transpose of the forward projector in gather form for gfx950 (include/naf_hip.h P5, DESIGN.md
// section 17): naf_backproject_scan_gather adds A^T y into a volume, and the column sums A^T 1 into a second one, with no atomics
// and a fixed summation order, so two calls on the same inputs return the same bits.  It is the operator of projector.hip and
// sart.hip, not a voxel-driven model: every weight is the scatter's own, from project_device.h (ray_span, span_point,
// trilinear_cell); backproject_gather_device.h only decides which (pixel, sample) pairs a voxel has to look at.
//
// Layout: one lane per voxel, a wave owns a 4 x 4 x 4 brick (its lanes' footprints overlap, so they read the same few rays), a
// workgroup four bricks along z.  Per view a lane walks its footprint rectangle in (row, col) order, takes each pixel's span -- from
// the table a pre-pass wrote into the caller's workspace, or recomputed when there is none: the same floats either way -- and sums
// the weights of the samples of its k-range in k order.  One plain load and one plain store per voxel and output; no LDS.  The
// checks of a scan call, its RayGeo and the view list are scan_launch.h's.
#include "scan_launch.h"
#include "backproject_gather_device.h"

namespace naf {

namespace {

struct GatherSpan {                  // what the gather needs of a RaySpan: NAF_GATHER_SPAN_BYTES each
    float p0[3], d[3];
    float seg, weight;
    uint32_t n;                      // 0: the ray adds nothing (empty segment, NaN / infinite ray, view outside the scan)
    uint32_t pad;
};
static_assert(sizeof(GatherSpan) == NAF_GATHER_SPAN_BYTES, "span record size is part of the ABI");

struct GatherViews {
    const uint32_t *__restrict__ index;   // a ViewList's two fields
    uint32_t n_scan_views;
    uint32_t first, count;                // launch views [first, first + count) of the call
};

__device__ __forceinline__ uint32_t gather_scan_view(const GatherViews &l, uint32_t j) {
    return scan_view(ViewList{l.index, l.n_scan_views}, l.first + j);
}

// The span of pixel (row, col) of scan view `view`, as the scatter gets it: make_pixel_ray -> ray_span.  n = 0 when it adds nothing.
__device__ __forceinline__ void pixel_span(const ProjVolume &v, const float *__restrict__ poses, uint32_t view, uint32_t row,
                                           uint32_t col, const RayGeo &g, GatherSpan &out) {
    float4 ray[2];
    make_pixel_ray(poses + (size_t)view * 12, row, col, g, ray);
    RaySpan s;
    out.n = 0u;
    if (ray_span(v, ray[0], ray[1], s) != kSpanOk) return;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        out.p0[a] = s.p0[a];
        out.d[a] = s.d[a];
    }
    out.seg = s.seg;
    out.weight = s.weight;
    out.n = s.n;
}

// Pre-pass: record j * H * W + row * W + col of the table = the span of that pixel of launch view first + j.
__global__ void __launch_bounds__(256)
gather_spans_kernel(ProjVolume v, const float *__restrict__ poses, RayGeo g, GatherViews list, GatherSpan *__restrict__ spans) {
    const uint64_t per_view = (uint64_t)g.W * g.H;
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= per_view * list.count) return;
    const uint32_t j = (uint32_t)(i / per_view), pixel = (uint32_t)(i - (uint64_t)j * per_view);
    const uint32_t view = gather_scan_view(list, j);
    GatherSpan s;
    s.n = 0u;
    if (view < list.n_scan_views) pixel_span(v, poses, view, pixel / g.W, pixel % g.W, g, s);
    if (s.n == 0u) {
#pragma unroll
        for (int a = 0; a < 3; ++a) s.p0[a] = s.d[a] = 0.0f;
        s.seg = s.weight = 0.0f;
    }
    s.pad = 0u;
    spans[i] = s;
}

// blockIdx.x = (bx * bricks_y + by) * blocks_z + bz: voxels [4 bx, 4 bx + 4) x [4 by, 4 by + 4) x [16 bz, 16 bz + 16).
template <bool kTable, bool kDen>
__global__ void __launch_bounds__(256)
backproject_gather_kernel(ProjVolume v, float *__restrict__ num, float *__restrict__ den,
                          const float *__restrict__ values, const float *__restrict__ poses, RayGeo g, GatherViews list,
                          const GatherSpan *__restrict__ spans, uint32_t bricks_y, uint32_t blocks_z) {
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    uint32_t b = blockIdx.x;
    const uint32_t bz = b % blocks_z;
    b /= blocks_z;
    const uint32_t by = b % bricks_y, bx = b / bricks_y;
    const uint32_t i[3] = {bx * 4u + (lane >> 4), by * 4u + ((lane >> 2) & 3u), (bz * 4u + wave) * 4u + (lane & 3u)};
    if (i[0] >= v.grid.n[0] || i[1] >= v.grid.n[1] || i[2] >= v.grid.n[2]) return;
    const uint64_t voxel = (uint64_t)i[0] * v.grid.stride[0] + (uint64_t)i[1] * v.grid.stride[1] + i[2];
    float lo[3], hi[3];
    gather_support(v.grid, i, lo, hi);
    const GatherDetector det{g.W, g.H, g.du, g.dv, g.ou, g.ov, g.DSD, g.parallel};
    const uint64_t per_view = (uint64_t)g.W * g.H;
    float acc = num[voxel], dacc = kDen ? den[voxel] : 0.0f;
    for (uint32_t j = 0; j < list.count; ++j) {
        const uint32_t view = gather_scan_view(list, j);
        if (view >= list.n_scan_views) continue;
        const GatherRect r = gather_footprint(lo, hi, poses + (size_t)view * 12, det);
        float s_num = 0.0f, s_den = 0.0f;
        for (uint32_t row = r.row0; row < r.row1; ++row) {
            for (uint32_t col = r.col0; col < r.col1; ++col) {
                const uint64_t pixel = (uint64_t)row * g.W + col;
                GatherSpan s;
                if (kTable) {
                    const float2 *__restrict__ q = reinterpret_cast<const float2 *>(spans + ((uint64_t)j * per_view + pixel));
                    const float2 q0 = q[0], q1 = q[1], q2 = q[2], q3 = q[3], q4 = q[4];
                    s.p0[0] = q0.x, s.p0[1] = q0.y, s.p0[2] = q1.x;
                    s.d[0] = q1.y, s.d[1] = q2.x, s.d[2] = q2.y;
                    s.seg = q3.x, s.weight = q3.y;
                    s.n = __float_as_uint(q4.x);
                } else {
                    pixel_span(v, poses, view, row, col, g, s);
                }
                if (s.n == 0u) continue;
                uint32_t k_lo, k_hi;
                if (!gather_k_range(lo, hi, s.p0, s.d, s.seg, s.n, k_lo, k_hi)) continue;
                RaySpan span;
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    span.p0[a] = s.p0[a];
                    span.d[a] = s.d[a];
                }
                span.seg = s.seg;
                float sw = 0.0f;
                for (uint32_t k = k_lo; k <= k_hi; ++k) {
                    float p[3], w[3];
                    span_point(span, k, p);
                    const uint64_t cell = trilinear_cell(v, p, w);
                    sw += gather_corner_weight(voxel, cell, v.grid.next, w);
                }
                if (sw == 0.0f) continue;
                s_num += (values[(uint64_t)(list.first + j) * per_view + pixel] * s.weight) * sw;
                if (kDen) s_den += s.weight * sw;
            }
        }
        acc += s_num;
        if (kDen) dacc += s_den;
    }
    num[voxel] = acc;
    if (kDen) den[voxel] = dacc;
}

}  // namespace

}  // namespace naf

using namespace naf;

extern "C" int naf_backproject_scan_gather(const float *values, const uint32_t *view_index, uint32_t n_sub, uint32_t n_scan_views,
                                           const uint32_t *dims, const float *dvoxel, const float *poses, const naf_detector *det,
                                           float step, float *volume, float *den, void *workspace,
                                           size_t workspace_bytes, void *stream) {
    if (n_sub == 0) return NAF_OK;
    const char *who = "backproject_scan_gather";
    ScanLaunch s;
    const int rc = make_scan_launch(who, volume, {values}, dims, dvoxel, poses, n_sub, det, step, &s, kScanVoxels, view_index,
                                    n_scan_views);
    if (rc != NAF_OK) return rc;
    const ProjVolume &v = s.v;
    const RayGeo &g = s.g;
    const uint64_t per_view = (uint64_t)g.W * g.H;
    const uint64_t bricks_x = (dims[0] + 3u) / 4u, bricks_y = (dims[1] + 3u) / 4u, blocks_z = (dims[2] + 15u) / 16u;
    const char *what = nullptr;
    if (!(g.du != 0.0f) || !(g.dv != 0.0f) || !std::isfinite(g.du) || !std::isfinite(g.dv)) what = "pixel pitch must be finite and not 0";
    else if (den == volume) what = "volume and den must be two volumes";
    else if (per_view > 0x7fffffffull) what = "too many pixels in a view";
    else if (bricks_x * bricks_y * blocks_z > 0x7fffffffull) what = "too many voxels for one call";
    else if (!aligned(workspace, 7u)) what = "workspace must be 8-byte aligned";
    else if (workspace && workspace_bytes < per_view * NAF_GATHER_SPAN_BYTES) what = "workspace too small for the spans of one view";
    if (what) return fail_who(who, what);
    GatherSpan *spans = static_cast<GatherSpan *>(workspace);
    // With a table the views go in groups that fit the workspace, each group a pre-pass and a gather; a voxel adds its views in
    // launch order either way, so the grouping does not change a bit.
    const uint64_t fit = workspace ? workspace_bytes / (per_view * NAF_GATHER_SPAN_BYTES) : n_sub;
    const uint32_t group = (uint32_t)std::min<uint64_t>({fit, n_sub, 0x7fffffffull * 256u / per_view});
    const dim3 grid_dim((uint32_t)(bricks_x * bricks_y * blocks_z));
    for (uint32_t first = 0; first < n_sub; first += group) {
        GatherViews list{view_index, n_scan_views, first, std::min(group, n_sub - first)};
        if (workspace) {
            const uint64_t blocks = (per_view * list.count + 255u) / 256u;
            const int rs = launch("gather_spans_kernel", gather_spans_kernel, dim3((uint32_t)blocks), dim3(256), 0, (hipStream_t)stream,
                                  v, poses, g, list, spans);
            if (rs != NAF_OK) return rs;
        }
        auto kernel = workspace ? (den ? backproject_gather_kernel<true, true> : backproject_gather_kernel<true, false>)
                                : (den ? backproject_gather_kernel<false, true> : backproject_gather_kernel<false, false>);
        const int rk = launch("backproject_gather_kernel", kernel, grid_dim, dim3(256), 0, (hipStream_t)stream, v, volume, den, values,
                              poses, g, list, (const GatherSpan *)spans, (uint32_t)bricks_y, (uint32_t)blocks_z);
        if (rk != NAF_OK) return rk;
    }
    return NAF_OK;
}
