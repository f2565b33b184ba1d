// volume_sample.hip -- trilinear samples of an fp32 volume at world points for gfx950 (naf_volume_sample_points), and the fused
// draw-and-sample that feeds the field fit (naf_volume_draw_sample, pretrain.fit_volume).  Defined in include/naf_hip.h (V4) and
// DESIGN.md section 24; the per-point arithmetic is csrc/volume_sample_device.h.
//
// Layout: one lane per point, 256 lanes per workgroup, no LDS, no atomics.  The work is eight dependent-free gathers per point from
// a volume that fits the caches at 256^3, so the kernel is latency work: all eight loads of a point are issued before the first is
// used (sample_corners), and the small register footprint leaves the occupancy at the hardware's limit to hide them.  The points are
// a contiguous [n, 3] stream: a lane reads its point with ONE 12-byte load (global_load_dwordx3; a wave covers 768 contiguous bytes
// with one instruction) rather than three 4-byte loads at a stride of 12 bytes, which would issue three instructions over the same
// six cache lines.  The draw kernel writes its points the same way.
#include <cmath>

#include "naf_host.h"
#include "volume_sample_device.h"

namespace naf {

namespace {

constexpr uint32_t kSampleThreads = 256;

struct Point3 {                        // 12 bytes, 4-byte aligned: one dwordx3 access
    float x, y, z;
};

struct DrawBox {
    float lo[3], hi[3];
};

__global__ void __launch_bounds__(kSampleThreads)
volume_sample_points_kernel(const float *__restrict__ f, VoxelGrid g, const Point3 *__restrict__ points, uint64_t n,
                            float *__restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * kSampleThreads + threadIdx.x;
    if (i >= n) return;
    const Point3 q = points[i];
    const float p[3] = {q.x, q.y, q.z};
    out[i] = sample_point(f, g, p);
}

__global__ void __launch_bounds__(kSampleThreads)
volume_draw_sample_kernel(const float *__restrict__ f, VoxelGrid g, DrawBox box, uint64_t seed, uint32_t step, uint32_t n,
                          Point3 *__restrict__ points_out, float *__restrict__ targets_out) {
    const uint32_t i = blockIdx.x * kSampleThreads + threadIdx.x;
    if (i >= n) return;
    float p[3];
    sample_draw(seed, step, i, box.lo, box.hi, p);
    const float v = sample_point(f, g, p);
    Point3 q;
    q.x = p[0];
    q.y = p[1];
    q.z = p[2];
    points_out[i] = q;
    targets_out[i] = v;
}

// Argument checks shared by the two entry points; fills the grid.
int sample_check(const char *who, const float *volume, uint32_t n1, uint32_t n2, uint32_t n3, const float *dvoxel, VoxelGrid *g) {
    if (!volume || !dvoxel) return fail_who(who, "null pointer");
    if (n1 == 0 || n2 == 0 || n3 == 0) return fail_who(who, "zero volume dimension");
    if (n1 > NAF_VOLUME_SAMPLE_MAX_EXTENT || n2 > NAF_VOLUME_SAMPLE_MAX_EXTENT || n3 > NAF_VOLUME_SAMPLE_MAX_EXTENT)
        return fail_who(who, "volume dimension above 2^24 (an index would not be exact in fp32)");
    for (int a = 0; a < 3; ++a) {
        if (!(dvoxel[a] > 0.0f) || !std::isfinite(dvoxel[a])) return fail_who(who, "voxel size must be > 0 and finite");
    }
    *g = voxel_grid(n1, n2, n3, dvoxel);
    return NAF_OK;
}

}  // namespace

}  // namespace naf

using namespace naf;

extern "C" int naf_volume_sample_points(const float *volume, uint32_t n1, uint32_t n2, uint32_t n3, const float *dvoxel,
                                        const float *points, uint64_t n, float *out, void *stream) {
    if (n == 0) return NAF_OK;
    VoxelGrid g;
    const int rc = sample_check("volume_sample_points", volume, n1, n2, n3, dvoxel, &g);
    if (rc != NAF_OK) return rc;
    if (!points || !out) return fail(NAF_ERR_INVALID_ARGUMENT, "volume_sample_points: null pointer");
    if (!aligned(volume, 3u) || !aligned(points, 3u) || !aligned(out, 3u)) return misaligned("volume_sample_points", "pointers", 4);
    const uint64_t blocks = (n + kSampleThreads - 1) / kSampleThreads;
    if (blocks > 0x7fffffffull) return fail(NAF_ERR_INVALID_ARGUMENT, "volume_sample_points: too many points for one call");
    return launch("volume_sample_points_kernel", volume_sample_points_kernel, dim3((uint32_t)blocks), dim3(kSampleThreads), 0,
                  (hipStream_t)stream, volume, g, reinterpret_cast<const Point3 *>(points), n, out);
}

extern "C" int naf_volume_draw_sample(const float *volume, const uint32_t *dims, const float *dvoxel, const float *lo, const float *hi,
                                      uint64_t seed, uint32_t step, uint32_t n, float *points_out, float *targets_out, void *stream) {
    if (n == 0) return NAF_OK;
    if (!dims) return fail(NAF_ERR_INVALID_ARGUMENT, "volume_draw_sample: null pointer");
    VoxelGrid g;
    const int rc = sample_check("volume_draw_sample", volume, dims[0], dims[1], dims[2], dvoxel, &g);
    if (rc != NAF_OK) return rc;
    if (!lo || !hi || !points_out || !targets_out) return fail(NAF_ERR_INVALID_ARGUMENT, "volume_draw_sample: null pointer");
    if (!aligned(volume, 3u) || !aligned(points_out, 3u) || !aligned(targets_out, 3u))
        return misaligned("volume_draw_sample", "pointers", 4);
    DrawBox box;
    for (int a = 0; a < 3; ++a) {
        if (!std::isfinite(lo[a]) || !std::isfinite(hi[a]) || !(lo[a] <= hi[a]) || !std::isfinite(hi[a] - lo[a]))
            return fail(NAF_ERR_INVALID_ARGUMENT, "volume_draw_sample: the box must be finite with lo <= hi");
        box.lo[a] = lo[a];
        box.hi[a] = hi[a];
    }
    const uint32_t blocks = (uint32_t)(((uint64_t)n + kSampleThreads - 1) / kSampleThreads);
    return launch("volume_draw_sample_kernel", volume_draw_sample_kernel, dim3(blocks), dim3(kSampleThreads), 0, (hipStream_t)stream,
                  volume, g, box, seed, step, n, reinterpret_cast<Point3 *>(points_out), targets_out);
}
