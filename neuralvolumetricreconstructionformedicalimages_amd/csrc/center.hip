// center.hip -- the centre-of-rotation search for gfx950 (naf_center_slices, naf_center_metrics): one slice back-projected from
// filtered detector rows for K candidate offsets of the detector's column axis at once, and the two scores of every such slice.
// Defined in include/naf_hip.h (A5) and DESIGN.md section 34; the per-pixel arithmetic is csrc/center_device.h.
//
//   center_slices_kernel   a workgroup of 256 lanes owns a 16 x 16 pixel tile, a group of at most 8 candidates and one slice.  A
//                          lane keeps one accumulator per candidate of the group in registers.  The filtered rows are staged in
//                          LDS as whole rows in chunks of consecutive views (center_chunk_views: 32 KB, or a single row of up to
//                          64 KB): a candidate's column is then an index into the staged row with no window to track, and the
//                          bounds of center_sample are the bounds of the staging.  Per view a lane forms (base, weight) once: two
//                          products and a sum for each rotated coordinate, one division for the magnification; per candidate it
//                          subtracts the candidate's shift and interpolates.  Views are added in index order, so equal inputs give
//                          equal bits.  cos / sin and the candidates' shifts are read at indices that do not depend on the lane.
//   center_partials_kernel a workgroup sums the negativity and the sharpness terms of 2048 consecutive pixels of one slice in fp64
//                          (block_sum.h) into one pair of partials.
//   center_reduce_kernel   one workgroup per slice adds its partials in index order.
//
// Bounds: q is read at [slice, view < N, column < W] only (the staging loop runs over e < views * W of the chunk); a staged row is
// read at floor(k) and floor(k) + 1 with 0 <= floor(k) <= W - 2; f is stored at pixels below n only; cand at k < K only; the
// partials at block < blocks of the slice.  No atomics anywhere.
#include <cmath>
#include <initializer_list>

#include "block_sum.h"
#include "center_device.h"
#include "naf_host.h"

namespace naf {

namespace {

constexpr uint32_t kThreads = 256;
constexpr uint32_t kPixelsPerLane = 8;
constexpr uint32_t kPixelsPerBlock = kThreads * kPixelsPerLane;
constexpr uint64_t kMaxBlocks = 0x7fffffffull;

static_assert(kCenterMaxW == NAF_CENTER_MAX_W && kCenterMaxK == NAF_CENTER_MAX_K && kCenterMaxN == NAF_CENTER_MAX_SIZE &&
                  kCenterGroup == NAF_CENTER_GROUP,
              "center_device.h and naf_hip.h disagree");
static_assert(kCenterTile * kCenterTile == kThreads, "one lane per pixel of the tile");

struct CenterShape {
    uint32_t S, N, W, K, n, tiles, groups, per_group, chunk;
    int parallel;
    float DSO, DSD, inv_du, ou, half, dx, dy, ox, oy, du;
};

__global__ void __launch_bounds__(kThreads)
center_slices_kernel(const float *__restrict__ q, const float *__restrict__ trig, const float *__restrict__ cand, CenterShape g,
                     float *__restrict__ f) {
    extern __shared__ float rows[];                                     // chunk * W floats
    const uint32_t tid = threadIdx.x;
    uint32_t b = blockIdx.x;                                            // tile fastest, then the candidate group, then the slice
    const uint32_t tile = b % (g.tiles * g.tiles);
    b /= g.tiles * g.tiles;
    const uint32_t group = b % g.groups, slice = b / g.groups;
    const uint32_t ix = (tile / g.tiles) * kCenterTile + (tid >> 4), iy = (tile % g.tiles) * kCenterTile + (tid & 15u);
    const bool inside = ix < g.n && iy < g.n;
    const uint32_t k0 = group * g.per_group;
    const uint32_t count = min(g.per_group, g.K - k0);

    float shift[kCenterGroup], acc[kCenterGroup];
#pragma unroll
    for (uint32_t j = 0; j < kCenterGroup; ++j) {
        shift[j] = j < count ? cand[k0 + j] / g.du : 0.0f;
        acc[j] = 0.0f;
    }
    const float x = center_coord(ix, g.n, g.dx, g.ox), y = center_coord(iy, g.n, g.dy, g.oy);
    const float *src = q + (uint64_t)slice * g.N * g.W;
    for (uint32_t i0 = 0; i0 < g.N; i0 += g.chunk) {
        const uint32_t views = min(g.chunk, g.N - i0);
        const uint32_t floats = views * g.W;                            // <= max(kCenterLdsFloats, W)
        __syncthreads();                                                // the previous chunk's readers are done
        for (uint32_t e = tid; e < floats; e += kThreads) rows[e] = src[(uint64_t)i0 * g.W + e];
        __syncthreads();
        if (inside) {
            for (uint32_t v = 0; v < views; ++v) {
                const float ca = trig[2u * (i0 + v)], sa = trig[2u * (i0 + v) + 1u];
                const CenterTerm term = center_term(g.parallel, x, y, ca, sa, g.DSO, g.DSD, g.ou, g.inv_du, g.half);
                center_accumulate(acc, shift, count, rows + v * g.W, g.W, term);
            }
        }
    }
    if (!inside) return;
    const uint64_t plane = (uint64_t)g.n * g.n;
#pragma unroll
    for (uint32_t j = 0; j < kCenterGroup; ++j)
        if (j < count) f[((uint64_t)slice * g.K + k0 + j) * plane + (uint64_t)ix * g.n + iy] = acc[j];
}

// blockIdx.x = image * blocks + block: the pixels [block * 2048, ..) of image (slice, candidate), lane tid taking tid, tid + 256, ..
__global__ void __launch_bounds__(kThreads)
center_partials_kernel(const float *__restrict__ f, uint32_t n, uint32_t blocks, double dx, double dy, double r,
                       double *__restrict__ partials) {
    __shared__ double red[2][kThreads];
    const uint32_t tid = threadIdx.x;
    const uint32_t image = blockIdx.x / blocks, block = blockIdx.x % blocks;
    const uint32_t pixels = n * n;                                      // n <= 4096
    const float *img = f + (uint64_t)image * pixels;
    double neg = 0.0, sharp = 0.0;
#pragma unroll
    for (uint32_t j = 0; j < kPixelsPerLane; ++j) {
        const uint32_t p = block * kPixelsPerBlock + j * kThreads + tid;
        if (p >= pixels) continue;
        const uint32_t ix = p / n, iy = p - ix * n;
        if (!center_in_mask(ix, iy, n, dx, dy, r)) continue;
        const float v = img[p];
        neg += center_negativity(v);
        if (ix + 1u < n && center_in_mask(ix + 1u, iy, n, dx, dy, r)) sharp += center_step(v, img[p + n]);
        if (iy + 1u < n && center_in_mask(ix, iy + 1u, n, dx, dy, r)) sharp += center_step(v, img[p + 1u]);
    }
    block_sum<kThreads>(red, neg, sharp, tid);
    if (tid == 0) {
        partials[2ull * blockIdx.x] = red[0][0];
        partials[2ull * blockIdx.x + 1u] = red[1][0];
    }
}

__global__ void __launch_bounds__(kThreads)
center_reduce_kernel(const double *__restrict__ partials, uint32_t blocks, double *__restrict__ out) {
    __shared__ double red[2][kThreads];
    const uint32_t tid = threadIdx.x;
    const double *mine = partials + 2ull * blockIdx.x * blocks;
    double neg = 0.0, sharp = 0.0;
    for (uint32_t i = tid; i < blocks; i += kThreads) {
        neg += mine[2u * i];
        sharp += mine[2u * i + 1u];
    }
    block_sum<kThreads>(red, neg, sharp, tid);
    if (tid == 0) {
        out[2ull * blockIdx.x] = red[0][0];
        out[2ull * blockIdx.x + 1u] = red[1][0];
    }
}

uint32_t metric_blocks(uint32_t n) { return (uint32_t)(((uint64_t)n * n + kPixelsPerBlock - 1u) / kPixelsPerBlock); }

bool finite_all(std::initializer_list<float> v) {
    for (float x : v)
        if (!std::isfinite(x)) return false;
    return true;
}

}  // namespace

}  // namespace naf

using namespace naf;

extern "C" int naf_center_slices(const float *q, const float *trig, const float *cand, uint32_t S, uint32_t N, uint32_t W, uint32_t K,
                                 uint32_t n, int parallel, float DSO, float DSD, float du, float ou, float dx, float dy, float ox, float oy,
                                 float *f, void *stream) {
    const char *who = "center_slices";
    if (S == 0 || n == 0) return NAF_OK;
    if (!q || !trig || !cand || !f) return fail_who(who, "null pointer");
    if (N < 1) return fail_who(who, "at least one view is needed");
    if (W < 1 || W > kCenterMaxW) return fail_who(who, "the row width must be in 1 .. 16384");
    if (K < 1 || K > kCenterMaxK) return fail_who(who, "the number of candidates must be in 1 .. 64");
    if (n > kCenterMaxN) return fail_who(who, "more than 4096 pixels along a side of the slice");
    if (parallel != 0 && parallel != 1) return fail_who(who, "parallel must be 0 or 1");
    if (!finite_all({du, ou, dx, dy, ox, oy}) || !(du > 0.0f) || !(dx > 0.0f) || !(dy > 0.0f))
        return fail_who(who, "du, dx and dy must be finite and above zero, ou and the origin finite");
    if (!parallel) {
        if (!finite_all({DSO, DSD}) || !(DSO > 0.0f) || !(DSD > 0.0f)) return fail_who(who, "DSO and DSD must be finite and above zero");
        const double hx = 0.5 * n * (double)dx + std::fabs((double)ox), hy = 0.5 * n * (double)dy + std::fabs((double)oy);
        if (!(std::sqrt(hx * hx + hy * hy) < (double)DSO)) return fail_who(who, "the source's orbit crosses the slice");
    }
    if (!aligned(q, 3u) || !aligned(trig, 3u) || !aligned(cand, 3u) || !aligned(f, 3u))
        return misaligned(who, "q, trig, cand and f", 4u);
    CenterShape g;
    g.S = S, g.N = N, g.W = W, g.K = K, g.n = n;
    g.tiles = (n + kCenterTile - 1u) / kCenterTile;
    g.groups = (K + kCenterGroup - 1u) / kCenterGroup;
    g.per_group = (K + g.groups - 1u) / g.groups;                       // the candidates split evenly: 33 -> 7, 7, 7, 7, 5
    g.groups = (K + g.per_group - 1u) / g.per_group;
    g.chunk = center_chunk_views(N, W);
    g.parallel = parallel;
    g.DSO = DSO, g.DSD = DSD, g.du = du, g.inv_du = 1.0f / du, g.ou = ou, g.half = 0.5f * (float)W - 0.5f;
    g.dx = dx, g.dy = dy, g.ox = ox, g.oy = oy;
    const uint64_t blocks = (uint64_t)g.tiles * g.tiles * g.groups * S;
    if (blocks > kMaxBlocks) return fail_who(who, "more than 2^31 - 1 workgroups");
    const uint32_t lds = g.chunk * W * (uint32_t)sizeof(float);          // <= 64 KB
    return launch("center_slices_kernel", center_slices_kernel, dim3((uint32_t)blocks), dim3(kThreads), lds, (hipStream_t)stream, q, trig,
                  cand, g, f);
}

extern "C" size_t naf_center_metrics_workspace_bytes(uint32_t S, uint32_t K, uint32_t n) {
    if (n > kCenterMaxN) return 0;
    return (size_t)S * K * metric_blocks(n) * 2u * sizeof(double);
}

extern "C" int naf_center_metrics(const float *f, uint32_t S, uint32_t K, uint32_t n, float dx, float dy, float r, double *out,
                                  void *workspace, size_t workspace_bytes, void *stream) {
    const char *who = "center_metrics";
    if (S == 0 || K == 0) return NAF_OK;
    if (!out) return fail_who(who, "null pointer");
    if (n > kCenterMaxN) return fail_who(who, "more than 4096 pixels along a side of the slice");
    if (!finite_all({dx, dy, r}) || !(dx > 0.0f) || !(dy > 0.0f) || !(r >= 0.0f))
        return fail_who(who, "dx and dy must be finite and above zero, r finite and not below zero");
    const uint32_t blocks = metric_blocks(n);
    const uint64_t images = (uint64_t)S * K;
    if (images * std::max(blocks, 1u) > kMaxBlocks) return fail_who(who, "more than 2^31 - 1 workgroups");
    if (!aligned(f, 3u)) return misaligned(who, "f", 4u);
    if (!aligned(out, 7u) || !aligned(workspace, 7u)) return misaligned(who, "out and workspace", 8u);
    if (n == 0) {
        if (hipMemsetAsync(out, 0, images * 2u * sizeof(double), (hipStream_t)stream) != hipSuccess) return fail(NAF_ERR_LAUNCH, who);
        return NAF_OK;
    }
    if (!f || !workspace) return fail_who(who, "null pointer");
    const uint64_t need = images * blocks * 2u * sizeof(double);
    if (workspace_bytes < need) return workspace_too_small(who, workspace_bytes, need);
    double *partials = (double *)workspace;
    const int rc = launch("center_partials_kernel", center_partials_kernel, dim3((uint32_t)(images * blocks)), dim3(kThreads), 0,
                          (hipStream_t)stream, f, n, blocks, (double)dx, (double)dy, (double)r, partials);
    if (rc != NAF_OK) return rc;
    return launch("center_reduce_kernel", center_reduce_kernel, dim3((uint32_t)images), dim3(kThreads), 0, (hipStream_t)stream,
                  (const double *)partials, blocks, out);
}
