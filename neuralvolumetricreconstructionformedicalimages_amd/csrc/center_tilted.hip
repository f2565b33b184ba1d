// center_tilted.hip -- the tilted-axis (laminographic) centre and tilt search for gfx950 (naf_center_slices_tilted): slices z = const
// back-projected from the filtered projections of a tilted parallel beam for K candidates (offset of the detector's column axis,
// tilt) at once.  Defined in include/naf_hip.h (A5) and DESIGN.md section 35; the per-pixel arithmetic is
// csrc/center_tilted_device.h.  The scores are naf_center_metrics (csrc/center.hip), unchanged.
//
//   center_slices_tilted_kernel   the work split of center_slices_kernel: a workgroup of 256 lanes owns a 16 x 16 pixel tile, a group
//                                 of at most 8 candidates and one slice; a lane keeps one accumulator per candidate of the group in
//                                 registers and forms (base, s) once per view.  A pixel's detector row moves with the view and the
//                                 candidate's tilt, so no whole rows are staged: the four taps of a sample are read from global
//                                 memory, where the 16 x 16 tile's footprint in a view is a patch of about 16 x 16 detector pixels
//                                 that neighbouring candidates share.  Views are added in index order, so equal inputs give equal
//                                 bits.  cos / sin, the candidates (kernel arguments) and z are read at indices that do not depend
//                                 on the lane.
//
// Bounds: q is read at [view < N, floor(r) + {0, 1} <= H - 1, floor(k) + {0, 1} <= W - 1] only (center_tilted_sample); f is stored at
// pixels below n only; the candidate table at k < K only; z at slice < S.  No atomics anywhere.
#include <hip/hip_runtime.h>

#include <cmath>
#include <initializer_list>

#include "center_tilted_device.h"
#include "naf_host.h"

namespace naf {

namespace {

constexpr uint32_t kThreads = 256;
constexpr uint64_t kMaxBlocks = 0x7fffffffull;

static_assert(kCenterMaxK == NAF_CENTER_MAX_K && kCenterGroup == NAF_CENTER_GROUP, "center_device.h and naf_hip.h disagree");
static_assert(kCenterTile * kCenterTile == kThreads, "one lane per pixel of the tile");

struct CenterTiltedShape {
    uint32_t S, N, H, W, K, n, tiles, groups, per_group;
    float inv_du, inv_dv, ou, ov, half_u, half_v, dx, dy, ox, oy;
    float cand[kCenterMaxK][3];                                         // (c_k / du, sin tau_k, cos tau_k), rows below K
};

__global__ void __launch_bounds__(kThreads)
center_slices_tilted_kernel(const float *__restrict__ q, const float *__restrict__ trig, const float *__restrict__ z, CenterTiltedShape g,
                            float *__restrict__ f) {
    const uint32_t tid = threadIdx.x;
    uint32_t b = blockIdx.x;                                            // tile fastest, then the candidate group, then the slice
    const uint32_t tile = b % (g.tiles * g.tiles);
    b /= g.tiles * g.tiles;
    const uint32_t group = b % g.groups, slice = b / g.groups;
    const uint32_t ix = (tile / g.tiles) * kCenterTile + (tid >> 4), iy = (tile % g.tiles) * kCenterTile + (tid & 15u);
    if (!(ix < g.n && iy < g.n)) return;                                // no barrier below
    const uint32_t k0 = group * g.per_group;
    const uint32_t count = min(g.per_group, g.K - k0);

    float cand[kCenterGroup][3], acc[kCenterGroup];
#pragma unroll
    for (uint32_t j = 0; j < kCenterGroup; ++j) {
        const uint32_t k = j < count ? k0 + j : k0;                      // k0 < K: a row that exists
#pragma unroll
        for (uint32_t c = 0; c < 3; ++c) cand[j][c] = g.cand[k][c];
        acc[j] = 0.0f;
    }
    const float x = center_coord(ix, g.n, g.dx, g.ox), y = center_coord(iy, g.n, g.dy, g.oy);
    const float height = z[slice];
    const uint64_t view_floats = (uint64_t)g.H * g.W;
    for (uint32_t i = 0; i < g.N; ++i) {
        const float ca = trig[2u * i], sa = trig[2u * i + 1u];
        const CenterTiltedTerm term = center_tilted_term(x, y, ca, sa, g.ou, g.inv_du, g.half_u);
        center_tilted_accumulate(acc, cand, count, q + i * view_floats, g.H, g.W, term, height, g.ov, g.inv_dv, g.half_v);
    }
    const uint64_t plane = (uint64_t)g.n * g.n;
#pragma unroll
    for (uint32_t j = 0; j < kCenterGroup; ++j)
        if (j < count) f[((uint64_t)slice * g.K + k0 + j) * plane + (uint64_t)ix * g.n + iy] = center_tilted_result(acc[j], cand[j][2]);
}

bool finite_all(std::initializer_list<float> v) {
    for (float x : v)
        if (!std::isfinite(x)) return false;
    return true;
}

}  // namespace

}  // namespace naf

using namespace naf;

extern "C" int naf_center_slices_tilted(const float *q, const float *trig, const float *cand_host, const float *z, uint32_t S, uint32_t N,
                                        uint32_t H, uint32_t W, uint32_t K, uint32_t n, float du, float dv, float ou, float ov, float dx,
                                        float dy, float ox, float oy, float *f, void *stream) {
    const char *who = "center_slices_tilted";
    if (!q || !trig || !cand_host || !z || !f) return fail_who(who, "null pointer");
    if (S < 1) return fail_who(who, "at least one slice is needed");
    if (N < 1) return fail_who(who, "at least one view is needed");
    if (H < 2 || H > (1u << 24)) return fail_who(who, "the number of detector rows must be in 2 .. 2^24");
    if (W < 2 || W > kCenterMaxW) return fail_who(who, "the row width must be in 2 .. 16384");
    if (K < 1 || K > kCenterMaxK) return fail_who(who, "the number of candidates must be in 1 .. 64");
    if (n > kCenterMaxN) return fail_who(who, "more than 4096 pixels along a side of the slice");
    if (!finite_all({du, dv, ou, ov, dx, dy, ox, oy}) || !(du > 0.0f) || !(dv > 0.0f) || !(dx > 0.0f) || !(dy > 0.0f))
        return fail_who(who, "du, dv, dx and dy must be finite and above zero, ou, ov and the origin finite");
    if (!aligned(q, 3u) || !aligned(trig, 3u) || !aligned(cand_host, 3u) || !aligned(z, 3u) || !aligned(f, 3u))
        return misaligned(who, "q, trig, cand_host, z and f", 4u);
    CenterTiltedShape g;
    for (uint32_t k = 0; k < K; ++k) {                                  // host memory: read here, passed by value
        const float c = cand_host[3u * k], st = cand_host[3u * k + 1u], ct = cand_host[3u * k + 2u];
        if (!finite_all({c, st, ct})) return fail_who(who, "a candidate is not finite");
        if (!(std::fabs((double)st * st + (double)ct * ct - 1.0) <= 1e-3)) return fail_who(who, "a candidate's (sin, cos) is not a unit vector");
        g.cand[k][0] = c, g.cand[k][1] = st, g.cand[k][2] = ct;
    }
    for (uint32_t k = K; k < kCenterMaxK; ++k) g.cand[k][0] = g.cand[k][1] = g.cand[k][2] = 0.0f;
    if (n == 0) return NAF_OK;
    g.S = S, g.N = N, g.H = H, g.W = W, g.K = K, g.n = n;
    g.tiles = (n + kCenterTile - 1u) / kCenterTile;
    g.groups = (K + kCenterGroup - 1u) / kCenterGroup;
    g.per_group = (K + g.groups - 1u) / g.groups;                       // the candidates split evenly: 33 -> 7, 7, 7, 7, 5
    g.groups = (K + g.per_group - 1u) / g.per_group;
    g.inv_du = 1.0f / du, g.inv_dv = 1.0f / dv, g.ou = ou, g.ov = ov;
    g.half_u = 0.5f * (float)W - 0.5f, g.half_v = 0.5f * (float)H - 0.5f;
    g.dx = dx, g.dy = dy, g.ox = ox, g.oy = oy;
    const uint64_t blocks = (uint64_t)g.tiles * g.tiles * g.groups * S;
    if (blocks > kMaxBlocks) return fail_who(who, "more than 2^31 - 1 workgroups");
    return launch("center_slices_tilted_kernel", center_slices_tilted_kernel, dim3((uint32_t)blocks), dim3(kThreads), 0, (hipStream_t)stream,
                  q, trig, z, g, f);
}
