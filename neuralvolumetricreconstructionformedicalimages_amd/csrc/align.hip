// align.hip -- reprojection alignment of projections for gfx950: the score table of a window of integer translations of every view
// against its reprojection (naf_align_shift_scores), the sub-pixel peak of each table (naf_align_peak) and the cubic-convolution
// resampler that undoes a view's shift (naf_align_shift_views).  Defined in include/naf_hip.h (A1) and DESIGN.md section 25; the
// per-view arithmetic is csrc/align_device.h.
//
//   align_scores_kernel   a workgroup owns one 16 x 64 tile of one view's interior window.  It stages that tile of p (and of w) and the
//                         (16 + 2 Rv) x (64 + 2 Ru) halo tile of b in LDS; lane t owns the shifts t, t + T, .. (T lanes, at most five
//                         shifts each for the largest window of 33 x 33) and walks the tile once, row-major, with one fp64 accumulator
//                         per owned shift.  p and w are LDS broadcasts.  The halo's row pitch is 64 + (2 Ru + 1) words, so the word a
//                         lane reads for shift s = j (2 Ru + 1) + i of pixel (r, c) is (r + j) pitch + c + i = s + const (mod 64):
//                         the lanes of a wave, which own consecutive s, read 64 different banks whatever the window.  The partial of
//                         (view, tile, shift) goes to the workspace.
//   align_reduce_kernel   one lane per (view, shift) adds that shift's tile partials in ascending tile order.
//   align_peak_kernel     one wave per view: each lane takes the best of its scores in ascending order, a fixed tree in LDS takes the
//                         best of the lanes (smaller value, then lower index), lane 0 refines it (align_refine).
//   align_shift_kernel    one lane per output pixel, 64 x 4 pixels per workgroup; the view's two shifts, and with them the tap offsets
//                         and weights of both axes, are uniform over the workgroup.
//
// No atomics anywhere, and every sum has one order that depends on the shapes alone: equal inputs give equal bits, and a view's
// scores do not depend on which other views are in the call.  T is the smallest multiple of 64 with ceil(S / T) = ceil(S / 256) for
// S shifts, so that few lanes idle when S is just above a multiple of 256 (S = 289 for R = 8: 192 lanes with two shifts or one).
#include <cmath>

#include "naf_host.h"
#include "align_device.h"

namespace naf {

namespace {

constexpr uint32_t kTileH = 16, kTileW = 64;
constexpr uint32_t kMaxR = NAF_ALIGN_MAX_SHIFT;
constexpr uint32_t kHaloH = kTileH + 2u * kMaxR;                       // 48 rows
constexpr uint32_t kHaloPitch = kTileW + 2u * kMaxR + 1u;              // at most 97 words
constexpr uint32_t kScoreThreads = 256;
constexpr uint32_t kPerLane = 5;                                       // ceil(33 * 33 / 256)
constexpr uint32_t kReduceThreads = 256;
constexpr uint32_t kPeakThreads = 64;
constexpr uint32_t kShiftW = 64, kShiftH = 4;
constexpr uint32_t kMaxExtent = NAF_ALIGN_MAX_EXTENT;

static_assert(kMaxR == kAlignMaxShift, "align_device.h and naf_hip.h disagree");
static_assert(kPerLane * kScoreThreads >= (2u * kMaxR + 1u) * (2u * kMaxR + 1u), "a lane owns at most kPerLane shifts");

struct ScorePlan {
    uint32_t H, W, Rv, Ru;
    uint32_t nu, S;                    // 2 Ru + 1 and the number of shifts
    uint32_t tiles_x, tiles;           // tiles along u and per view
    uint32_t threads, per_lane;
    uint32_t pitch;                    // words between halo rows
};

template <bool kHasW>
__global__ void __launch_bounds__(kScoreThreads)
align_scores_kernel(const float *__restrict__ b, const float *__restrict__ p, const float *__restrict__ w, ScorePlan g,
                    double *__restrict__ partials) {
    __shared__ float sb[kHaloH * kHaloPitch];
    __shared__ float sp[kTileH * kTileW];
    __shared__ float sw[kHasW ? kTileH * kTileW : 1];
    const uint32_t tid = threadIdx.x, T = g.threads;
    const uint32_t n = blockIdx.x / g.tiles, tile = blockIdx.x % g.tiles;
    const uint32_t r0 = (tile / g.tiles_x) * kTileH, c0 = (tile % g.tiles_x) * kTileW;
    const uint32_t Hi = g.H - 2u * g.Rv, Wi = g.W - 2u * g.Ru;          // the interior window; r0 < Hi and c0 < Wi
    const uint32_t th = min(kTileH, Hi - r0), tw = min(kTileW, Wi - c0);
    const uint32_t hh = th + 2u * g.Rv, hw = tw + 2u * g.Ru;            // r0 + hh <= H and c0 + hw <= W
    const uint64_t view = (uint64_t)n * g.H * g.W;
    const float *bn = b + view, *pn = p + view;
    for (uint32_t e = tid; e < hh * hw; e += T) {
        const uint32_t hr = e / hw, hc = e % hw;
        sb[hr * g.pitch + hc] = bn[(uint64_t)(r0 + hr) * g.W + c0 + hc];
    }
    for (uint32_t e = tid; e < th * tw; e += T) {
        const uint32_t lr = e / tw, lc = e % tw;
        const uint64_t at = (uint64_t)(g.Rv + r0 + lr) * g.W + g.Ru + c0 + lc;
        sp[lr * kTileW + lc] = pn[at];
        if (kHasW) sw[lr * kTileW + lc] = w[view + at];
    }
    __syncthreads();
    double acc[kPerLane];
    uint32_t off[kPerLane];
#pragma unroll
    for (uint32_t k = 0; k < kPerLane; ++k) {
        const uint32_t s = tid + k * T;
        acc[k] = 0.0;
        off[k] = s < g.S ? (s / g.nu) * g.pitch + s % g.nu : 0u;          // a shift past the table reads word 0 and is not stored
    }
    for (uint32_t lr = 0; lr < th; ++lr) {
        for (uint32_t lc = 0; lc < tw; ++lc) {
            const float pv = sp[lr * kTileW + lc];
            const float wv = kHasW ? sw[lr * kTileW + lc] : 1.0f;
            const uint32_t at = lr * g.pitch + lc;
#pragma unroll
            for (uint32_t k = 0; k < kPerLane; ++k)
                if (k < g.per_lane) acc[k] += kHasW ? align_term(sb[at + off[k]], pv, wv) : align_term(sb[at + off[k]], pv);
        }
    }
    double *out = partials + (uint64_t)blockIdx.x * g.S;
#pragma unroll
    for (uint32_t k = 0; k < kPerLane; ++k) {
        const uint32_t s = tid + k * T;
        if (k < g.per_lane && s < g.S) out[s] = acc[k];
    }
}

__global__ void __launch_bounds__(kReduceThreads)
align_reduce_kernel(const double *__restrict__ partials, uint64_t total, uint32_t S, uint32_t tiles, double *__restrict__ scores) {
    const uint64_t e = (uint64_t)blockIdx.x * kReduceThreads + threadIdx.x;           // n * S + s
    if (e >= total) return;
    const uint64_t n = e / S, s = e % S;
    const double *q = partials + n * tiles * S + s;
    double sum = 0.0;
    for (uint32_t t = 0; t < tiles; ++t) sum += q[(uint64_t)t * S];
    scores[e] = sum;
}

__global__ void __launch_bounds__(kPeakThreads)
align_peak_kernel(const double *__restrict__ scores, uint32_t Rv, uint32_t Ru, float *__restrict__ shifts, int32_t *__restrict__ flags) {
    __shared__ double sv[kPeakThreads];
    __shared__ uint32_t si[kPeakThreads];
    __shared__ uint32_t sbad[kPeakThreads];
    constexpr uint32_t kNone = 0xffffffffu;
    const uint32_t lane = threadIdx.x, S = (2u * Rv + 1u) * (2u * Ru + 1u);
    const double *t = scores + (uint64_t)blockIdx.x * S;
    double best = 0.0;
    uint32_t at = kNone, bad = 0u;
    for (uint32_t s = lane; s < S; s += kPeakThreads) {                  // ascending: a strict < keeps the lowest index
        const double v = t[s];
        if (!align_finite(v)) bad = 1u;
        else if (at == kNone || v < best) best = v, at = s;
    }
    sv[lane] = best, si[lane] = at, sbad[lane] = bad;
    __syncthreads();
    for (uint32_t h = kPeakThreads / 2; h > 0; h >>= 1) {
        if (lane < h) {
            const uint32_t o = lane + h;
            sbad[lane] |= sbad[o];
            if (si[o] != kNone && (si[lane] == kNone || align_better(sv[o], si[o], sv[lane], si[lane]))) sv[lane] = sv[o], si[lane] = si[o];
        }
        __syncthreads();
    }
    if (lane == 0) {
        float shift[2] = {0.0f, 0.0f};
        int f = kAlignFlagNonFinite;
        if (!sbad[0]) align_refine(t, Rv, Ru, si[0], shift, &f);
        shifts[2u * blockIdx.x] = shift[0];
        shifts[2u * blockIdx.x + 1u] = shift[1];
        flags[blockIdx.x] = f;
    }
}

__global__ void __launch_bounds__(kShiftW * kShiftH)
align_shift_kernel(const float *__restrict__ views, const float *__restrict__ shifts, uint32_t H, uint32_t W, uint32_t bx, uint32_t by,
                   float *__restrict__ out) {
    const uint32_t per_view = bx * by;
    const uint32_t n = blockIdx.x / per_view, rest = blockIdx.x % per_view;
    const uint32_t c = (rest % bx) * kShiftW + threadIdx.x % kShiftW, r = (rest / bx) * kShiftH + threadIdx.x / kShiftW;
    const AlignAxis au = align_axis(shifts[2u * n], W), av = align_axis(shifts[2u * n + 1u], H);
    if (r >= H || c >= W) return;
    const uint64_t view = (uint64_t)n * H * W;
    out[view + (uint64_t)r * W + c] = align_sample(views + view, H, W, r, c, av, au);
}

// The window of a view: 0 <= R <= 16 and 2 R < extent on each axis, extents in 1 .. 2^24.
const char *window_error(uint32_t H, uint32_t W, uint32_t Rv, uint32_t Ru) {
    if (H == 0 || W == 0) return "zero view dimension";
    if (H > kMaxExtent || W > kMaxExtent) return "view dimension above 2^24";
    if (Rv > kMaxR || Ru > kMaxR) return "max shift above 16";
    if (2u * Rv >= H || 2u * Ru >= W) return "the search window needs 2 R < extent on each axis";
    return nullptr;
}

bool plan_scores(uint32_t N, uint32_t H, uint32_t W, uint32_t Rv, uint32_t Ru, ScorePlan *g, uint64_t *blocks) {
    g->H = H, g->W = W, g->Rv = Rv, g->Ru = Ru;
    g->nu = 2u * Ru + 1u;
    g->S = g->nu * (2u * Rv + 1u);
    g->tiles_x = (W - 2u * Ru + kTileW - 1u) / kTileW;
    const uint64_t tiles = (uint64_t)g->tiles_x * ((H - 2u * Rv + kTileH - 1u) / kTileH);
    g->per_lane = (g->S + kScoreThreads - 1u) / kScoreThreads;
    g->threads = (((g->S + g->per_lane - 1u) / g->per_lane) + 63u) & ~63u;
    g->pitch = kTileW + g->nu;
    *blocks = tiles * N;
    if (*blocks > 0x7fffffffull) return false;
    g->tiles = (uint32_t)tiles;
    return true;
}

}  // namespace

}  // namespace naf

using namespace naf;

extern "C" size_t naf_align_scores_workspace_bytes(uint32_t N, uint32_t H, uint32_t W, uint32_t Rv, uint32_t Ru) {
    ScorePlan g;
    uint64_t blocks;
    if (window_error(H, W, Rv, Ru) || !plan_scores(N, H, W, Rv, Ru, &g, &blocks)) return 0;
    return (size_t)(blocks * g.S * sizeof(double));
}

extern "C" int naf_align_shift_scores(const float *b, const float *p, const float *w, uint32_t N, uint32_t H, uint32_t W, uint32_t Rv,
                                      uint32_t Ru, void *workspace, size_t workspace_bytes, double *scores, void *stream) {
    const char *who = "align_shift_scores";
    if (N == 0) return NAF_OK;
    if (!b || !p || !scores || !workspace) return fail_who(who, "null pointer");
    if (const char *err = window_error(H, W, Rv, Ru)) return fail_who(who, err);
    if (!aligned(b, 3u) || !aligned(p, 3u) || !aligned(w, 3u)) return misaligned(who, "views", 4);
    if (!aligned(scores, 7u) || !aligned(workspace, 7u)) return misaligned(who, "scores and workspace", 8);
    ScorePlan g;
    uint64_t blocks;
    if (!plan_scores(N, H, W, Rv, Ru, &g, &blocks)) return fail_who(who, "too many tiles for one call");
    const uint64_t need = blocks * g.S * sizeof(double);
    if (workspace_bytes < need) return workspace_too_small(who, workspace_bytes, need);
    const uint64_t total = (uint64_t)N * g.S;
    const uint64_t reduce_blocks = (total + kReduceThreads - 1u) / kReduceThreads;
    hipStream_t s = (hipStream_t)stream;
    double *partials = static_cast<double *>(workspace);
    auto kernel = w ? align_scores_kernel<true> : align_scores_kernel<false>;
    const int launched = launch("align_scores_kernel", kernel, dim3((uint32_t)blocks), dim3(g.threads), 0, s, b, p, w, g, partials);
    if (launched != NAF_OK) return launched;
    return launch("align_reduce_kernel", align_reduce_kernel, dim3((uint32_t)reduce_blocks), dim3(kReduceThreads), 0, s, partials, total,
                  g.S, g.tiles, scores);
}

extern "C" int naf_align_peak(const double *scores, uint32_t N, uint32_t Rv, uint32_t Ru, float *shifts, int32_t *flags, void *stream) {
    const char *who = "align_peak";
    if (N == 0) return NAF_OK;
    if (!scores || !shifts || !flags) return fail_who(who, "null pointer");
    if (Rv > kMaxR || Ru > kMaxR) return fail_who(who, "max shift above 16");
    if (N > 0x7fffffffu) return fail_who(who, "too many views for one call");
    if (!aligned(scores, 7u) || !aligned(shifts, 3u) || !aligned(flags, 3u)) return fail_who(who, "misaligned pointer");
    hipStream_t s = (hipStream_t)stream;
    return launch("align_peak_kernel", align_peak_kernel, dim3(N), dim3(kPeakThreads), 0, s, scores, Rv, Ru, shifts, flags);
}

extern "C" int naf_align_shift_views(const float *views, const float *shifts, uint32_t N, uint32_t H, uint32_t W, float *out,
                                     void *stream) {
    const char *who = "align_shift_views";
    if (N == 0) return NAF_OK;
    if (!views || !shifts || !out) return fail_who(who, "null pointer");
    if (H == 0 || W == 0) return fail_who(who, "zero view dimension");
    if (H > kMaxExtent || W > kMaxExtent) return fail_who(who, "view dimension above 2^24");
    if (views == out) return fail_who(who, "out must not be the views: every output pixel reads sixteen input pixels");
    if (!aligned(views, 3u) || !aligned(shifts, 3u) || !aligned(out, 3u)) return misaligned(who, "pointers", 4);
    const uint32_t bx = (W + kShiftW - 1u) / kShiftW, by = (H + kShiftH - 1u) / kShiftH;
    const uint64_t blocks = (uint64_t)bx * by * N;
    if (blocks > 0x7fffffffull) return fail_who(who, "too many pixels for one call");
    hipStream_t s = (hipStream_t)stream;
    return launch("align_shift_kernel", align_shift_kernel, dim3((uint32_t)blocks), dim3(kShiftW * kShiftH), 0, s, views, shifts, H, W,
                  bx, by, out);
}
