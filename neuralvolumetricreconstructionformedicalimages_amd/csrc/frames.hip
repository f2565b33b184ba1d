// frames.hip -- raw-frame conditioning for gfx950 (naf_frames_condition): flat-field, zinger / dead-pixel median and -log in one
// launch.  Defined in include/naf_hip.h (A3) and DESIGN.md section 29; the per-pixel arithmetic is csrc/frames_device.h.
//
//   frames_condition_kernel   a workgroup of 256 lanes owns a tile of 16 rows x 64 columns of one view.  It stages the window word
//                             (the key of the transmission, or the bad mark) of the tile and of its h-wide reflected halo in LDS:
//                             every word is computed at staging from raw, dark, flat and bad, so a halo pixel is recomputed by each
//                             tile that needs it and nothing is exchanged.  A wave then owns a row of the tile, lane = column, four
//                             rows per wave one after another: the 64 lanes of every window read are 64 consecutive words, free of
//                             bank conflicts.  Per pixel the lane reads its window's minimum (size^2 reads) and, only where that does
//                             not already prove "keep", selects the median by counting (size^4 reads).  The two replacement counts
//                             are summed in LDS and added once per workgroup with one global integer atomic each: integer sums do
//                             not depend on their order, so the counts are the same on every run.
//
// The tile is cut to the image (th x tw pixels), and only the (th + 2 h) x (tw + 2 h) words a lane can reach are staged: their source
// indices lie in [-h, extent - 1 + h], inside what stripe_reflect maps for size <= extent.  The kernel holds no array of its own, so
// it uses no scratch; LDS is 22 x 70 words at size 7.
#include <cmath>

#include "naf_host.h"
#include "frames_device.h"

namespace naf {

namespace {

constexpr uint32_t kThreads = 256, kTileH = 16, kTileW = 64;
constexpr uint32_t kMaxExtent = 1u << 24;
constexpr uint64_t kMaxBlocks = 0x7fffffffull;

static_assert(kFramesLog == NAF_FRAMES_LOG && kFramesClampNonneg == NAF_FRAMES_CLAMP_NONNEG, "frames_device.h and naf_hip.h disagree");
static_assert(kFramesMaxSize == NAF_FRAMES_MAX_SIZE && kTileH == NAF_FRAMES_TILE_H && kTileW == NAF_FRAMES_TILE_W,
              "frames.hip and naf_hip.h disagree");
static_assert(kThreads % kTileW == 0u && kTileH % (kThreads / kTileW) == 0u, "a wave owns whole rows of the tile");

struct FramesPlan {
    uint32_t H, W;
    uint32_t tiles_x, tiles;           // tiles along u, tiles of one view
};

template <typename Raw, uint32_t kSize>
__global__ void __launch_bounds__(kThreads)
frames_condition_kernel(const Raw *__restrict__ raw, const float *__restrict__ dark, const float *__restrict__ flat,
                        const uint8_t *__restrict__ bad, FramesPlan g, float dif, float t_min, uint32_t flags, float *__restrict__ out,
                        uint32_t *__restrict__ counts) {
    constexpr uint32_t h = kSize / 2u, kStride = kTileW + 2u * h, kRows = kTileH + 2u * h;
    __shared__ uint32_t keys[kRows * kStride];
    __shared__ uint32_t tally[2];
    const uint32_t tid = threadIdx.x;
    const uint32_t view = blockIdx.x / g.tiles, tile = blockIdx.x % g.tiles;
    const uint32_t v0 = (tile / g.tiles_x) * kTileH, u0 = (tile % g.tiles_x) * kTileW;
    const uint32_t th = min(kTileH, g.H - v0), tw = min(kTileW, g.W - u0);
    const uint64_t frame = (uint64_t)view * g.H * g.W;
    if (tid < 2u) tally[tid] = 0u;
    for (uint32_t e = tid; e < (th + 2u * h) * kStride; e += kThreads) {
        const uint32_t r = e / kStride, c = e % kStride;
        if (c >= tw + 2u * h) continue;
        const uint32_t v = stripe_reflect((int32_t)(v0 + r) - (int32_t)h, g.H), u = stripe_reflect((int32_t)(u0 + c) - (int32_t)h, g.W);
        const uint64_t at = (uint64_t)v * g.W + u;
        keys[e] = frames_transmission(frames_load(raw, frame + at), dark[at], flat[at], bad != nullptr && bad[at] != 0);
    }
    __syncthreads();
    uint32_t outliers = 0u, bads = 0u;
    const uint32_t c = tid % kTileW;
    if (c < tw) {
        for (uint32_t r = tid / kTileW; r < th; r += kThreads / kTileW) {
            const float t = frames_decide<kSize>(keys + r * kStride + c, kStride, dif, outliers, bads);
            out[frame + (uint64_t)(v0 + r) * g.W + u0 + c] = frames_tail(t, t_min, flags);
        }
    }
    if (counts == nullptr) return;
    if (outliers) atomicAdd(&tally[0], outliers);
    if (bads) atomicAdd(&tally[1], bads);
    __syncthreads();
    if (tid < 2u && tally[tid]) atomicAdd(&counts[2ull * view + tid], tally[tid]);
}

int refuse(const char *what) { return fail_who("frames_condition", what); }

bool overlap(const void *a, uint64_t a_bytes, const void *b, uint64_t b_bytes) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + b_bytes && b0 < a0 + a_bytes;
}

template <typename Raw, uint32_t kSize>
int launch_frames(const void *raw, const float *dark, const float *flat, const uint8_t *bad, const FramesPlan &g, uint32_t blocks, float dif,
                  float t_min, uint32_t flags, float *out, uint32_t *counts, hipStream_t st) {
    return launch("frames_condition_kernel", (frames_condition_kernel<Raw, kSize>), dim3(blocks), dim3(kThreads), 0, st,
                  static_cast<const Raw *>(raw), dark, flat, bad, g, dif, t_min, flags, out, counts);
}

template <typename Raw>
int launch_size(uint32_t size, const void *raw, const float *dark, const float *flat, const uint8_t *bad, const FramesPlan &g,
                uint32_t blocks, float dif, float t_min, uint32_t flags, float *out, uint32_t *counts, hipStream_t st) {
    if (size == 3u) return launch_frames<Raw, 3u>(raw, dark, flat, bad, g, blocks, dif, t_min, flags, out, counts, st);
    if (size == 5u) return launch_frames<Raw, 5u>(raw, dark, flat, bad, g, blocks, dif, t_min, flags, out, counts, st);
    return launch_frames<Raw, 7u>(raw, dark, flat, bad, g, blocks, dif, t_min, flags, out, counts, st);
}

}  // namespace

}  // namespace naf

using namespace naf;

extern "C" int naf_frames_condition(const void *raw, int raw_dtype, const float *dark, const float *flat, const uint8_t *bad, uint32_t N,
                                    uint32_t H, uint32_t W, uint32_t size, float dif, float t_min, uint32_t flags, float *out,
                                    uint32_t *counts, void *stream) {
    if (N == 0 || H == 0 || W == 0) return NAF_OK;
    if (!raw || !dark || !flat || !out) return refuse("null pointer");
    if (raw_dtype != NAF_FRAMES_RAW_F32 && raw_dtype != NAF_FRAMES_RAW_U16) return refuse("raw_dtype must be NAF_FRAMES_RAW_F32 or NAF_FRAMES_RAW_U16");
    if (H > kMaxExtent || W > kMaxExtent) return refuse("view dimension above 2^24");
    if (size != 3u && size != 5u && size != 7u) return refuse("size must be 3, 5 or 7");
    if (size > H) return refuse("size above the number of detector rows");
    if (size > W) return refuse("size above the number of detector columns");
    if (!std::isfinite(dif) || dif < 0.0f) return refuse("dif must be finite and not negative");
    if (!std::isfinite(t_min) || !(t_min > 0.0f)) return refuse("t_min must be finite and above zero");
    if (flags & ~(NAF_FRAMES_LOG | NAF_FRAMES_CLAMP_NONNEG)) return refuse("unknown flag bits");
    if ((flags & NAF_FRAMES_CLAMP_NONNEG) && !(flags & NAF_FRAMES_LOG)) return refuse("NAF_FRAMES_CLAMP_NONNEG needs NAF_FRAMES_LOG");
    const bool f32 = raw_dtype == NAF_FRAMES_RAW_F32;
    if (!aligned(raw, f32 ? 3u : 1u)) return refuse(f32 ? "float32 raw must be 4-byte aligned" : "uint16 raw must be 2-byte aligned");
    if (!aligned(dark, 3u) || !aligned(flat, 3u) || !aligned(out, 3u) || !aligned(counts, 3u))
        return refuse("dark, flat, out and counts must be 4-byte aligned");
    FramesPlan g;
    g.H = H, g.W = W;
    g.tiles_x = (W + kTileW - 1u) / kTileW;
    const uint64_t tiles = (uint64_t)g.tiles_x * ((H + kTileH - 1u) / kTileH);
    if (tiles > kMaxBlocks / N) return refuse("more than 2^31 - 1 tiles of 16 x 64 pixels");
    g.tiles = (uint32_t)tiles;
    const uint64_t frame = (uint64_t)H * W, all = frame * N;               // below 2^41 elements once the tiles fit
    if (overlap(out, all * 4u, raw, all * (f32 ? 4u : 2u)) || overlap(out, all * 4u, dark, frame * 4u) ||
        overlap(out, all * 4u, flat, frame * 4u) || (bad && overlap(out, all * 4u, bad, frame)))
        return refuse("out must not overlap raw, dark, flat or bad");
    const uint32_t blocks = (uint32_t)(tiles * N);
    hipStream_t st = (hipStream_t)stream;
    if (f32) return launch_size<float>(size, raw, dark, flat, bad, g, blocks, dif, t_min, flags, out, counts, st);
    return launch_size<uint16_t>(size, raw, dark, flat, bad, g, blocks, dif, t_min, flags, out, counts, st);
}
