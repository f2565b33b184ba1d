// filter.hip -- detector-row filter for gfx950 (naf_filter_rows, naf_filter_rows_views): the ramp filter of the FDK baseline, as a
// dense convolution of every detector row with a symmetric tap array.  Defined in include/naf_hip.h (P3) and DESIGN.md sections 15
// and 26; the per-output arithmetic is csrc/filter_device.h.
//
// Layout: one detector row per workgroup.  The workgroup stages the pre-weighted row x[k] = pre[r, k] * in[i, r, k] (times
// col[i, k], the per-view column weight of naf_filter_rows_views, where one is given) and the taps in LDS, then every lane owns
// kR = 8 consecutive outputs n0 .. n0 + 7 and walks k = 0 .. W - 1.  Output n0 + j needs taps[|n0 + j - k|]
// at step k, which is what output n0 + j - 1 used at step k - 1: the lane keeps the eight taps in a register window and each step
// slides one new tap, taps[|n0 - k - 1|], into it.  A step is one broadcast read of x[k] (every lane the same address), one read
// of the new tap and eight FMAs.  The lanes' tap addresses are 8 words apart, which is eight lanes to a bank; the taps are therefore
// stored with one spare word after every eight (slot m + m / 8), which makes that stride 9 and the read conflict-free.
// The window is rotated by register renaming: the k loop is unrolled by eight and the window's slots are addressed by constants.
// A row wider than 8 x 256 outputs is covered in passes by the same workgroup.  No atomics; every output is one fma chain in
// ascending k, so two calls return the same bits.  The whole row is staged before the first store, so `out` may be `in`.
#include <cstdio>

#include "naf_host.h"
#include "filter_device.h"

namespace naf {

namespace {

constexpr uint32_t kR = 8;                 // consecutive outputs per lane = depth of the tap window
constexpr uint32_t kMaxThreads = 256;

__host__ __device__ __forceinline__ uint32_t tap_slot(uint32_t m) { return m + (m >> 3); }
__host__ __device__ __forceinline__ uint32_t row_words(uint32_t W) { return (W + 7u) & ~7u; }
// the row, then the taps 0 .. W in their slots (tap W is a zero that the last slide of a lane reads and never uses)
uint32_t filter_lds_bytes(uint32_t W) { return (row_words(W) + tap_slot(W) + 1u) * (uint32_t)sizeof(float); }

// kCount steps k0 .. k0 + kCount - 1 for the eight outputs of one lane.  On entry win[j] is the tap of output n0 + j at step k0; at
// step k0 + s that tap lives in win[(j - s) mod 8], and the new tap of output n0 replaces the one output n0 + 7 is done with.
// After eight steps the window is back in order.
template <uint32_t kCount>
__device__ __forceinline__ void filter_steps(const float *xs, const float *ts, uint32_t n0, uint32_t k0, float (&win)[kR],
                                             float (&acc)[kR]) {
#pragma unroll
    for (uint32_t s = 0; s < kCount; ++s) {
        const uint32_t k = k0 + s;
        const float x = xs[k];
        const float next = ts[tap_slot(filter_tap_index(n0, k + 1u))];      // |n0 - k - 1| <= W: inside the staged taps
#pragma unroll
        for (uint32_t j = 0; j < kR; ++j) acc[j] = filter_step(acc[j], win[(j + kR - s) % kR], x);
        win[(kR - 1u) - s] = next;
    }
}

__global__ void __launch_bounds__(kMaxThreads)
filter_rows_kernel(const float *in, uint32_t H, uint32_t W, const float *__restrict__ taps, const float *__restrict__ pre,
                   const float *__restrict__ post, const float *__restrict__ view_scale, const float *__restrict__ col, float *out) {
    extern __shared__ __align__(16) float lds[];
    float *xs = lds;                               // [W]
    float *ts = lds + row_words(W);                // tap m at ts[tap_slot(m)], m = 0 .. W

    const uint32_t tid = threadIdx.x, threads = blockDim.x;
    const uint32_t row = blockIdx.x, r = row % H, view = row / H;
    const uint64_t base = (uint64_t)row * W, wbase = (uint64_t)r * W;      // 64-bit: 720 x 2048 x 2048 values is 12 GB
    const uint64_t cbase = (uint64_t)view * W;

    const bool has_pre = pre != nullptr, has_col = col != nullptr;
    for (uint32_t k = tid; k < W; k += threads) {
        xs[k] = filter_stage(in[base + k], has_pre, has_pre ? pre[wbase + k] : 1.0f, has_col, has_col ? col[cbase + k] : 1.0f);
        ts[tap_slot(k)] = taps[k];
    }
    if (tid == 0) ts[tap_slot(W)] = 0.0f;
    __syncthreads();                               // the whole row is in LDS: from here on `out` may overwrite `in`

    const bool has_post = post != nullptr, has_scale = view_scale != nullptr;
    const float scale = has_scale ? view_scale[view] : 1.0f;
    const uint32_t full = W & ~(kR - 1u);
    for (uint32_t n0 = tid * kR; n0 < W; n0 += threads * kR) {
        float win[kR], acc[kR];
#pragma unroll
        for (uint32_t j = 0; j < kR; ++j) {
            win[j] = n0 + j < W ? ts[tap_slot(n0 + j)] : 0.0f;             // step 0: taps[n0 + j]; outputs past the row are not stored
            acc[j] = 0.0f;
        }
        for (uint32_t k = 0; k < full; k += kR) filter_steps<kR>(xs, ts, n0, k, win, acc);
        switch (W - full) {                        // the last W mod 8 steps; the window is in order at every multiple of eight
            case 1: filter_steps<1>(xs, ts, n0, full, win, acc); break;
            case 2: filter_steps<2>(xs, ts, n0, full, win, acc); break;
            case 3: filter_steps<3>(xs, ts, n0, full, win, acc); break;
            case 4: filter_steps<4>(xs, ts, n0, full, win, acc); break;
            case 5: filter_steps<5>(xs, ts, n0, full, win, acc); break;
            case 6: filter_steps<6>(xs, ts, n0, full, win, acc); break;
            case 7: filter_steps<7>(xs, ts, n0, full, win, acc); break;
            default: break;
        }
#pragma unroll
        for (uint32_t j = 0; j < kR; ++j) {
            const uint32_t n = n0 + j;
            if (n < W) out[base + n] = filter_finish(acc[j], has_post, has_post ? post[wbase + n] : 1.0f, has_scale, scale);
        }
    }
}

}  // namespace

}  // namespace naf

using namespace naf;

namespace {

// Both entry points: `col` is NULL for naf_filter_rows; `name` heads the error messages.
int filter_rows_launch(const char *name, const float *in, uint32_t n_views, uint32_t H, uint32_t W, const float *taps, const float *pre,
                       const float *post, const float *view_scale, const float *col, float *out, void *stream) {
    char msg[160];
    if (W == 0 || W > NAF_FILTER_MAX_WIDTH) {
        std::snprintf(msg, sizeof(msg), "%s: row width %u is outside 1 .. %u (the row and its taps are staged in LDS)", name, W,
                      (unsigned)NAF_FILTER_MAX_WIDTH);
        return fail(NAF_ERR_INVALID_ARGUMENT, msg);
    }
    const uint64_t rows = (uint64_t)n_views * H;
    if (rows == 0) return NAF_OK;
    if (!in || !taps || !out) return fail_who(name, "null pointer");
    if (rows > 0x7fffffffull) return fail_who(name, "more than 2^31 - 1 rows in one call");
    const uint32_t lanes = (W + kR - 1u) / kR;
    const uint32_t threads = std::min(kMaxThreads, (lanes + 63u) & ~63u);
    const uint32_t lds = filter_lds_bytes(W);
    int rc = raise_lds_limit(filter_rows_kernel, lds, "filter_rows: could not raise the dynamic LDS limit");
    if (rc != NAF_OK) return rc;
    return launch("filter_rows_kernel", filter_rows_kernel, dim3((uint32_t)rows), dim3(threads), lds, (hipStream_t)stream, in, H, W, taps,
                  pre, post, view_scale, col, out);
}

}  // namespace

extern "C" int naf_filter_rows(const float *in, uint32_t n_views, uint32_t H, uint32_t W, const float *taps, const float *pre,
                               const float *post, const float *view_scale, float *out, void *stream) {
    return filter_rows_launch("filter_rows", in, n_views, H, W, taps, pre, post, view_scale, nullptr, out, stream);
}

extern "C" int naf_filter_rows_views(const float *in, uint32_t n_views, uint32_t H, uint32_t W, const float *taps, const float *pre,
                                     const float *post, const float *view_scale, const float *col, float *out, void *stream) {
    return filter_rows_launch("filter_rows_views", in, n_views, H, W, taps, pre, post, view_scale, col, out, stream);
}
