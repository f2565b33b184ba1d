// frames_device.h -- the per-pixel arithmetic of raw-frame conditioning (include/naf_hip.h A3): the
// transmission and bad test of one pixel, the lower median among the valid keys of a window, the replace decision and the log tail.
// Read by hipcc for csrc/frames.hip and by a plain host compiler for tools/frames_host_check.cpp.  Every float operation is one IEEE
// fp32 operation in the order written (the library and the host check are built with -ffp-contract=off).
//
// A window holds one uint32 per pixel: stripe_key of the transmission's bits, or kFramesBadKey for a bad pixel.  That word is the
// validity mask.  A pixel that is not bad has a finite transmission, and kFramesBadKey is the key of the NaN 0x7fffffff, so no valid
// entry has it; it is the largest key, so it is never below or equal to a valid one and the counting below skips it unasked.
#pragma once

#include <cmath>
#include <cstdint>

#include "host_device.h"
#include "stripe_device.h"

namespace naf {

constexpr uint32_t kFramesMinSize = 3u, kFramesMaxSize = 7u;
constexpr uint32_t kFramesLog = 1u, kFramesClampNonneg = 2u;        // NAF_FRAMES_LOG, NAF_FRAMES_CLAMP_NONNEG
constexpr uint32_t kFramesBadKey = 0xffffffffu;
constexpr uint32_t kFramesOneBits = 0x3f800000u;                    // 1.0f, the transmission of a window with no valid pixel

NAF_HD uint32_t frames_bits(float x) { return __builtin_bit_cast(uint32_t, x); }
NAF_HD float frames_float(uint32_t bits) { return __builtin_bit_cast(float, bits); }

// A raw sample as fp32; every uint16 is an fp32 exactly.
NAF_HD float frames_load(const float *raw, uint64_t at) { return raw[at]; }
NAF_HD float frames_load(const uint16_t *raw, uint64_t at) { return (float)raw[at]; }

// The window word of one pixel: t = (raw - dark) / (flat - dark); bad iff marked, or the denominator is not above zero (a NaN
// included), or t is not finite.
NAF_HD uint32_t frames_transmission(float raw, float dark, float flat, bool marked) {
    const float den = flat - dark;
    const float num = raw - dark;
    const float t = num / den;
    const bool bad = marked || !(den > 0.0f) || (t - t) != 0.0f;
    return bad ? kFramesBadKey : stripe_key(frames_bits(t));
}

// The smallest word of the kSize x kSize window whose first entry is window[0] and whose rows are `stride` words apart.
template <uint32_t kSize, typename Ptr>
NAF_HD uint32_t frames_window_min(Ptr window, uint32_t stride) {
    uint32_t lowest = kFramesBadKey;
    NAF_UNROLL
    for (uint32_t a = 0; a < kSize; ++a) {
        NAF_UNROLL
        for (uint32_t b = 0; b < kSize; ++b) {
            const uint32_t y = window[a * stride + b];
            lowest = y < lowest ? y : lowest;
        }
    }
    return lowest;
}

// The bits of the lower median of the window's valid entries: with c of them, the one of rank (c - 1) / 2, found by counting as
// stripe_select does (fewer than rank + 1 entries below it, at least rank + 1 below or equal).  Equal keys are equal bits, so
// whichever candidate the loop meets first it returns the same.  c == 0 gives 1.0f.  O(kSize^4) reads and no array of its own.
template <uint32_t kSize, typename Ptr>
NAF_HD uint32_t frames_select(Ptr window, uint32_t stride) {
    uint32_t valid = 0u;
    NAF_UNROLL
    for (uint32_t a = 0; a < kSize; ++a) {
        NAF_UNROLL
        for (uint32_t b = 0; b < kSize; ++b) valid += window[a * stride + b] != kFramesBadKey ? 1u : 0u;
    }
    if (valid == 0u) return kFramesOneBits;
    const uint32_t rank = (valid - 1u) / 2u;
    for (uint32_t i = 0; i < kSize; ++i) {
        for (uint32_t j = 0; j < kSize; ++j) {
            const uint32_t x = window[i * stride + j];
            if (x == kFramesBadKey) continue;
            uint32_t below = 0u, equal = 0u;
            NAF_UNROLL
            for (uint32_t a = 0; a < kSize; ++a) {
                NAF_UNROLL
                for (uint32_t b = 0; b < kSize; ++b) {
                    const uint32_t y = window[a * stride + b];
                    below += y < x ? 1u : 0u;
                    equal += y == x ? 1u : 0u;
                }
            }
            if (below <= rank && rank < below + equal) return stripe_unkey(x);
        }
    }
    return kFramesOneBits;                              // never reached: the median always satisfies the test
}

// The repaired transmission t' of the pixel in the middle of the window, and which of the two replacements it took.  A bad pixel
// takes the median m.  Any other keeps t unless (t - m) > dif.  The selection is skipped where t - min(valid window) <= dif: the
// pixel itself is valid, so m >= min, and a correctly rounded subtraction is monotone, so (t - m) <= (t - min) <= dif and the
// answer is "keep" with the same bits.
template <uint32_t kSize, typename Ptr>
NAF_HD float frames_decide(Ptr window, uint32_t stride, float dif, uint32_t &outliers, uint32_t &bads) {
    const uint32_t centre = window[(kSize / 2u) * stride + kSize / 2u];
    if (centre == kFramesBadKey) {
        bads += 1u;
        return frames_float(frames_select<kSize>(window, stride));
    }
    const float t = frames_float(stripe_unkey(centre));
    const float lowest = frames_float(stripe_unkey(frames_window_min<kSize>(window, stride)));
    if (!((t - lowest) > dif)) return t;
    const float m = frames_float(frames_select<kSize>(window, stride));
    if ((t - m) > dif) {
        outliers += 1u;
        return m;
    }
    return t;
}

// out = t' or, with kFramesLog, -logf(max(t', t_min)); with kFramesClampNonneg on top the result is no less than zero.  t' is never
// a NaN.  The clamp is fmaxf(p, 0) with the zero's sign pinned: -logf(1) is -0, and the clamp returns +0 for it.
NAF_HD float frames_tail(float t, float t_min, uint32_t flags) {
    if (!(flags & kFramesLog)) return t;
    const float p = -logf(fmaxf(t, t_min));
    if (flags & kFramesClampNonneg) return p > 0.0f ? p : 0.0f;
    return p;
}

}  // namespace naf
