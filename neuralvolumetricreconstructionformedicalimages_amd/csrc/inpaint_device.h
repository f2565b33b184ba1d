// inpaint_device.h -- the bitmap search and the per-pixel arithmetic of sinogram in-painting (include/naf_hip.h A4, DESIGN.md section
// 32): the nearest valid columns left and right of a masked pixel in its detector row, and the value interpolated between them.
// Read by hipcc for csrc/inpaint.hip and by a plain host compiler for tools/inpaint_host_check.cpp.  Every float operation is one IEEE
// fp32 operation in the order written (the library and the host check are built with -ffp-contract=off).
//
// A row's validity is a bitmap: bit (u & 63) of words[u >> 6] is set iff column u is not masked; the bits from W on are clear.  Beside
// it go two tables of one entry per word: last[w], the largest index <= w of a word that is not zero, and next[w], the smallest
// index >= w of one, or kInpaintNone.  A search looks in the pixel's own word first and crosses words through a table, so it reads
// at most two words and one table entry whatever the length of the span.
#pragma once

#include <cmath>
#include <cstdint>

#include "host_device.h"

namespace naf {

constexpr uint32_t kInpaintMaxW = 16384u;                           // NAF_INPAINT_MAX_W
constexpr uint32_t kInpaintMaxWords = kInpaintMaxW / 64u;
constexpr uint32_t kInpaintNone = 0xffffffffu;

NAF_HD uint32_t inpaint_words(uint32_t W) { return (W + 63u) / 64u; }
NAF_HD uint32_t inpaint_high_bit(uint64_t x) { return 63u - (uint32_t)__builtin_clzll(x); }             // x != 0
NAF_HD uint32_t inpaint_low_bit(uint64_t x) { return (uint32_t)__builtin_ctzll(x); }                    // x != 0

// The entries of the two tables for word w: a walk over the words, at most `nwords` of them when the row is all masked.
template <typename Words>
NAF_HD uint32_t inpaint_last_word(Words words, uint32_t w) {
    for (uint32_t j = w + 1u; j-- > 0u;)
        if (words[j] != 0ull) return j;
    return kInpaintNone;
}

template <typename Words>
NAF_HD uint32_t inpaint_next_word(Words words, uint32_t nwords, uint32_t w) {
    for (uint32_t j = w; j < nwords; ++j)
        if (words[j] != 0ull) return j;
    return kInpaintNone;
}

// L: the largest valid column below u, or kInpaintNone.
template <typename Words, typename Table>
NAF_HD uint32_t inpaint_left(Words words, Table last, uint32_t u) {
    const uint32_t w = u >> 6, b = u & 63u;
    const uint64_t below = words[w] & ((1ull << b) - 1ull);
    if (below != 0ull) return (w << 6) + inpaint_high_bit(below);
    if (w == 0u) return kInpaintNone;
    const uint32_t j = last[w - 1u];
    return j == kInpaintNone ? kInpaintNone : (j << 6) + inpaint_high_bit(words[j]);
}

// R: the smallest valid column above u, or kInpaintNone.
template <typename Words, typename Table>
NAF_HD uint32_t inpaint_right(Words words, Table next, uint32_t nwords, uint32_t u) {
    const uint32_t w = u >> 6, b = u & 63u;
    const uint64_t above = b == 63u ? 0ull : words[w] & (~0ull << (b + 1u));
    if (above != 0ull) return (w << 6) + inpaint_low_bit(above);
    if (w + 1u >= nwords) return kInpaintNone;
    const uint32_t j = next[w + 1u];
    return j == kInpaintNone ? kInpaintNone : (j << 6) + inpaint_low_bit(words[j]);
}

// g[u] and q[u] of column u: `prior` is the row of the prior sinogram or null, and then g = 1 and q = p.
NAF_HD float inpaint_gain(const float *prior, float eps, uint32_t u) { return prior != nullptr ? fmaxf(prior[u], eps) : 1.0f; }
NAF_HD float inpaint_q(const float *p, const float *prior, float eps, uint32_t u) {
    return prior != nullptr ? p[u] / fmaxf(prior[u], eps) : p[u];
}

// The output of column u of the row `p` (W floats; `prior` likewise or null).  A valid pixel and a masked pixel of a row with no
// valid pixel return p[u] itself.  `replaced` and `kept` count the masked pixels of the two kinds.  Reads p and prior at u and at
// valid columns only, which is what makes out == p safe.
template <typename Words, typename Table>
NAF_HD float inpaint_pixel(const float *p, const float *prior, float eps, Words words, Table last, Table next, uint32_t nwords, uint32_t u,
                           uint32_t &replaced, uint32_t &kept) {
    if ((words[u >> 6] >> (u & 63u)) & 1ull) return p[u];
    const uint32_t L = inpaint_left(words, last, u), R = inpaint_right(words, next, nwords, u);
    if (L == kInpaintNone && R == kInpaintNone) {
        kept += 1u;
        return p[u];
    }
    replaced += 1u;
    float val;
    if (R == kInpaintNone) {
        val = inpaint_q(p, prior, eps, L);
    } else if (L == kInpaintNone) {
        val = inpaint_q(p, prior, eps, R);
    } else {
        const float qL = inpaint_q(p, prior, eps, L), qR = inpaint_q(p, prior, eps, R);
        const float w = (float)(u - L) / (float)(R - L);
        const float d = qR - qL;
        val = qL + w * d;
    }
    return prior != nullptr ? val * inpaint_gain(prior, eps, u) : val;
}

}  // namespace naf
