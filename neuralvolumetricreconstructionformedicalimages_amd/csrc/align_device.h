// align_device.h -- the per-view arithmetic of reprojection alignment (include/naf_hip.h A1): one term of a
// shift score, the peak of a score table, and the cubic-convolution resampler of a view.  It includes nothing of HIP, so a host
// compiler reads it too: tools/align_host_check.cpp runs these very functions on the CPU under AddressSanitizer / UBSan over heap
// views of exactly H W floats.  Every operation is a single IEEE operation in the order written (the library and the host check are
// built with -ffp-contract=off); every fused multiply-add is asked for by name.
//
// Conventions.  Views are [N, H, W] fp32, u along the last axis, v along the rows.  A view's shift is (du, dv) in pixels and the
// measured view b is the ideal view p translated by +shift: b(r, c) ~ p(r - dv, c - du).
//
// Score term: d = b - p (one fp32 subtraction), then ((double)d * (double)d) * (double)w: the square is exact in fp64, the product
// with w rounds once.  Without weights the term is the square alone, which has the bits of the product with 1.
//
// Peak of S[2Rv+1, 2Ru+1] (fp64): the argmin in row-major order, ties to the lowest index; per axis a with R_a > 0, the minimum off
// that axis' border and den = S- - 2 S0 + S+ > 0 (formed as (S- - S0) + (S+ - S0)): delta = 1/2 (S- - S+) / den in fp64, clamped
// to [-1/2, 1/2]; otherwise delta = 0.  shift_a = fp32((double)(index_a - R_a) + delta).  Flag bit 0: the minimum lies on the
// border of an axis with R_a > 0; bit 1: some score is not finite, and then the shift is (0, 0) and bit 0 is not set.
//
// Resampler: out(r, c) = b(r + dv, c + du), Keys' cubic convolution (a = -1/2), clamp-to-edge.  Per axis, with extent n and shift s:
//   s' = min(max(s, -(n + 1)), n + 1)       on the float, before any conversion: fmaxf / fminf return the other operand for a NaN,
//                                           so a NaN becomes -(n + 1) and +-inf the nearer bound; beyond |s| = n + 1 every tap of
//                                           every pixel is the edge pixel, so the clamp changes no value
//   i  = (int)floorf(s'),  t = s' - floorf(s')   one subtraction, in [0, 1]; a NaN s gives t = NaN instead: it never chose an index
//   taps k = 0 .. 3 at index clamp(x + i + k - 1, 0, n - 1) of output coordinate x, in integers
//   u  = 1 - t
//   w0 = (-1/2 t) (u u)                     K(1 + t)
//   w1 = u fma(t, fma(-3/2, t, 1), 1)       K(t)     = (1 - t)(1 + t - 3/2 t^2)
//   w2 = t fma(u, fma(-3/2, u, 1), 1)       K(1 - t) = t (1 + u - 3/2 u^2)
//   w3 = (-1/2 u) (t t)                     K(2 - t)
// so K(0) = 1 and K(1) = K(2) = 0 hold exactly: t = 0 gives (0, 1, 0, 0) and t = 1 gives (0, 0, 1, 0).  The four taps are combined
// as fma(w3, v3, fma(w2, v2, fma(w1, v1, w0 v0))), except that t = 0 returns v1 itself (no product with 0 is formed: the bits of
// the source, its signed zeros and infinities included, and a NaN neighbour is not picked up).  Rows first (the four taps along u
// in each of the four tap rows), then the four row results along v.  The shift is uniform over a view, and so are i, t and the
// weights of both axes.
#pragma once

#include <cmath>
#include <cstdint>

#include "host_device.h"

namespace naf {

constexpr uint32_t kAlignMaxShift = 16;              // NAF_ALIGN_MAX_SHIFT
constexpr int kAlignFlagBorder = 1, kAlignFlagNonFinite = 2;

// ---- score ---------------------------------------------------------------------------------------------------------------------------
NAF_HD double align_term(float b, float p) {
    const float d = b - p;
    return (double)d * (double)d;
}

NAF_HD double align_term(float b, float p, float w) { return align_term(b, p) * (double)w; }

// ---- peak ----------------------------------------------------------------------------------------------------------------------------
NAF_HD bool align_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }          // false for a NaN and for +-inf

// The better of two candidates (value, row-major index): the smaller value, on a tie the lower index.  Values are finite here.
NAF_HD bool align_better(double va, uint32_t ia, double vb, uint32_t ib) { return va < vb || (va == vb && ia < ib); }

// Parabola through (-1, sm), (0, s0), (1, sp) with s0 the smallest: the vertex' offset, clamped to [-1/2, 1/2]; 0 if not convex.
NAF_HD double align_vertex(double sm, double s0, double sp) {
    const double den = (sm - s0) + (sp - s0);
    if (!(den > 0.0)) return 0.0;
    const double delta = 0.5 * (sm - sp) / den;
    return fmin(fmax(delta, -0.5), 0.5);
}

// Shift and flags of a table whose scores are all finite, given its argmin `at` (row-major).
NAF_HD void align_refine(const double *S, uint32_t Rv, uint32_t Ru, uint32_t at, float shift[2], int *flags) {
    const uint32_t nu = 2u * Ru + 1u, nv = 2u * Rv + 1u;
    const uint32_t j = at / nu, i = at % nu;
    const bool edge_u = Ru > 0u && (i == 0u || i == nu - 1u), edge_v = Rv > 0u && (j == 0u || j == nv - 1u);
    double du = (double)i - (double)Ru, dv = (double)j - (double)Rv;
    if (Ru > 0u && !edge_u) du += align_vertex(S[at - 1u], S[at], S[at + 1u]);
    if (Rv > 0u && !edge_v) dv += align_vertex(S[at - nu], S[at], S[at + nu]);
    shift[0] = (float)du;
    shift[1] = (float)dv;
    *flags = (edge_u || edge_v) ? kAlignFlagBorder : 0;
}

// The whole peak of one table, serially: what the kernel's parallel argmin must equal.
NAF_HD void align_peak(const double *S, uint32_t Rv, uint32_t Ru, float shift[2], int *flags) {
    const uint32_t count = (2u * Rv + 1u) * (2u * Ru + 1u);
    uint32_t at = 0;
    bool finite = true;
    for (uint32_t s = 0; s < count; ++s) {
        const double v = S[s];
        if (!align_finite(v)) finite = false;
        else if (v < S[at]) at = s;                                        // a strict < keeps the lowest index
    }
    if (!finite) {
        shift[0] = 0.0f;
        shift[1] = 0.0f;
        *flags = kAlignFlagNonFinite;
        return;
    }
    align_refine(S, Rv, Ru, at, shift, flags);
}

// ---- resampler -----------------------------------------------------------------------------------------------------------------------
struct AlignAxis {
    int32_t i;                         // floor of the clamped shift, in [-(n + 1), n + 1]
    float t;                           // its fraction in [0, 1], or NaN
    float w[4];                        // Keys weights of taps i - 1 .. i + 2
};

// One axis of a view's shift; n is the extent (1 .. 2^24).
NAF_HD AlignAxis align_axis(float s, uint32_t n) {
    const float bound = (float)(n + 1u);
    const float c = fminf(fmaxf(s, -bound), bound);                       // a NaN leaves fmaxf as -bound
    const float f = floorf(c);
    AlignAxis a;
    a.i = (int32_t)f;                                                      // |f| <= 2^24 + 1: defined
    const float t = s != s ? s : c - f;                                    // the NaN is handed on; it never chose an index
    const float u = 1.0f - t;
    a.t = t;
    a.w[0] = (-0.5f * t) * (u * u);
    a.w[1] = u * fmaf(t, fmaf(-1.5f, t, 1.0f), 1.0f);
    a.w[2] = t * fmaf(u, fmaf(-1.5f, u, 1.0f), 1.0f);
    a.w[3] = (-0.5f * u) * (t * t);
    return a;
}

// Index of tap k of output coordinate x: clamp(x + i + k - 1, 0, n - 1), all in int64 (no wrap whatever the extents).
NAF_HD uint32_t align_tap(uint32_t x, const AlignAxis &a, int k, uint32_t n) {
    const int64_t at = (int64_t)x + (int64_t)a.i + (int64_t)k - 1;
    return at < 0 ? 0u : (at > (int64_t)n - 1 ? n - 1u : (uint32_t)at);
}

NAF_HD float align_blend(const float v[4], const AlignAxis &a) {
    if (a.t == 0.0f) return v[1];
    return fmaf(a.w[3], v[3], fmaf(a.w[2], v[2], fmaf(a.w[1], v[1], a.w[0] * v[0])));
}

// out(r, c) of one view `b` [H, W] under the axes of its shift: the sixteen taps are loaded before the first is used.
NAF_HD float align_sample(const float *b, uint32_t H, uint32_t W, uint32_t r, uint32_t c, const AlignAxis &av, const AlignAxis &au) {
    float v[4][4];
    uint32_t col[4];
    NAF_UNROLL
    for (int k = 0; k < 4; ++k) col[k] = align_tap(c, au, k, W);
    NAF_UNROLL
    for (int m = 0; m < 4; ++m) {
        const float *row = b + (uint64_t)align_tap(r, av, m, H) * W;
        NAF_UNROLL
        for (int k = 0; k < 4; ++k) v[m][k] = row[col[k]];
    }
    float rows[4];
    NAF_UNROLL
    for (int m = 0; m < 4; ++m) rows[m] = align_blend(v[m], au);
    return align_blend(rows, av);
}

}  // namespace naf
