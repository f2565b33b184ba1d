// filter_device.h -- the per-output arithmetic of the detector-row filter (include/naf_hip.h P3).
// It includes nothing of HIP, so a host compiler reads it too: tools/filter_host_check.cpp runs these very functions on the CPU
// under AddressSanitizer / UBSan and compares them with the float64 convolution of the tests.  Every operation is a single IEEE
// fp32 multiply or fused multiply-add in the order written; the fma is asked for by name, since the library and the host check are
// built with -ffp-contract=off and the compiler forms none on its own.
#pragma once

#include <cstdint>

#include "host_device.h"

namespace naf {

// x[k] = pre[r, k] * in[i, r, k]: the value the sum reads (staged once per row by the kernel).  naf_filter_rows_views applies it a
// second time, x[k] = col[i, k] * (pre[r, k] * in[i, r, k]): one more multiply, after pre's.
NAF_HD float filter_weigh(float v, float w) { return w * v; }

// The staged value with every factor that is present, in the kernel's order: pre, then col.
NAF_HD float filter_stage(float v, bool has_pre, float pre, bool has_col, float col) {
    if (has_pre) v = filter_weigh(v, pre);
    if (has_col) v = filter_weigh(v, col);
    return v;
}

// The tap that output n applies to input k: taps[|n - k|].
NAF_HD uint32_t filter_tap_index(uint32_t n, uint32_t k) { return n >= k ? n - k : k - n; }

// One link of the chain: acc <- fma(tap, x, acc).
NAF_HD float filter_step(float acc, float tap, float x) { return __builtin_fmaf(tap, x, acc); }

// out = view_scale * (post * acc); an absent factor is skipped, not replaced by 1.
NAF_HD float filter_finish(float acc, bool has_post, float post, bool has_scale, float scale) {
    float v = acc;
    if (has_post) v = post * v;
    if (has_scale) v = scale * v;
    return v;
}

// sum_{k = 0 .. W - 1} taps[|n - k|] * x[k] as the kernel forms it: from +0, one fma per k, k ascending.  The kernel walks eight
// outputs per lane through this very chain with the taps in a register window; this loop is the same sequence for one output.
NAF_HD float filter_output(const float *taps, const float *x, uint32_t W, uint32_t n) {
    float acc = 0.0f;
    for (uint32_t k = 0; k < W; ++k) acc = filter_step(acc, taps[filter_tap_index(n, k)], x[k]);
    return acc;
}

}  // namespace naf
