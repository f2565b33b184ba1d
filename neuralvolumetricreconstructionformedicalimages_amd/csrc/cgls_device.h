// cgls_device.h -- the per-element arithmetic of the CGLS vector kernels (include/naf_hip.h K1): the fp64
// term of a weighted sum of squares, the step lengths alpha and beta from the fp64 scalars, and the two fused updates.  It includes
// nothing of HIP, so a host compiler reads it too: tools/cgls_host_check.cpp runs these very functions on the CPU under
// AddressSanitizer / UBSan and compares them with float64.  The library and the host check are built with -ffp-contract=off, so
// every fused multiply-add here is asked for by name; everything else is a single IEEE operation in the order written.
#pragma once

#include <cmath>

#include "host_device.h"

namespace naf {

// One term of sum_i w_i a_i^2 in fp64: (double)a * (double)a is exact (24-bit significands), the product with w rounds once.
NAF_HD double cgls_term(float a) { return (double)a * (double)a; }
NAF_HD double cgls_term(float a, float w) { return (double)w * ((double)a * (double)a); }

// Whether iteration k takes a step: not stopped earlier, and both gamma = ||s||^2 and delta = ||q||_W^2 are > 0.  The compares are
// written so that a NaN in either scalar stops the iteration instead of reaching a division.
NAF_HD bool cgls_live(double gamma, double delta, double stopped_plus_1) {
    return !(stopped_plus_1 > 0.0) && gamma > 0.0 && delta > 0.0;
}

// alpha = gamma / delta and beta = gamma_next / gamma, each divided in fp64 and rounded to fp32 once; 0 when the iteration is not live.
NAF_HD float cgls_alpha(double gamma, double delta, bool live) { return live ? (float)(gamma / delta) : 0.0f; }
NAF_HD float cgls_beta(double gamma, double gamma_next, bool live) { return live ? (float)(gamma_next / gamma) : 0.0f; }

// r <- r - alpha q as one fma; a stopped iteration returns r itself, whatever q holds (a non-finite q included).
NAF_HD float cgls_residual(float r, float q, float alpha, bool live) { return live ? fmaf(-alpha, q, r) : r; }

// x <- x + alpha p and p <- s + beta p, one fma each; a stopped iteration leaves both as they are, whatever s holds.
NAF_HD void cgls_direction(float &x, float &p, float s, float alpha, float beta, bool live) {
    if (!live) return;
    x = fmaf(alpha, p, x);
    p = fmaf(beta, p, s);
}

}  // namespace naf
