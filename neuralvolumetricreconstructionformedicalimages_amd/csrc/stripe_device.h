// stripe_device.h -- the integer arithmetic of sinogram stripe removal by sorting (include/naf_hip.h A2): the
// order-preserving key of a float's bits, the reflected column index, the partner and direction of a compare-exchange of the bitonic
// network, and the selection of a window's median.  Read by hipcc for csrc/stripe.hip and by a plain host compiler for
// tools/stripe_host_check.cpp.  Nothing here compares or computes with floats: a float is its 32 bits throughout.
#pragma once

#include <cstdint>

#include "host_device.h"

namespace naf {

constexpr uint32_t kStripeMaxSize = 63u, kStripeMaxViews = 4096u;
constexpr uint64_t kStripePad = ~0ull;                  // sorts after every packed word: a real word's low half is below 4096

// key(x): sign bit set -> all bits inverted, otherwise the sign bit set.  Ascending keys are ascending floats, -0 before +0, the
// NaNs with the sign bit set before -Inf and the others after +Inf, each group in the order of its payload.
NAF_HD uint32_t stripe_key(uint32_t bits) { return (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u); }
NAF_HD uint32_t stripe_unkey(uint32_t key) { return (key & 0x80000000u) ? (key & 0x7fffffffu) : ~key; }

// The word the network sorts: the key above the view index, so that equal keys stay in view order.
NAF_HD uint64_t stripe_pack(uint32_t key, uint32_t view) { return ((uint64_t)key << 32) | view; }
NAF_HD uint32_t stripe_word_key(uint64_t word) { return (uint32_t)(word >> 32); }
NAF_HD uint32_t stripe_word_view(uint64_t word) { return (uint32_t)word; }

// The smallest power of two >= n, n in 1 .. 4096.
NAF_HD uint32_t stripe_pad_count(uint32_t n) {
    uint32_t m = 1u;
    while (m < n) m <<= 1;
    return m;
}

// r(index) for index in [-W, 2 W - 1]: reflection with the edge sample repeated (-1 -> 0, -2 -> 1, W -> W - 1).
NAF_HD uint32_t stripe_reflect(int32_t index, uint32_t W) {
    if (index < 0) return (uint32_t)(-index - 1);
    if ((uint32_t)index >= W) return 2u * W - 1u - (uint32_t)index;
    return (uint32_t)index;
}

// The bitonic network over n = 2^k words: for stage = 2, 4, .. n and stride = stage / 2, stage / 4, .. 1, the n / 2 compare-exchanges
// q = 0 .. n / 2 - 1 of a step touch disjoint pairs (low, low | stride); the pair ends ascending where (low & stage) == 0.
NAF_HD uint32_t stripe_bitonic_low(uint32_t q, uint32_t stride) { return ((q & ~(stride - 1u)) << 1) | (q & (stride - 1u)); }
NAF_HD bool stripe_bitonic_ascending(uint32_t low, uint32_t stage) { return (low & stage) == 0u; }
// Whether the words at low and low | stride change places.
NAF_HD bool stripe_bitonic_swaps(uint64_t at_low, uint64_t at_high, bool ascending) { return ascending ? at_low > at_high : at_low < at_high; }

// The key of rank h among the 2 h + 1 keys window[0 .. 2 h], by counting: a key is the answer when fewer than h + 1 keys are below
// it and at least h + 1 are below or equal to it.  Exactly the keys equal to the median satisfy both, so whichever the loop meets
// first it returns the same bits.  O(size^2) reads of `window` and no array of its own.
template <typename Ptr>
NAF_HD uint32_t stripe_select(Ptr window, uint32_t h) {
    const uint32_t size = 2u * h + 1u;
    for (uint32_t a = 0; a < size; ++a) {
        const uint32_t x = window[a];
        uint32_t below = 0u, equal = 0u;
        for (uint32_t b = 0; b < size; ++b) {
            const uint32_t y = window[b];
            below += y < x ? 1u : 0u;
            equal += y == x ? 1u : 0u;
        }
        if (below <= h && h < below + equal) return x;
    }
    return window[h];                                   // never reached: the median always satisfies the test
}

}  // namespace naf
