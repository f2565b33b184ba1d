// stripe.hip -- sinogram stripe removal by sorting for gfx950 (naf_stripe_remove_sorting; Vo, Atwood and Drakopoulos 2018, algorithm
// 3).  Defined in include/naf_hip.h (A2) and DESIGN.md section 27; the integer arithmetic is csrc/stripe_device.h.
//
//   stripe_sort_kernel     a workgroup owns C adjacent columns of one detector row.  It loads their N values (for a view the C floats
//                          are one segment of 4 C bytes), packs (key << 32 | view) into 64-bit LDS words laid out [view][column],
//                          pads the views to Npad = 2^k with all-ones words and runs the bitonic network over all C columns at once:
//                          a step is C Npad / 2 independent compare-exchanges, dealt to the 256 lanes column-fastest, and one
//                          barrier.  Rank j of column c is then word [j][c]; the float goes to s and the view to perm, both
//                          [row][j][u], so the second kernel reads rows of u.  C = 16 while 16 Npad words fit 64 KiB (N <= 512), else
//                          8192 / Npad (8, 4, 2 for N to 1024, 2048, 4096): the workgroup never holds more than 64 KiB, so two share
//                          a CU's 160 KiB.  With [view][column] the 32 lanes of an LDS access group read 32 consecutive words at
//                          every stride of at least 32 / C (C = 16: all but the last of a stage); at a shorter stride they read
//                          runs that span twice as many words, a 2-way bank conflict and never more.
//   stripe_median_kernel   a workgroup owns a run of 256 u of one (row, rank).  It stages the run and its h-wide reflected halo as keys
//                          in LDS; lane t selects the key of rank h among words t .. t + 2 h by counting (stripe_select: consecutive
//                          lanes read consecutive words) and stores its float to out[perm]: a scatter along views to distinct
//                          addresses.
//
// No atomics, no float comparison, no arithmetic on the data: the result is bit-defined.  Neither kernel has an array of its own, so
// neither uses scratch.
#include <cstdio>

#include "naf_host.h"
#include "stripe_device.h"

namespace naf {

namespace {

constexpr uint32_t kThreads = 256;
constexpr uint32_t kSortMaxWords = 8192;                // 64 KiB of 64-bit words per workgroup
constexpr uint32_t kSortMaxColumns = 16;                // a view's segment is 64 bytes
constexpr uint32_t kRun = 256;                          // columns per workgroup of the median kernel
constexpr uint32_t kMaxExtent = 1u << 24;
constexpr uint64_t kMaxBlocks = 0x7fffffffull;

static_assert(kStripeMaxSize == NAF_STRIPE_MAX_SIZE && kStripeMaxViews == NAF_STRIPE_MAX_VIEWS, "stripe_device.h and naf_hip.h disagree");
static_assert(kSortMaxWords >= 2u * kStripeMaxViews, "the largest N still sorts two columns per workgroup");

struct SortPlan {
    uint32_t N, H, W;
    uint32_t Npad, C;                  // both powers of two, C Npad <= kSortMaxWords
    uint32_t tiles;                    // ceil(W / C)
};

__global__ void __launch_bounds__(kThreads)
stripe_sort_kernel(const uint32_t *__restrict__ p, SortPlan g, uint32_t v0, uint32_t *__restrict__ s, uint16_t *__restrict__ perm) {
    extern __shared__ uint64_t words[];                                  // [Npad][C]
    const uint32_t tid = threadIdx.x, C = g.C, cmask = C - 1u, cshift = __ffs(C) - 1u;
    const uint32_t row = blockIdx.x / g.tiles, u0 = (blockIdx.x % g.tiles) * C;
    const uint32_t v = v0 + row;
    const uint32_t real = g.N * C, all = g.Npad * C;
    for (uint32_t e = tid; e < all; e += kThreads) {
        const uint32_t i = e >> cshift, u = u0 + (e & cmask);
        uint64_t word = kStripePad;
        if (e < real && u < g.W) word = stripe_pack(stripe_key(p[((uint64_t)i * g.H + v) * g.W + u]), i);
        words[e] = word;
    }
    __syncthreads();
    const uint32_t pairs = all >> 1;
    for (uint32_t stage = 2u; stage <= g.Npad; stage <<= 1) {
        for (uint32_t stride = stage >> 1; stride > 0u; stride >>= 1) {
            for (uint32_t e = tid; e < pairs; e += kThreads) {
                const uint32_t low = stripe_bitonic_low(e >> cshift, stride);
                const uint32_t a = (low << cshift) | (e & cmask), b = a + (stride << cshift);
                const uint64_t wa = words[a], wb = words[b];
                if (stripe_bitonic_swaps(wa, wb, stripe_bitonic_ascending(low, stage))) words[a] = wb, words[b] = wa;
            }
            __syncthreads();
        }
    }
    const uint64_t base = (uint64_t)row * g.N * g.W;
    for (uint32_t e = tid; e < real; e += kThreads) {
        const uint32_t j = e >> cshift, u = u0 + (e & cmask);
        if (u >= g.W) continue;
        const uint64_t word = words[e], at = base + (uint64_t)j * g.W + u;
        s[at] = stripe_unkey(stripe_word_key(word));
        perm[at] = (uint16_t)stripe_word_view(word);
    }
}

__global__ void __launch_bounds__(kThreads)
stripe_median_kernel(const uint32_t *__restrict__ s, const uint16_t *__restrict__ perm, uint32_t N, uint32_t H, uint32_t W, uint32_t h,
                     uint32_t v0, uint32_t tiles, uint32_t *__restrict__ out) {
    __shared__ uint32_t keys[kRun + kStripeMaxSize - 1u];
    const uint32_t tid = threadIdx.x;
    const uint32_t line = blockIdx.x / tiles, u0 = (blockIdx.x % tiles) * kRun;          // line = row * N + j
    const uint32_t run = min(kRun, W - u0);
    const uint64_t base = (uint64_t)line * W;
    for (uint32_t e = tid; e < run + 2u * h; e += kThreads)
        keys[e] = stripe_key(s[base + stripe_reflect((int32_t)(u0 + e) - (int32_t)h, W)]);
    __syncthreads();
    if (tid >= run) return;
    const uint32_t u = u0 + tid, v = v0 + line / N;
    const uint32_t median = stripe_select(keys + tid, h);
    out[((uint64_t)perm[base + u] * H + v) * W + u] = stripe_unkey(median);
}

const char *shape_error(uint32_t N, uint32_t H, uint32_t W) {
    if (N > kStripeMaxViews) return "more than 4096 views";
    if (H > kMaxExtent || W > kMaxExtent) return "view dimension above 2^24";
    return nullptr;
}

uint64_t round8(uint64_t bytes) { return (bytes + 7u) & ~7ull; }

// s then perm for `rows` rows of N W elements each.
uint64_t workspace_bytes(uint32_t N, uint32_t W, uint64_t rows) {
    const uint64_t elements = rows * N * W;
    return round8(elements * sizeof(float)) + round8(elements * sizeof(uint16_t));
}

}  // namespace

}  // namespace naf

using namespace naf;

extern "C" size_t naf_stripe_workspace_bytes(uint32_t N, uint32_t H, uint32_t W, uint32_t rows) {
    if (N == 0 || H == 0 || W == 0 || rows == 0 || rows > H || shape_error(N, H, W)) return 0;
    return (size_t)workspace_bytes(N, W, rows);
}

extern "C" int naf_stripe_remove_sorting(const float *p, uint32_t N, uint32_t H, uint32_t W, uint32_t size, void *ws, size_t ws_bytes,
                                         float *out, void *stream) {
    const char *who = "stripe_remove_sorting";
    if (N == 0 || H == 0 || W == 0) return NAF_OK;
    if (!p || !out || !ws) return fail_who(who, "null pointer");
    if (const char *err = shape_error(N, H, W)) return fail_who(who, err);
    if (size < 3u || size > kStripeMaxSize || size % 2u == 0u) return fail_who(who, "size must be odd and in [3, 63]");
    if (size > W) return fail_who(who, "size above the number of detector columns");
    if (!aligned(p, 3u) || !aligned(out, 3u)) return misaligned(who, "projections", 4);
    if (!aligned(ws, 7u)) return misaligned(who, "workspace", 8);
    const uint64_t one_row = workspace_bytes(N, W, 1);
    if (ws_bytes < one_row) {
        char msg[160];
        std::snprintf(msg, sizeof(msg), "workspace too small (%llu bytes, one detector row needs %llu)", (unsigned long long)ws_bytes,
                      (unsigned long long)one_row);
        return fail_who(who, msg);
    }
    SortPlan g;
    g.N = N, g.H = H, g.W = W;
    g.Npad = stripe_pad_count(N);
    g.C = std::min(kSortMaxColumns, kSortMaxWords / g.Npad);
    g.tiles = (W + g.C - 1u) / g.C;
    const uint32_t h = size / 2u, run_tiles = (W + kRun - 1u) / kRun;
    const uint32_t lds = g.C * g.Npad * (uint32_t)sizeof(uint64_t);
    // the rows of a group: what the workspace holds (s and perm each rounded up once, so rows * one_row is an upper bound of the
    // group's bytes), and no more than either launch can index with 2^31 - 1 workgroups
    uint64_t group = std::min<uint64_t>(H, ws_bytes / one_row);
    group = std::min(group, kMaxBlocks / g.tiles);
    group = std::min(group, kMaxBlocks / ((uint64_t)N * run_tiles));
    hipStream_t st = (hipStream_t)stream;
    const uint32_t *bits = reinterpret_cast<const uint32_t *>(p);
    uint32_t *out_bits = reinterpret_cast<uint32_t *>(out);
    for (uint32_t v0 = 0; v0 < H; v0 += (uint32_t)group) {
        const uint32_t rows = (uint32_t)std::min<uint64_t>(group, H - v0);
        uint32_t *s = static_cast<uint32_t *>(ws);
        uint16_t *perm = reinterpret_cast<uint16_t *>(static_cast<char *>(ws) + round8((uint64_t)rows * N * W * sizeof(float)));
        const int sorted = launch("stripe_sort_kernel", stripe_sort_kernel, dim3(rows * g.tiles), dim3(kThreads), lds, st, bits, g, v0, s,
                                  perm);
        if (sorted != NAF_OK) return sorted;
        const int done = launch("stripe_median_kernel", stripe_median_kernel, dim3(rows * N * run_tiles), dim3(kThreads), 0, st, s, perm,
                                N, H, W, h, v0, run_tiles, out_bits);
        if (done != NAF_OK) return done;
    }
    return NAF_OK;
}
