// inpaint.hip -- sinogram in-painting for gfx950 (naf_inpaint_rows): the pixels of a metal trace replaced, in every detector row of
// every view, by interpolation between their nearest valid neighbours.  Defined in include/naf_hip.h (A4) and DESIGN.md section 32;
// the bitmap search and the per-pixel arithmetic are csrc/inpaint_device.h.
//
//   inpaint_rows_kernel   a workgroup of 256 lanes owns one detector row of one view.  It walks the row's mask in passes of 256
//                         columns; in every pass each wave ballots "not masked" and one lane stores the 64-bit word, so the row's
//                         validity is a bitmap of at most 256 words (2 KB) in LDS.  Lane w then fills the two word-level tables
//                         (the last and the next word that is not zero), and a second walk over the row gives every masked pixel
//                         its neighbours by count-leading / count-trailing zeros in its own word, or through a table entry in one
//                         other word.  q[L] and q[R] are read from global memory: the row was read a moment ago by this workgroup
//                         or is being read by it, and a span's lanes all read the same two addresses.  The two counts are summed in
//                         LDS and added once per workgroup with one global integer atomic each: integer sums do not depend on their
//                         order, so the counts are the same on every run.
//
// Bounds: the mask, p, prior and out are touched at columns below W only (the ballot's `u < W` comes first).  A pass stores word
// u >> 6 of its wave's first column, and the guard `word < nwords` drops the waves that lie wholly past the row's end; nwords <= 256
// is the size of the three LDS arrays.  The tables are read at w - 1 >= 0 and w + 1 < nwords only, and hold indices below nwords.
// The kernel holds no array of its own, so it uses no scratch; LDS is 2 KB of words, 2 x 1 KB of tables and 8 bytes.
#include <cmath>

#include "naf_host.h"
#include "inpaint_device.h"

namespace naf {

namespace {

constexpr uint32_t kThreads = 256;
constexpr uint32_t kMaxRows = 1u << 24;
constexpr uint64_t kMaxBlocks = 0x7fffffffull;

static_assert(kInpaintMaxW == NAF_INPAINT_MAX_W, "inpaint_device.h and naf_hip.h disagree");
static_assert(kInpaintMaxWords == kThreads, "one lane fills one entry of each table");

// p and out carry no __restrict__: out may be p.  `in_place` skips the stores that would put a pixel's own bits back.
__global__ void __launch_bounds__(kThreads)
inpaint_rows_kernel(const float *p, const uint8_t *__restrict__ mask, const float *__restrict__ prior, float eps, uint32_t H, uint32_t W,
                    float *out, uint32_t *__restrict__ counts, uint32_t in_place) {
    __shared__ uint64_t words[kInpaintMaxWords];
    __shared__ uint32_t last[kInpaintMaxWords], next[kInpaintMaxWords];
    __shared__ uint32_t tally[2];
    const uint32_t tid = threadIdx.x;
    const uint32_t nwords = inpaint_words(W);
    const uint64_t row = (uint64_t)blockIdx.x * W;
    const uint8_t *m = mask + row;
    if (tid < 2u) tally[tid] = 0u;
    for (uint32_t base = 0; base < W; base += kThreads) {              // uniform bounds: every lane of a wave takes the ballot
        const uint32_t u = base + tid;
        const uint64_t ballot = __ballot(u < W && m[u] == 0);
        const uint32_t word = u >> 6;
        if ((tid & 63u) == 0u && word < nwords) words[word] = ballot;
    }
    __syncthreads();
    if (tid < nwords) {
        last[tid] = inpaint_last_word(words, tid);
        next[tid] = inpaint_next_word(words, nwords, tid);
    }
    __syncthreads();
    const float *src = p + row;
    const float *pri = prior != nullptr ? prior + row : nullptr;
    float *dst = out + row;
    uint32_t replaced = 0u, kept = 0u;
    for (uint32_t u = tid; u < W; u += kThreads) {
        const uint32_t before = replaced;
        const float x = inpaint_pixel(src, pri, eps, words, last, next, nwords, u, replaced, kept);
        if (!in_place || replaced != before) dst[u] = x;
    }
    if (counts == nullptr) return;
    if (replaced) atomicAdd(&tally[0], replaced);
    if (kept) atomicAdd(&tally[1], kept);
    __syncthreads();
    if (tid < 2u && tally[tid]) atomicAdd(&counts[2ull * (blockIdx.x / H) + tid], tally[tid]);
}

int refuse(const char *what) { return fail_who("inpaint_rows", what); }

bool overlap(const void *a, uint64_t a_bytes, const void *b, uint64_t b_bytes) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + b_bytes && b0 < a0 + a_bytes;
}

}  // namespace

}  // namespace naf

using namespace naf;

extern "C" int naf_inpaint_rows(const float *p, const uint8_t *mask, const float *prior, float eps, uint32_t N, uint32_t H, uint32_t W,
                                float *out, uint32_t *counts, void *stream) {
    if (N == 0 || H == 0 || W == 0) return NAF_OK;
    if (!p || !mask || !out) return refuse("null pointer");
    if (W > kInpaintMaxW) return refuse("more than 16384 detector columns");
    if (H > kMaxRows) return refuse("more than 2^24 detector rows");
    if ((uint64_t)N * H > kMaxBlocks) return refuse("more than 2^31 - 1 detector rows over all views");
    if (!aligned(p, 3u) || !aligned(prior, 3u) || !aligned(out, 3u) || !aligned(counts, 3u))
        return misaligned("inpaint_rows", "p, prior, out and counts", 4u);
    const uint64_t all = (uint64_t)N * H * W;                               // below 2^45 elements
    if (out != p && overlap(out, all * 4u, p, all * 4u)) return refuse("out must be p itself or not overlap it");
    if (overlap(out, all * 4u, mask, all) || (prior && overlap(out, all * 4u, prior, all * 4u)))
        return refuse("out must not overlap mask or prior");
    if (prior && (!std::isfinite(eps) || !(eps > 0.0f))) return refuse("eps must be finite and above zero");
    return launch("inpaint_rows_kernel", inpaint_rows_kernel, dim3((uint32_t)((uint64_t)N * H)), dim3(kThreads), 0, (hipStream_t)stream, p,
                  mask, prior, eps, H, W, out, counts, out == p ? 1u : 0u);
}
