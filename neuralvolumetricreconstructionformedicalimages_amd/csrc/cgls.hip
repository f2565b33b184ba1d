// cgls.hip -- the vector half of a CGLS iteration on fp32 arrays for gfx950 (naf_cgls_wdot, naf_cgls_residual_step,
// naf_cgls_direction_step): the Krylov baseline reconstruct.cgls.  Defined in include/naf_hip.h (K1) and DESIGN.md section 19;
// the per-element arithmetic is csrc/cgls_device.h.  The projector pair (P1 / P2 / P5) is the other half and is not touched here.
//
//   cgls_wdot_kernel       one fp64 partial of sum w a^2 per workgroup
//   cgls_residual_kernel   the same partial of sum w r^2, then r <- r - alpha q and y <- w r in the same pass
//   cgls_reduce_kernel     one workgroup adds the partials in a fixed order into one scalar (csrc/block_sum.h: two calls return
//                          the same bits) and, after a residual pass, records a breakdown in the sticky stop mark
//   cgls_direction_kernel  x <- x + alpha p, p <- s + beta p: three arrays read, two written
//
// The scalars gamma, delta, the history and the stop mark live in device memory and every kernel reads them there, so a solve is
// one stream of launches with no host read-back.  No scalar race: the scalars are written only by cgls_reduce_kernel, a launch of
// one workgroup that follows the kernels which read them, and gamma rotates by iteration parity (gamma of iteration k sits in slot
// k & 1, the caller has gamma' summed into the other slot), so no launch rewrites a scalar that a workgroup of the same launch
// still reads and nothing has to be copied between iterations.
//
// Summation order.  Element i belongs to group i / 4, group j to thread j % (blocks * 256) of the launch, which adds its groups in
// ascending order and the four terms of a group in ascending order; the grid is a function of n alone.  The float4 path and the
// element path (for pointers that are not 16-byte aligned) therefore add the same terms in the same order.
#include <cmath>

#include "block_sum.h"
#include "naf_host.h"
#include "cgls_device.h"

namespace naf {

namespace {

constexpr uint32_t kThreads = 256;
constexpr uint32_t kMaxBlocks = 2048;              // 8 workgroups per CU; each thread then strides over its groups
constexpr uint32_t kReduceThreads = 256;
constexpr uint32_t kHeader = NAF_CGLS_SCALARS;     // fp64 scalars in front of the history
constexpr uint32_t kSlotDelta = NAF_CGLS_SLOT_DELTA, kSlotStopped = NAF_CGLS_SLOT_STOPPED;

uint64_t groups_of(uint64_t n) { return (n + 3u) / 4u; }

uint32_t blocks_of(uint64_t n) {
    const uint64_t want = (groups_of(n) + kThreads - 1u) / kThreads;
    return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(want, kMaxBlocks));
}

// fp64 values in front of the partials: the header and the history, rounded up so that the partials start on a 256-byte line.
uint64_t scalar_count(uint32_t n_iter_max) { return ((uint64_t)kHeader + n_iter_max + 31u) & ~(uint64_t)31u; }

uint64_t workspace_bytes(uint64_t n, uint32_t n_iter_max) { return (scalar_count(n_iter_max) + blocks_of(n)) * sizeof(double); }

// The four elements of group j, or fewer at the end of the array: `count` of them are valid.
template <bool kVec>
__device__ __forceinline__ void load_group(const float *__restrict__ a, uint64_t j, uint32_t count, float v[4]) {
    if (kVec && count == 4u) {
        const float4 t = reinterpret_cast<const float4 *>(a)[j];
        v[0] = t.x, v[1] = t.y, v[2] = t.z, v[3] = t.w;
    } else {
#pragma unroll
        for (uint32_t e = 0; e < 4u; ++e) v[e] = e < count ? a[4u * j + e] : 0.0f;
    }
}

template <bool kVec>
__device__ __forceinline__ void store_group(float *__restrict__ a, uint64_t j, uint32_t count, const float v[4]) {
    if (kVec && count == 4u) {
        reinterpret_cast<float4 *>(a)[j] = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (uint32_t e = 0; e < 4u; ++e)
            if (e < count) a[4u * j + e] = v[e];
    }
}

__device__ __forceinline__ uint32_t group_count(uint64_t j, uint64_t n) {
    const uint64_t left = n - 4u * j;
    return left < 4u ? (uint32_t)left : 4u;
}

template <bool kVec, bool kHasW>
__global__ void __launch_bounds__(kThreads)
cgls_wdot_kernel(const float *__restrict__ a, const float *__restrict__ w, uint64_t n, double *__restrict__ partials) {
    __shared__ double red[kThreads];
    const uint64_t tid = (uint64_t)blockIdx.x * kThreads + threadIdx.x, stride = (uint64_t)gridDim.x * kThreads;
    const uint64_t groups = (n + 3u) / 4u;
    double sum = 0.0;
    for (uint64_t j = tid; j < groups; j += stride) {
        const uint32_t count = group_count(j, n);
        float av[4], wv[4];
        load_group<kVec>(a, j, count, av);
        if (kHasW) load_group<kVec>(w, j, count, wv);
#pragma unroll
        for (uint32_t e = 0; e < 4u; ++e)
            if (e < count) sum += kHasW ? cgls_term(av[e], wv[e]) : cgls_term(av[e]);
    }
    block_sum<kThreads>(red, sum, threadIdx.x);
    if (threadIdx.x == 0) partials[blockIdx.x] = red[0];
}

template <bool kVec, bool kHasW>
__global__ void __launch_bounds__(kThreads)
cgls_residual_kernel(float *__restrict__ r, const float *__restrict__ q, const float *__restrict__ w, float *__restrict__ y,
                     uint64_t n, const double *__restrict__ scalars, uint32_t parity, double *__restrict__ partials) {
    __shared__ double red[kThreads];
    const double gamma = scalars[parity], delta = scalars[kSlotDelta];
    const bool live = cgls_live(gamma, delta, scalars[kSlotStopped]);
    const float alpha = cgls_alpha(gamma, delta, live);
    const uint64_t tid = (uint64_t)blockIdx.x * kThreads + threadIdx.x, stride = (uint64_t)gridDim.x * kThreads;
    const uint64_t groups = (n + 3u) / 4u;
    double sum = 0.0;
    for (uint64_t j = tid; j < groups; j += stride) {
        const uint32_t count = group_count(j, n);
        float rv[4], qv[4], wv[4], yv[4];
        load_group<kVec>(r, j, count, rv);
        load_group<kVec>(q, j, count, qv);
        if (kHasW) load_group<kVec>(w, j, count, wv);
#pragma unroll
        for (uint32_t e = 0; e < 4u; ++e) {
            if (e < count) sum += kHasW ? cgls_term(rv[e], wv[e]) : cgls_term(rv[e]);          // of the r that came in
            rv[e] = cgls_residual(rv[e], qv[e], alpha, live);
            yv[e] = kHasW ? wv[e] * rv[e] : rv[e];
        }
        store_group<kVec>(r, j, count, rv);
        store_group<kVec>(y, j, count, yv);
    }
    block_sum<kThreads>(red, sum, threadIdx.x);
    if (threadIdx.x == 0) partials[blockIdx.x] = red[0];
}

// scalars[slot] <- the sum of the partials.  With `mark_k` >= 0 (after a residual pass of iteration mark_k) it also sets the stop
// mark to mark_k + 1 if that iteration was a breakdown and no earlier one was; the kernels of that pass have finished by now, and
// the mark is the last thing this one workgroup reads.
__global__ void __launch_bounds__(kReduceThreads)
cgls_reduce_kernel(const double *__restrict__ partials, uint32_t n_partials, double *__restrict__ scalars, uint32_t slot,
                   int64_t mark_k) {
    __shared__ double red[kReduceThreads];
    const uint32_t tid = threadIdx.x;
    block_sum<kReduceThreads>(red, strided_sum<kReduceThreads>(partials, n_partials, tid), tid);
    if (tid == 0) {
        scalars[slot] = red[0];
        if (mark_k >= 0) {
            const double stopped = scalars[kSlotStopped];
            if (!(stopped > 0.0) && !cgls_live(scalars[mark_k & 1], scalars[kSlotDelta], stopped))
                scalars[kSlotStopped] = (double)(mark_k + 1);
        }
    }
}

template <bool kVec>
__global__ void __launch_bounds__(kThreads)
cgls_direction_kernel(float *__restrict__ x, float *__restrict__ p, const float *__restrict__ s, uint64_t n,
                      const double *__restrict__ scalars, uint32_t parity) {
    const double gamma = scalars[parity], gamma_next = scalars[parity ^ 1u], delta = scalars[kSlotDelta];
    const bool live = cgls_live(gamma, delta, scalars[kSlotStopped]);
    if (!live) return;                             // uniform: x and p stay as they are, s is not read
    const float alpha = cgls_alpha(gamma, delta, live), beta = cgls_beta(gamma, gamma_next, live);
    const uint64_t tid = (uint64_t)blockIdx.x * kThreads + threadIdx.x, stride = (uint64_t)gridDim.x * kThreads;
    const uint64_t groups = (n + 3u) / 4u;
    for (uint64_t j = tid; j < groups; j += stride) {
        const uint32_t count = group_count(j, n);
        float xv[4], pv[4], sv[4];
        load_group<kVec>(x, j, count, xv);
        load_group<kVec>(p, j, count, pv);
        load_group<kVec>(s, j, count, sv);
#pragma unroll
        for (uint32_t e = 0; e < 4u; ++e) cgls_direction(xv[e], pv[e], sv[e], alpha, beta, live);
        store_group<kVec>(x, j, count, xv);
        store_group<kVec>(p, j, count, pv);
    }
}

struct Workspace {
    double *scalars, *partials;
    uint32_t blocks;
};

// The checks every entry point shares; splits the workspace.
int cgls_check(const char *who, uint64_t n, uint32_t n_iter_max, void *workspace, size_t bytes, Workspace *ws) {
    if (!workspace) return fail_who(who, "null pointer");
    if (!aligned(workspace, 7u)) return misaligned(who, "workspace", 8);
    const uint64_t need = workspace_bytes(n, n_iter_max);
    if (bytes < need) return workspace_too_small(who, bytes, need);
    ws->scalars = static_cast<double *>(workspace);
    ws->partials = ws->scalars + scalar_count(n_iter_max);
    ws->blocks = blocks_of(n);
    return NAF_OK;
}

int reduce(const Workspace &ws, uint32_t slot, int64_t mark_k, hipStream_t stream) {
    return launch("cgls_reduce_kernel", cgls_reduce_kernel, dim3(1), dim3(kReduceThreads), 0, stream, ws.partials, ws.blocks, ws.scalars,
                  slot, mark_k);
}

template <bool kVec, bool kHasW>
int launch_wdot(const Workspace &ws, const float *a, const float *w, uint64_t n, hipStream_t stream) {
    return launch("cgls_wdot_kernel", cgls_wdot_kernel<kVec, kHasW>, dim3(ws.blocks), dim3(kThreads), 0, stream, a, w, n, ws.partials);
}

template <bool kVec, bool kHasW>
int launch_residual(const Workspace &ws, float *r, const float *q, const float *w, float *y, uint64_t n, uint32_t parity,
                    hipStream_t stream) {
    return launch("cgls_residual_kernel", cgls_residual_kernel<kVec, kHasW>, dim3(ws.blocks), dim3(kThreads), 0, stream, r, q, w, y, n,
                  ws.scalars, parity, ws.partials);
}

}  // namespace

}  // namespace naf

using namespace naf;

extern "C" size_t naf_cgls_workspace_bytes(uint64_t n_max, uint32_t n_iter_max) { return (size_t)workspace_bytes(n_max, n_iter_max); }

extern "C" int naf_cgls_wdot(const float *a, const float *w, uint64_t n, uint32_t slot, uint32_t n_iter_max, void *workspace,
                             size_t workspace_bytes, void *stream) {
    if (n == 0) return NAF_OK;
    if (!a) return fail(NAF_ERR_INVALID_ARGUMENT, "cgls_wdot: null pointer");
    if (slot > kSlotDelta) return fail(NAF_ERR_INVALID_ARGUMENT, "cgls_wdot: slot must be one of the two gamma slots or delta (0, 1, 2)");
    if (!aligned(a, 3u) || !aligned(w, 3u)) return misaligned("cgls_wdot", "pointers", 4);
    Workspace ws;
    const int rc = cgls_check("cgls_wdot", n, n_iter_max, workspace, workspace_bytes, &ws);
    if (rc != NAF_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    const bool vec = aligned(a, 15u) && aligned(w, 15u);
    const int launched = w ? (vec ? launch_wdot<true, true>(ws, a, w, n, s) : launch_wdot<false, true>(ws, a, w, n, s))
                           : (vec ? launch_wdot<true, false>(ws, a, w, n, s) : launch_wdot<false, false>(ws, a, w, n, s));
    if (launched != NAF_OK) return launched;
    return reduce(ws, slot, -1, s);
}

extern "C" int naf_cgls_residual_step(float *r, const float *q, const float *w, float *y, uint64_t n, uint32_t k,
                                      uint32_t n_iter_max, void *workspace, size_t workspace_bytes, void *stream) {
    if (n == 0) return NAF_OK;
    if (!r || !q || !y) return fail(NAF_ERR_INVALID_ARGUMENT, "cgls_residual_step: null pointer");
    if (y == q || y == r || r == q || (w && (w == y || w == r)))
        return fail(NAF_ERR_INVALID_ARGUMENT, "cgls_residual_step: y must not be q or r, and r, q, w, y must be four arrays");
    if (k >= n_iter_max) return fail(NAF_ERR_INVALID_ARGUMENT, "cgls_residual_step: k has no history slot (k >= n_iter_max)");
    if (!aligned(r, 3u) || !aligned(q, 3u) || !aligned(w, 3u) || !aligned(y, 3u)) return misaligned("cgls_residual_step", "pointers", 4);
    Workspace ws;
    const int rc = cgls_check("cgls_residual_step", n, n_iter_max, workspace, workspace_bytes, &ws);
    if (rc != NAF_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    const bool vec = aligned(r, 15u) && aligned(q, 15u) && aligned(w, 15u) && aligned(y, 15u);
    const uint32_t parity = k & 1u;
    const int launched =
        w ? (vec ? launch_residual<true, true>(ws, r, q, w, y, n, parity, s) : launch_residual<false, true>(ws, r, q, w, y, n, parity, s))
          : (vec ? launch_residual<true, false>(ws, r, q, w, y, n, parity, s) : launch_residual<false, false>(ws, r, q, w, y, n, parity, s));
    if (launched != NAF_OK) return launched;
    return reduce(ws, kHeader + k, (int64_t)k, s);
}

extern "C" int naf_cgls_direction_step(float *x, float *p, const float *s, uint64_t n, uint32_t k, uint32_t n_iter_max,
                                       void *workspace, size_t workspace_bytes, void *stream) {
    if (n == 0) return NAF_OK;
    if (!x || !p || !s) return fail(NAF_ERR_INVALID_ARGUMENT, "cgls_direction_step: null pointer");
    if (x == p || x == s || p == s) return fail(NAF_ERR_INVALID_ARGUMENT, "cgls_direction_step: x, p and s must be three arrays");
    if (k >= n_iter_max) return fail(NAF_ERR_INVALID_ARGUMENT, "cgls_direction_step: k is not an iteration of this workspace (k >= n_iter_max)");
    if (!aligned(x, 3u) || !aligned(p, 3u) || !aligned(s, 3u)) return misaligned("cgls_direction_step", "pointers", 4);
    Workspace ws;
    const int rc = cgls_check("cgls_direction_step", n, n_iter_max, workspace, workspace_bytes, &ws);
    if (rc != NAF_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    const uint32_t parity = k & 1u;
    auto kernel = aligned(x, 15u) && aligned(p, 15u) && aligned(s, 15u) ? cgls_direction_kernel<true> : cgls_direction_kernel<false>;
    return launch("cgls_direction_kernel", kernel, dim3(ws.blocks), dim3(kThreads), 0, st, x, p, s, n, ws.scalars, parity);
}
