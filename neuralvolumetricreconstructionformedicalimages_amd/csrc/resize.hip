// resize.hip -- cubic B-spline resampling of an fp32 volume for gfx950 (naf_resize_volume): the resize step of the reference's
// `loadImage` (dataGenerator/generateData.py:111-150), scipy.ndimage.zoom(order=3, prefilter=False), defined in include/naf_hip.h
// (V1) and DESIGN.md section 12.
//
// Layout: a prologue kernel writes, per axis and output index, the first tap (floor(x) - 1, not yet mirrored) and the four fp32
// weights, formed in fp64.  A 256-lane workgroup owns a kT0 x kT1 x kT2 = 4 x 4 x 64 tile of output voxels.
//   tiled form   stages the tile's input footprint (first tap of its first output .. last tap of its last output, per axis) in
//                LDS with the mirrored indices resolved and the affine applied, then runs the three 4-tap passes inside the tile
//                (axis 0, axis 1, axis 2: 12 multiply-adds per voxel); a wave stores 64 consecutive voxels of axis 2 at a time.
//   direct form  gathers the 64 taps of every output voxel from global memory; for shapes whose footprint does not fit the LDS
//                budget (strong down-sampling).
// The choice is a pure function of the two shapes (resize_plan): tiled while the footprint fits and stays below four staged
// inputs per output voxel.  No full-size intermediate exists.  Every workgroup writes the
// minimum and maximum of its tile to the workspace and a one-workgroup kernel folds them in a fixed order (no atomics).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "naf_host.h"

namespace naf {

namespace {

constexpr uint32_t kT0 = 4, kT1 = 4, kT2 = 64;     // output voxels per workgroup along axes 0, 1, 2
constexpr uint32_t kThreads = 256, kWaves = kThreads / 64, kPairs = kT0 * kT1;
constexpr uint32_t kLdsBudget = 65536 - 256;       // dynamic LDS of the tiled form (the default limit less the static part)
constexpr uint32_t kStagedPerOutput = 4;           // the tiled form is chosen up to this many staged inputs per output voxel
constexpr uint32_t kFoldThreads = 1024;

struct ResizePlan {
    uint32_t tiles[3];      // workgroup tiles per axis
    uint32_t fmax[3];       // upper bound of a tile's input footprint per axis
    uint64_t blocks, total; // total = b1 + b2 + b3 table entries
    uint32_t lds_bytes;     // dynamic LDS of the tiled form
    bool fits;              // the tiled form's footprint fits the LDS budget
    bool tiled;             // the form the call takes: a pure function of the two shapes
    uint64_t w_off, base_off, partial_off, bytes;   // workspace layout
};

// r of the definition: (a - 1) / (b - 1) in IEEE double, 1 for a single output.
__host__ __device__ inline double axis_ratio(uint32_t a, uint32_t b) { return b > 1 ? (double)(a - 1) / (double)(b - 1) : 1.0; }

ResizePlan resize_plan(const uint32_t *a, const uint32_t *b) {
    ResizePlan p;
    const uint32_t t[3] = {kT0, kT1, kT2};
    p.blocks = 1;
    p.total = 0;
    uint64_t outputs = 1;
    for (int k = 0; k < 3; ++k) {
        p.tiles[k] = (b[k] + t[k] - 1) / t[k];
        p.blocks *= p.tiles[k];
        p.total += b[k];
        // first taps of the tile's first and last output differ by floor(x1) - floor(x0) < (x1 - x0) + 1, and x1 - x0 is
        // (n - 1) r up to two roundings of products below 2^32 (< 2^-20): at most floor((n - 1) r) + 1; the last output adds 4 taps.
        const uint32_t n = std::min(t[k], b[k]);
        outputs *= n;
        const double span = std::floor((double)(n - 1) * axis_ratio(a[k], b[k]));
        p.fmax[k] = (uint32_t)std::min(span, 1e9) + 1u + 1u + 4u;      // + 1 more: slack for the roundings named above
    }
    const uint64_t floats = (uint64_t)p.fmax[1] * p.fmax[2] * ((uint64_t)p.fmax[0] + kT0);
    p.fits = floats * 4u <= kLdsBudget;
    p.lds_bytes = p.fits ? (uint32_t)(floats * 4u) : 0u;
    // Staging pays per footprint element, the direct form per output: measured on an MI355X the tiled form is 2.1x faster at 1.3
    // staged inputs per output (2x up-sampling) and 1.6x slower at 11 (2x down-sampling); DESIGN.md section 12.
    p.tiled = p.fits && (uint64_t)p.fmax[0] * p.fmax[1] * p.fmax[2] <= kStagedPerOutput * outputs;
    auto up = [](uint64_t v) { return (v + 255u) & ~(uint64_t)255u; };
    p.w_off = 0;
    p.base_off = up(p.total * 16u);
    p.partial_off = p.base_off + up(p.total * 4u);
    p.bytes = p.partial_off + up(p.blocks * 8u);
    return p;
}

// Whole-sample symmetric mirror of tap index i on an axis of a samples (a == 1: every tap is sample 0).
__device__ __forceinline__ uint32_t mirror(int64_t i, uint32_t a) {
    if ((uint64_t)i < (uint64_t)a) return (uint32_t)i;
    if (a == 1) return 0;
    const int64_t p = 2 * ((int64_t)a - 1);
    int64_t m = i % p;
    if (m < 0) m += p;
    return (uint32_t)(m >= (int64_t)a ? p - m : m);
}

struct Dims3 {
    uint32_t v[3];
};

// one thread per (axis, output index): first tap and weights of the definition, in fp64, rounded to fp32 once
__global__ void __launch_bounds__(256)
resize_tables_kernel(Dims3 a, Dims3 b, float4 *__restrict__ w, int32_t *__restrict__ base) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    const uint64_t total = (uint64_t)b.v[0] + b.v[1] + b.v[2];
    if (i >= total) return;
    uint32_t k = 0, j = (uint32_t)i;
    if (i >= b.v[0]) { k = 1; j = (uint32_t)(i - b.v[0]); }
    if (i >= (uint64_t)b.v[0] + b.v[1]) { k = 2; j = (uint32_t)(i - b.v[0] - b.v[1]); }
    const double x = (double)j * axis_ratio(a.v[k], b.v[k]);
    const double f = floor(x), t = x - f, u = 1.0 - t;
    const double t2 = t * t, t3 = t2 * t;
    w[i] = make_float4((float)(u * u * u / 6.0), (float)((3.0 * t3 - 6.0 * t2 + 4.0) / 6.0),
                       (float)((-3.0 * t3 + 3.0 * t2 + 3.0 * t + 1.0) / 6.0), (float)(t3 / 6.0));
    base[i] = (int32_t)f - 1;
}

struct Tile {
    uint32_t j0[3], n[3];   // first output and output count per axis
};

__device__ __forceinline__ Tile tile_of(uint32_t block, const Dims3 &b, uint32_t tiles1, uint32_t tiles2) {
    Tile t;
    const uint32_t tz = block % tiles2, rest = block / tiles2;
    t.j0[0] = (rest / tiles1) * kT0;
    t.j0[1] = (rest % tiles1) * kT1;
    t.j0[2] = tz * kT2;
    t.n[0] = min(kT0, b.v[0] - t.j0[0]);
    t.n[1] = min(kT1, b.v[1] - t.j0[1]);
    t.n[2] = min(kT2, b.v[2] - t.j0[2]);
    return t;
}

// minimum / maximum of the workgroup's outputs -> partials[block]; a NaN output makes both NaN.  Fixed order: two calls, same bits.
__device__ __forceinline__ void tile_minmax(float lo, float hi, bool nan, float2 *__restrict__ partials) {
    __shared__ float wlo[kWaves], whi[kWaves];
    __shared__ int wnan[kWaves];
    int bad = nan ? 1 : 0;
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        lo = fminf(lo, __shfl_xor(lo, d, 64));
        hi = fmaxf(hi, __shfl_xor(hi, d, 64));
        bad |= __shfl_xor(bad, d, 64);
    }
    const uint32_t wave = threadIdx.x / 64u;
    if ((threadIdx.x & 63u) == 0) {
        wlo[wave] = lo;
        whi[wave] = hi;
        wnan[wave] = bad;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (uint32_t k = 1; k < kWaves; ++k) {
            lo = fminf(lo, wlo[k]);
            hi = fmaxf(hi, whi[k]);
            bad |= wnan[k];
        }
        const float q = __builtin_nanf("");
        partials[blockIdx.x] = bad ? make_float2(q, q) : make_float2(lo, hi);
    }
}

__global__ void __launch_bounds__(kThreads)
resize_tiled_kernel(const float *__restrict__ in, Dims3 a, float scale, float shift, float *__restrict__ out, Dims3 b,
                    const float4 *__restrict__ w, const int32_t *__restrict__ base, uint32_t tiles1, uint32_t tiles2,
                    float2 *__restrict__ partials) {
    extern __shared__ __align__(16) float lds[];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid / 64u;
    const Tile t = tile_of(blockIdx.x, b, tiles1, tiles2);
    const uint32_t o1 = b.v[0], o2 = b.v[0] + b.v[1];                  // table offsets of axes 1 and 2
    const int32_t lo0 = base[t.j0[0]], lo1 = base[o1 + t.j0[1]], lo2 = base[o2 + t.j0[2]];
    const uint32_t F0 = (uint32_t)(base[t.j0[0] + t.n[0] - 1] + 4 - lo0);
    const uint32_t F1 = (uint32_t)(base[o1 + t.j0[1] + t.n[1] - 1] + 4 - lo1);
    const uint32_t F2 = (uint32_t)(base[o2 + t.j0[2] + t.n[2] - 1] + 4 - lo2);
    const uint32_t F12 = F1 * F2;
    float *S = lds;                        // [F0][F1][F2] staged inputs
    float *A = lds + F0 * F12;             // [n0][F1][F2] after the axis-0 pass
    float *B = lds;                        // [n0][n1][F2] after the axis-1 pass (S is dead by then; F0 >= 4 > n1 rows per t0)

    // stage: a wave takes rows (e0, e1) in turn, its lanes run along axis 2 (coalesced where nothing is mirrored)
    {
        const uint64_t s1 = a.v[2], s0 = (uint64_t)a.v[1] * a.v[2];
        const uint32_t rows = F0 * F1;
        for (uint32_t e2 = lane; e2 < F2; e2 += 64u) {
            const uint32_t i2 = mirror((int64_t)lo2 + e2, a.v[2]);
            uint32_t e0 = wave / F1, e1 = wave % F1;
            for (uint32_t row = wave; row < rows; row += kWaves) {
                const uint64_t off = mirror((int64_t)lo0 + e0, a.v[0]) * s0 + mirror((int64_t)lo1 + e1, a.v[1]) * s1 + i2;
                S[row * F2 + e2] = fmaf(in[off], scale, shift);
                e1 += kWaves;
                while (e1 >= F1) {
                    e1 -= F1;
                    ++e0;
                }
            }
        }
    }
    __syncthreads();
    // axis 0: A[t0][e1][e2] = sum_k w0[t0][k] S[first tap of t0 + k][e1][e2]
    for (uint32_t t0 = 0; t0 < t.n[0]; ++t0) {
        const float4 c = w[t.j0[0] + t0];
        const float *s = S + (uint32_t)(base[t.j0[0] + t0] - lo0) * F12;
        for (uint32_t e = tid; e < F12; e += kThreads) {
            float v = c.x * s[e];
            v = fmaf(c.y, s[e + F12], v);
            v = fmaf(c.z, s[e + 2u * F12], v);
            v = fmaf(c.w, s[e + 3u * F12], v);
            A[t0 * F12 + e] = v;
        }
    }
    __syncthreads();
    // axis 1: B[t0][t1][e2]; a wave takes the (t0, t1) pairs wave, wave + 4, ... here and in the axis-2 pass
    for (uint32_t p = wave; p < kPairs; p += kWaves) {
        const uint32_t t0 = p / kT1, t1 = p % kT1;
        if (t0 >= t.n[0] || t1 >= t.n[1]) continue;
        const float4 c = w[o1 + t.j0[1] + t1];
        const float *s = A + t0 * F12 + (uint32_t)(base[o1 + t.j0[1] + t1] - lo1) * F2;
        for (uint32_t e2 = lane; e2 < F2; e2 += 64u) {
            float v = c.x * s[e2];
            v = fmaf(c.y, s[e2 + F2], v);
            v = fmaf(c.z, s[e2 + 2u * F2], v);
            v = fmaf(c.w, s[e2 + 3u * F2], v);
            B[p * F2 + e2] = v;
        }
    }
    __syncthreads();
    // axis 2: one lane per output of axis 2, 64 consecutive voxels per store
    float lo = INFINITY, hi = -INFINITY;
    bool nan = false;
    if (lane < t.n[2]) {
        const float4 c = w[o2 + t.j0[2] + lane];
        const uint32_t off2 = (uint32_t)(base[o2 + t.j0[2] + lane] - lo2);
        for (uint32_t p = wave; p < kPairs; p += kWaves) {
            const uint32_t t0 = p / kT1, t1 = p % kT1;
            if (t0 >= t.n[0] || t1 >= t.n[1]) continue;
            const float *s = B + p * F2 + off2;
            float v = c.x * s[0];
            v = fmaf(c.y, s[1], v);
            v = fmaf(c.z, s[2], v);
            v = fmaf(c.w, s[3], v);
            out[((uint64_t)(t.j0[0] + t0) * b.v[1] + (t.j0[1] + t1)) * b.v[2] + (t.j0[2] + lane)] = v;   // 64-bit: 1024^3 is 4 GiB
            lo = fminf(lo, v);
            hi = fmaxf(hi, v);
            nan |= v != v;
        }
    }
    if (partials) tile_minmax(lo, hi, nan, partials);
}

__global__ void __launch_bounds__(kThreads)
resize_direct_kernel(const float *__restrict__ in, Dims3 a, float scale, float shift, float *__restrict__ out, Dims3 b,
                     const float4 *__restrict__ w, const int32_t *__restrict__ base, uint32_t tiles1, uint32_t tiles2,
                     float2 *__restrict__ partials) {
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid / 64u;
    const Tile t = tile_of(blockIdx.x, b, tiles1, tiles2);
    const uint32_t o1 = b.v[0], o2 = b.v[0] + b.v[1];
    const uint64_t s1 = a.v[2], s0 = (uint64_t)a.v[1] * a.v[2];
    float lo = INFINITY, hi = -INFINITY;
    bool nan = false;
    if (lane < t.n[2]) {
        const uint32_t j2 = t.j0[2] + lane;
        const float4 c2 = w[o2 + j2];
        const int32_t f2 = base[o2 + j2];
        uint32_t i2[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) i2[k] = mirror((int64_t)f2 + k, a.v[2]);
        for (uint32_t p = wave; p < kPairs; p += kWaves) {
            const uint32_t t0 = p / kT1, t1 = p % kT1;
            if (t0 >= t.n[0] || t1 >= t.n[1]) continue;
            const uint32_t j0 = t.j0[0] + t0, j1 = t.j0[1] + t1;
            const float4 c0 = w[j0], c1 = w[o1 + j1];
            const float w0[4] = {c0.x, c0.y, c0.z, c0.w}, w1[4] = {c1.x, c1.y, c1.z, c1.w};
            const int32_t f0 = base[j0], f1 = base[o1 + j1];
            float v = 0.0f;
#pragma unroll
            for (int k0 = 0; k0 < 4; ++k0) {
                const uint64_t r0 = mirror((int64_t)f0 + k0, a.v[0]) * s0;
                float plane = 0.0f;
#pragma unroll
                for (int k1 = 0; k1 < 4; ++k1) {
                    const float *row = in + (r0 + mirror((int64_t)f1 + k1, a.v[1]) * s1);
                    float r = c2.x * fmaf(row[i2[0]], scale, shift);
                    r = fmaf(c2.y, fmaf(row[i2[1]], scale, shift), r);
                    r = fmaf(c2.z, fmaf(row[i2[2]], scale, shift), r);
                    r = fmaf(c2.w, fmaf(row[i2[3]], scale, shift), r);
                    plane = k1 == 0 ? w1[0] * r : fmaf(w1[k1], r, plane);
                }
                v = k0 == 0 ? w0[0] * plane : fmaf(w0[k0], plane, v);
            }
            out[((uint64_t)j0 * b.v[1] + j1) * b.v[2] + j2] = v;
            lo = fminf(lo, v);
            hi = fmaxf(hi, v);
            nan |= v != v;
        }
    }
    if (partials) tile_minmax(lo, hi, nan, partials);
}

// one workgroup folds the per-tile pairs in a fixed order
__global__ void __launch_bounds__(kFoldThreads)
resize_minmax_kernel(const float2 *__restrict__ partials, uint64_t n, float *__restrict__ minmax) {
    __shared__ float slo[kFoldThreads], shi[kFoldThreads];
    __shared__ int snan[kFoldThreads];
    const uint32_t tid = threadIdx.x;
    float lo = INFINITY, hi = -INFINITY;
    int bad = 0;
    for (uint64_t i = tid; i < n; i += kFoldThreads) {
        const float2 p = partials[i];
        bad |= p.x != p.x;
        lo = fminf(lo, p.x);
        hi = fmaxf(hi, p.y);
    }
    slo[tid] = lo;
    shi[tid] = hi;
    snan[tid] = bad;
    __syncthreads();
    for (uint32_t h = kFoldThreads / 2; h > 0; h >>= 1) {
        if (tid < h) {
            slo[tid] = fminf(slo[tid], slo[tid + h]);
            shi[tid] = fmaxf(shi[tid], shi[tid + h]);
            snan[tid] |= snan[tid + h];
        }
        __syncthreads();
    }
    if (tid == 0) {
        const float q = __builtin_nanf("");
        minmax[0] = snan[0] ? q : slo[0];
        minmax[1] = snan[0] ? q : shi[0];
    }
}

// Diagnostics / tests: NAF_RESIZE_FORM=tiled|direct in the environment forces a form (read per call; the library keeps no mode).
int forced_form() {
    const char *e = std::getenv("NAF_RESIZE_FORM");
    if (!e || !*e) return 0;
    if (!std::strcmp(e, "tiled")) return 1;
    if (!std::strcmp(e, "direct")) return 2;
    return -1;
}

}  // namespace

}  // namespace naf

using namespace naf;

extern "C" size_t naf_resize_volume_workspace_bytes(const uint32_t *in_dims, const uint32_t *out_dims) {
    if (!in_dims || !out_dims) return 0;
    for (int k = 0; k < 3; ++k)
        if (in_dims[k] == 0 || out_dims[k] == 0) return 0;
    return (size_t)resize_plan(in_dims, out_dims).bytes;
}

extern "C" int naf_resize_volume(const float *in, const uint32_t *in_dims, float scale, float shift, float *out,
                                 const uint32_t *out_dims, float *minmax, void *workspace, size_t workspace_bytes, void *stream) {
    if (!in || !in_dims || !out || !out_dims || !workspace) return fail(NAF_ERR_INVALID_ARGUMENT, "resize_volume: null pointer");
    char msg[200];
    for (int k = 0; k < 3; ++k)
        if (in_dims[k] == 0 || out_dims[k] == 0) {
            std::snprintf(msg, sizeof(msg), "resize_volume: zero extent (input %u x %u x %u, output %u x %u x %u)", in_dims[0],
                          in_dims[1], in_dims[2], out_dims[0], out_dims[1], out_dims[2]);
            return fail(NAF_ERR_UNSUPPORTED, msg);
        }
    for (int k = 0; k < 3; ++k)
        if (in_dims[k] > 0x40000000u || out_dims[k] > 0x40000000u)
            return fail(NAF_ERR_INVALID_ARGUMENT, "resize_volume: an extent above 2^30 is not supported");
    const ResizePlan p = resize_plan(in_dims, out_dims);
    if (p.blocks > 0x7fffffffull) return fail(NAF_ERR_INVALID_ARGUMENT, "resize_volume: volume too large for one call");
    if (workspace_bytes < p.bytes) return workspace_too_small("resize_volume", workspace_bytes, p.bytes);
    if (!aligned(workspace, 15u)) return misaligned("resize_volume", "workspace", 16);
    const int forced = forced_form();
    if (forced < 0) return fail(NAF_ERR_INVALID_ARGUMENT, "resize_volume: NAF_RESIZE_FORM must be tiled or direct");
    if (forced == 1 && !p.fits) return fail(NAF_ERR_UNSUPPORTED, "resize_volume: the tiled form does not fit the LDS budget at these shapes");
    const bool tiled = forced ? forced == 1 : p.tiled;

    char *ws = static_cast<char *>(workspace);
    float4 *w = reinterpret_cast<float4 *>(ws + p.w_off);
    int32_t *base = reinterpret_cast<int32_t *>(ws + p.base_off);
    float2 *partials = minmax ? reinterpret_cast<float2 *>(ws + p.partial_off) : nullptr;
    const Dims3 a = {{in_dims[0], in_dims[1], in_dims[2]}}, b = {{out_dims[0], out_dims[1], out_dims[2]}};
    hipStream_t s = (hipStream_t)stream;
    int rc = launch("resize_tables_kernel", resize_tables_kernel, dim3((uint32_t)((p.total + 255u) / 256u)), dim3(256), 0, s, a, b, w,
                    base);
    if (rc != NAF_OK) return rc;
    rc = tiled ? launch("resize_tiled_kernel", resize_tiled_kernel, dim3((uint32_t)p.blocks), dim3(kThreads), p.lds_bytes, s, in, a, scale,
                        shift, out, b, w, base, p.tiles[1], p.tiles[2], partials)
               : launch("resize_direct_kernel", resize_direct_kernel, dim3((uint32_t)p.blocks), dim3(kThreads), 0, s, in, a, scale, shift, out,
                        b, w, base, p.tiles[1], p.tiles[2], partials);
    if (rc != NAF_OK || !minmax) return rc;
    return launch("resize_minmax_kernel", resize_minmax_kernel, dim3(1), dim3(kFoldThreads), 0, s, partials, p.blocks, minmax);
}
