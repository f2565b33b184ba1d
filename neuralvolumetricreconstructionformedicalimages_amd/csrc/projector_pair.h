// projector_pair.h -- the library's two matched projector pairs as policies, so that every kernel and entry point of projector.hip
// and sart.hip is written once and instantiated per pair:
//   InterpolatedPair  P1 / P2 / P4: trilinear samples at a step (project_device.h, backproject_device.h)
//   SiddonPair        P6 / P7 / P8: exact chord lengths per voxel (siddon_device.h, which includes nothing of HIP)
// A pair says what its kernels take (`Field` to read a volume, `Grid` beside the volumes a transpose adds into), how the host makes
// that from a checked ProjVolume (whose VoxelGrid both pairs read), its forward line integral, its OS-SART residual, its transpose
// walk with the two deposits, and the layout of its forward scan kernel.  The host checks are make_volume's and make_scan_launch's
// for both: the Siddon entry points have no sample step and pass 1.  The Siddon pair has no residual(): its residual kernel is
// written out in sart.hip.  The shapes here (integral takes the two float4, the rest a Ray made in the kernel, Residual is {y, res}) are the
// ones that compile to the hand-written kernels' machine code; check with tools/compare_kernel_asm.py
// before changing them.
#pragma once

#include "backproject_device.h"
#include "scan_launch.h"
#include "siddon_device.h"

namespace naf {

// What the OS-SART residual of one ray gives: y, the weighted residual the transpose takes, and res = b - (A x).
struct Residual {
    float y, res;
};

struct InterpolatedPair {
    using Field = ProjVolume;
    using Grid = ProjVolume;
    using ValueDeposit = DepositValue;
    using PairDeposit = DepositPair;
#ifdef NAF_PROJECT_ROW_STRIP
    static constexpr ScanLayout kForwardLayout = kScanRowStrip;   // the layout A/B of DESIGN.md section 10
#else
    static constexpr ScanLayout kForwardLayout = kScanTiles;
#endif

    struct Ray {
        float4 a, b;                 // (o, d.x) and (d.y, d.z, near, far)
    };

    static Field field(const ProjVolume &v) { return v; }
    static const Grid &grid(const Field &f) { return f; }
    __device__ static __forceinline__ Ray ray(float4 a, float4 b) { return Ray{a, b}; }

    // Midpoint-rule line integral of one ray (o, d, near, far); d is un-normalised.  0 on an empty span, NaN on an unbounded one.
    __device__ static __forceinline__ float integral(const Field &v, float4 a, float4 b) {
        RaySpan s;
        const SpanKind kind = ray_span(v, a, b, s);
        if (kind == kSpanEmpty) return 0.0f;
        if (kind == kSpanUnbounded) return __builtin_nanf("");
        return span_sum(v, s) * s.weight;
    }

    // res = b - (A x) with P1's own sum and product, and y = res / len; NaN for both on an unbounded span.
    __device__ static __forceinline__ Residual residual(const Field &v, const Ray &ray, float measured) {
        const float nan = __builtin_nanf("");
        Residual out{nan, nan};
        RaySpan s;
        const SpanKind kind = ray_span(v, ray.a, ray.b, s);
        if (kind == kSpanEmpty) {
            out.res = measured;
            out.y = 0.0f;
        } else if (kind == kSpanOk) {
            out.res = measured - span_sum(v, s) * s.weight;
            out.y = out.res / s.len;
        }
        return out;
    }

    template <class Deposit>
    __device__ static __forceinline__ void transpose(const Grid &v, const Ray &ray, const Deposit &deposit) {
        scatter_ray(v, ray.a, ray.b, deposit);
    }
};

// P7's deposit: fl(y * len) into one volume; a ray with y == 0 sends nothing, a NaN y is sent.
struct SiddonDepositValue {
    float *__restrict__ volume;
    float y;
    __device__ __forceinline__ bool wanted() const { return y != 0.0f; }
    __device__ __forceinline__ void operator()(uint64_t offset, float len) const {
        atomicAdd(volume + offset, y * len);                  // no-return global_atomic_add_f32
    }
};

// P8's deposit: len into `den` where one is given, then fl(y * len) into `num` when y != 0.  Unlike P7's it does not decline a ray
// with y == 0 while a den is wanted: such a ray still owes its chord lengths to the column sums.
struct SiddonDepositPair {
    float *__restrict__ num;
    float *__restrict__ den;                                  // may be null
    float y;
    __device__ __forceinline__ bool wanted() const { return y != 0.0f || den; }
    __device__ __forceinline__ void operator()(uint64_t offset, float len) const {
        if (den) atomicAdd(den + offset, len);
        if (y != 0.0f) atomicAdd(num + offset, y * len);
    }
};

struct SiddonPair {
    // What a Siddon kernel is handed of a VoxelGrid: the fields its walk reads, side by side, which it fetches from the argument
    // segment with one scalar load less than out of a whole VoxelGrid.  grid() is the VoxelGrid again: imax
    // and next, which no walk reads, come from the one place that defines them and fold away.
    struct Grid {
        uint32_t n[3];
        uint64_t stride[3];
        float half[3], d[3], inv_d[3];

        template <class From, class To>
        __host__ __device__ static __forceinline__ void copy(const From &f, To &t) {
            NAF_UNROLL
            for (int a = 0; a < 3; ++a)
                t.n[a] = f.n[a], t.stride[a] = f.stride[a], t.half[a] = f.half[a], t.d[a] = f.d[a], t.inv_d[a] = f.inv_d[a];
        }
        __host__ __device__ __forceinline__ VoxelGrid grid() const {
            VoxelGrid g;
            copy(*this, g);
            voxel_grid_corners(g);
            return g;
        }
    };
    struct Field {
        Grid grid;
        const float *volume;
    };
    using ValueDeposit = SiddonDepositValue;
    using PairDeposit = SiddonDepositPair;
    static constexpr ScanLayout kForwardLayout = kScanTiles;

    static Field field(const ProjVolume &v) {
        Field f;
        Grid::copy(v.grid, f.grid);
        f.volume = v.data;
        return f;
    }
    using Ray = SiddonRay;

    static const Grid &grid(const Field &f) { return f.grid; }
    // (o, d.x) and (d.y, d.z, near, far), as make_pixel_ray writes them and as a ray list holds them.
    __device__ static __forceinline__ Ray ray(float4 a, float4 b) { return Ray{{a.x, a.y, a.z}, {a.w, b.x, b.y}, b.z, b.w}; }

    // P6's line integral of one ray: 0 on an empty span, NaN on a non-finite one.
    __device__ static __forceinline__ float integral(const Field &f, float4 a, float4 b) {
        const float *volume = f.volume;
        SiddonIntegral sum;
        const SiddonKind kind = siddon_forward(f.grid.grid(), ray(a, b), [volume](uint64_t offset) { return volume[offset]; }, sum);
        if (kind == kSiddonEmpty) return 0.0f;
        if (kind == kSiddonNotFinite) return __builtin_nanf("");
        return sum.acc;
    }

    template <class Deposit>
    __device__ static __forceinline__ void transpose(const Grid &grid, const Ray &ray, const Deposit &deposit) {
        siddon_transpose(grid.grid(), ray, deposit);
    }
};

}  // namespace naf
