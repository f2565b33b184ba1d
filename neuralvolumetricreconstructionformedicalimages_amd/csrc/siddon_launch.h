// siddon_launch.h -- what siddon.hip, siddon_backproject.hip and siddon_sart.hip share around the walks of siddon_device.h (which
// includes nothing of HIP): a ray from its two float4, the two deposits of the transpose walk, and the host checks of an entry
// point that has no sample step.
#pragma once

#include "scan_launch.h"
#include "siddon_device.h"

namespace naf {

// (o, d.x) and (d.y, d.z, near, far), as make_pixel_ray writes them and as a ray list holds them.
__device__ __forceinline__ SiddonRay siddon_ray(float4 a, float4 b) { return SiddonRay{{a.x, a.y, a.z}, {a.w, b.x, b.y}, b.z, b.w}; }

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

// Host: P1's argument checks of a volume (there is no sample step here: any valid one passes them) and its grid.
inline int make_siddon_grid(const char *who, const float *volume, uint32_t n1, uint32_t n2, uint32_t n3, const float *dvoxel,
                            SiddonGrid *grid) {
    ProjVolume checked;
    const int rc = make_volume(who, volume, n1, n2, n3, dvoxel, 1.0f, &checked);
    if (rc == NAF_OK) siddon_grid(n1, n2, n3, dvoxel, grid);
    return rc;
}

// Host: make_scan_launch for a scan call that has no sample step, and the grid of its volume.
inline int make_siddon_scan_launch(const char *who, const float *volume, std::initializer_list<const void *> others,
                                   const uint32_t *dims, const float *dvoxel, const float *poses, uint32_t n_sub,
                                   const naf_detector *det, ScanLaunch *s, SiddonGrid *grid, const uint32_t *view_index = nullptr,
                                   uint32_t n_scan_views = 0xffffffffu) {
    const int rc = make_scan_launch(who, volume, others, dims, dvoxel, poses, n_sub, det, 1.0f, s, kScanTiles, view_index, n_scan_views);
    if (rc == NAF_OK) siddon_grid(dims[0], dims[1], dims[2], dvoxel, grid);
    return rc;
}

}  // namespace naf
