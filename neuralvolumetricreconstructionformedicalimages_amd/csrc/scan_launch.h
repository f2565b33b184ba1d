// scan_launch.h -- what the scan entry points (naf_project_scan, naf_backproject_scan, naf_sart_residual_scan,
// naf_sart_backproject_scan, naf_backproject_scan_gather and the _siddon ones) share: the host checks of "a scan is ..." with the
// launch grid, the view list, and the decode of a workgroup into a detector pixel; and, for the four
// ray-list entry points, the host checks of "a list of rays is ...".
//
// Layout of the tile kernels: one lane per detector pixel, 16 x 16 pixels per workgroup, 8 x 8 per wave, so that the samples of
// neighbouring rays at equal k land in the same or neighbouring cache lines; blockIdx.x = launch view * tiles_per_view + tile.  The
// gather launches over voxels and takes only the checks and the RayGeo from here.
#pragma once

#include <initializer_list>

#include "draw_device.h"
#include "project_device.h"

namespace naf {

struct ViewList {
    const uint32_t *__restrict__ index;   // device u32 [n_sub], or null: the identity
    uint32_t n_scan_views;
};

// Scan view of launch view j, or n_scan_views (no such view: it adds nothing) when the list holds an index outside the scan.
__device__ __forceinline__ uint32_t scan_view(const ViewList &l, uint32_t j) {
    const uint32_t view = l.index ? l.index[j] : j;
    return view < l.n_scan_views ? view : l.n_scan_views;
}

enum ScanLayout {
    kScanTiles,      // 16 x 16 pixels per workgroup
    kScanRowStrip,   // 256 consecutive pixels of one detector row per workgroup (the interpolated forward's A/B)
    kScanVoxels,     // no pixel grid: the launch is over the volume
};
constexpr uint32_t kScanStrip = 256;

struct ScanLaunch {
    ProjVolume v;
    RayGeo g;
    uint32_t tiles_x, tiles_per_view;   // the grid is tiles_per_view * n_sub workgroups of 256
};

// Host: the checks of a scan call and what its launch needs.  `volume` is any of the call's volume pointers and `others` its
// further device pointers, all checked for null.  Without a view list, launch view j is scan view j.
inline int make_scan_launch(const char *who, const float *volume, std::initializer_list<const void *> others, const uint32_t *dims,
                            const float *dvoxel, const float *poses, uint32_t n_sub, const naf_detector *det, float step, ScanLaunch *s,
                            ScanLayout layout = kScanTiles, const uint32_t *view_index = nullptr, uint32_t n_scan_views = 0xffffffffu) {
    if (!dims) return fail_who(who, "null pointer");
    const int rc = make_volume(who, volume, dims[0], dims[1], dims[2], dvoxel, step, &s->v);
    if (rc != NAF_OK) return rc;
    bool null = !poses || !det;
    for (const void *p : others) null |= !p;
    const char *what = null ? "null pointer" : detector_refusal(*det, n_sub, /*marched=*/true);
    uint32_t tx = 0;
    uint64_t tiles = 0;
    if (!what) {
        const uint32_t tile_w = layout == kScanRowStrip ? kScanStrip : kProjTile, tile_h = layout == kScanRowStrip ? 1u : kProjTile;
        tx = (det->det_w + tile_w - 1u) / tile_w;
        tiles = layout == kScanVoxels ? 0u : (uint64_t)tx * ((det->det_h + tile_h - 1u) / tile_h);
        if (!view_index && n_sub > n_scan_views) what = "without a view list n_sub must be <= n_scan_views";
        else if (n_scan_views == 0) what = "a scan of zero views";
        else if (tiles * n_sub > 0x7fffffffull) what = "too many pixels for one call";
    }
    if (what) return fail_who(who, what);
    s->g = ray_geo(*det);
    s->tiles_x = tx;
    s->tiles_per_view = (uint32_t)tiles;
    return NAF_OK;
}

// Host: the checks of a ray-list call (`rays` is [n_rays, 8], read as two float4 per ray; `other` is the call's one further device
// pointer) and its grid: one lane per ray, `blocks` workgroups of 256.
inline int make_ray_launch(const char *who, const float *rays, const void *other, uint64_t n_rays, uint32_t *blocks) {
    const char *what = nullptr;
    if (!rays || !other) what = "null pointer";
    else if (!aligned(rays, 15u)) what = "rays must be 16-byte aligned";
    else if ((n_rays + 255u) / 256u > 0x7fffffffull) what = "too many rays for one call";
    if (what) return fail_who(who, what);
    *blocks = (uint32_t)((n_rays + 255u) / 256u);
    return NAF_OK;
}

struct ScanPixel {
    uint32_t j, row, col;   // launch view, detector row and column
    uint64_t pixel;         // row * W + col
};

// Device: the pixel of this lane, from blockIdx.x and threadIdx.x.  False outside the detector (a ragged last tile).
template <ScanLayout kLayout = kScanTiles>
__device__ __forceinline__ bool scan_pixel(uint32_t tiles_x, uint32_t tiles_per_view, const RayGeo &g, ScanPixel &p) {
    p.j = blockIdx.x / tiles_per_view;
    const uint32_t tile = blockIdx.x - p.j * tiles_per_view;
    const uint32_t ty = tile / tiles_x, tx = tile - ty * tiles_x;
    if (kLayout == kScanRowStrip) {
        p.row = ty;
        p.col = tx * kScanStrip + threadIdx.x;
    } else {
        tile_pixel(tx, ty, threadIdx.x, p.row, p.col);
    }
    if (p.row >= g.H || p.col >= g.W) return false;
    p.pixel = (uint64_t)p.row * g.W + p.col;
    return true;
}

}  // namespace naf
