// slab_grid.h -- the launch grid of the slice-marching operators (tv.hip, tvprox.hip, ssim.hip) and its decode in the kernel.
//
// Layout: one lane per (axis 1, axis 2) column of a kSlabTileY x kSlabTileZ tile, lanes along the contiguous axis 2; a workgroup of
// 256 lanes owns the tile and one chunk of axis 0 and marches through the chunk's slices.  blockIdx.x = (chunk * tiles_y + tile y)
// * tiles_z + tile z.  The host part is plain integers in, plain integers out and includes nothing of HIP, so a host compiler reads
// it too; tests/test_slab_grid_cpu.py restates slab_grid() and holds the workspace sizes of TV and SSIM to it.
#pragma once

#include <algorithm>
#include <cstdint>

namespace naf {

constexpr uint32_t kSlabTileY = 8, kSlabTileZ = 32;    // columns per workgroup along axes 1 and 2 (256 lanes)
constexpr uint32_t kSlabTargetBlocks = 2048;           // split axis 0 until the grid has about this many workgroups (8 per CU)

struct SlabGrid {
    uint32_t tiles_y, tiles_z, chunks, chunk;          // chunk = slices of axis 0 per workgroup
    uint64_t blocks;
};

// The grid over m1 x m2 x m3 columns' worth of work; no chunk is shorter than `min_chunk` (what a chunk pays to start: halo or
// warm-up slices).  The extents are those of the lanes' work: SSIM passes its window starts, n - 6 on each axis.
inline SlabGrid slab_grid(uint32_t m1, uint32_t m2, uint32_t m3, uint32_t min_chunk) {
    SlabGrid g;
    g.tiles_y = (m2 + kSlabTileY - 1) / kSlabTileY;
    g.tiles_z = (m3 + kSlabTileZ - 1) / kSlabTileZ;
    const uint64_t tiles = (uint64_t)g.tiles_y * g.tiles_z;
    uint64_t want = (kSlabTargetBlocks + tiles - 1) / tiles;
    const uint64_t most = (m1 + min_chunk - 1) / min_chunk;
    want = std::max<uint64_t>(1, std::min(want, most));
    g.chunk = (uint32_t)((m1 + want - 1) / want);
    g.chunks = (m1 + g.chunk - 1) / g.chunk;
    g.blocks = tiles * g.chunks;
    return g;
}

#if defined(__HIPCC__)
struct SlabLane {
    uint32_t y0, z0;       // origin of the workgroup's tile
    uint32_t ly, lz;       // this lane's column within the tile
    uint32_t a_begin;      // first slice of the workgroup's chunk; the caller forms the end, min(a_begin + chunk, its extent)
};

__device__ __forceinline__ SlabLane slab_lane(uint32_t tiles_y, uint32_t tiles_z, uint32_t chunk) {
    const uint32_t tz_tile = blockIdx.x % tiles_z, rest = blockIdx.x / tiles_z;
    const uint32_t ty_tile = rest % tiles_y, c = rest / tiles_y;
    return {ty_tile * kSlabTileY, tz_tile * kSlabTileZ, threadIdx.x / kSlabTileZ, threadIdx.x % kSlabTileZ, c * chunk};
}
#endif

}  // namespace naf
