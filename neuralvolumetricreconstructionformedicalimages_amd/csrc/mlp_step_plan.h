// mlp_step_plan.h -- the launch plan of the step's MLP kernels: which kernel a step takes, how many tile ranges a ray is cut into,
// how many slabs the backward writes, which grid each launch gets.  Plain integers in, plain integers out: it includes nothing of HIP
// (naf_hip.h, which names the cfg flags, is plain C), so a host compiler reads it too -- tools/step_plan_host_check.cpp prints these
// very functions over a grid of batch sizes and tests/test_step_plan_cpu.py ties the restatement of tests/_mlp16_oracle.py to them.
// Included by mlp_tile_io.h (the kernels read the constants) and by render_step.h, whose drivers call these functions and nothing
// else for these decisions.
#pragma once

#include <algorithm>
#include <cstdint>

#include "../../include/naf_hip.h"

namespace naf {

constexpr uint32_t kMaxSamplesLds = 1024;   // samples of a ray whose depths a wave keeps in LDS (mlp_tile_io.h: fill_depths)
constexpr uint32_t kBackwardBlocks = 512;   // 2 workgroups of 4 waves per CU; also the number of dW slabs
constexpr uint32_t kBackwardBlocks16 = 768; // the 16-point bf16 kernel fits three workgroups per CU (0.89 -> 0.835 ms at 65 536 rays)
constexpr uint32_t kForwardBlocks = 256u * 8u;      // workgroups at most of the one-wave-per-ray forward kernels (eight per CU)

#ifndef NAF_FWD_SPLIT_GRID
#define NAF_FWD_SPLIT_GRID 1024u      // workgroups at most (four fit a CU); A/B builds override it
#endif
constexpr uint32_t kForwardSplitBlocks = NAF_FWD_SPLIT_GRID;

#ifndef NAF_MLP_TRAIN_MAX_RAYS
#define NAF_MLP_TRAIN_MAX_RAYS 3072u      // the largest step with one work item per wave.  A/B builds may lower it; the one launch won
                                          // at every size of the sweep (256 .. 3 072 rays: DESIGN.md section 4.3), so nothing smaller is set
#endif
constexpr uint32_t kMlpTrainMaxRays = NAF_MLP_TRAIN_MAX_RAYS;
static_assert(kMlpTrainMaxRays <= 4u * kBackwardBlocks16, "one work item per wave");

// the two cfg flags the plan looks at (both diagnostic)
inline bool one_wave_per_simd(uint32_t cfg_flags) { return (cfg_flags & NAF_CFG_BACKWARD_ONE_WAVE_PER_SIMD) != 0u; }
inline bool keeps_mlp_pair(uint32_t cfg_flags) { return (cfg_flags & (NAF_CFG_MLP_TWO_KERNELS | NAF_CFG_BACKWARD_ONE_WAVE_PER_SIMD)) != 0u; }

// `want` workgroups, at least one and at most `cap`
inline uint32_t plan_grid(uint64_t want, uint32_t cap) { return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(want, cap)); }

// Tile ranges per ray of the 16-point backward.  Fewer rays than the chip holds waves of that kernel (3 per SIMD = 3 072): `parts`
// ranges per ray, never more ranges than tiles, so that the resident waves all get one item of equal length where the numbers allow
// it (1 024 rays x 12 tiles: 3 parts of 4 tiles).  NAF_CFG_BACKWARD_ONE_WAVE_PER_SIMD in `cfg_flags` (diagnostic): the old goal of one
// wave per SIMD.
inline uint32_t backward16_parts(uint32_t n_samples, uint32_t n_rays, uint32_t cfg_flags) {
    const uint32_t tiles = (n_samples + 15u) / 16u;
    const uint64_t wave_goal = one_wave_per_simd(cfg_flags) ? 1024u : 4u * kBackwardBlocks16;
    return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(std::min<uint64_t>(tiles, 12u), wave_goal / std::max<uint32_t>(n_rays, 1u)));
}

// Waves per workgroup of mlp16_train_kernel for a training step of n_rays rays, or 0: the step runs the forward / backward pair.
// The kernel wants whole rays and whole slabs per workgroup -- a multiple of `parts` and of 4 waves, at most 12 (three waves per SIMD
// of one CU; parts = 5, 7 .. 11, i.e. 257 .. 438 and 513 .. 614 rays at 12 tiles, keep the pair) -- and one work item per wave
// (n_rays * parts <= 3 072, which kMlpTrainMaxRays implies).  `bf16_c2`: the 16-point kernels apply (bf16 mode, C == 2);
// either diagnostic flag in `cfg_flags` keeps the pair (keeps_mlp_pair).
inline uint32_t mlp_train_waves(bool bf16_c2, uint32_t n_samples, uint32_t n_rays, uint32_t cfg_flags) {
    if (!bf16_c2 || keeps_mlp_pair(cfg_flags)) return 0u;
    if (n_rays == 0u || n_rays > kMlpTrainMaxRays || n_samples == 0u || n_samples > kMaxSamplesLds / 2u) return 0u;
    const uint32_t parts = backward16_parts(n_samples, n_rays, cfg_flags);
    return 4u % parts == 0u ? 4u : 12u % parts == 0u ? 12u : 0u;
}

// The bf16 forward of a ray batch takes mlp16_forward_split_kernel: fewer rays than two waves per SIMD, line integrals only
// (`per_sample_outputs`: sigma or the optical depth is asked for too), the terms of a ray fit half a depth buffer, and every one of
// the four waves of a ray gets a tile.
inline bool forward16_splits(uint32_t n_rays, uint32_t n_samples, bool per_sample_outputs, uint32_t cfg_flags) {
    const uint32_t tiles = (n_samples + 15u) / 16u;
    return !per_sample_outputs && n_rays < 2048u && n_samples <= kMaxSamplesLds / 2u && tiles >= 4u && !one_wave_per_simd(cfg_flags);
}
inline uint32_t forward16_split_grid(uint32_t n_rays) { return plan_grid(n_rays, kForwardSplitBlocks); }      // a workgroup per ray

// The one-wave-per-item forward kernels (mlp_forward_kernel: 32-point tiles, mlp16_forward_kernel and fused_forward_kernel: 16):
// an item is a ray, or a tile of a point list; four waves per workgroup.
inline uint32_t forward_grid(uint32_t n_items, bool rays, uint32_t tile_points) {
    const uint64_t waves = rays ? n_items : ((uint64_t)n_items + tile_points - 1u) / tile_points;
    return plan_grid((waves + 3) / 4, kForwardBlocks);
}

// The backward kernels write one slab per workgroup, so their grids are the slab counts; mlp16_train_kernel writes the same
// backward16_slabs() slabs as the pair, `waves` / 4 per workgroup, and takes one work item per wave.
inline uint32_t backward_slabs(uint32_t n_rays) { return plan_grid(((uint64_t)n_rays + 3) / 4, kBackwardBlocks); }      // fp32: a wave per ray
inline uint32_t backward16_slabs(uint32_t n_rays, uint32_t parts) { return plan_grid(((uint64_t)n_rays * parts + 3) / 4, kBackwardBlocks16); }
inline uint32_t mlp_train_grid(uint32_t n_rays, uint32_t parts, uint32_t waves) { return (n_rays * parts + waves - 1u) / waves; }

}  // namespace naf
