// render_step.h -- the host drivers of the fused step: the workspace layout (carve), the cfg check, the launches of the encoder, the
// MLP kernels and the table scatter (run_*), and the bodies of the entry points (*_impl).  The launch decisions are mlp_step_plan.h's
// (MLP kernels) and scatter_host.h's (binned scatter), every launch itself is naf_host.h's launch() / launch_as(): profile name,
// launch, check.  The structs below name a call's buffers once, in the entry point, so that
// nothing here passes them by position.  Included from render_fused.hip only: FxRecords is no template, so it instantiates its
// kernels in every translation unit that declares it (scatter_host.h).
#pragma once

#include <algorithm>
#include <type_traits>

#include "naf_host.h"
#include "hash_kernels.h"
#include "encode_kernel.h"
#include "field_mlp.h"
#include "field_mlp16.h"
#include "fused_forward.h"
#include "levels_gather.h"
#include "mlp16_kernels.h"
#include "mlp_slabs.h"
#include "mlp_step_plan.h"
#include "scatter_binned.h"
#include "scatter_v2.h"
#include "scatter_host.h"

namespace naf {

static SrcRays make_src(const float *rays, const float *t_rand, const naf_render_cfg *cfg) {
    SrcRays s;
    s.rays = rays; s.t_rand = t_rand; s.S = cfg->n_samples; s.perturb = cfg->perturb != 0; s.bound = cfg->bound;
    s.explicit_z = (cfg->flags & NAF_CFG_EXPLICIT_DEPTHS) != 0u;
    s.seed = cfg->seed; s.ray_base = cfg->ray_index_base;
    s.div_magic = (uint32_t)((1ull << 32) / s.S);
    s.lin_step = 1.0f / (float)(s.S - 1u);
    s.rden = 1.0f / (2.0f * s.bound);
    return s;
}

// ---- a call's arguments, named once ---------------------------------------------------------------------------------------------------
struct RayBatch {                        // the rays of a call, with its cfg, workspace and stream
    const float *rays, *t_rand; uint32_t n_rays; const naf_render_cfg *cfg; void *ws; hipStream_t s;
    uint32_t points() const { return n_rays * cfg->n_samples; }
    SrcRays src() const { return make_src(rays, t_rand, cfg); }
};
struct Field { const void *emb; const int32_t *offsets; const float *mlp; };      // hash tables, their level offsets, the MLP's parameter block
// line integrals (or sigma per point), optional per-sample outputs, where point p writes
struct ForwardOut { float *out; float *sigma = nullptr, *depth = nullptr; OutMap omap = OutMap{0u, 0u, 0u, 0u}; };
// of a training step; a plain backward pass (naf_render_backward) has the two gradients only
struct TrainBuffers { const float *target, *ray_weight; float *acc, *grad_emb, *grad_mlp, *loss_out; };
struct StepTail {                        // what rides on the step's last launches; all absent by default
    const naf_grad_buckets *buckets = nullptr;
    const AdamTail *adam = nullptr;      // the table's update in the reducer
    const MlpAdam *madam = nullptr;      // the MLP's update in the slab reduction
    bool loss_assign = false;            // loss_out[0] = loss instead of +=
    DrawJob *next_draw = nullptr;        // the next step's pixel draw in pass 1 of the binned scatter
};
struct BackwardSource {                  // where a backward pass gets d loss / d acc and its features from
    const float *grad_acc = nullptr;     // the upstream gradient (naf_render_backward); nullptr: a training step, TrainBuffers has the loss's inputs
    bool features_valid = false;         // the workspace holds the features of these rays
    bool one_launch = false;             // the forward has not run: mlp16_train_kernel does both passes
};
struct LevelRange { uint32_t begin, end; };
struct LevelBlocks { const void *blocks; size_t stride; uint32_t n_ranks; LevelRange lv; };      // naf_levels_scatter's gradient blocks

// ---- workspace ------------------------------------------------------------------------------------------------------------------------
template <typename P>
static uint32_t forward_lds_bytes() { return ((MlpShared<P>::kBytes + 15u) & ~15u) + 4u * kMaxSamplesLds * 4u; }
template <typename P>
static uint32_t backward_lds_bytes() {
    const uint32_t sh = (MlpShared<P>::kBytes + 15u) & ~15u;
    const uint32_t imgs = ((4u * 3u * 32u * P::kTrPitch * (uint32_t)sizeof(typename P::tr_t)) + 15u) & ~15u;
    return sh + std::max<uint32_t>(imgs + 4u * kMaxSamplesLds * 4u, (kMlpParams + 2u) * 4u);
}

struct Workspace {
    unsigned char *feat, *dfeat;
    float *slabs, *grad_acc;
    BinRegions bin;              // binned scatter only (scatter_host.h)
    BinPlan plan;
    bool binned;
    size_t bytes;
};

// the features are held in the MLP's operand precision (P::feat_t); a feature tensor [L, n_points, C] is rounded up to 256 bytes
static size_t feature_elem_bytes(const naf_render_cfg *cfg) { return cfg->mlp_precision == NAF_F32 ? 4 : 2; }
static size_t feature_bytes(const naf_render_cfg *cfg, uint64_t n_points) {
    return ((size_t)n_points * cfg->L * cfg->C * feature_elem_bytes(cfg) + 255) & ~(size_t)255;
}

static Workspace carve(void *base, const naf_render_cfg *cfg, uint64_t n_points) {
    const size_t feat_bytes = feature_bytes(cfg, n_points);
    const size_t slab_bytes = (size_t)std::max(kBackwardBlocks, kBackwardBlocks16) * kSlabStride * 4;
    const size_t n_rays_max = (size_t)(n_points / std::max<uint32_t>(cfg->n_samples, 1u)) + 1;
    Workspace w;
    w.feat = (unsigned char *)base;
    w.dfeat = w.feat + feat_bytes;
    w.slabs = (float *)(w.dfeat + feat_bytes);
    w.grad_acc = (float *)((unsigned char *)w.slabs + slab_bytes);
    w.bytes = 2 * feat_bytes + slab_bytes + ((n_rays_max * 4 + 255) & ~(size_t)255) + 512;      // + partial sums of the loss
    w.binned = make_bin_plan(cfg, n_points, &w.plan);
    w.bin = BinRegions{};
    if (w.binned) {
        w.bin = carve_bin_regions((unsigned char *)base + w.bytes, cfg, w.plan);
        w.bytes += w.bin.bytes;
    }
    return w;
}

constexpr uint32_t kKnownCfgFlags =
    NAF_CFG_PER_LEVEL_LAUNCHES | NAF_CFG_EXPLICIT_DEPTHS | NAF_CFG_LEVELS_INTERLEAVED | NAF_CFG_FORWARD_FUSED | NAF_CFG_FUSED_STORE_FEATURES |
    NAF_CFG_ENCODE_TWO_GATHERS | NAF_CFG_ENCODE_WINDOWS | NAF_CFG_BACKWARD_ONE_WAVE_PER_SIMD | NAF_CFG_ENCODE_LEVEL_MAJOR | NAF_CFG_TEST_TINY_BLOCKS |
    NAF_CFG_ENCODE_GROUPS_2 | NAF_CFG_ENCODE_GROUPS_4 | NAF_CFG_MIN_BUCKETS_MASK | NAF_CFG_SCATTER_PAIR12 | NAF_CFG_LEVELS_GATHER_PASS | NAF_CFG_MLP_TWO_KERNELS;

static int check_cfg(const naf_render_cfg *cfg) {
    if (!cfg) return fail(NAF_ERR_INVALID_ARGUMENT, "render: null cfg");
    if (cfg->L * cfg->C != 32u || !(cfg->C == 1 || cfg->C == 2 || cfg->C == 4 || cfg->C == 8))
        return fail(NAF_ERR_UNSUPPORTED, "fused field: encoder output L*C must be 32 with C in {1,2,4,8} "
                                         "(other shapes run through the unfused operators)");
    if (cfg->mlp_precision != NAF_F32 && cfg->mlp_precision != NAF_BF16)
        return fail(NAF_ERR_UNSUPPORTED, "fused field: mlp_precision must be NAF_F32 or NAF_BF16");
    if (cfg->table_dtype < NAF_F32 || cfg->table_dtype > NAF_BF16) return fail(NAF_ERR_UNSUPPORTED, "fused field: bad table_dtype");
    if (cfg->last_activation < 0 || cfg->last_activation > 3) return fail(NAF_ERR_UNSUPPORTED, "fused field: bad last_activation");
    if (!(cfg->bound > 0.0f)) return fail(NAF_ERR_INVALID_ARGUMENT, "fused field: bound must be > 0");
    if (cfg->flags & ~kKnownCfgFlags) return fail(NAF_ERR_INVALID_ARGUMENT, "fused field: unknown cfg flag");
    if (cfg->scatter_mode < NAF_SCATTER_AUTO || cfg->scatter_mode > NAF_SCATTER_BINNED)
        return fail(NAF_ERR_INVALID_ARGUMENT, "fused field: scatter_mode must be NAF_SCATTER_AUTO, _ATOMIC or _BINNED");
    return NAF_OK;
}

template <typename P, uint32_t C>
static uint32_t train_waves(const naf_render_cfg *cfg, uint32_t n_rays) {      // mlp_step_plan.h takes plain values
    return mlp_train_waves(std::is_same<P, PrecBF16>::value && C == 2, cfg->n_samples, n_rays, cfg->flags);
}

// ---- encoder --------------------------------------------------------------------------------------------------------------------------
struct EncodeLevels { uint32_t begin = 0u, end = ~0u, chunk = 0u; };      // default: every level, one chunk

template <typename P, uint32_t C, typename Src>
static int dispatch_encode(const Src &src, const Field &f, void *feat, uint32_t B, const naf_render_cfg *cfg, hipStream_t s,
                           const EncodeLevels &lv = EncodeLevels{}) {
    // encode_kernel.h; features are written in the MLP's operand precision (P::feat_t), whatever the table stores
    using FT = typename P::feat_t;
    switch (cfg->table_dtype) {
        case NAF_F32: return launch_encode<F32, FT, C, Src>(src, f.emb, f.offsets, feat, B, cfg->H, cfg->L, cfg->flags, s, lv.begin, lv.end, lv.chunk);
        case NAF_F16: return launch_encode<F16, FT, C, Src>(src, f.emb, f.offsets, feat, B, cfg->H, cfg->L, cfg->flags, s, lv.begin, lv.end, lv.chunk);
        default: return launch_encode<BF16, FT, C, Src>(src, f.emb, f.offsets, feat, B, cfg->H, cfg->L, cfg->flags, s, lv.begin, lv.end, lv.chunk);
    }
}

// ---- MLP forward ----------------------------------------------------------------------------------------------------------------------
template <typename P, uint32_t C, bool kRays>
static int run_mlp_forward(const void *feat, const float *mlp, const SrcRays &src, const ForwardOut &o, uint32_t n_items, uint32_t B,
                           const naf_render_cfg *cfg, hipStream_t s) {
    if constexpr (std::is_same<P, PrecBF16>::value && C == 2) {
        // (depth buffers of the four waves, which also stage the weights in the prologue: Mlp16Shared::build_staged)
        const uint32_t lds16 = ((Mlp16Shared::kBytes + 15u) & ~15u) + std::max<uint32_t>(4u * kMaxSamplesLds * 4u, Mlp16Shared::kStageFloats * 4u);
        // (every forward instantiation is timed as mlp_forward_kernel, the row bench.py reads; a failed launch names the kernel itself)
        if (kRays && forward16_splits(n_items, src.S, o.sigma != nullptr || o.depth != nullptr, cfg->flags))
            return launch_as("mlp_forward_kernel", "mlp16_forward_split_kernel", mlp16_forward_split_kernel, dim3(forward16_split_grid(n_items)), dim3(256), lds16, s,
                             (const uint16_t *)feat, mlp, src, o.out, n_items, B, cfg->last_activation);
        return launch_as("mlp_forward_kernel", "mlp16_forward_kernel", mlp16_forward_kernel<kRays>, dim3(forward_grid(n_items, kRays, 16u)), dim3(256), lds16, s,
                         (const uint16_t *)feat, mlp, src, o.out, o.sigma, o.depth, n_items, B, cfg->last_activation, o.omap);
    }
    // (no `else`: the 32-point kernels stay instantiated for bf16, C = 2 as well, though nothing launches them there)
    return launch("mlp_forward_kernel", mlp_forward_kernel<P, C, kRays>, dim3(forward_grid(n_items, kRays, 32u)), dim3(256), forward_lds_bytes<P>(), s,
                  (const typename P::feat_t::store_t *)feat, mlp, src, o.out, o.sigma, o.depth, n_items, B, cfg->last_activation, o.omap);
}

// ---- MLP backward ---------------------------------------------------------------------------------------------------------------------
// What the backward pass hands down so that its small jobs ride on kernels it launches anyway: `clear_words` -- the overflow
// counters of the binned scatter, zeroed by the MLP backward kernel (which always precedes the scatter on the stream; three memset
// launches of ~5 us each were 4 % of the reference-size step); `loss_assign` -- loss_out[0] = loss instead of +=; `deferred` --
// where to leave the description of the slab reduction instead of launching it (the first scatter_bin launch then runs it in spare
// workgroups, beside its own: one dependent launch of ~11 us less per step).
struct StepExtras { uint32_t *clear_words; bool loss_assign; SlabReduce *deferred; hipEvent_t after_backward = nullptr;      // after_backward: recorded once
                    float *acc_out = nullptr; };                                      // the feature gradients are final, before the slab reduction
// acc_out: the forward has NOT run; mlp16_train_kernel does both passes and leaves the line integrals there (train_waves() != 0)

// One MLP backward launch.  `loss.target` != nullptr: training step -- d loss / d acc is formed inside the kernel from (acc, target,
// weight), the loss itself travels through the slabs into loss_out (+=).  Otherwise `grad_acc` is the upstream gradient
// (naf_render_backward).
struct MlpBackwardJob {
    const void *feat; const float *mlp, *grad_acc; LossInputs loss; void *dfeat; float *slabs;
    uint32_t *gmax_bits; float *grad_mlp, *loss_out; const MlpAdam *madam; StepExtras ex;
};

// The end of every MLP backward launch (`launched`: what it returned): record the event, then reduce its n_slabs slabs
// (mlp_grad_reduce_kernel) -- or leave the reduction's description where the scatter picks it up (`ex.deferred`).
static int finish_mlp_backward(int launched, const MlpBackwardJob &j, uint32_t n_slabs, hipStream_t s) {
    if (launched != NAF_OK) return launched;
    if (j.ex.after_backward != nullptr && hipEventRecord(j.ex.after_backward, s) != hipSuccess) return fail(NAF_ERR_LAUNCH, "mlp backward: cannot record the event");
    const MlpAdam none{nullptr, nullptr, nullptr, AdamArgs{}};
    const SlabReduce sr{j.slabs, n_slabs, j.grad_mlp, j.loss_out, j.loss.target == nullptr ? kLossNone : j.ex.loss_assign ? kLossAssign : kLossAdd,
                        j.madam != nullptr ? *j.madam : none, j.gmax_bits};
    if (j.ex.deferred != nullptr) { *j.ex.deferred = sr; return NAF_OK; }
    return launch("mlp_grad_reduce_kernel", mlp_grad_reduce_kernel, dim3(kSlabReduceBlocks), dim3(kReduceParams * kReduceGroups), 0, s, sr);
}

template <typename P, uint32_t C>
static int run_mlp_backward(const MlpBackwardJob &j, const SrcRays &src, uint32_t n_rays, uint32_t B, const naf_render_cfg *cfg, hipStream_t s) {
    if constexpr (std::is_same<P, PrecBF16>::value && C == 2) {
        const uint32_t sh16 = (Mlp16Shared::kBytes + 15u) & ~15u;
        const uint32_t parts = backward16_parts(cfg->n_samples, n_rays, cfg->flags);
        const uint32_t n_slabs = backward16_slabs(n_rays, parts);
        if (j.ex.acc_out != nullptr) {                       // both passes in one launch; the same slabs as from the pair
            const uint32_t nw = train_waves<P, C>(cfg, n_rays);
            if (nw == 0u || j.loss.target == nullptr || j.grad_acc != nullptr) return fail(NAF_ERR_LAUNCH, "mlp backward: this step cannot run mlp16_train_kernel");
            auto kern = nw == 4u ? mlp16_train_kernel<4u> : mlp16_train_kernel<12u>;
            const uint32_t lds = sh16 + nw * (3u * kImg16 + kMaxSamplesLds * 4u);
            if (int rc = raise_lds_limit(kern, lds, "mlp16_train_kernel: cannot raise dynamic LDS limit")) return rc;
            // (the 16-point kernels are timed under the aggregate names bench.py reads, mlp_train_kernel and mlp_backward_kernel)
            const int rc = launch_as("mlp_train_kernel", "mlp16_train_kernel", kern, dim3(mlp_train_grid(n_rays, parts, nw)), dim3(64u * nw), lds, s, (const uint16_t *)j.feat, j.mlp,
                                     src, j.loss, j.ex.acc_out, (uint16_t *)j.dfeat, j.slabs, n_rays, B, cfg->last_activation, parts, n_slabs, j.ex.clear_words);
            return finish_mlp_backward(rc, j, n_slabs, s);
        }
        const uint32_t lds16 = sh16 + std::max<uint32_t>(4u * 3u * 1024u + 4u * kMaxSamplesLds * 4u, (kMlpParams + 2u) * 4u);
        const int rc = launch_as("mlp_backward_kernel", "mlp16_backward_kernel", mlp16_backward_kernel, dim3(n_slabs), dim3(256), lds16, s, (const uint16_t *)j.feat, j.mlp, src,
                                 j.grad_acc, j.loss, (uint16_t *)j.dfeat, j.slabs, n_rays, B, cfg->last_activation, parts, j.ex.clear_words);
        return finish_mlp_backward(rc, j, n_slabs, s);
    }
    auto kern = mlp_backward_kernel<P, C>;                   // (no `else`: see run_mlp_forward)
    const uint32_t lds = backward_lds_bytes<P>(), n_slabs = backward_slabs(n_rays);
    if (int rc = raise_lds_limit(kern, lds, "mlp_backward_kernel: cannot raise dynamic LDS limit")) return rc;      // fp32 images need > 64 KiB
    const int rc = launch("mlp_backward_kernel", kern, dim3(n_slabs), dim3(256), lds, s, (const typename P::feat_t::store_t *)j.feat, j.mlp, src, j.grad_acc, j.loss,
                          (typename P::feat_t::store_t *)j.dfeat, j.slabs, n_rays, B, cfg->last_activation, j.ex.clear_words);
    return finish_mlp_backward(rc, j, n_slabs, s);
}

// ---- table scatter --------------------------------------------------------------------------------------------------------------------
// The Adam tail (naf_render_train_adam, naf_levels_scatter) needs the binned scatter, level-major launches and every reducer launch
// over the levels [lv_begin, lv_end) unsplit.
static bool adam_tail_possible(const naf_render_cfg *cfg, const Workspace &w, uint32_t lv_begin, uint32_t lv_end) {
    if (!w.binned || per_level_launches(cfg)) return false;
    const uint32_t NB = 1u << w.plan.log2_nb;
    for (uint32_t l0 = lv_begin; l0 < lv_end; l0 += w.plan.levels_per_pass)
        if (reducer_split(NB, std::min(w.plan.levels_per_pass, lv_end - l0)) != 1u) return false;
    return true;
}

// The record family of scatter_v2.h (launch_binned_scatter, scatter_host.h): 8-byte records, the canonical two-channel bf16 shape.  Pass 1 also runs the next step's pixel draw
// when the caller hands one over, and on the level-parallel path reads the all-to-all's gradient blocks in place (`from_blocks`).
#ifndef NAF_V2_LV_FEW
#define NAF_V2_LV_FEW 4u      // levels per bin workgroup when tiles are scarce.  A/B builds (tools/build_variant.sh) override it: 2 gains 2 us at
                              // 512 rays and loses 9 at 4 096, 8 the other way round (profiles/round4_ab_reducer_nt_loads_and_levels_per_bin_workgroup.jsonl)
#endif
struct FxRecords {
    using Rec = PairFx;
    static constexpr uint32_t kThreads = 512u, kPoints = 2u, kLvMany = 16u, kLvFew = NAF_V2_LV_FEW;
    static constexpr bool kHasBig = true;
    const SrcRays &src;
    const void *dfeat;
    uint32_t B;
    DrawJob *next_draw;                  // taken along by the first launch, which sets its count to 0
    const GradBlocks *from_blocks;

    template <bool kFromBlocks>
    static auto bin_kernel_of(bool big, bool nb64, bool many) {
        constexpr uint32_t NT = kThreads;
        return big ? (many ? scatter_bin2_kernel<2u * NT, kLvMany, 0u, kFromBlocks> : scatter_bin2_kernel<2u * NT, kLvFew, 0u, kFromBlocks>)
                   : nb64 ? (many ? scatter_bin2_kernel<NT, kLvMany, 6u, kFromBlocks> : scatter_bin2_kernel<NT, kLvFew, 6u, kFromBlocks>)
                          : (many ? scatter_bin2_kernel<NT, kLvMany, 0u, kFromBlocks> : scatter_bin2_kernel<NT, kLvFew, 0u, kFromBlocks>);
    }
    auto bin_kernel(const BinPlan &plan, bool big, bool many) const {
        // 64 buckets per level (every table up to 2^19 rows per level): the variant whose waves scan the bucket counters themselves
        const bool nb64 = plan.log2_nb == 6u;
        return from_blocks != nullptr ? bin_kernel_of<true>(big, nb64, many) : bin_kernel_of<false>(big, nb64, many);
    }
    auto reduce_kernel(const AdamTail *adam) const {
        const bool fast = adam != nullptr && adam->lp != nullptr;        // tables with a 16-bit shadow: adam_math.h
        return adam == nullptr ? scatter_reduce2_kernel<false, false> : fast ? scatter_reduce2_kernel<true, true> : scatter_reduce2_kernel<true, false>;
    }
    uint32_t bin_lds(const BinPlan &plan) const {      // counters, staging, side list
        return (3u * (1u << plan.log2_nb) + 4u) * 4u + (plan.slots + 1u) * (uint32_t)sizeof(PairFx) + side_list_capacity(plan.slots) * 12u;
    }
    template <typename K>
    int launch_bin(const char *timed, K bin, dim3 grid, uint32_t threads, uint32_t lds, hipStream_t s, const BinPass &p) const {
        DrawJob dj{};
        if (next_draw != nullptr && next_draw->count != 0u) { dj = *next_draw; next_draw->count = 0u; }
        grid.x += (dj.count + threads - 1u) / threads;                    // the draw's spare workgroups
        const GradBlocks gb = from_blocks != nullptr ? *from_blocks : GradBlocks{};
        return launch_as(timed, "scatter_bin_kernel", bin, grid, dim3(threads), lds, s, src, (const uint16_t *)dfeat, p.offsets, p.grad_table, (PairFx *)p.w.regions,
                         p.w.counts, p.w.overflow, B, p.H, p.l0, p.nl, p.plan, p.job, dj, gb);
    }
};

// The table-gradient scatter of a call: the gradients `dfeat` of the B points of `src` into `grad_table`, and what rides on it.
struct ScatterJob {
    const SrcRays &src; const void *dfeat; const int32_t *offsets; float *grad_table; uint32_t B;
    const naf_render_cfg *cfg; const Workspace &w; hipStream_t s;
    const naf_grad_buckets *buckets = nullptr;       // per-bucket reduction + events
    const AdamTail *adam = nullptr;
    const SlabReduce *slab_job = nullptr;            // the deferred slab reduction (StepExtras)
    DrawJob *next_draw = nullptr;
    const GradBlocks *from_blocks = nullptr;         // dfeat is the all-to-all's blocks, read in place
};

// Table-gradient scatter of the levels [lv_begin, lv_end).
template <typename P, uint32_t C>
static int run_hash_backward_levels(const ScatterJob &j, uint32_t lv_begin, uint32_t lv_end) {
    using FT = typename P::feat_t;
    const naf_render_cfg *cfg = j.cfg;
    const Workspace &w = j.w;
    if (j.from_blocks != nullptr && !(w.binned && scatter_v2(cfg))) return fail(NAF_ERR_LAUNCH, "hash backward: only the 8-byte-record scatter reads gradient blocks in place");
    if (w.binned) {
        auto scatter = [&](auto fam) { return launch_binned_scatter(fam, cfg, w.plan, w.bin, j.offsets, j.grad_table, lv_begin, lv_end, j.buckets, j.s, j.adam, j.slab_job); };
        if (scatter_v2(cfg)) return scatter(FxRecords{j.src, j.dfeat, j.B, j.next_draw, j.from_blocks});
        // fp32 records in parity mode, bf16 ones packed in pairs otherwise; the features are [L, B, C]: strides (B, 1)
        if (cfg->mlp_precision == NAF_F32) return scatter(PairRecords<FT, C, SrcRays, PairF32<C>, 16u, true>{j.src, j.dfeat, j.B, j.B, 1u});
        return scatter(PairRecords<FT, C, SrcRays, PairBF16<C>, 16u, true>{j.src, j.dfeat, j.B, j.B, 1u});
    }
    if (j.adam != nullptr) return fail(NAF_ERR_LAUNCH, "hash backward: the Adam tail needs the binned scatter");
    const auto kern = hash_backward_kernel<FT, 3, C, SrcRays>;
    if (per_level_launches(cfg)) {                           // a level's launch is timed under its own name; a failed one ends the loop
        static const char *const names[32] = NAF_LEVEL_NAMES("hash_backward_kernel_L");
        for (uint32_t l = lv_begin; l < lv_end; ++l)
            if (int rc = launch_as(level_name(names, l), "hash_backward_kernel", kern, dim3(hash_grid_x(j.B), 1), dim3(256), 0, j.s, j.src,
                                   (const typename FT::store_t *)j.dfeat, j.offsets, j.grad_table, j.B, cfg->L, cfg->H, false, l)) return rc;
        return NAF_OK;
    }
    return launch("hash_backward_kernel", kern, dim3(hash_grid_x(j.B), lv_end - lv_begin), dim3(256), 0, j.s, j.src,
                  (const typename FT::store_t *)j.dfeat, j.offsets, j.grad_table, j.B, cfg->L, cfg->H, false, lv_begin);
}

// All levels, in the order of `buckets` when given (data-parallel training: each bucket's event is recorded on the stream as
// soon as its rows of the gradient table are final, so that the caller can start that bucket's all-reduce while the next
// bucket is still being binned and reduced).
template <typename P, uint32_t C>
static int run_hash_backward(const ScatterJob &j) {
    // (the overflow counters were zeroed by the MLP backward kernel of this call: StepExtras)
    const naf_grad_buckets *buckets = j.buckets;
    if (buckets == nullptr) return run_hash_backward_levels<P, C>(j, 0u, j.cfg->L);
    if (j.adam != nullptr) return fail(NAF_ERR_INVALID_ARGUMENT, "render_train: the Adam tail cannot be combined with gradient buckets");
    ScatterJob plain{j.src, j.dfeat, j.offsets, j.grad_table, j.B, j.cfg, j.w, j.s};      // nothing rides on a bucketed scatter
    if (j.w.binned && !per_level_launches(j.cfg) && j.w.plan.levels_per_pass >= j.cfg->L) {      // one bin pass, per-bucket reduction + events
        plain.buckets = buckets;
        return run_hash_backward_levels<P, C>(plain, 0u, j.cfg->L);
    }
    for (uint32_t b = 0; b < buckets->n_buckets; ++b) {
        if (int rc = run_hash_backward_levels<P, C>(plain, buckets->level_begin[b], buckets->level_end[b])) return rc;
        if (buckets->ready[b] != nullptr && hipEventRecord((hipEvent_t)buckets->ready[b], j.s) != hipSuccess)
            return fail(NAF_ERR_LAUNCH, "render_train: cannot record a bucket event");
    }
    return NAF_OK;
}

// ---- forward-only calls ----------------------------------------------------------------------------------------------
// They need the [L, n_points, C] features and nothing else of the training workspace -- or, where the single fused kernel
// applies (NAF_CFG_FORWARD_FUSED, the canonical field in bf16 mode), no workspace at all.
static bool forward_fused(const naf_render_cfg *cfg) {
    return (cfg->flags & NAF_CFG_FORWARD_FUSED) != 0u && cfg->mlp_precision == NAF_BF16 && cfg->C == 2u && cfg->L == kFusedLevels;
}
static size_t forward_workspace_bytes(const naf_render_cfg *cfg, uint64_t n_points) {
    if (forward_fused(cfg) && (cfg->flags & NAF_CFG_FUSED_STORE_FEATURES) == 0u) return 256;
    return feature_bytes(cfg, n_points) + 256;
}

template <typename TT, typename Src>
static int launch_fused_forward(const Src &src, const Field &f, const ForwardOut &o, void *feat, uint32_t n_items, uint32_t B, const naf_render_cfg *cfg,
                                hipStream_t s) {
    constexpr bool kRays = std::is_same<Src, SrcRays>::value;
    const uint32_t lds = ((Mlp16Shared::kBytes + 15u) & ~15u) + kFusedLevels * (uint32_t)sizeof(LevelRec) + (kRays ? 4u * kMaxSamplesLds * 4u : 0u);
    uint16_t *fout = (cfg->flags & NAF_CFG_FUSED_STORE_FEATURES) != 0u ? (uint16_t *)feat : nullptr;
    return launch("fused_forward_kernel", fused_forward_kernel<TT, Src>, dim3(forward_grid(n_items, kRays, 16u)), dim3(256), lds, s, src,
                  (const typename TT::store_t *)f.emb, f.offsets, f.mlp, o.out, o.sigma, o.depth, fout, n_items, B, cfg->H, cfg->last_activation, o.omap);
}
template <typename Src>
static int run_fused_forward(const Src &src, const Field &f, const ForwardOut &o, void *feat, uint32_t n_items, uint32_t B, const naf_render_cfg *cfg,
                             hipStream_t s) {
    switch (cfg->table_dtype) {
        case NAF_F32: return launch_fused_forward<F32>(src, f, o, feat, n_items, B, cfg, s);
        case NAF_F16: return launch_fused_forward<F16>(src, f, o, feat, n_items, B, cfg, s);
        default: return launch_fused_forward<BF16>(src, f, o, feat, n_items, B, cfg, s);
    }
}

// encoder + MLP forward of a ray batch; the features stay at the workspace base (a training step's backward pass reads them there)
template <typename P, uint32_t C>
static int encode_and_forward(const RayBatch &b, const Field &f, const ForwardOut &o) {
    const SrcRays src = b.src();
    if (int rc = dispatch_encode<P, C>(src, f, b.ws, b.points(), b.cfg, b.s)) return rc;
    return run_mlp_forward<P, C, true>(b.ws, f.mlp, src, o, b.n_rays, b.points(), b.cfg, b.s);
}

template <typename P, uint32_t C>
static int render_forward_impl(const RayBatch &b, const Field &f, const ForwardOut &o) {
    if (forward_fused(b.cfg)) return run_fused_forward(b.src(), f, o, b.ws, b.n_rays, b.points(), b.cfg, b.s);
    return encode_and_forward<P, C>(b, f, o);
}

// a point list (SrcRaw) or a generated grid (SrcGrid, with its OutMap in `o`)
template <typename P, uint32_t C, typename Src>
static int field_forward_impl(const Src &src, const Field &f, const ForwardOut &o, uint32_t B, const naf_render_cfg *cfg, void *ws, hipStream_t s) {
    if (forward_fused(cfg)) return run_fused_forward(src, f, o, ws, B, B, cfg, s);
    if (int rc = dispatch_encode<P, C>(src, f, ws, B, cfg, s)) return rc;
    SrcRays none{};
    return run_mlp_forward<P, C, false>(ws, f.mlp, none, o, B, B, cfg, s);
}

// ---- backward pass, training step -----------------------------------------------------------------------------------------------------
template <typename P, uint32_t C>
static int render_backward_impl(const RayBatch &b, const Field &f, const TrainBuffers &t, const BackwardSource &from, const StepTail &tail) {
    const naf_render_cfg *cfg = b.cfg;
    const uint32_t B = b.points();
    const Workspace w = carve(b.ws, cfg, B);
    const SrcRays src = b.src();
    const bool from_train = t.target != nullptr;
    AdamTail adam;
    if (tail.adam != nullptr) {                              // the overflow counters live in this call's workspace
        adam = *tail.adam;
        adam.overflow = w.bin.overflow;
    }
    // (a fused forward of the same cfg left no features behind unless it was asked to store them)
    if (!from.features_valid || (forward_fused(cfg) && (cfg->flags & NAF_CFG_FUSED_STORE_FEATURES) == 0u && !from_train))
        if (int rc = dispatch_encode<P, C>(src, f, w.feat, B, cfg, b.s)) return rc;
    // Single-GPU steps on the binned scatter defer the slab reduction (MLP gradient / Adam, loss, gradient maximum) to spare workgroups
    // of the scatter's first launch; data-parallel steps need the MLP gradient final BEFORE the scatter (its all-reduce starts at
    // `mlp_ready`), per-level diagnostics keep their launches apart.
    SlabReduce job{};
    const bool defer = w.binned && tail.buckets == nullptr && !per_level_launches(cfg);
    // the masked squared error and its gradient are formed inside the backward kernel (LossInputs); the loss reaches loss_out
    // through the slab reduction that also finishes the MLP gradient
    MlpBackwardJob mj{w.feat, f.mlp, from.grad_acc, LossInputs{t.acc, t.target, t.ray_weight}, w.dfeat, w.slabs, w.bin.gmax, t.grad_mlp, t.loss_out, tail.madam,
                      StepExtras{w.bin.overflow, tail.loss_assign, defer ? &job : nullptr}};
    if (from.one_launch) mj.ex.acc_out = t.acc;
    if (int rc = run_mlp_backward<P, C>(mj, src, b.n_rays, B, cfg, b.s)) return rc;
    // grad_mlp (and, in the training entry point, the loss) are final here, before the table scatter starts
    if (tail.buckets != nullptr && tail.buckets->mlp_ready != nullptr && hipEventRecord((hipEvent_t)tail.buckets->mlp_ready, b.s) != hipSuccess)
        return fail(NAF_ERR_LAUNCH, "render_train: cannot record the MLP-gradient event");
    ScatterJob sj{src, w.dfeat, f.offsets, t.grad_emb, B, cfg, w, b.s};
    sj.buckets = tail.buckets;
    if (tail.adam != nullptr) sj.adam = &adam;
    if (defer) sj.slab_job = &job;
    sj.next_draw = tail.next_draw;
    return run_hash_backward<P, C>(sj);
}

template <typename P, uint32_t C>
static int render_train_impl(const RayBatch &b, const Field &f, const TrainBuffers &t, const StepTail &tail) {
    // small bf16 steps: the encoder alone here, forward and backward of the MLP in one launch below (mlp16_train_kernel)
    BackwardSource from;
    from.features_valid = true;
    from.one_launch = train_waves<P, C>(b.cfg, b.n_rays) != 0u;
    if (from.one_launch) {
        if (int rc = dispatch_encode<P, C>(b.src(), f, b.ws, b.points(), b.cfg, b.s)) return rc;
    } else if (int rc = encode_and_forward<P, C>(b, f, ForwardOut{t.acc})) return rc;
    return render_backward_impl<P, C>(b, f, t, from, tail);
}

// ---- level-parallel training (naf_levels_*, naf_hip.h): each rank owns a range of levels ----------------------------------
template <typename P, uint32_t C>
static int levels_encode_impl(const RayBatch &b, const Field &f, void *features, const LevelRange &lv, uint32_t n_ranks) {
    EncodeLevels el;
    el.begin = lv.begin; el.end = lv.end; el.chunk = b.points() / n_ranks;
    return dispatch_encode<P, C>(b.src(), f, features, b.points(), b.cfg, b.s, el);
}

template <typename P, uint32_t C>
static int levels_field_impl(const RayBatch &b, const void *features, const float *mlp, const TrainBuffers &t, void *feature_grads, hipEvent_t grads_ready) {
    const uint32_t B = b.points();
    const Workspace w = carve(b.ws, b.cfg, B);
    const SrcRays src = b.src();
    const bool one_launch = train_waves<P, C>(b.cfg, b.n_rays) != 0u;
    if (!one_launch)
        if (int rc = run_mlp_forward<P, C, true>(features, mlp, src, ForwardOut{t.acc}, b.n_rays, B, b.cfg, b.s)) return rc;
    MlpBackwardJob mj{};                                     // no upstream gradient, gradient maximum or MLP update; no counters to clear and
    mj.feat = features; mj.mlp = mlp;                        // no deferred reduction: the scatter runs on other ranks
    mj.loss = LossInputs{t.acc, t.target, t.ray_weight};
    mj.dfeat = feature_grads; mj.slabs = w.slabs; mj.grad_mlp = t.grad_mlp; mj.loss_out = t.loss_out;
    mj.ex.loss_assign = true;
    mj.ex.after_backward = grads_ready;
    if (one_launch) mj.ex.acc_out = t.acc;
    return run_mlp_backward<P, C>(mj, src, b.n_rays, B, b.cfg, b.s);
}

template <typename P, uint32_t C>
static int levels_scatter_impl(const RayBatch &b, const LevelBlocks &in, const int32_t *offsets, float *grad_emb, const AdamTail *adam, int *adam_applied) {
    using T = typename RawWord<sizeof(typename P::feat_t::store_t)>::type;          // the gradients as raw 16- or 32-bit words
    const naf_render_cfg *cfg = b.cfg;
    const uint32_t B = b.points(), n_ranks = in.n_ranks, lv_begin = in.lv.begin, lv_end = in.lv.end, nl = lv_end - lv_begin;
    const Workspace w = carve(b.ws, cfg, B);
    const SrcRays src = b.src();
    hipStream_t s = b.s;
    const uint32_t run = B / n_ranks * C;                                        // elements of one (rank, level)
    uint32_t *gmax = w.binned ? w.bin.gmax : reinterpret_cast<uint32_t *>(w.grad_acc);      // (the atomic scatter has no use for it)
    if (w.binned) {
        if (hipMemsetAsync(w.bin.overflow, 0, 34 * sizeof(uint32_t), s) != hipSuccess) return fail(NAF_ERR_LAUNCH, "levels_scatter: memset failed");      // counters + maximum
    } else if (hipMemsetAsync(gmax, 0, sizeof(uint32_t), s) != hipSuccess) return fail(NAF_ERR_LAUNCH, "levels_scatter: memset failed");
    AdamTail tail;
    const bool fuse = adam != nullptr && adam_tail_possible(cfg, w, lv_begin, lv_end);
    if (fuse) { tail = *adam; tail.overflow = w.bin.overflow; }
    if (adam_applied != nullptr) *adam_applied = fuse ? 1 : 0;
    ScatterJob sj{src, w.dfeat, offsets, grad_emb, B, cfg, w, s};
    if (fuse) sj.adam = &tail;
    // The canonical shape (two bf16 channels, 8-byte records) reads the blocks in place: pass 1 finds a point's gradient inside its
    // rank's block and takes the maximum on its way (scatter_v2.h, GradBlocks).  Other shapes, the fp32 parity mode and
    // NAF_CFG_LEVELS_GATHER_PASS keep the pass below.
    if constexpr (sizeof(T) == 2u && C == 2u) {
        const bool in_place = w.binned && scatter_v2(cfg) && (cfg->flags & NAF_CFG_LEVELS_GATHER_PASS) == 0u && in.stride % 4u == 0u &&
                              ((uintptr_t)in.blocks & 3u) == 0u && (uint64_t)n_ranks * (in.stride / 4u) < (1ull << 32) && B / n_ranks >= 2u;
        if (in_place) {
            const GradBlocks gb = make_grad_blocks(B / n_ranks, (uint32_t)(in.stride / 4u), lv_begin, gmax);
            sj.dfeat = in.blocks;
            sj.from_blocks = &gb;
            return run_hash_backward_levels<P, C>(sj, lv_begin, lv_end);
        }
    }
    const bool vec = (run * sizeof(T)) % 16u == 0u && in.stride % 16u == 0u && ((uintptr_t)in.blocks & 15u) == 0u && ((uintptr_t)w.dfeat & 15u) == 0u;
    if ((uint64_t)n_ranks * nl > 65535u) return fail(NAF_ERR_INVALID_ARGUMENT, "levels_scatter: too many (rank, level) blocks");
    const uint32_t units = vec ? run / (uint32_t)(16u / sizeof(T)) : run;
    // ~512 workgroups in all: each ends with ONE atomic on the same word, and same-address atomics retire ~12 ns apart
    const uint32_t gx = std::max<uint32_t>(1u, std::min<uint32_t>((units + 1023u) / 1024u, std::max<uint32_t>(1u, 512u / (n_ranks * nl))));
    auto kern = vec ? levels_gather_kernel<T, true> : levels_gather_kernel<T, false>;
    if (int rc = launch("levels_gather_kernel", kern, dim3(gx, n_ranks * nl), dim3(256), 0, s, (const unsigned char *)in.blocks, in.stride, (T *)w.dfeat, n_ranks, nl, run,
                        lv_begin, gmax)) return rc;
    return run_hash_backward_levels<P, C>(sj, lv_begin, lv_end);
}

#define NAF_DISPATCH_PC(FN, ...)                                                                      \
    do {                                                                                              \
        if (cfg->mlp_precision == NAF_F32) {                                                          \
            switch (cfg->C) {                                                                         \
                case 1: return FN<PrecF32, 1>(__VA_ARGS__);                                           \
                case 2: return FN<PrecF32, 2>(__VA_ARGS__);                                           \
                case 4: return FN<PrecF32, 4>(__VA_ARGS__);                                           \
                default: return FN<PrecF32, 8>(__VA_ARGS__);                                          \
            }                                                                                         \
        }                                                                                             \
        switch (cfg->C) {                                                                             \
            case 1: return FN<PrecBF16, 1>(__VA_ARGS__);                                              \
            case 2: return FN<PrecBF16, 2>(__VA_ARGS__);                                              \
            case 4: return FN<PrecBF16, 4>(__VA_ARGS__);                                              \
            default: return FN<PrecBF16, 8>(__VA_ARGS__);                                             \
        }                                                                                             \
    } while (0)

}  // namespace naf
