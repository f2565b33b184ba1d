// render_fused.hip -- fused NAF ray-march pipeline for gfx950: rays -> samples -> hash features -> sigma-MLP (MFMA)
// -> attenuation line integral -> masked MSE gradient -> MLP backward (MFMA) -> hash-table scatter.
//
// Replaces the ATen / cuBLAS kernel soup behind reference src/render/render.py:82-212, src/network/network.py:34-58,
// src/loss/loss.py:37-39 and the autograd of train.py:69-127.  Points are never materialised: every kernel recomputes
// its sample position from the 32-byte ray record and the jitter (explicit t_rand or the counter-based generator).
//
// Kernels of one training step (B = n_rays * S points, feature tensors are [L, B, C]):
//   1 encode_kernel                  gathers  -> feat                 level-major, or XCD groups taking alternate levels below 500 k
//                                                                      points; 16-byte window gathers below 600 k points, two gathers above
//   2 mlp_forward_kernel             feat -> sigma -> acc[r]          one wave per ray, wave-reduced line integral
//   3 mlp_backward_kernel            feat, (acc, target, weight | d acc) -> dfeat, per-workgroup slabs: dW, loss share, max |dfeat|
//   4 scatter_bin / scatter_reduce (scatter_binned.h)   dfeat -> grad table (or, with the Adam tail, straight into the table's update),
//     no global atomics; spare workgroups of the first scatter_bin launch reduce the slabs of 3 (mlp_slabs.h): MLP gradient or the
//     MLP's Adam update, loss, gradient maximum.  hash_backward_kernel<SrcRays> (hash_kernels.h, fp32 atomics like the reference)
//     below 2^13 points per call, with mlp_grad_reduce_kernel as a launch of its own (also on data-parallel steps).
//
// This file holds the entry points (naf_hip.h) and their argument checks.  The step's source, all of it compiled here and nowhere else:
//   mlp_step_plan.h    which MLP kernel a step takes, tile ranges per ray, slabs, grids (no HIP: a host compiler reads it too)
//   mlp_tile_io.h      feature-tile loads / stores, the per-wave depth buffer, per-sample outputs, OutMap
//   mlp_kernels.h      2, 3: mlp_forward_kernel, mlp_backward_kernel (32-point tiles)
//   mlp16_kernels.h    2b, 3b, 3c, 5: the 16-point bf16 kernels, mlp16_train_kernel, mlp_grad_reduce_kernel
//   fused_forward.h    2c: fused_forward_kernel
//   levels_gather.h    levels_gather_kernel (level-parallel training)
//   render_step.h      the host drivers: workspace, launches (each through naf_host.h's launch / launch_as), the bodies of the entry points
#include <cmath>
#include <cstdio>
#include <cstring>

#include "render_step.h"

using namespace naf;

#ifdef NAF_REDUCE_STAMPS
extern "C" int naf_debug_reduce_stamps(uint32_t *host, uint32_t n_words) {      // diagnostic builds only (tools/reduce_stamps.py)
    return hipMemcpyFromSymbol(host, HIP_SYMBOL(naf::g_reduce_stamps), (size_t)std::min<uint32_t>(n_words, 2048u * 8u) * 4u) == hipSuccess ? 0 : 1;
}
#endif

extern "C" int naf_scatter_overflow_count(const naf_render_cfg *cfg, uint64_t n_points, const void *workspace, uint32_t *count_host) {
    if (!cfg || !workspace || !count_host) return fail(NAF_ERR_INVALID_ARGUMENT, "scatter_overflow_count: null pointer");
    const Workspace w = carve(const_cast<void *>(workspace), cfg, n_points);
    *count_host = 0;
    if (!w.binned) return NAF_OK;
    if (hipMemcpy(count_host, w.bin.overflow, 4, hipMemcpyDeviceToHost) != hipSuccess) return fail(NAF_ERR_LAUNCH, "scatter_overflow_count: copy failed");
    return NAF_OK;
}

extern "C" int naf_scatter_overflow_levels(const naf_render_cfg *cfg, uint64_t n_points, const void *workspace, uint32_t *counts_host) {
    if (!cfg || !workspace || !counts_host) return fail(NAF_ERR_INVALID_ARGUMENT, "scatter_overflow_levels: null pointer");
    const Workspace w = carve(const_cast<void *>(workspace), cfg, n_points);
    std::memset(counts_host, 0, 32 * sizeof(uint32_t));
    if (!w.binned) return NAF_OK;
    if (hipMemcpy(counts_host, w.bin.overflow + 1, 32 * 4, hipMemcpyDeviceToHost) != hipSuccess) return fail(NAF_ERR_LAUNCH, "scatter_overflow_levels: copy failed");
    return NAF_OK;
}

extern "C" size_t naf_render_workspace_bytes(const naf_render_cfg *cfg, uint64_t n_points) {
    if (!cfg) return 0;
    return carve(nullptr, cfg, n_points).bytes;
}

extern "C" size_t naf_forward_workspace_bytes(const naf_render_cfg *cfg, uint64_t n_points) {
    if (!cfg) return 0;
    return forward_workspace_bytes(cfg, n_points);
}

static int check_points(uint64_t n_points) {
    if (n_points >= (1ull << 31)) return fail(NAF_ERR_INVALID_ARGUMENT, "fused field: more than 2^31 points per call; split the batch");
    return NAF_OK;
}
// NAF_CFG_EXPLICIT_DEPTHS makes t_rand the [n_rays, n_samples] depths themselves: it cannot be absent then
static int check_depths(const naf_render_cfg *cfg, const float *t_rand) {
    if ((cfg->flags & NAF_CFG_EXPLICIT_DEPTHS) != 0u && t_rand == nullptr)
        return fail(NAF_ERR_INVALID_ARGUMENT, "render: NAF_CFG_EXPLICIT_DEPTHS needs the depths in t_rand");
    return NAF_OK;
}

// The checks a ray entry point opens with, in the one order all of them keep: the cfg, the depths, the level range of a level-parallel
// call (`levels`); then, for a batch that is not empty, the buffers (`missing`: one the call needs is null) and the rank count
// (`n_ranks`, naf_levels_scatter); then n_samples >= 2 and the point count, which calls with `empty_ok` skip for an empty batch too.
enum EmptyBatch { kEmptyChecked, kEmptyOk };      // kEmptyOk: an empty batch skips the n_samples and point-count checks
static int check_ray_call(const char *who, const naf_render_cfg *cfg, const float *t_rand, uint32_t n_rays, bool missing, EmptyBatch empty_ok = kEmptyChecked,
                          const LevelRange *levels = nullptr, const uint32_t *n_ranks = nullptr) {
    if (int rc = check_cfg(cfg)) return rc;
    if (int rc = check_depths(cfg, t_rand)) return rc;
    if (levels != nullptr && (levels->begin >= levels->end || levels->end > cfg->L))
        return fail(NAF_ERR_INVALID_ARGUMENT, "levels: empty or out-of-range level range");
    if (n_rays == 0 && empty_ok == kEmptyOk) return NAF_OK;
    if (n_rays != 0 && missing) return fail_who(who, "null pointer");
    if (n_ranks != nullptr && (*n_ranks == 0 || n_rays % *n_ranks != 0))
        return fail_who(who, "every rank must contribute the same number of rays");
    if (cfg->n_samples < 2) return fail_who(who, "n_samples must be >= 2");
    return check_points((uint64_t)n_rays * cfg->n_samples);
}

// naf_table_adam -> the reducer's Adam tail, after the checks every entry point that takes one makes (`who` names it)
static int make_adam_tail(const char *who, const naf_table_adam *adam, const float *grad_embeddings, AdamTail *tail) {
    if (adam->step == 0) return fail_who(who, "step is 1-based");
    if (adam->param_lp != nullptr && adam->lp_dtype != NAF_F16 && adam->lp_dtype != NAF_BF16)
        return fail_who(who, "lp_dtype must be NAF_F16 or NAF_BF16 when param_lp is given", NAF_ERR_UNSUPPORTED);
    if (((uintptr_t)adam->param | (uintptr_t)adam->exp_avg | (uintptr_t)adam->exp_avg_sq | (uintptr_t)grad_embeddings) & 15u)
        return fail_who(who, "buffers must be 16-byte aligned");
    tail->param = adam->param; tail->m = adam->exp_avg; tail->v = adam->exp_avg_sq;
    tail->lp = adam->param_lp; tail->lp_dtype = adam->lp_dtype; tail->overflow = nullptr;
    tail->a = make_adam_args(adam->lr, adam->beta1, adam->beta2, adam->eps, adam->step, adam->grad_scale);
    return NAF_OK;
}

extern "C" int naf_render_forward(const float *rays, const float *t_rand, const void *embeddings, const int32_t *offsets,
                                  const float *mlp, float *acc, uint32_t n_rays, const naf_render_cfg *cfg, void *workspace,
                                  void *stream) {
    if (int rc = check_ray_call("render_forward", cfg, t_rand, n_rays, !rays || !embeddings || !offsets || !mlp || !acc || !workspace)) return rc;
    if (n_rays == 0) return NAF_OK;
    const RayBatch b{rays, t_rand, n_rays, cfg, workspace, (hipStream_t)stream};
    NAF_DISPATCH_PC(render_forward_impl, b, Field{embeddings, offsets, mlp}, ForwardOut{acc});
}

extern "C" int naf_render_forward_samples(const float *rays, const float *t_rand, const void *embeddings, const int32_t *offsets,
                                          const float *mlp, float *acc, float *sigma, float *optical_depth, uint32_t n_rays,
                                          const naf_render_cfg *cfg, void *workspace, void *stream) {
    if (int rc = check_ray_call("render_forward_samples", cfg, t_rand, n_rays, !rays || !embeddings || !offsets || !mlp || !acc || !workspace)) return rc;
    if (n_rays == 0) return NAF_OK;
    const RayBatch b{rays, t_rand, n_rays, cfg, workspace, (hipStream_t)stream};
    NAF_DISPATCH_PC(render_forward_impl, b, Field{embeddings, offsets, mlp}, ForwardOut{acc, sigma, optical_depth});
}

extern "C" int naf_render_backward(const float *rays, const float *t_rand, const float *grad_acc, const void *embeddings,
                                   const int32_t *offsets, const float *mlp, float *grad_embeddings, float *grad_mlp,
                                   uint32_t n_rays, const naf_render_cfg *cfg, void *workspace, int features_valid, void *stream) {
    if (int rc = check_ray_call("render_backward", cfg, t_rand, n_rays,
                                !rays || !grad_acc || !embeddings || !offsets || !mlp || !grad_embeddings || !grad_mlp || !workspace)) return rc;
    if (n_rays == 0) return NAF_OK;
    const RayBatch b{rays, t_rand, n_rays, cfg, workspace, (hipStream_t)stream};
    TrainBuffers t{};                                        // no loss: the two gradients only
    t.grad_emb = grad_embeddings; t.grad_mlp = grad_mlp;
    BackwardSource from;
    from.grad_acc = grad_acc; from.features_valid = features_valid != 0;
    NAF_DISPATCH_PC(render_backward_impl, b, Field{embeddings, offsets, mlp}, t, from, StepTail{});
}

static int check_buckets(const naf_grad_buckets *b, uint32_t L) {
    if (b->n_buckets == 0 || b->n_buckets > NAF_MAX_GRAD_BUCKETS) return fail(NAF_ERR_INVALID_ARGUMENT, "render_train_bucketed: n_buckets must be in [1, 16]");
    uint32_t seen = 0;                                       // every level exactly once (L <= 32 on the fused path)
    for (uint32_t i = 0; i < b->n_buckets; ++i) {
        if (b->level_begin[i] >= b->level_end[i] || b->level_end[i] > L) return fail(NAF_ERR_INVALID_ARGUMENT, "render_train_bucketed: empty or out-of-range bucket");
        for (uint32_t l = b->level_begin[i]; l < b->level_end[i]; ++l) {
            if (seen & (1u << l)) return fail(NAF_ERR_INVALID_ARGUMENT, "render_train_bucketed: buckets overlap");
            seen |= 1u << l;
        }
    }
    if (seen != (L >= 32u ? 0xffffffffu : (1u << L) - 1u)) return fail(NAF_ERR_INVALID_ARGUMENT, "render_train_bucketed: buckets do not cover all levels");
    return NAF_OK;
}

// The arguments every training entry point takes, named once (render_step.h).
#define NAF_TRAIN_CALL(b, f, t)                                                                \
    const RayBatch b{rays, t_rand, n_rays, cfg, workspace, (hipStream_t)stream};                \
    const Field f{embeddings, offsets, mlp};                                                     \
    const TrainBuffers t{target, ray_weight, acc, grad_embeddings, grad_mlp, loss_out}

static int render_train_entry(const RayBatch &b, const Field &f, const TrainBuffers &t, const StepTail &tail) {
    const naf_render_cfg *cfg = b.cfg;
    const naf_grad_buckets *buckets = tail.buckets;
    if (int rc = check_ray_call("render_train", cfg, b.t_rand, b.n_rays,
                                !b.rays || !t.target || !t.ray_weight || !f.emb || !f.offsets || !f.mlp || !t.acc || !t.grad_emb || !t.grad_mlp || !b.ws))
        return rc;
    if (buckets != nullptr)
        if (int rc = check_buckets(buckets, cfg->L)) return rc;
    if (b.n_rays == 0) {                                     // an empty shard still has to signal its (zero) gradients as final
        if (tail.loss_assign && t.loss_out != nullptr && hipMemsetAsync(t.loss_out, 0, 4, b.s) != hipSuccess) return fail(NAF_ERR_LAUNCH, "render_train: memset failed");
        if (buckets != nullptr) {
            if (buckets->mlp_ready && hipEventRecord((hipEvent_t)buckets->mlp_ready, b.s) != hipSuccess) return fail(NAF_ERR_LAUNCH, "render_train: event");
            for (uint32_t i = 0; i < buckets->n_buckets; ++i)
                if (buckets->ready[i] && hipEventRecord((hipEvent_t)buckets->ready[i], b.s) != hipSuccess) return fail(NAF_ERR_LAUNCH, "render_train: event");
        }
        return NAF_OK;
    }
    NAF_DISPATCH_PC(render_train_impl, b, f, t, tail);
}

extern "C" int naf_render_train(const float *rays, const float *t_rand, const float *target, const float *ray_weight,
                                const void *embeddings, const int32_t *offsets, const float *mlp, float *acc,
                                float *grad_embeddings, float *grad_mlp, float *loss_out, uint32_t n_rays,
                                const naf_render_cfg *cfg, void *workspace, void *stream) {
    NAF_TRAIN_CALL(b, f, t);
    return render_train_entry(b, f, t, StepTail{});
}

extern "C" int naf_render_train_bucketed(const float *rays, const float *t_rand, const float *target, const float *ray_weight,
                                         const void *embeddings, const int32_t *offsets, const float *mlp, float *acc,
                                         float *grad_embeddings, float *grad_mlp, float *loss_out, uint32_t n_rays,
                                         const naf_render_cfg *cfg, void *workspace, const naf_grad_buckets *buckets, void *stream) {
    if (!buckets) return fail(NAF_ERR_INVALID_ARGUMENT, "render_train_bucketed: null buckets");
    NAF_TRAIN_CALL(b, f, t);
    StepTail tail;
    tail.buckets = buckets;
    return render_train_entry(b, f, t, tail);
}

static_assert(kAdamLpF16 == NAF_F16 && kAdamLpBF16 == NAF_BF16, "adam_math.h mirrors naf_dtype");

static int render_train_adam_impl(const RayBatch &b, const Field &f, const TrainBuffers &t, const naf_table_adam *adam, DrawJob *next_draw) {
    const naf_render_cfg *cfg = b.cfg;
    if (!adam) return fail(NAF_ERR_INVALID_ARGUMENT, "render_train_adam: null adam");
    if (!adam->param || !adam->exp_avg || !adam->exp_avg_sq || !t.grad_emb) return fail(NAF_ERR_INVALID_ARGUMENT, "render_train_adam: null pointer");
    AdamTail table_adam;
    if (int rc = make_adam_tail("render_train_adam", adam, t.grad_emb, &table_adam)) return rc;
    if (int rc = check_cfg(cfg)) return rc;
    // the MLP's own update rides on the slab reduction when the caller hands over its state (an empty batch still has to step it)
    MlpAdam madam{adam->mlp_param, adam->mlp_exp_avg, adam->mlp_exp_avg_sq, table_adam.a};
    StepTail tail;
    tail.loss_assign = true;
    if (adam->mlp_param != nullptr) {
        if (!adam->mlp_exp_avg || !adam->mlp_exp_avg_sq || !t.grad_mlp) return fail(NAF_ERR_INVALID_ARGUMENT, "render_train_adam: null MLP optimiser state");
        if (adam->mlp_param != f.mlp) return fail(NAF_ERR_INVALID_ARGUMENT, "render_train_adam: mlp_param must be the parameter block the step reads (`mlp`)");
        if (b.n_rays != 0) tail.madam = &madam;
        else if (int rc = launch_adam(adam->mlp_param, adam->mlp_exp_avg, adam->mlp_exp_avg_sq, t.grad_mlp, nullptr, 0, NAF_MLP_PARAMS, table_adam.a, true, b.s)) return rc;
    }
    const uint64_t n_points = (uint64_t)b.n_rays * cfg->n_samples;
    if (b.n_rays != 0 && b.ws != nullptr && n_points < (1ull << 31) && adam_tail_possible(cfg, carve(b.ws, cfg, n_points), 0u, cfg->L)) {
        tail.adam = &table_adam;
        tail.next_draw = next_draw;
        return render_train_entry(b, f, t, tail);
    }
    // small batches (atomic scatter), split reducer launches, per-level diagnostics, empty batches: the two passes one after the other
    if (int rc = render_train_entry(b, f, t, tail)) return rc;
    return launch_adam(adam->param, adam->exp_avg, adam->exp_avg_sq, t.grad_emb, adam->param_lp, adam->lp_dtype, adam->n, table_adam.a, true, b.s);
}

extern "C" int naf_render_train_adam(const float *rays, const float *t_rand, const float *target, const float *ray_weight,
                                     const void *embeddings, const int32_t *offsets, const float *mlp, float *acc,
                                     float *grad_embeddings, float *grad_mlp, float *loss_out, uint32_t n_rays,
                                     const naf_render_cfg *cfg, void *workspace, const naf_table_adam *adam, void *stream) {
    NAF_TRAIN_CALL(b, f, t);
    return render_train_adam_impl(b, f, t, adam, /*next_draw=*/nullptr);
}

// ... and the same step carrying the pixel draw of the NEXT one (naf_hip.h): in spare workgroups of pass 1 of the binned scatter where
// the step runs it (the canonical bf16 shape), as a launch of its own behind the step everywhere else -- same results either way.
extern "C" int naf_render_train_adam_draw(const float *rays, const float *t_rand, const float *target, const float *ray_weight,
                                          const void *embeddings, const int32_t *offsets, const float *mlp, float *acc,
                                          float *grad_embeddings, float *grad_mlp, float *loss_out, uint32_t n_rays,
                                          const naf_render_cfg *cfg, void *workspace, const naf_table_adam *adam,
                                          const naf_next_draw *next, void *stream) {
    NAF_TRAIN_CALL(b, f, t);
    if (next == nullptr) return render_train_adam_impl(b, f, t, adam, /*next_draw=*/nullptr);
    if (next->rays == rays || (next->target != nullptr && next->target == target))
        return fail(NAF_ERR_INVALID_ARGUMENT, "render_train_adam_draw: the next step's rays / targets must not be the buffers this step reads");
    DrawJob job;
    if (int rc = make_draw_job(&next->draw, next->poses, next->projections, next->pixels, next->target, next->rays, next->first_draw, next->n_draws,
                               next->n_projections, &next->det, next->seed, &job)) return rc;
    if (int rc = render_train_adam_impl(b, f, t, adam, &job)) return rc;
    return launch_draw(job, (hipStream_t)stream);            // count == 0 when pass 1 took it along
}

/* ---- level-parallel training (naf_hip.h) --------------------------------------------------------------------------------- */

extern "C" int naf_levels_encode(const float *rays, const float *t_rand, const void *embeddings, const int32_t *offsets, void *features,
                                 uint32_t n_rays, uint32_t n_ranks, const naf_render_cfg *cfg, uint32_t level_begin, uint32_t level_end,
                                 void *stream) {
    const LevelRange lv{level_begin, level_end};
    if (int rc = check_ray_call("levels_encode", cfg, t_rand, n_rays, !rays || !embeddings || !offsets || !features, kEmptyChecked, &lv)) return rc;
    if (n_rays == 0) return NAF_OK;
    if (n_ranks == 0 || n_rays % n_ranks != 0) return fail(NAF_ERR_INVALID_ARGUMENT, "levels_encode: every rank must contribute the same number of rays");
    const RayBatch b{rays, t_rand, n_rays, cfg, /*workspace=*/nullptr, (hipStream_t)stream};
    NAF_DISPATCH_PC(levels_encode_impl, b, Field{embeddings, offsets, /*mlp=*/nullptr}, features, lv, n_ranks);
}

extern "C" int naf_levels_field_step(const float *rays, const float *t_rand, const float *target, const float *ray_weight, const void *features,
                                     const float *mlp, float *acc, void *feature_grads, float *grad_mlp, float *loss_out, uint32_t n_rays,
                                     const naf_render_cfg *cfg, void *workspace, void *grads_ready, void *stream) {
    if (int rc = check_ray_call("levels_field_step", cfg, t_rand, n_rays,
                                !rays || !target || !ray_weight || !features || !mlp || !acc || !feature_grads || !grad_mlp || !loss_out || !workspace, kEmptyOk))
        return rc;
    if (n_rays == 0) {
        if (grads_ready != nullptr && hipEventRecord((hipEvent_t)grads_ready, (hipStream_t)stream) != hipSuccess) return fail(NAF_ERR_LAUNCH, "levels_field_step: event");
        return NAF_OK;
    }
    const RayBatch b{rays, t_rand, n_rays, cfg, workspace, (hipStream_t)stream};
    const TrainBuffers t{target, ray_weight, acc, /*grad_emb=*/nullptr, grad_mlp, loss_out};
    NAF_DISPATCH_PC(levels_field_impl, b, features, mlp, t, feature_grads, (hipEvent_t)grads_ready);
}

extern "C" int naf_levels_scatter(const float *rays, const float *t_rand, const void *grad_blocks, size_t block_stride_bytes, uint32_t n_ranks,
                                  const int32_t *offsets, float *grad_embeddings, uint32_t n_rays, const naf_render_cfg *cfg,
                                  uint32_t level_begin, uint32_t level_end, void *workspace, const naf_table_adam *adam, int *adam_applied,
                                  void *stream) {
    if (adam_applied != nullptr) *adam_applied = 0;
    const LevelRange lv{level_begin, level_end};
    if (int rc = check_ray_call("levels_scatter", cfg, t_rand, n_rays, !rays || !grad_blocks || !offsets || !grad_embeddings || !workspace, kEmptyOk, &lv,
                                &n_ranks)) return rc;
    if (n_rays == 0) return NAF_OK;
    const size_t esz = feature_elem_bytes(cfg);
    if (block_stride_bytes < (size_t)(level_end - level_begin) * (n_rays / n_ranks) * cfg->n_samples * cfg->C * esz || block_stride_bytes % esz != 0)
        return fail(NAF_ERR_INVALID_ARGUMENT, "levels_scatter: block stride smaller than a rank's block");
    AdamTail tail;
    const AdamTail *tp = nullptr;
    if (adam != nullptr) {
        if (!adam->param || !adam->exp_avg || !adam->exp_avg_sq) return fail(NAF_ERR_INVALID_ARGUMENT, "levels_scatter: null optimiser state");
        if (int rc = make_adam_tail("levels_scatter", adam, grad_embeddings, &tail)) return rc;
        tp = &tail;
    }
    const RayBatch b{rays, t_rand, n_rays, cfg, workspace, (hipStream_t)stream};
    const LevelBlocks blocks{grad_blocks, block_stride_bytes, n_ranks, lv};
    NAF_DISPATCH_PC(levels_scatter_impl, b, blocks, offsets, grad_embeddings, tp, adam_applied);
}

extern "C" int naf_field_forward(const float *pts, const void *embeddings, const int32_t *offsets, const float *mlp,
                                 float *sigma, uint32_t B, const naf_render_cfg *cfg, void *workspace, void *stream) {
    if (int rc = check_cfg(cfg)) return rc;
    if (B != 0 && (!pts || !embeddings || !offsets || !mlp || !sigma || !workspace)) return fail(NAF_ERR_INVALID_ARGUMENT, "field_forward: null pointer");
    if (int rc = check_points(B)) return rc;
    if (B == 0) return NAF_OK;
    const SrcRaw src{pts, cfg->bound};
    NAF_DISPATCH_PC(field_forward_impl, src, Field{embeddings, offsets, mlp}, ForwardOut{sigma}, B, cfg, workspace, (hipStream_t)stream);
}

extern "C" int naf_field_forward_grid(const double *start, const double *stop, const uint32_t *dims, const void *embeddings,
                                      const int32_t *offsets, const float *mlp, float *sigma, const naf_render_cfg *cfg,
                                      void *workspace, size_t workspace_bytes, void *stream) {
    if (int rc = check_cfg(cfg)) return rc;
    if (!start || !stop || !dims || !embeddings || !offsets || !mlp || !sigma || !workspace)
        return fail(NAF_ERR_INVALID_ARGUMENT, "field_forward_grid: null pointer");
    SrcGrid src;
    uint64_t total = 1;
    for (int d = 0; d < 3; ++d) {
        if (dims[d] == 0) return fail(NAF_ERR_INVALID_ARGUMENT, "field_forward_grid: empty axis");
        // the reference raises for points outside [-bound, bound] (hashgrid.py:122-123); a grid is checked at its ends
        if (!(std::fabs(start[d]) <= (double)cfg->bound) || !(std::fabs(stop[d]) <= (double)cfg->bound))
            return fail(NAF_ERR_INVALID_ARGUMENT, "field_forward_grid: grid exceeds [-bound, bound]");
        src.start[d] = start[d];
        src.stop[d] = stop[d];
        src.step[d] = dims[d] > 1 ? (stop[d] - start[d]) / (double)(dims[d] - 1) : 0.0;      // numpy.linspace's step
        src.n[d] = dims[d];
        total *= dims[d];                                    // < 2^31 * 2^32 per step: checked before it can wrap
        if (int rc = check_points(total)) return rc;
    }
    src.bound = cfg->bound;
    // The grid is walked in ranges of its traversal order that fit the caller's workspace (every point is evaluated on its own,
    // so the ranges give the same bits as one call): a 1024^3 query needs 64 GiB of features at once, or any smaller buffer.
    const size_t per_point = forward_workspace_bytes(cfg, 1u << 20) > 256 ? (size_t)cfg->L * cfg->C * feature_elem_bytes(cfg) : 0u;
    uint64_t chunk = total;
    if (per_point != 0u) {
        if (workspace_bytes < 512u + 1024u * per_point) return fail(NAF_ERR_INVALID_ARGUMENT, "field_forward_grid: workspace too small (see naf_forward_workspace_bytes)");
        chunk = std::min<uint64_t>(total, ((workspace_bytes - 512u) / per_point) & ~(uint64_t)1023u);
    }
    for (uint64_t first = 0; first < total; first += chunk) {
        src.first = (uint32_t)first;
        const uint32_t B = (uint32_t)std::min<uint64_t>(chunk, total - first);
        ForwardOut out{sigma};
        out.omap = OutMap{src.n[0], src.n[1], src.n[2], src.first};
        const int rc = [&]() -> int { NAF_DISPATCH_PC(field_forward_impl, src, Field{embeddings, offsets, mlp}, out, B, cfg, workspace, (hipStream_t)stream); }();
        if (rc != NAF_OK) return rc;
    }
    return NAF_OK;
}
