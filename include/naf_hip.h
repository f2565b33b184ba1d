/*
 * naf_hip.h -- C ABI of libnaf_hip.so, the MI355X (gfx950) native NAF hot path.
 *
 * This is the drop-in boundary for the reference's native operator module `_hash_encoder`
 * (reference: src/encoder/hashencoder/src/bindings.cpp:5-8, hashencoder.h:13-14) plus the fused
 * field / ray-march / optimiser entry points that replace the ATen kernels behind
 * src/render/render.py:82-212, src/network/network.py:34-58 and src/trainer.py:54-58,134-142.
 *
 * Conventions
 *   - plain pointers and sizes only; every pointer is a DEVICE pointer unless stated otherwise;
 *   - the caller allocates everything, the callee writes in place (reference ownership model,
 *     hashgrid.py:30-35,59-64); "(+=)" marks buffers the callee accumulates into (caller zeroes them);
 *   - `stream` is a hipStream_t passed as void* (NULL = legacy default stream, which is what the
 *     reference uses, hashencoder.cu:306,336);
 *   - every function returns NAF_OK (0) or a negative naf_status; naf_last_error() returns a
 *     thread-local human readable message for the last failure on the calling thread;
 *   - launches are asynchronous; no function synchronises or allocates device memory;
 *   - the library keeps NO mutable process-wide state besides the opt-in profiler (naf_profile_*): everything a call
 *     depends on is in its arguments, so it is re-entrant across threads, streams and devices.
 */
#ifndef NAF_HIP_H
#define NAF_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum naf_status {
    NAF_OK = 0,
    NAF_ERR_INVALID_ARGUMENT = -1, /* null pointer, zero size, misaligned pointer ...            */
    NAF_ERR_UNSUPPORTED = -2,      /* reference: std::runtime_error("GridEncoding: C must be 1, 2, 4, or 8.") hashencoder.cu:310,324 */
    NAF_ERR_LAUNCH = -3            /* hipGetLastError() != hipSuccess after the launch            */
} naf_status;

/* storage type of tables / features; arithmetic is always fp32 (hashencoder.cu:107-143) */
typedef enum naf_dtype { NAF_F32 = 0, NAF_F16 = 1, NAF_BF16 = 2 } naf_dtype;

/* layout of per-point feature tensors */
typedef enum naf_layout {
    NAF_LAYOUT_LBC = 0, /* [L, B, C]  level-major, what kernel_grid writes (hashencoder.cu:95)        */
    NAF_LAYOUT_BLC = 1  /* [B, L*C]   what _hash_encode.forward returns after permute (hashgrid.py:40) */
} naf_layout;

const char *naf_last_error(void);
int naf_abi_version(void);

/* Optional per-kernel timing for bench.py: when enabled, every kernel launched through this library is bracketed
 * by a pair of HIP events on ITS launch stream.  naf_profile_collect() synchronises them and writes one text line
 * per kernel ("<kernel> <launches> <total_ms>\n") into `buf`, then clears the log.  Up to 8192 launches are kept. */
int naf_profile_enable(int on);
int naf_profile_collect(char *buf, size_t buflen);

/* ------------------------------------------------------------------------------------------------
 * E6  hash_encode_forward   (replaces hashencoder.cu:373-396 / hashencoder.h:13)
 *   inputs      f32  [B, D]   in [0,1]
 *   embeddings  dtype [sum_l T_l, C]
 *   offsets     i32  [L+1]    (device)
 *   outputs     dtype, layout `out_layout`
 *   dy_dx       dtype [B, L, D, C]  written iff calc_grad_inputs != 0 (may be NULL otherwise)
 * D in {2,3}, C in {1,2,4,8} else NAF_ERR_UNSUPPORTED.
 * calc_grad_inputs: NAF_GRAD_INPUTS_NONE, NAF_GRAD_INPUTS_EXACT (d feature / d x for x in [0,1], including the level
 * scale 2^l*H-1 that the chain rule needs), or NAF_GRAD_INPUTS_REFERENCE (what hashencoder.cu:153-197 stores: the scale
 * factor is commented out there, :164-165, and the loop picks the interpolated dimensions with `nd > gd`, :170, so for
 * gd < D-1 one coordinate is never set -- the reference reads an uninitialised register there; this mode uses the base
 * corner for it, the only defined reading).
 */
#define NAF_GRAD_INPUTS_NONE 0
#define NAF_GRAD_INPUTS_EXACT 1
#define NAF_GRAD_INPUTS_REFERENCE 2
int naf_hash_encode_forward(const float *inputs, const void *embeddings, const int32_t *offsets, void *outputs,
                            uint32_t B, uint32_t D, uint32_t C, uint32_t L, uint32_t H, int calc_grad_inputs,
                            void *dy_dx, int dtype, int out_layout, void *stream);

/* E7/E8  hash_encode_backward  (replaces hashencoder.cu:398-428 / hashencoder.h:14)
 *   grad             dtype, layout `grad_layout`
 *   grad_embeddings  f32 [sum_l T_l, C]  (+=)   -- always fp32 (the reference accumulates in scalar_t)
 *   grad_inputs      f32 [B, D]          (+=)   iff calc_grad_inputs != 0
 */
int naf_hash_encode_backward(const void *grad, const float *inputs, const void *embeddings, const int32_t *offsets,
                             float *grad_embeddings, uint32_t B, uint32_t D, uint32_t C, uint32_t L, uint32_t H,
                             int calc_grad_inputs, const void *dy_dx, float *grad_inputs, int dtype, int grad_layout,
                             void *stream);

/* E7 with a workspace.  The reference scheme above -- one global float atomic per corner and channel (hashencoder.cu:257-269) --
 * runs at the memory side's request rate on MI355X (50.7 of 52.9 ms of a 16 384-ray step).  A caller that lends a
 * workspace gets the two-pass binned scatter of the training path instead: same contract (grad_embeddings += the same sums,
 * fp32; grad_inputs as above), the sums formed in a fixed order (bit-reproducible), no allocation inside the library.
 *   naf_hash_encode_workspace_bytes: bytes `naf_hash_encode_backward_ws` needs for this shape, or 0 when the shape is one the
 *       binned scatter does not cover (D = 2, C = 1 or 8, fewer than 2^13 points): then -- and whenever `workspace` is NULL or too
 *       small -- naf_hash_encode_backward_ws IS naf_hash_encode_backward.
 *   log2_hashmap_size: log2 of the largest level (encoder hyper-parameter, hashgrid.py:96); the levels described by `offsets`
 *       must not exceed it.   workspace: device memory, 256-byte aligned, contents undefined before and after the call.       */
size_t naf_hash_encode_workspace_bytes(uint32_t B, uint32_t D, uint32_t C, uint32_t L, uint32_t log2_hashmap_size, int dtype);
int naf_hash_encode_backward_ws(const void *grad, const float *inputs, const void *embeddings, const int32_t *offsets,
                                float *grad_embeddings, uint32_t B, uint32_t D, uint32_t C, uint32_t L, uint32_t H,
                                int calc_grad_inputs, const void *dy_dx, float *grad_inputs, int dtype, int grad_layout,
                                uint32_t log2_hashmap_size, void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------------
 * R2  stratified sampling along rays  (replaces the ATen ops of render.py:87-105)
 *   rays    f32 [n_rays, 8]  = origin(3) direction(3) near far   (tigre.py:248-255)
 *   t_rand  f32 [n_rays, S]  jitter in [0,1) or NULL; with NULL and perturb != 0 the jitter is the
 *           counter-based generator naf_jitter(seed, ray, sample) documented in DESIGN.md
 *   z_vals  f32 [n_rays, S]  out
 *   pts     f32 [n_rays, S, 3] out, clamped to +-(bound - 1e-6); NULL: depths only
 */
int naf_sample_rays(const float *rays, const float *t_rand, float *z_vals, float *pts, uint32_t n_rays,
                    uint32_t n_samples, int perturb, float bound, uint64_t seed, uint32_t ray_index_base,
                    void *stream);

/* R5  coarse -> fine resampling in one pass (replaces raw2outputs' weights + sample_pdf + sort, render.py:113-126,203-247):
 *   sigma        f32 [n_rays, S]        coarse network output per sample (naf_render_forward_samples)
 *   t_rand       as in naf_sample_rays: the jitter the COARSE pass used (its depths are recomputed here)
 *   u            f32 [n_rays, n_fine]   uniforms of the inverse-transform sampling, NULL with det != 0 (evenly spaced
 *                                       quantiles, render.py:228) or to use the counter-based generator
 *   z_out        f32 [n_rays, S+n_fine] the coarse depths and the new samples, sorted ascending (render.py:123)
 *   weights_out  f32 [n_rays, S]        optional: the normalised weights ("weights0" of the render dict); the division is by
 *                                       the maximum over the WHOLE call, like the reference's chunk
 *   scratch      >= 4 bytes of device memory
 * One wave per ray: the cdf is an inclusive wave prefix sum, the merge a bitonic sort in LDS.  S <= 1024, S + n_fine <= 2048. */
int naf_fine_depths(const float *rays, const float *t_rand, const float *sigma, const float *u, float *z_out, float *weights_out,
                    uint32_t n_rays, uint32_t n_samples, uint32_t n_fine, int perturb, int det, uint64_t seed,
                    uint32_t ray_index_base, void *scratch, void *stream);

/* G3/G4  ray generation (replaces the precomputed rays[N,H,W,8] of tigre.py:247-255,402-456,463-528)
 *   poses   f32 [n_projections, 3, 4]  = [R | t] of angle2pose (tigre.py:530-572), cast to fp32 like torch.Tensor(pose)
 *   pixels  i64 [n] flat pixel index  proj*H*W + row*W + col, or NULL for the dense range first_pixel .. first_pixel+n-1
 *   rays    f32 [n, 8] out (16-byte aligned): origin, direction (cone: un-normalised, tigre.py:434-437), near, far
 *   det     the detector, the one description every entry point that makes rays of a scan takes: pixel (row, col) sits at
 *           u = (col + 1/2 - det_w / 2) * du + ou along the columns and v = (row + 1/2 - det_h / 2) * dv + ov along the rows
 *           (tigre.py:423-429); a cone beam's rays leave the source through it at distance DSD, a parallel beam's leave it along
 *           the pose's axis and DSD is not read; every ray carries near and far.  HOST memory, read during the call; a null `det`
 *           is refused like any other null pointer ("<entry point>: null pointer")
 */
typedef struct naf_detector {
    uint32_t det_w, det_h;                  /* columns, rows */
    float du, dv, ou, ov, DSD, near, far;   /* metres; near/far as get_near_far */
    int32_t parallel;                       /* 0 cone, 1 parallel */
} naf_detector;
int naf_generate_rays(const float *poses, const int64_t *pixels, int64_t first_pixel, float *rays, uint64_t n,
                      uint32_t n_projections, const naf_detector *det, void *stream);

/* G6  the data side of a training step (replaces np.random.choice(..., replace=False) + the fancy-indexing gathers of
 * TIGREDataset.__getitem__, tigre.py:354-372): for each of `n_segments` projections, `rays_per_segment` DISTINCT entries of
 * its list of valid pixels (flat indices proj*H*W + row*W + col whose measured value is non-zero) are drawn uniformly at
 * random through a keyed bijection of [0, n_valid) -- draw index i -> valid[perm_seed(i)] -- then the measured value is
 * gathered and the ray generated, all in one launch and without any host round trip.
 *   pixels  i64 [n_draws] out, optional      target  f32 [n_draws] out, optional (= projections[pixel])
 *   det     the detector of naf_generate_rays (naf_detector, G3)
 *   rays    f32 [n_draws, 8] out
 * [first_draw, first_draw + n_draws) is a slice of the n_segments * rays_per_segment draws (segment-major): ranks of a
 * data-parallel job that pass the same seed each take their slice of ONE draw.  A list shorter than rays_per_segment is
 * refused with the reference's message ("Cannot take a larger sample than population when 'replace=False'"). */
#define NAF_MAX_DRAW_SEGMENTS 16
typedef struct naf_scan_draw {
    uint32_t n_segments;
    uint32_t rays_per_segment;
    const int64_t *valid[NAF_MAX_DRAW_SEGMENTS];   /* device pointers */
    uint32_t n_valid[NAF_MAX_DRAW_SEGMENTS];
} naf_scan_draw;
int naf_draw_scan_rays(const naf_scan_draw *draw, const float *poses, const float *projections, int64_t *pixels, float *target,
                       float *rays, uint32_t first_draw, uint32_t n_draws, uint32_t n_projections, const naf_detector *det, uint64_t seed,
                       void *stream);

/* R4  line integral acc = sum_s sigma_s * dist_s  (render.py:192-201), and its backward.
 *   sigma f32 [n_rays, S]; z_vals f32 [n_rays, S]; rays f32 [n_rays, 8]; acc f32 [n_rays]
 *   backward: grad_sigma[r,s] = grad_acc[r] * dist[r,s]
 */
int naf_integrate_forward(const float *sigma, const float *z_vals, const float *rays, float *acc, uint32_t n_rays,
                          uint32_t n_samples, void *stream);
int naf_integrate_backward(const float *grad_acc, const float *z_vals, const float *rays, float *grad_sigma,
                           uint32_t n_rays, uint32_t n_samples, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Fused field + ray march for the canonical NAF network (network.py:6-58 with num_layers=4,
 * hidden_dim=32, skips=[2], out_dim=1, in_dim = L*C = 32; config/NAME.yaml:7-19).
 *
 * MLP parameter block `mlp` (f32, 4225 values, row-major like nn.Linear.weight):
 *   W0[32][32] b0[32] W1[32][32] b1[32] W2[32][64] b2[32] W3[1][32] b3[1]
 * `grad_mlp` (+=) has the same layout.
 */
#define NAF_MLP_PARAMS 4225

typedef struct naf_render_cfg {
    uint32_t n_samples;      /* S (render.py:87)                                                  */
    int32_t perturb;         /* stratified jitter on/off (render.py:94-100)                       */
    float bound;             /* network bound (render.py:103, hashgrid.py:125)                    */
    uint32_t L, C, H;        /* encoder levels / level_dim / base_resolution (hashgrid.py:78-86)  */
    int32_t table_dtype;     /* naf_dtype of `embeddings`                                         */
    int32_t mlp_precision;   /* NAF_F32: exact fp32 MFMA (parity mode); NAF_BF16: bf16 MFMA, fp32 accumulate */
    int32_t last_activation; /* 0 sigmoid, 1 leaky-relu, 2 tanh, 3 none (network.py:23-32)        */
    uint64_t seed;           /* jitter seed when t_rand == NULL                                   */
    uint32_t ray_index_base; /* global index of ray 0 of this call (jitter stream is per global ray) */
    uint32_t log2_hashmap_size; /* hashgrid.py:81 (sizes the binned gradient scatter; 0 = unknown -> plain atomics) */
    int32_t scatter_mode;    /* how naf_render_backward / _train scatter the table gradient (NAF_SCATTER_*); part of the
                                cfg because the workspace layout depends on it                                      */
    uint32_t flags;          /* NAF_CFG_* bits                                                                     */
} naf_render_cfg;

#define NAF_SCATTER_AUTO 0   /* binned two-pass scatter from 2^13 points per call, plain fp32 atomics below          */
#define NAF_SCATTER_ATOMIC 1 /* always fp32 atomics: the reference's scheme (hashencoder.cu:257-269)                 */
#define NAF_SCATTER_BINNED 2 /* always the binned scatter                                                            */

#define NAF_CFG_PER_LEVEL_LAUNCHES 1u /* diagnostics: one launch per level instead of level-major grids, so that
                                         naf_profile_collect() reports per-level times (changes the workspace size) */
#define NAF_CFG_EXPLICIT_DEPTHS 2u    /* the `t_rand` argument of the naf_render_* entry points holds the sample DEPTHS
                                         z[n_rays, S] themselves (the fine pass renders at the merged, sorted depths of
                                         naf_fine_depths, render.py:123-126); `perturb` is ignored                    */
#define NAF_CFG_LEVELS_INTERLEAVED 4u /* diagnostics: the encoder walks all levels of a point tile at once instead of one
                                         level at a time chip-wide -- same results, the cache behaviour of a kernel that
                                         gathers every level of a tile (what a single fused gather+MLP kernel would see) */

#define NAF_CFG_FORWARD_FUSED 8u      /* forward-only entry points (naf_render_forward, _forward_samples, naf_field_forward, _grid):
                                         gathers + MLP + line integral in ONE kernel where the shape allows it (16 levels x 2
                                         channels, bf16 MLP operands); the [L, B, C] features then never reach HBM and the calls
                                         need no workspace (naf_forward_workspace_bytes).  Bit-identical to the two-kernel path. */
#define NAF_CFG_ENCODE_TWO_GATHERS 32u /* diagnostics: the encoder fetches the two x-neighbour corners of a cell with two gathers
                                         at every batch size instead of one 16-byte window (same results; A/B timing only) */
#define NAF_CFG_BACKWARD_ONE_WAVE_PER_SIMD 128u /* diagnostics: the MLP backward splits rays into tile ranges only up to one wave per SIMD (rounds 1-2) instead of three, and the bf16 MLP forward keeps one wave per ray at small batches (no mlp16_forward_split_kernel, no mlp16_train_kernel) */
#define NAF_CFG_ENCODE_LEVEL_MAJOR 256u /* diagnostics: the encoder never splits the XCDs into groups (see NAF_CFG_ENCODE_GROUPS_*)       */
#define NAF_CFG_ENCODE_WINDOWS 64u     /* diagnostics: the 16-byte window form at every batch size (default: below 600 000 points per
                                          call and for fp32 tables; two gathers with four points per lane in flight above)        */
#define NAF_CFG_FUSED_STORE_FEATURES 16u /* diagnostics: the fused kernel also stores the features it computed              */
#define NAF_CFG_ENCODE_GROUPS_2 512u     /* the encoder splits the eight XCDs into 2 groups that take alternate levels, so that a level's
                                            slice of the table is pulled through four L2s instead of eight (encode_kernel); without a
                                            flag the batch size decides: 4 groups below 160 000 points per call, 2 below 500 000    */
#define NAF_CFG_ENCODE_GROUPS_4 1024u    /* ... into 4 groups (levels mod 4); both flags: 8 groups, one level per XCD at a time       */
#define NAF_CFG_MIN_BUCKETS_SHIFT 13u    /* bits 13-14: the binned scatter uses at least 64 << value row buckets per level (default: as few as the
                                            reducer's LDS allows, 64 at T = 2^19).  A level-parallel rank that owns two or four levels asks
                                            for 256 / 128, so that its reducer launch has 512 workgroups that each own their rows (no split
                                            launches, the Adam tail applies) -- naf_levels_scatter                                        */
#define NAF_CFG_MIN_BUCKETS_MASK (3u << NAF_CFG_MIN_BUCKETS_SHIFT)
#define NAF_CFG_SCATTER_PAIR12 2048u     /* diagnostics: the binned scatter of the canonical shape (two bf16 channels) keeps the 12-byte pair
                                            records and the kernels of rounds 2-3 (scatter_binned.h) instead of scatter_v2.h's 8-byte ones */
#define NAF_CFG_LEVELS_GATHER_PASS 32768u /* diagnostics: naf_levels_scatter re-orders the gradient blocks into [level][point][C] with a pass of
                                            its own (rounds 3-4) even where pass 1 of the scatter can read them in place (two bf16
                                            channels) -- same results bit for bit; A/B timing and tests                              */
#define NAF_CFG_MLP_TWO_KERNELS 65536u    /* diagnostics: small bf16 training steps keep the MLP forward / backward kernel pair instead of
                                            the one launch that does both (mlp16_train_kernel) -- same results bit for bit; A/B timing
                                            and tests.  NAF_CFG_BACKWARD_ONE_WAVE_PER_SIMD describes that pair and selects it as well  */
#define NAF_CFG_TEST_TINY_BLOCKS 4096u   /* tests: the record blocks of pass 1 hold a quarter of a tile's records, so that most
                                            records take the overflow route (counted global atomics) and the reducer's Adam tail has
                                            spilled contributions to fold in                                                        */


/* Diagnostic (synchronous, host result): number of gradient contributions of the LAST binned backward on this
 * workspace that did not fit their bucket stream and were applied with plain atomics instead (still correct). */
int naf_scatter_overflow_count(const naf_render_cfg *cfg, uint64_t n_points, const void *workspace, uint32_t *count_host);

/* The same per level: counts_host[32] (host memory), entry l = records of level l that fell back to atomics. */
int naf_scatter_overflow_levels(const naf_render_cfg *cfg, uint64_t n_points, const void *workspace, uint32_t *counts_host);

/* Workspace size in bytes for naf_render_* / naf_field_forward over `n_points` points (= n_rays * n_samples for the
 * render entry points): feature and feature-gradient tensors [L, n_points, C] plus the MLP-gradient slabs. */
size_t naf_render_workspace_bytes(const naf_render_cfg *cfg, uint64_t n_points);

/* Workspace size in bytes for the FORWARD-ONLY entry points (naf_render_forward, naf_render_forward_samples,
 * naf_field_forward, naf_field_forward_grid) over `n_points` points: the [L, n_points, C] feature tensor and nothing else --
 * 64 B per point in bf16 mode, 128 B in fp32 mode, against ~1.1 KB per point of the training layout -- or 256 bytes when
 * NAF_CFG_FORWARD_FUSED applies.  A workspace of naf_render_workspace_bytes() is always large enough as well. */
size_t naf_forward_workspace_bytes(const naf_render_cfg *cfg, uint64_t n_points);

/* Forward only (eval, train.py:235-239): acc[r] = sum_s sigma(pts[r,s]) * dist[r,s]. */
int naf_render_forward(const float *rays, const float *t_rand, const void *embeddings, const int32_t *offsets,
                       const float *mlp, float *acc, uint32_t n_rays, const naf_render_cfg *cfg, void *workspace,
                       void *stream);

/* Forward with the per-sample quantities the coarse -> fine pass consumes (render.py:113-126, 203-211):
 *   sigma          f32 [n_rays, S]  network output at every sample (NULL: not wanted)
 *   optical_depth  f32 [n_rays, S]  running line integral tau[r,s] = sum_{s' <= s} sigma[r,s'] * dist[r,s'] -- an inclusive
 *                                   wave prefix sum over the samples of a ray; tau[r,S-1] == acc[r] (NULL: not wanted) */
int naf_render_forward_samples(const float *rays, const float *t_rand, const void *embeddings, const int32_t *offsets,
                               const float *mlp, float *acc, float *sigma, float *optical_depth, uint32_t n_rays,
                               const naf_render_cfg *cfg, void *workspace, void *stream);

/* Backward of naf_render_forward for an arbitrary upstream gradient grad_acc[r] = dLoss/dacc[r]
 * (what autograd hands to the renderer): grad_embeddings (+=), grad_mlp (+=).
 * features_valid != 0 promises that `workspace` still holds the features naf_render_forward wrote for the SAME
 * rays / t_rand / parameters; with 0 they are recomputed first.
 */
int naf_render_backward(const float *rays, const float *t_rand, const float *grad_acc, const void *embeddings,
                        const int32_t *offsets, const float *mlp, float *grad_embeddings, float *grad_mlp, uint32_t n_rays,
                        const naf_render_cfg *cfg, void *workspace, int features_valid, void *stream);

/* Training step body (train.py:69-127 + trainer.py:134-142 minus the optimiser):
 *   acc = render(rays); loss = sum_r weight[r] * (acc[r] - target[r])^2  with weight[r] = mask/len
 *   (the caller encodes the reference's masked chunk means in `ray_weight`);
 *   grad_embeddings (+=), grad_mlp (+=), loss_out[0] (+=).
 */
int naf_render_train(const float *rays, const float *t_rand, const float *target, const float *ray_weight,
                     const void *embeddings, const int32_t *offsets, const float *mlp, float *acc,
                     float *grad_embeddings, float *grad_mlp, float *loss_out, uint32_t n_rays,
                     const naf_render_cfg *cfg, void *workspace, void *stream);

/* The same step for data-parallel training (one process per GPU): the levels of the table are scattered in
 * the order of `buckets`, and each bucket's event is recorded on `stream` as soon as its rows of grad_embeddings are
 * final, so the caller can all-reduce that slice (RCCL, on another stream that waits for the event) while the next
 * bucket is still being binned and reduced.  `mlp_ready` is recorded once grad_mlp and loss_out are final, which is
 * before the table scatter starts.  Events are hipEvent_t handles owned by the caller; NULL entries are skipped.
 * The buckets must be disjoint level ranges that cover [0, L).  Numerically identical to naf_render_train. */
#define NAF_MAX_GRAD_BUCKETS 16
typedef struct naf_grad_buckets {
    uint32_t n_buckets;
    uint32_t level_begin[NAF_MAX_GRAD_BUCKETS];
    uint32_t level_end[NAF_MAX_GRAD_BUCKETS];
    void *ready[NAF_MAX_GRAD_BUCKETS];
    void *mlp_ready;
} naf_grad_buckets;
int naf_render_train_bucketed(const float *rays, const float *t_rand, const float *target, const float *ray_weight,
                              const void *embeddings, const int32_t *offsets, const float *mlp, float *acc,
                              float *grad_embeddings, float *grad_mlp, float *loss_out, uint32_t n_rays,
                              const naf_render_cfg *cfg, void *workspace, const naf_grad_buckets *buckets, void *stream);

/* Field query sigma(x) for a point list (volume query, train.py:246-250): pts f32 [B,3] in [-bound,bound]. */
int naf_field_forward(const float *pts, const void *embeddings, const int32_t *offsets, const float *mlp,
                      float *sigma, uint32_t B, const naf_render_cfg *cfg, void *workspace, void *stream);

/* The same on a regular grid that is generated instead of read (the volume query of train.py:246-250 on the voxel grid
 * of tigre.py:388-400): axis k holds dims[k] values numpy.linspace(start[k], stop[k], dims[k]) (float64, cast to float32
 * like the dataset does), sigma is [dims[0], dims[1], dims[2]] in 'ij' order.  Bit-identical to naf_field_forward on the
 * materialised grid; the kernel walks the grid with axis 0 fastest, which turns most gathers of the hashed levels into L1
 * hits.  start / stop / dims are HOST arrays of three; the grid must lie inside [-bound, bound].
 * `workspace_bytes` is the size of `workspace`: the grid is evaluated in as many ranges of its traversal as that buffer needs
 * (at least naf_forward_workspace_bytes(cfg, 1024); same bits for every split), so a 1024^3 query (foot_50) runs in any budget. */
int naf_field_forward_grid(const double *start, const double *stop, const uint32_t *dims, const void *embeddings,
                           const int32_t *offsets, const float *mlp, float *sigma, const naf_render_cfg *cfg, void *workspace,
                           size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------------
 * T4  Adam (torch.optim.Adam semantics, trainer.py:54: lr, betas=(0.9,0.999), eps=1e-8, no weight decay,
 * amsgrad off).  `step` is the 1-based step count.  If param_lp != NULL a low-precision copy of the
 * updated parameters (naf_dtype lp_dtype) is written too (16-bit tables keep an fp32 master).
 * If zero_grad != 0 the gradient buffer is cleared in the same pass.  param / exp_avg / exp_avg_sq / grad must be 16-byte
 * aligned when n >= 4 (fewer elements are stepped one by one: the ragged head of a row range).
 */
/* One training step of the TABLE in one call (single-GPU steps): naf_render_train whose gradient reducer applies the Adam
 * update to the table rows it has just finished instead of writing their gradient out for naf_adam_step to read back and
 * clear -- the 57 MB (T=2^19) gradient table is then neither written, re-read nor zeroed.  Same results, bit for bit, as
 * naf_render_train followed by naf_adam_step(param, exp_avg, exp_avg_sq, grad_embeddings, param_lp, lp_dtype, n, ...,
 * zero_grad = 1): `grad_embeddings` must be all zero on entry and is all zero on return; the MLP gradient is written as usual
 * (the caller steps the 4 225 MLP parameters with naf_adam_step, or hands their state over in `adam`); loss_out[0] is
 * OVERWRITTEN with this step's loss (a whole optimiser step has nothing to accumulate into; it spares the caller a clear).  Batches that take the atomic scatter
 * (< 2^13 points) or split reducer launches run the two passes one after the other inside the call.
 * `embeddings` is what the kernels gather from (the 16-bit shadow `param_lp` in 16-bit mode, `param` itself in fp32 mode). */
typedef struct naf_table_adam {
    float *param;          /* fp32 master table [rows, C] */
    float *exp_avg;        /* Adam moments, same shape */
    float *exp_avg_sq;
    void *param_lp;        /* 16-bit shadow table or NULL */
    int32_t lp_dtype;      /* NAF_F16 / NAF_BF16 when param_lp != NULL */
    uint64_t n;            /* rows * C */
    float lr, beta1, beta2, eps;
    uint32_t step;         /* 1-based */
    float grad_scale;      /* gradient multiplier (1 unless the loss was scaled) */
    /* Optional: the MLP's Adam state (4 225 fp32 values each, same hyper-parameters and step).  With mlp_param set (it must be
     * the `mlp` block the call reads) the reduction of the weight-gradient slabs applies the MLP's update itself: grad_mlp is
     * consumed (+= semantics: whatever it held is added first) and left zero, bit for bit what naf_adam_step(mlp ..., zero_grad
     * = 1) after the call would have done.  NULL: grad_mlp is written as usual and the caller steps the MLP. */
    float *mlp_param, *mlp_exp_avg, *mlp_exp_avg_sq;
} naf_table_adam;
int naf_render_train_adam(const float *rays, const float *t_rand, const float *target, const float *ray_weight,
                          const void *embeddings, const int32_t *offsets, const float *mlp, float *acc, float *grad_embeddings,
                          float *grad_mlp, float *loss_out, uint32_t n_rays, const naf_render_cfg *cfg, void *workspace,
                          const naf_table_adam *adam, void *stream);

/* The same step carrying the pixel draw of the NEXT step (G6, naf_draw_scan_rays): nothing in a step depends on the next step's
 * pixels, and the draw is 6 us of latency in a launch of four workgroups, so the step takes it along in spare workgroups of the
 * scatter's first launch (the canonical two-channel bf16 shape on the binned scatter; every other shape runs it as a launch of its
 * own behind the step).  `next` holds the arguments of naf_draw_scan_rays; its rays / target buffers must not be the ones this step
 * reads (double-buffer them).  NULL: exactly naf_render_train_adam. */
typedef struct naf_next_draw {
    naf_scan_draw draw;
    const float *poses, *projections;
    int64_t *pixels;           /* optional */
    float *target;             /* optional */
    float *rays;
    uint32_t first_draw, n_draws, n_projections;
    naf_detector det;
    uint64_t seed;
} naf_next_draw;
int naf_render_train_adam_draw(const float *rays, const float *t_rand, const float *target, const float *ray_weight,
                               const void *embeddings, const int32_t *offsets, const float *mlp, float *acc, float *grad_embeddings,
                               float *grad_mlp, float *loss_out, uint32_t n_rays, const naf_render_cfg *cfg, void *workspace,
                               const naf_table_adam *adam, const naf_next_draw *next, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Level-parallel training for small steps on several GPUs (one process per GPU; no counterpart in the reference, which has no
 * distributed code -- it shards trainer.py:134-142 around train.py:48-135 like the data-parallel step does, with the same result).
 * Rank k of N owns the levels [k L/N, (k+1) L/N) of the table: their rows, Adam moments and 16-bit shadow.  A step is
 *   1. naf_levels_encode       the owned levels of EVERY rank's sample points      -> features [rank][owned levels][its points][C]
 *      all-to-all (RCCL, xGMI point to point): every rank receives all L levels of ITS points, [L][own points][C]
 *   2. naf_levels_field_step   MLP forward, loss, MLP backward on the own rays      -> feature gradients [L][own points][C],
 *                              grad_mlp (+=), loss_out (+=)   (summed over ranks by a 17 KB all-reduce)
 *      all-to-all back: every rank receives the gradients of its levels for every rank's points, one block per source rank
 *   3. naf_levels_scatter      table-gradient scatter of the owned levels over all points, Adam on their rows
 * Per rank and step 2 x (N-1)/N x points x L x C x 2 B cross the links (25 MB at the reference's 1 024 rays x 192 samples) instead
 * of the (N-1)/N x (57 + 28.5) MB a gradient exchange of the T = 2^19 table needs whatever the batch, and the optimiser pass shrinks
 * to 1/N of the table.  Above ~3 000 rays per GPU and step the gradient exchange is the smaller one (engine.py picks).
 * `rays` of calls 1 and 3 are all ranks' rays in rank order, cfg->ray_index_base the global index of the first of them, so that
 * every point gets the jitter the rank that renders it uses.  Features are bf16 (mlp_precision NAF_BF16) or fp32 (NAF_F32). */

/* features: one block per destination rank, [n_ranks][level_end - level_begin][B / n_ranks][C] (what the all-to-all sends as it is);
 * n_rays = all ranks' rays (a multiple of n_ranks), B = n_rays * n_samples points. */
int naf_levels_encode(const float *rays, const float *t_rand, const void *embeddings, const int32_t *offsets, void *features,
                      uint32_t n_rays, uint32_t n_ranks, const naf_render_cfg *cfg, uint32_t level_begin, uint32_t level_end,
                      void *stream);

/* features / feature_grads: [L][B][C] of the n_rays own rays.  acc[n_rays] is written; grad_mlp (+=) as in naf_render_train,
 * loss_out[0] is OVERWRITTEN with this rank's share of the loss.  `workspace`: naf_render_workspace_bytes(cfg, B).
 * `grads_ready` (hipEvent_t owned by the caller, or NULL) is recorded on `stream` as soon as feature_grads are final -- before the
 * reduction that finishes grad_mlp and loss_out -- so that the all-to-all of the gradients can start behind it on another stream. */
int naf_levels_field_step(const float *rays, const float *t_rand, const float *target, const float *ray_weight, const void *features,
                          const float *mlp, float *acc, void *feature_grads, float *grad_mlp, float *loss_out, uint32_t n_rays,
                          const naf_render_cfg *cfg, void *workspace, void *grads_ready, void *stream);

/* grad_blocks: n_ranks blocks `block_stride_bytes` apart, block r = [level_end - level_begin][B / n_ranks][C] feature gradients of
 * rank r's points (what the all-to-all delivers); n_rays = all ranks' rays (a multiple of n_ranks), `workspace`:
 * naf_render_workspace_bytes(cfg, B).  grad_embeddings (+=) receives the gradient of the owned levels' rows -- unless `adam` is
 * given and the reducer can apply the update itself (as in naf_render_train_adam; *adam_applied = 1): then the rows of the owned
 * levels in adam->param / exp_avg / exp_avg_sq / param_lp are stepped and grad_embeddings stays zero.  With *adam_applied = 0
 * the caller steps those rows with naf_adam_step.  adam->mlp_* are ignored (the MLP is replicated: its gradient is all-reduced).
 * With two bf16 channels (the canonical shape) the blocks are read in place by pass 1 of the scatter -- they must stay untouched until
 * the call's kernels have run; other shapes copy them into the workspace first (NAF_CFG_LEVELS_GATHER_PASS: always). */
int naf_levels_scatter(const float *rays, const float *t_rand, const void *grad_blocks, size_t block_stride_bytes, uint32_t n_ranks,
                       const int32_t *offsets, float *grad_embeddings, uint32_t n_rays, const naf_render_cfg *cfg,
                       uint32_t level_begin, uint32_t level_end, void *workspace, const naf_table_adam *adam, int *adam_applied,
                       void *stream);

int naf_adam_step(float *param, float *exp_avg, float *exp_avg_sq, float *grad, void *param_lp, int lp_dtype,
                  uint64_t n, float lr, float beta1, float beta2, float eps, uint32_t step, float grad_scale,
                  int zero_grad, void *stream);

/* E2  encoder input stage (hashgrid.py:122-125) without host round trips:
 *   out01[i] = (x[i] + size) / (2*size)   (IEEE fp32 add and divide, as torch evaluates it on the host)
 *   flag[0] |= 1 if any x[i] < -size or x[i] > size (or NaN); flag[1], flag[2] = min / max of the x[i] that are not NaN as
 *   order-preserving int32 (caller initialises flag to {0, INT32_MAX, INT32_MIN}; an input of NaN alone leaves those two).
 * out01 may be NULL (range check only).
 */
int naf_normalize_inputs(const float *x, uint64_t n, float size, float *out01, int32_t *flag, void *stream);

/* P1  forward projector: line integrals of a voxel volume (the job of TIGRE's `Ax` in the reference's
 * dataGenerator/generateData.py:178,189; bit-parity with TIGRE is not pinned).
 *   volume  f32 [n1, n2, n3], axis 0 = x, C-contiguous; voxel centres on the get_voxels grid (tigre.py:388-400), the box
 *           |p_a| <= h_a = fp32(n_a * dvoxel[a] / 2) centred at the origin (no origin offset)
 *   dvoxel  HOST f32 [3] voxel size in metres (> 0);  dims  HOST u32 [3] = n1, n2, n3 (naf_project_scan)
 *   step    target sample spacing in metres (> 0): accuracy * min(dvoxel), accuracy = 0.5 like TIGRE's geo.accuracy
 * Value at p: trilinear, clamp-to-edge inside the box, zero outside.  u_a = (p_a + h_a) / dvoxel_a - 1/2 clamped to
 * [0, n_a - 1], i_a = min(floor(u_a), n_a - 2), w_a = u_a - i_a; an axis with n_a == 1 is constant.
 * Line integral of a ray (o, d, near, far) of the [n, 8] ray format (d un-normalised for cone beams), all in fp32:
 *   [t0, t1] = slab intersection of the ray with the box, clipped to [near, far]; empty -> 0
 *   len = (t1 - t0) * |d|,  n = max(1, ceil(len / step)),  seg = (t1 - t0) / n
 *   result = (sum_{k < n} f(o + (t0 + (k + 1/2) * seg) * d)) * (len / n), summed in k order (bit-reproducible, no atomics);
 *   sample k is evaluated as fma(s_k, d, fma(t0, d, o)) with s_k = (k + 1/2) * seg, straight from k
 * naf_project_rays: rays f32 [n_rays, 8] (16-byte aligned) -> out f32 [n_rays].
 * naf_project_scan: out f32 [n_projections, det_h, det_w]; pixel (p, row, col) integrates the ray naf_generate_rays makes for
 *   flat pixel p*H*W + row*W + col (same poses, the same `det`: naf_detector, G3), generated in the kernel and never stored.
 * Empty batches (n_rays == 0, n_projections == 0) return NAF_OK without examining the pointers. */
int naf_project_rays(const float *volume, uint32_t n1, uint32_t n2, uint32_t n3, const float *dvoxel, const float *rays,
                     uint64_t n_rays, float step, float *out, void *stream);
int naf_project_scan(const float *volume, const uint32_t *dims, const float *dvoxel, const float *poses, uint32_t n_projections,
                     const naf_detector *det, float step, float *out, void *stream);

/* P2  back-projector: the transpose of P1.  With A the linear map volume -> projections of naf_project_rays / naf_project_scan,
 * these add A^T y into `volume`.
 *   values / projections  f32, one value y_r per ray: [n_rays], or [n_projections, det_h, det_w] with the rays of naf_project_scan
 *           (the same poses and `det`: naf_detector, G3)
 *   volume  f32 [n1, n2, n3] as in P1, ACCUMULATED INTO (+=): the caller zeroes it, so a scan can be back-projected in groups of views
 * Ray r takes P1's own t0, t1, len, n and seg in fp32, the same sample positions fma(s_k, d, fma(t0, d, o)) and the same trilinear
 * cell and weights (u_a clamped, i_a = min(floor(u_a), n_a - 2), w_a = u_a - i_a, an axis of one voxel constant: its w_a is 0).
 * Sample k adds y_r * (len / n) * w_c to each of its eight corner voxels c, w_c = prod_a (w_a or 1 - w_a).  A ray with an empty
 * segment adds nothing, and neither does a NaN / infinite ray for which P1 returns NaN.  Consecutive samples of a ray that share a
 * cell have their w_c summed in registers first and y_r * (len / n) applied to the sum; terms that are exactly 0 are not sent.
 * The sums into the volume are fp32 hardware float atomics, so the result equals A^T y up to rounding and SUMMATION ORDER: this is
 * the one place in the non-training kernels where two calls on the same inputs need not return the same bits.
 * All volume offsets are 64-bit.  Empty batches (n_rays == 0, n_projections == 0) return NAF_OK without examining the pointers. */
int naf_backproject_rays(const float *values, const float *rays, uint64_t n_rays, uint32_t n1, uint32_t n2, uint32_t n3,
                         const float *dvoxel, float step, float *volume, void *stream);
int naf_backproject_scan(const float *projections, const uint32_t *dims, const float *dvoxel, const float *poses,
                         uint32_t n_projections, const naf_detector *det, float step, float *volume, void *stream);

/* P3  detector-row filter: every row of a stack of projections convolved with one symmetric tap array, the ramp filter of the FDK
 * baseline (reconstruct.fdk).
 *   in, out     f32 [n_views, H, W], C-contiguous; W = detector pixels along u, the axis perpendicular to the rotation axis
 *   taps        f32 [W]: taps[m] multiplies the input m pixels away, to either side
 *   pre, post   f32 [H, W] or NULL: weights applied to the input before the sum and to the sum after it (FDK's cosine weights)
 *   view_scale  f32 [n_views] or NULL: one factor per view (FDK's angular weight and constants)
 *   out[i, r, n] = view_scale[i] * (post[r, n] * sum_{k = 0 .. W - 1} taps[|n - k|] * (pre[r, k] * in[i, r, k]))
 * a linear convolution: the row is zero outside 0 .. W - 1.  All arithmetic is fp32: x_k = pre * in is one multiply, the sum starts
 * from +0 and takes one fused multiply-add per k in ascending k, acc <- fma(taps[|n - k|], x_k, acc), then one multiply by post and
 * one by view_scale; a NULL factor is skipped.  No atomics: two calls on the same inputs return the same bits.
 * `out` may be exactly `in` (a workgroup stages its whole row before it stores); any other overlap is the caller's error.
 * The row and its taps are staged in LDS, so W is limited: W == 0 or W > NAF_FILTER_MAX_WIDTH returns NAF_ERR_INVALID_ARGUMENT and
 * launches nothing, whatever the other arguments.  Otherwise n_views * H == 0 returns NAF_OK without examining the pointers.
 * All offsets are 64-bit.  The cost is W^2 FMAs per row (the dense form; no FFT). */
#define NAF_FILTER_MAX_WIDTH 16384u
int naf_filter_rows(const float *in, uint32_t n_views, uint32_t H, uint32_t W, const float *taps, const float *pre, const float *post,
                    const float *view_scale, float *out, void *stream);
/* The same filter with one more factor, a weight per view and detector column (the short-scan weights of reconstruct.fdk, DESIGN.md
 * section 26):
 *   col         f32 [n_views, W] or NULL
 *   out[i, r, n] = view_scale[i] * (post[r, n] * sum_{k = 0 .. W - 1} taps[|n - k|] * ((pre[r, k] * in[i, r, k]) * col[i, k]))
 * x_k takes one more fp32 multiply, after pre's; everything else, the argument checks included, is naf_filter_rows, which is this
 * call with col == NULL, bit for bit. */
int naf_filter_rows_views(const float *in, uint32_t n_views, uint32_t H, uint32_t W, const float *taps, const float *pre,
                          const float *post, const float *view_scale, const float *col, float *out, void *stream);

/* P4 the subset step of OS-SART (reconstruct.os_sart): for a list s of views of a scan,
 *   x <- x + relax * C_s (.) A_s^T (R_s (.) (b_s - A_s x)),  R = 1 / (A 1),  C_s = 1 / (A_s^T 1),  then x <- max(x, 0)
 * as three launches, with A and A^T those of P1 and P2 restricted to the list.  All arithmetic is fp32, all offsets are 64-bit.
 *   view_index   DEVICE u32 [n_sub], or NULL for the identity (then n_sub <= n_scan_views).  Launch view j is scan view
 *                v = view_index[j]; the caller keeps every entry < n_scan_views (an entry that is not gives NaN in y and r and
 *                adds nothing in the transpose; nothing is read or written through it)
 *   poses        f32 [n_scan_views, 12] and  projections  f32 [n_scan_views, det_h, det_w]: the WHOLE scan, read in place
 *   y, r         f32 [n_sub, det_h, det_w], indexed by launch view
 *   det and the other geometry arguments are naf_project_scan's / naf_backproject_scan's
 * naf_sart_residual_scan: pixel (j, row, col) takes the ray naf_generate_rays makes for (v, row, col), P1's own t0, t1, len, n, sample
 *   positions and trilinear cell, and sums A x exactly as P1 does (same operations in the same order), then writes
 *     r = b - A x  (r may be NULL)  and  y = r / len,  b = projections[v, row, col], len = (t1 - t0) * |d| as P1 holds it in fp32
 *   an empty segment gives r = b and y = 0; a NaN / infinite ray, for which P1 returns NaN, gives NaN in both.  Clamp-to-edge makes
 *   the eight weights of every sample sum to 1, so the row sum (A 1)_r is n * (len / n) = len up to rounding: y is R (.) (b - A x)
 *   and no stored A 1 is needed.  No atomics: two calls return the same bits.  `projections` is only read.
 * naf_sart_backproject_scan: the transpose over the same list.  Sample k of the ray of pixel (j, row, col) adds
 *   y[j, row, col] * (len / n) * w_c to num and, where den is not NULL, (len / n) * w_c to den, for each of its eight corners c.
 *   num, den  f32 [n1, n2, n3], two different volumes, ACCUMULATED INTO.  P2's merge of consecutive samples that share a cell: one
 *   set of eight register sums serves both outputs; terms that are exactly 0 are not sent; fp32 hardware atomics, so the sums are
 *   exact up to rounding and summation order, as in P2.
 * naf_sart_update: for each of the n elements of x, num and den (4-byte aligned, no overlap)
 *     c = den_is_reciprocal ? den : (den > 0 ? 1.0f / den : 0.0f)
 *     x = x + relax * (c * num);  if nonneg: x = x < 0 ? 0 : x  (a NaN stays);  num = 0;  if zero_den: den = 0
 *   one IEEE operation at a time.  den_is_reciprocal = 1 takes `den` as a stored C_s and only reads it (zero_den must then be 0).
 *   No reduction and no atomics: two calls on the same inputs return the same bits, whatever the alignment of the three pointers.
 * Empty calls (n_sub == 0, n == 0) return NAF_OK without examining the pointers. */
int naf_sart_residual_scan(const float *volume, const uint32_t *dims, const float *dvoxel, const float *poses, uint32_t n_sub,
                           const naf_detector *det, float step, const uint32_t *view_index, uint32_t n_scan_views, const float *projections,
                           float *y, float *r, void *stream);
int naf_sart_backproject_scan(const float *y, const uint32_t *view_index, uint32_t n_sub, uint32_t n_scan_views, const uint32_t *dims,
                              const float *dvoxel, const float *poses, const naf_detector *det, float step, float *num, float *den,
                              void *stream);
int naf_sart_update(float *x, float *num, float *den, uint64_t n, float relax, int nonneg, int den_is_reciprocal, int zero_den,
                    void *stream);

/* P5  back-projector in gather form: the operator of P2 / P4's transpose, evaluated per voxel with no atomics.
 *   values       f32 [n_sub, det_h, det_w], one value y_r per ray, indexed by LAUNCH view (P4's y)
 *   view_index, n_sub, n_scan_views, poses  as in P4: launch view j is scan view v = view_index[j] (j itself when NULL, then
 *                n_sub <= n_scan_views); poses f32 [n_scan_views, 12] is the whole scan, read in place; an index >= n_scan_views
 *                adds nothing and nothing is read through it
 *   det          the detector of P1 (naf_detector, G3)
 *   volume       f32 [n1, n2, n3], ACCUMULATED INTO: volume += A_s^T values
 *   den          f32 [n1, n2, n3] or NULL, another volume, ACCUMULATED INTO: den += A_s^T 1, from the same march.  Whether den is
 *                given does not change a bit of `volume`
 *   workspace    DEVICE, 8-byte aligned, or NULL.  With one, a pre-pass writes the span (p0, d, seg, len / n, n) of every ray into
 *                it, NAF_GATHER_SPAN_BYTES per ray, and the gather reads them; the views go in groups of
 *                workspace_bytes / (NAF_GATHER_SPAN_BYTES * det_h * det_w), which must be >= 1.  Without one every span is
 *                recomputed where it is needed.  The spans are the same floats either way: the result has the same bits
 * Ray r takes P1's own t0, t1, len, n, seg, sample positions, trilinear cell and weights, as in P2.  One lane owns one voxel c and,
 * view after view in launch order, forms
 *     s_view = sum over the view's pixels in ascending (row, col) of  (y_r * (len / n)) * W_r,   W_r = sum_{k ascending} w_c(r, k)
 * in fp32 (rays with W_r == 0 are skipped; den takes (len / n) * W_r), then volume[c] = (...((volume[c] + s_1) + s_2)...).  w_c(r, k)
 * is the weight P2's sample k of ray r gives c: the same (x * y) * z product of the same w_a or 1 - w_a.  Only the pixels of c's
 * footprint rectangle and the samples of a k-range are visited (csrc/backproject_gather_device.h); both are supersets of the pairs
 * with w_c != 0, so the sums are those of A^T.  The order is fixed: two calls on the same inputs return the same bits, and so does
 * a scan split into several calls in view order.  Against P2 the result differs by rounding only (P2 sums per cell run and in
 * hardware order).  No atomics, no LDS.  All offsets are 64-bit.
 * n_sub == 0 returns NAF_OK without examining the pointers; a pixel pitch that is 0 or not finite is refused. */
#define NAF_GATHER_SPAN_BYTES 40u
int naf_backproject_scan_gather(const float *values, const uint32_t *view_index, uint32_t n_sub, uint32_t n_scan_views,
                                const uint32_t *dims, const float *dvoxel, const float *poses, const naf_detector *det, float step,
                                float *volume, float *den, void *workspace, size_t workspace_bytes, void *stream);

/* P6  ray-voxel intersection ("Siddon") forward projector: the second forward model beside P1, the one TIGRE's `Ax` takes by
 * default (bit-parity with TIGRE is not pinned).  The volume is piecewise constant: voxel (i, j, k) is the box
 *   [-h_a + i_a * dvoxel_a, -h_a + (i_a + 1) * dvoxel_a] per axis,  h_a = fp32(n_a * dvoxel_a / 2) as in P1,
 * the value is volume[i, j, k] inside it and zero outside the volume.  volume, dvoxel, dims, rays, poses and the detector `det`
 * are P1's; there is no sample step (TIGRE's geo.accuracy plays no part).
 * A ray (o, d, near, far) is clipped by the function that clips P1's (clip_ray of csrc/voxel_grid.h): the float32 slab test
 * intersected with [near, far], p0 = fma(t0, d, o), s_end = t1 - t0.  The result is
 *     sum over voxels of  volume[voxel] * (length of the clipped segment inside that voxel):  exact chord lengths.
 *   an empty span returns 0;  a non-finite p0 or s_end returns NaN;  a ray lying exactly in a voxel plane has measure zero and is
 *   attributed to one of the two neighbours (the upper one; the last voxel on the face +h_a).
 * Traversal (csrc/siddon_device.h), all in fp32, parametrised from p0 so that s runs over [0, s_end]:
 *   i0_a, i1_a = floor((p_a + h_a) * (1 / dvoxel_a)) of the two end points p0 and fma(s_end, d, p0), clamped to [0, n_a - 1];
 *   axis a has |i1_a - i0_a| plane crossings and the walk rem_x + rem_y + rem_z + 1 steps, fixed before the first of them;
 *   plane m of axis a is crossed at s = (fma((float)m, dvoxel_a, -h_a) - p0_a) / d_a, computed from m itself;
 *   each step takes the smallest next crossing among the axes that have crossings left (x before y before z on a tie; the others
 *   of a tie follow as zero-length segments), clamps it to [s_prev, s_end], loads the current voxel once and adds
 *   volume[voxel] * ((s_next - s_prev) * |d|) to an fp32 sum in traversal order;  the last step runs to s_end.
 * INVARIANT: float comparisons only choose which axis WITH crossings left steps next.  No comparison moves an index past i1_a or
 * adds a step, so a NaN or a rounding error cannot cause an out-of-range load or an unbounded loop.
 * No atomics: two calls on the same inputs return the same bits.  All volume offsets are 64-bit.
 * naf_project_rays_siddon: rays f32 [n_rays, 8] (16-byte aligned) -> out f32 [n_rays].
 * naf_project_scan_siddon: out f32 [n_projections, det_h, det_w]; pixel (p, row, col) integrates the ray naf_generate_rays makes for
 *   it, as in naf_project_scan.  Both refuse what their P1 counterparts refuse, before any launch; empty batches return NAF_OK. */
int naf_project_rays_siddon(const float *volume, uint32_t n1, uint32_t n2, uint32_t n3, const float *dvoxel, const float *rays,
                            uint64_t n_rays, float *out, void *stream);
int naf_project_scan_siddon(const float *volume, const uint32_t *dims, const float *dvoxel, const float *poses, uint32_t n_projections,
                            const naf_detector *det, float *out, void *stream);

/* P7  the transpose of P6.  Let A be P6's linear map volume -> projections.  Its entry for ray r and voxel v
 * is the fp32 number P6's walk itself forms for that step, a_rv = fl(fl(s_next - s_prev) * |d|); a ray visits a voxel at most once
 * with positive length.  These entry points add A^T y into `volume`, A^T the transpose of exactly that matrix.
 *   values / projections  f32, one value y_r per ray: [n_rays], or [n_projections, det_h, det_w] with the rays of P6's scan
 *   volume  f32 [n1, n2, n3] as in P6, ACCUMULATED INTO (+=): the caller zeroes it, as in P2
 * Ray r takes P6's own span, end-point indices, trip count, crossings and tie order (siddon_span, siddon_begin and siddon_step of
 * csrc/siddon_device.h, the functions the forward kernel runs), and each step adds fl(y_r * a_rv) to volume[v] with one fp32
 * hardware atomic.  What sends nothing:
 *   a step whose length is exactly 0, whatever y_r is (ties, the padding of the last group, the exit voxel's fixed point);
 *   a ray with y_r == 0;  an empty span;  a ray for which P6 returns NaN (non-finite p0 or s_end), as in P2.
 * A NaN or Inf y_r on a valid ray reaches exactly the voxels of positive chord length.
 * The result equals A^T y up to rounding and SUMMATION ORDER; like P2 it is not bit-reproducible.  All offsets are 64-bit.
 * P6's INVARIANT carries over: no float comparison moves an index or adds a step, so no atomic can land outside the volume.
 * Both refuse what naf_project_rays_siddon / naf_project_scan_siddon refuse, before any launch; empty batches (n_rays == 0,
 * n_projections == 0) return NAF_OK without examining the pointers.  The argument lists are P2's without the sample step. */
int naf_backproject_rays_siddon(const float *values, const float *rays, uint64_t n_rays, uint32_t n1, uint32_t n2, uint32_t n3,
                                const float *dvoxel, float *volume, void *stream);
int naf_backproject_scan_siddon(const float *projections, const uint32_t *dims, const float *dvoxel, const float *poses,
                                uint32_t n_projections, const naf_detector *det, float *volume, void *stream);

/* P8  the subset step of OS-SART on the Siddon pair (reconstruct.os_sart(kind="siddon")): P4's step with A
 * = P6 and A^T = P7 restricted to a list of views.  view_index, n_sub, n_scan_views, poses, projections, y and r are P4's (the whole
 * scan read in place, y and r indexed by launch view); the argument lists are P4's without the sample step.  All arithmetic is fp32,
 * all offsets are 64-bit.  naf_sart_update is the third launch, unchanged: it knows nothing of the projector.
 * naf_sart_residual_scan_siddon: pixel (j, row, col) takes the ray naf_generate_rays makes for (v, row, col) and walks it once as P6
 *   does (the same span, steps, grouped loads and order of additions), keeping beside  acc += volume[voxel] * a  the row sum
 *   row += a,  a = fl(fl(s_next - s_prev) * |d|).  acc has the bits naf_project_scan_siddon returns for the pixel and row the bits it
 *   returns on a volume of ones, so
 *     r = b - acc  (r may be NULL)  and  y = row > 0 ? r / row : 0,   b = projections[v, row, col]
 *   is R (.) (b - A x) with R = 1 / (A 1) of the fp32 matrix P7 defines, and no A 1 is stored or computed in a pass of its own.  An
 *   empty span gives r = b and y = 0; a non-finite span, or a view index >= n_scan_views, gives NaN in both, and nothing is read
 *   through such an index.  No atomics: two calls return the same bits.  `projections` is only read.
 * naf_sart_backproject_scan_siddon: the transpose over the same list.  Every step of positive length of the ray of pixel
 *   (j, row, col) adds fl(y * a) to num[voxel] when y = y[j, row, col] != 0 and, where den is not NULL, a to den[voxel], one no-return
 *   fp32 hardware atomic each.  A ray with y == 0 still sends its a to den.  A step of length 0, an empty or non-finite span and an
 *   out-of-range view send nothing.  num, den  f32 [n1, n2, n3], two different volumes (den == num is refused), ACCUMULATED INTO.
 *   With den == NULL the numerator has P7's terms; whether den is given changes no term sent to num.  Sums are exact up to rounding
 *   and summation order, as in P7.  P6's INVARIANT carries over: no atomic can land outside the volume.
 * Both refuse what their P4 counterparts refuse, before any launch; n_sub == 0 returns NAF_OK without examining the pointers. */
int naf_sart_residual_scan_siddon(const float *volume, const uint32_t *dims, const float *dvoxel, const float *poses, uint32_t n_sub,
                                  const naf_detector *det, const uint32_t *view_index, uint32_t n_scan_views, const float *projections,
                                  float *y, float *r, void *stream);
int naf_sart_backproject_scan_siddon(const float *y, const uint32_t *view_index, uint32_t n_sub, uint32_t n_scan_views,
                                     const uint32_t *dims, const float *dvoxel, const float *poses, const naf_detector *det,
                                     float *num, float *den, void *stream);

/* M1 3-D SSIM of two volumes: the `ssim_3d` evaluation metric of the reference (src/utils/util.py:87-139, train.py:220-288),
 * i.e. skimage.metrics.structural_similarity 0.19.3 with its defaults on the whole 3-D volume (the reference's three transposed
 * views are equal up to rounding: a cubic window makes S invariant under axis permutation).  DESIGN.md section 11.
 *   x, y  f32 [n1, n2, n3] C-contiguous, converted to fp64 on load; all arithmetic in fp64
 *   7 x 7 x 7 uniform window, N_P = 343, cov_norm = 343 / 342, R = 2 (data_range of float input), C1 = (0.01 R)^2, C2 = (0.03 R)^2
 *   box means ux, uy, uxx, uyy, uxy;  vx = cov_norm (uxx - ux^2), vy = cov_norm (uyy - uy^2), vxy = cov_norm (uxy - ux uy)
 *   S = (2 ux uy + C1)(2 vxy + C2) / ((ux^2 + uy^2 + C1)(vx + vy + C2))
 *   out[0] (fp64, DEVICE) = mean of S over the interior [3, n - 4] of every axis, (n1 - 6)(n2 - 6)(n3 - 6) windows
 * Every extent must be >= 7.  A NaN in any interior window gives NaN.  No full-size intermediate; the per-workgroup partial sums
 * go to `workspace` (naf_ssim_3d_workspace_bytes(n1, n2, n3) bytes, 8-byte aligned; 0 for an extent < 7) and are added in a
 * fixed order: two calls on the same inputs return the same bits.  No host synchronisation inside the call. */
size_t naf_ssim_3d_workspace_bytes(uint32_t n1, uint32_t n2, uint32_t n3);
int naf_ssim_3d(const float *x, const float *y, uint32_t n1, uint32_t n2, uint32_t n3, double *out, void *workspace,
                size_t workspace_bytes, void *stream);

/* V1  resize a volume with the cubic B-spline, no prefilter: the resize of the reference's `loadImage`
 * (dataGenerator/generateData.py:111-150), scipy.ndimage.zoom(order=3, prefilter=False) with its default grid.  DESIGN.md section 12.
 *   in   f32 [a1, a2, a3], out f32 [b1, b2, b3], both C-contiguous; in_dims / out_dims HOST u32 [3], every extent >= 1
 *   coordinates  output index j of an axis with a inputs and b outputs sits at x = j * r, r = (a - 1) / (b - 1) for b > 1 and
 *                r = 1 for b = 1; the division and the product are IEEE double
 *   weights      f = floor(x), t = x - f; the taps f - 1 .. f + 2 carry (1-t)^3/6, (3t^3 - 6t^2 + 4)/6, (-3t^3 + 3t^2 + 3t + 1)/6,
 *                t^3/6, formed in double and rounded to fp32 once
 *   boundary     a tap index i outside [0, a - 1] is mirrored about the edge samples (whole-sample symmetric): i mod 2(a - 1),
 *                then 2(a - 1) - i if that is >= a; an axis with a = 1 maps every tap to 0
 *   sum          out = the separable 4 x 4 x 4 weighted sum in fp32 of v = fma(in, scale, shift) (the weights sum to 1, so this
 *                equals resizing scale * in + shift); there is no prefilter: an axis with a = b is still filtered with
 *                (1/6, 4/6, 1/6), the result is a smoothing and not an interpolation
 *   minmax       NULL, or DEVICE f32 [2] = minimum and maximum of `out`; both NaN if any output is NaN.  Per-workgroup pairs go to
 *                the workspace and are folded in a fixed order (no atomics): two calls return the same bits
 * A zero extent is NAF_ERR_UNSUPPORTED.  `workspace`: naf_resize_volume_workspace_bytes(in_dims, out_dims) bytes (0 for a null
 * pointer or a zero extent), 16-byte aligned; it holds the per-axis tap tables and the per-workgroup pairs.  No full-size
 * intermediate, no host synchronisation inside the call.  Offsets are 64-bit (a 1024^3 output is 4 GiB). */
size_t naf_resize_volume_workspace_bytes(const uint32_t *in_dims, const uint32_t *out_dims);
int naf_resize_volume(const float *in, const uint32_t *in_dims, float scale, float shift, float *out, const uint32_t *out_dims,
                      float *minmax, void *workspace, size_t workspace_bytes, void *stream);

/* V2  3-D total variation of a volume, its gradient, and normalised steepest descent on it: the regulariser of the ASD-POCS
 * baseline (TIGRE's minimizeTV, which the reference's baselines used).  DESIGN.md section 14.
 *   f  f32 [n1, n2, n3] C-contiguous, every extent >= 1;  eps > 0 and finite (TIGRE's value is 1e-8)
 *   D_a f[v] = f[v] - f[v - e_a] if v_a > 0, else 0                  (a = 0, 1, 2: backward differences)
 *   m[v]     = sqrt(eps + (D_0 f[v])^2 + (D_1 f[v])^2 + (D_2 f[v])^2)
 *   TV(f)    = sum_v m[v]
 *   g[v]     = dTV/df[v] = (D_0 + D_1 + D_2) f[v] / m[v]  -  sum_a [v_a < n_a - 1] D_a f[v + e_a] / m[v + e_a]
 * g is the exact gradient of TV as written: there is no separate boundary rule, an axis of extent 1 contributes nothing, g of a
 * (1, 1, 1) volume is 0, and |g[v]| <= sqrt(3) + 3.  All per-voxel arithmetic is fp32, one IEEE operation at a time in the order
 * of csrc/tv_device.h (squares added in axis order, the three neighbour terms subtracted in axis order, true divisions).
 *   stats    DEVICE f64 [2]: stats[0] = TV(f) = sum of (double)m[v], stats[1] = sum of (double)g[v]^2.  Per-workgroup partial sums
 *            go to `workspace` and are added in a fixed order (no atomics): two calls on the same input return the same bits
 * naf_tv_gradient writes g to `grad` (f32 [n1, n2, n3], not x itself) and the two sums of x to `stats`.
 * naf_tv_descent runs n_steps times  f <- f - s g(f),  s = step / fp32(sqrt(sum g(f)^2))  (s = 0 when that sum is not > 0: a volume
 * whose gradient vanishes stays as it is, nothing becomes NaN), each step as f[v] - s * g[v] in fp32.  The steps alternate between
 * `x` and `scratch` (f32 [n1, n2, n3], not x itself; contents lost); the result ends in `x` whatever the parity of n_steps (an
 * odd count starts from a device copy of x in scratch).  `stats` receives the two sums of the volume BEFORE THE LAST STEP.
 * n_steps = 0 returns NAF_OK and touches nothing.  step must be finite and >= 0.
 * `workspace`: naf_tv_workspace_bytes(n1, n2, n3) bytes (0 for a zero extent), 8-byte aligned.  No full-size intermediate (a descent
 * step reads the volume twice and writes it once), no allocation and no host synchronisation inside the calls.  All volume offsets
 * are 64-bit. */
size_t naf_tv_workspace_bytes(uint32_t n1, uint32_t n2, uint32_t n3);
int naf_tv_gradient(const float *x, uint32_t n1, uint32_t n2, uint32_t n3, float eps, float *grad, double *stats, void *workspace,
                    size_t workspace_bytes, void *stream);
int naf_tv_descent(float *x, float *scratch, uint32_t n1, uint32_t n2, uint32_t n3, float step, uint32_t n_steps, float eps,
                   double *stats, void *workspace, size_t workspace_bytes, void *stream);

/* V3  the proximal map of the exact isotropic total variation (no eps), optionally with x >= 0: the regulariser step of the FISTA-TV
 * baseline (reconstruct.fista_tv) and a denoiser on its own (tv.tv_prox).  DESIGN.md section 18.
 *   b  f32 [n1, n2, n3] C-contiguous, every extent >= 1;  p, r, r_next  f32 [3, n1, n2, n3] (the dual variable, one plane per axis)
 *   D_a f[v]   = f[v] - f[v - e_a] if v_a > 0, else 0                                   (the differences of V2)
 *   TV(f)      = sum_v sqrt((D_0 f[v])^2 + (D_1 f[v])^2 + (D_2 f[v])^2)
 *   (D^T p)[v] = sum_a ( [v_a > 0] p_a[v] - [v_a < n_a - 1] p_a[v + e_a] )
 *   P_C(t)     = t, or with `nonneg`  t < 0 ? 0 : t  (a NaN stays NaN)
 *   prox_{lambda TV + C}(b) = P_C(b - lambda D^T p*), p* the limit of the fast gradient projection of Beck and Teboulle (2009).
 * The masks are applied on every read: whatever lies in p_a[v] (or r_a[v]) at v_a = 0 has no effect, and the step writes 0 there.
 * An axis of extent 1 contributes nothing.
 * naf_tv_prox_step is one iteration of that method at the extrapolated point r, with p = p_{k-1} on entry and p_k on return:
 *   u         = P_C(b - lambda D^T r)
 *   q_a[v]    = r_a[v] + (1 / (12 lambda)) D_a u[v]                                     (12 >= ||D D^T|| in 3-D)
 *   p_k[v]    = q[v] / max(1, sqrt(q_0^2 + q_1^2 + q_2^2))
 *   r_next[v] = p_k[v] + momentum (p_k[v] - p_{k-1}[v])
 * `p` is updated in place (its update is point-wise); `r` is read at neighbours, so `r_next` must be another buffer than `r`; it
 * may be NULL (the last iteration needs none).  lambda must be finite and > 0, momentum finite and >= 0: the caller forms
 * t_{k+1} = (1 + sqrt(1 + 4 t_k^2)) / 2 and momentum = (t_k - 1) / t_{k+1} in double and rounds once.
 * naf_tv_prox_primal writes x = P_C(b - lambda D^T p); x may be b itself; lambda must be finite and >= 0.
 * All arithmetic is fp32, one IEEE operation at a time without contraction, in the order of csrc/tvprox_device.h (the three terms
 * of D^T and the three squares added in axis order, true divisions).  No reduction and no atomic: two calls return the same bits.
 * A zero extent is NAF_ERR_UNSUPPORTED; any overlap of buffers other than those named above is the caller's error.  No workspace,
 * no allocation and no host synchronisation inside the calls; all offsets are 64-bit. */
int naf_tv_prox_step(const float *b, const float *r, float *p, float *r_next, uint32_t n1, uint32_t n2, uint32_t n3, float lambda,
                     float momentum, int nonneg, void *stream);
int naf_tv_prox_primal(const float *b, const float *p, float *x, uint32_t n1, uint32_t n2, uint32_t n3, float lambda, int nonneg,
                       void *stream);

/* K1  the vector half of CGLS, conjugate gradients on A^T W A x = A^T W b with one weight w_r >= 0 per ray: the Krylov baseline
 * reconstruct.cgls.  DESIGN.md section 19.  A and A^T are P1 and P2 / P5; these three entry points are everything else of an
 * iteration, and they keep its scalars on the device, so a solve is one stream of launches without a host read-back:
 *   q = A p;                     naf_cgls_wdot(q, w, .., NAF_CGLS_SLOT_DELTA)          delta  = sum w q^2
 *                                naf_cgls_residual_step(r, q, w, y, .., k)             history[k] = sum w r^2;  r -= alpha q;  y = w r
 *   s = A^T y;                   naf_cgls_wdot(s, NULL, .., (k + 1) & 1)               gamma' = sum s^2
 *                                naf_cgls_direction_step(x, p, s, .., k)               x += alpha p;  p = s + beta p
 * with alpha = gamma / delta and beta = gamma' / gamma, divided in fp64 and rounded to fp32 once.
 * `workspace`: naf_cgls_workspace_bytes(n_max, n_iter_max) bytes, 8-byte aligned, for arrays of up to n_max elements and n_iter_max
 * iterations; the same n_iter_max is passed to every call.  It starts with the scalars, fp64:
 *   [0], [1]  gamma: iteration k reads gamma from slot k & 1 and gamma' from slot (k + 1) & 1, so "gamma <- gamma'" is the parity
 *   [2]       delta                                           (NAF_CGLS_SLOT_DELTA)
 *   [3]       the stop mark: 0 while running, k + 1 once iteration k was a breakdown (NAF_CGLS_SLOT_STOPPED); sticky
 *   [4 .. 7]  reserved, 0
 *   [NAF_CGLS_SCALARS + k]  history: sum w r^2 of the r that iteration k was given, k < n_iter_max
 * followed by the per-workgroup partial sums.  A workspace of zero bytes is a fresh solve (hipMemsetAsync).
 * Iteration k is live if the stop mark is 0 and gamma > 0 and delta > 0 (a NaN in either is not > 0).  If it is not, the residual
 * step sets the stop mark to k + 1 where it is still 0, and both steps leave r, x and p exactly as they are (y = w r is still
 * written, and the history slot too): once stopped, stay stopped, and no NaN or Inf is formed from gamma / 0.
 * naf_cgls_wdot: scalars[slot] <- sum_i w_i a_i^2, slot 0, 1 or 2 (w == NULL: sum a_i^2).  Each term is (double)a * (double)a, which
 * is exact, times (double)w; every workgroup adds its terms in a fixed order into one fp64 partial, and one workgroup adds the
 * partials in a fixed order: no atomics, two calls return the same bits, whatever the alignment of the pointers.  A NaN propagates.
 * naf_cgls_residual_step: r <- fma(-alpha, q, r), y <- w * r (y <- r for w == NULL), and sum w r^2 of the r that came in, by the
 * path of naf_cgls_wdot, into history slot k.  y must not be q or r; k < n_iter_max.
 * naf_cgls_direction_step: x <- fma(alpha, p, x), p <- fma(beta, p, s) in one pass that reads three arrays and writes two.
 * No launch rewrites a scalar that a workgroup of the same launch reads: the scalars are written by the single-workgroup reduce
 * that follows each pass.  All element offsets are 64-bit; n == 0 returns NAF_OK without examining the pointers; pointers are
 * 4-byte aligned (16-byte aligned ones take the float4 path, with the same bits).  No allocation, no host synchronisation. */
#define NAF_CGLS_SLOT_DELTA 2u
#define NAF_CGLS_SLOT_STOPPED 3u
#define NAF_CGLS_SCALARS 8u
size_t naf_cgls_workspace_bytes(uint64_t n_max, uint32_t n_iter_max);
int naf_cgls_wdot(const float *a, const float *w, uint64_t n, uint32_t slot, uint32_t n_iter_max, void *workspace,
                  size_t workspace_bytes, void *stream);
int naf_cgls_residual_step(float *r, const float *q, const float *w, float *y, uint64_t n, uint32_t k, uint32_t n_iter_max,
                           void *workspace, size_t workspace_bytes, void *stream);
int naf_cgls_direction_step(float *x, float *p, const float *s, uint64_t n, uint32_t k, uint32_t n_iter_max, void *workspace,
                            size_t workspace_bytes, void *stream);

/* V4  trilinear samples of a volume at world points, and the fused draw-and-sample that feeds the field fit (pretrain.fit_volume:
 * a neural field started from a reconstructed volume).  DESIGN.md section 24; the arithmetic is csrc/volume_sample_device.h.
 *   volume  f32 [n1, n2, n3] C-contiguous, axis 0 = x, every extent in 1 .. NAF_VOLUME_SAMPLE_MAX_EXTENT; voxel centres on the
 *           get_voxels grid (tigre.py:388-400), the box |p_a| <= h_a = fp32(n_a * dvoxel[a] / 2) centred at the origin, as in P1
 *   dvoxel  HOST f32 [3] voxel size in metres (> 0, finite);  dims  HOST u32 [3] = n1, n2, n3
 * Value at p: trilinear between voxel centres, clamp-to-edge EVERYWHERE (a point outside the box returns the value of the nearest
 * point of the centre hull; P1 returns zero there because it never samples outside).  The cell is P1's and P2's (voxel_cell of csrc/voxel_grid.h):
 *   u_a = (p_a + h_a) * fp32(1 / dvoxel_a) - 1/2, one add, one multiply, one subtract; clamped on the float to [0, n_a - 1];
 *   i_a = min(floor(u_a), n_a - 2), w_a = u_a - i_a (exact); an axis of one voxel is constant: its w_a is 0, it has no upper corner.
 * The eight corners are blended by seven interpolations fma(w, b, fma(-w, a, a)), axis 2 first, then axis 1, then axis 0.  A weight
 * of 0 returns a's bits and a weight of 1 b's: a point whose three u_a are whole numbers returns that voxel's bits.  At the float32 voxel centres of
 * get_voxels that is so whenever every step of u_a is exact (a voxel size that is a power of two, for one); for any other voxel size
 * the centre's u_a carries the rounding of its three operations and the value that of DESIGN.md section 24's bound.
 * The clamp is applied to the float before it becomes an index, so no load leaves the volume whatever the floats hold:
 *   a coordinate of +-infinity, or a finite one far outside, returns the edge value like any outside point;
 *   a NaN coordinate returns NaN (its index is 0, its weight NaN); the other points of the call are unaffected.
 * No atomics and no reduction: the same inputs return the same bits.  All volume offsets are 64-bit.  Pointers are 4-byte aligned.
 * naf_volume_sample_points: points f32 [n, 3] -> out f32 [n].  n == 0 returns NAF_OK without examining the pointers.
 * naf_volume_draw_sample: draws n points and samples the volume there in one pass; points_out f32 [n, 3], targets_out f32 [n].
 *   Point i of step `step` is uniform in the box [lo, hi] (HOST f32 [3] each, finite, lo <= hi, hi - lo finite):
 *     bits  = three rounds of the 32-bit finaliser m (x ^= x >> 16, x *= 0x7feb352d, x ^= x >> 15, x *= 0x846ca68b, x ^= x >> 16), all uint32:
 *             h = m(lo32(seed) ^ i * 0x9e3779b1);  h = m(h ^ hi32(seed) ^ step * 0x85ebca77 ^ 0x27d4eb2f);  bits = m(h ^ (axis + 1) * 0xc2b2ae3d)
 *     r     = (bits >> 8) * 2^-24, in [0, 1)
 *     p_a   = min(lo_a + r * (hi_a - lo_a), hi_a)     one subtract, one multiply, one add, one minimum: lo_a <= p_a <= hi_a
 *   The draw keeps no state and reads no other generator: equal arguments give equal bits, and targets_out holds exactly what
 *   naf_volume_sample_points returns for points_out.  n == 0 returns NAF_OK without examining the pointers. */
#define NAF_VOLUME_SAMPLE_MAX_EXTENT 16777216u
int naf_volume_sample_points(const float *volume, uint32_t n1, uint32_t n2, uint32_t n3, const float *dvoxel, const float *points,
                             uint64_t n, float *out, void *stream);
int naf_volume_draw_sample(const float *volume, const uint32_t *dims, const float *dvoxel, const float *lo, const float *hi,
                           uint64_t seed, uint32_t step, uint32_t n, float *points_out, float *targets_out, void *stream);

/* A1  reprojection alignment of projections: the scores of a window of integer translations of every view against its reprojection,
 * the sub-pixel peak of each score table, and the resampler that undoes a view's shift (align.py, reconstruct.align_projections).
 * DESIGN.md section 25; the arithmetic is csrc/align_device.h.
 *   views   f32 [N, H, W] C-contiguous, u along the last axis, v along the rows; H, W in 1 .. NAF_ALIGN_MAX_EXTENT
 *   shifts  f32 [N, 2] = (du, dv) in pixels; the measured view b is the ideal view p translated by +shift:
 *           b[n](r, c) ~ p[n](r - dv, c - du)
 * naf_align_shift_scores: scores f64 [N, 2 Rv + 1, 2 Ru + 1], for integer dv = j - Rv and du = i - Ru
 *     S[n, j, i] = sum_r sum_c w[n, r, c] * (b[n, r + dv, c + du] - p[n, r, c])^2,   r in [Rv, H - 1 - Rv], c in [Ru, W - 1 - Ru]:
 *   the same pixels of p and the same count for every shift, so the scores of a view are comparable.  d = b - p is one fp32
 *   subtraction; the term is ((double)d * (double)d) * (double)w (w == NULL: the square alone, all weights one).  The window is cut
 *   into tiles of 16 x 64 pixels; a tile's terms are added in row-major order into one fp64 partial per shift, and the partials of a
 *   shift in ascending tile order: no atomics, a fixed order that depends on H, W, Rv and Ru alone.  Equal inputs give equal bits,
 *   and a view's scores do not depend on the other views of the call.  0 <= R <= NAF_ALIGN_MAX_SHIFT and 2 R < extent on each axis;
 *   R = 0 searches nothing on that axis.  `workspace`: naf_align_scores_workspace_bytes(N, H, W, Rv, Ru) bytes (0 for arguments the
 *   call would refuse), 8-byte aligned; more is allowed and changes nothing.  A NaN or Inf pixel makes the scores it enters NaN or Inf.
 * naf_align_peak: scores -> shifts f32 [N, 2] and flags i32 [N].  The argmin over (j, i), ties to the lowest row-major index; per
 *   axis a with R_a > 0, the minimum off that axis' border and den = (S- - S0) + (S+ - S0) > 0: delta = 1/2 (S- - S+) / den in fp64,
 *   clamped to [-1/2, 1/2], otherwise 0;  shift_a = fp32(index_a - R_a + delta).  flags bit 0: the minimum lies on the border of the
 *   window on an axis with R_a > 0;  bit 1: a score of the view is not finite: its shift is (0, 0) and bit 0 is clear.
 * naf_align_shift_views: out[n, r, c] = views[n](r + dv_n, c + du_n) by cubic convolution (Keys, a = -1/2): 4 x 4 taps in fp32, rows
 *   first then columns, clamp-to-edge.  Per axis the shift is clamped on the float to [-(n + 1), n + 1] (beyond it every tap is the
 *   edge pixel), split into floor and fraction t, and the tap indices are clamped in integers: no load leaves the view whatever the
 *   shift holds.  The weight polynomials are factored so that K(0) = 1 and K(1) = K(2) = 0 exactly, and t = 0 copies the tap: a
 *   whole-number shift returns the source's bits (of the clamped pixel).  A NaN shift makes that view NaN and no other; +-inf is a
 *   far shift, every pixel an edge value.  out must not be views.
 * All three take the stream, allocate nothing and never synchronise; N == 0 returns NAF_OK without examining the pointers; element
 * offsets are 64-bit; float pointers are 4-byte and fp64 pointers 8-byte aligned. */
#define NAF_ALIGN_MAX_SHIFT 16u
#define NAF_ALIGN_MAX_EXTENT 16777216u
#define NAF_ALIGN_FLAG_BORDER 1
#define NAF_ALIGN_FLAG_NON_FINITE 2
size_t naf_align_scores_workspace_bytes(uint32_t N, uint32_t H, uint32_t W, uint32_t Rv, uint32_t Ru);
int naf_align_shift_scores(const float *b, const float *p, const float *w, uint32_t N, uint32_t H, uint32_t W, uint32_t Rv, uint32_t Ru,
                           void *workspace, size_t workspace_bytes, double *scores, void *stream);
int naf_align_peak(const double *scores, uint32_t N, uint32_t Rv, uint32_t Ru, float *shifts, int32_t *flags, void *stream);
int naf_align_shift_views(const float *views, const float *shifts, uint32_t N, uint32_t H, uint32_t W, float *out, void *stream);

/* A2  sinogram stripe removal by sorting (Vo, Atwood and Drakopoulos, Opt. Express 2018, algorithm 3; stripe.py).  DESIGN.md section
 * 27; the integer arithmetic is csrc/stripe_device.h.  There is no floating-point arithmetic and no float comparison: every output
 * is one of the input's bit patterns.
 *   p     f32 [N, H, W] C-contiguous: N views, H detector rows (v), W detector columns (u)
 *   size  = 2 h + 1, the width of the median window along u
 *   key(x)  the order-preserving uint32 of a float's bits: sign bit set -> all bits inverted, otherwise the sign bit set.  A total
 *           order on all bit patterns: -0 sorts before +0 and NaNs sort at the two ends by payload.
 * For every (v, u) the N pairs (key(p[i, v, u]), i) are sorted ascending, the view index breaking ties:
 *     perm[j, v, u]  the view of rank j,          s[j, v, u] = p[perm[j, v, u], v, u]
 *     m[j, v, u]     the element of rank h, by key, among s[j, v, r(u + t)], t = -h .. h, where r reflects with the edge sample
 *                    repeated (-1 -> 0, -2 -> 1, W -> W - 1, W + 1 -> W - 2); equal keys are equal bits
 *     out[perm[j, v, u], v, u] = m[j, v, u]
 * Limits, refused before any launch: 1 <= N <= NAF_STRIPE_MAX_VIEWS (perm is uint16); size odd, 3 <= size <= NAF_STRIPE_MAX_SIZE and
 * size <= W; H, W <= 2^24; pointers non-null and 4-byte aligned, the workspace 8-byte aligned.  N H W == 0 returns NAF_OK without
 * examining anything else.  out may be p: the second kernel reads only the workspace.  Non-finite inputs sort as their bits say.
 * naf_stripe_workspace_bytes: the bytes for `rows` detector rows (1 <= rows <= H): s as f32 [rows, N, W] then perm as uint16
 *   [rows, N, W], each rounded up to 8 bytes; 0 for arguments the call would refuse.
 * naf_stripe_remove_sorting: detector rows are independent; the call walks them in groups of floor(ws_bytes / bytes of one row) rows
 *   (at most H), two launches per group, and refuses a workspace smaller than one row.  Any grouping returns the same bits.  It
 *   takes the stream, allocates nothing and never synchronises; element offsets are 64-bit. */
#define NAF_STRIPE_MAX_SIZE 63u
#define NAF_STRIPE_MAX_VIEWS 4096u
size_t naf_stripe_workspace_bytes(uint32_t N, uint32_t H, uint32_t W, uint32_t rows);
int naf_stripe_remove_sorting(const float *p, uint32_t N, uint32_t H, uint32_t W, uint32_t size, void *ws, size_t ws_bytes, float *out,
                              void *stream);

/* A3  raw-frame conditioning: flat-field, zinger / dead-pixel median and -log in one launch (frames.py).  DESIGN.md section 29; the
 * per-pixel arithmetic is csrc/frames_device.h.  The inverse of the forward model of dataset.add_noise, I = i0 exp(-p), for measured
 * frames.
 *   raw        [N, H, W] C-contiguous, float32 (raw_dtype NAF_FRAMES_RAW_F32) or uint16 (NAF_FRAMES_RAW_U16, converted exactly)
 *   dark, flat f32 [H, W], one averaged frame each
 *   bad        u8 [H, W] or NULL: non-zero marks a known defective pixel
 *   size       = 2 h + 1 in {3, 5, 7}, size <= H and size <= W
 *   dif        f32 >= 0, finite;   t_min  f32 > 0, finite
 *   flags      NAF_FRAMES_LOG: write -ln;  NAF_FRAMES_CLAMP_NONNEG (only with LOG): no result below zero
 *   out        f32 [N, H, W];   counts  u32 [N, 2] (+=) or NULL
 * Per view i and pixel (v, u), every operation one IEEE fp32 operation in the order written, the division correctly rounded:
 *   1. den = flat[v,u] - dark[v,u],  num = raw[i,v,u] - dark[v,u],  t = num / den
 *   2. the pixel is bad in this view iff bad[v,u] != 0, or !(den > 0), or t is not finite ((t - t) != 0)
 *   3. the window is the size x size pixels (r(v + a), r(u + b)), a, b in [-h, h], of the same view, r the reflection of A2 (the edge
 *      sample repeated: scipy's mode="reflect"); an entry counts once per occurrence.  With c entries that are not bad, m is the one
 *      of rank (c - 1) / 2 (integer division: the lower median) in the order of A2's key of their bits; c == 0: m = 1.0f
 *   4. t' = m for a bad pixel; otherwise t' = m if (t - m) > dif (bright outliers only), else t' = t
 *   5. out = t', or with LOG  p = -logf(fmaxf(t', t_min)),  and with CLAMP_NONNEG on top  p > 0 ? p : +0  (fmaxf(p, 0) with the
 *      zero's sign pinned: -logf(1) is -0, which the clamp returns as +0)
 *   6. counts[i, 0] += the pixels of view i replaced as outliers, counts[i, 1] += those replaced as bad: summed within a workgroup and
 *      added with one integer atomic each, so equal inputs give equal counts.  The caller zeroes them.
 * Without LOG every output is a quotient of step 1 or one of the window's floats: equal inputs give equal bits, the bits of a float32
 * numpy restatement (tests/_frames_oracle.py).  With LOG the result is as accurate as the device's logf.
 * `out` must not overlap raw, dark, flat or bad: a workgroup reads the halo of its tile from `raw` while its neighbours store, so
 * aliasing is refused rather than given a workspace.
 * Refused before any launch (NAF_ERR_INVALID_ARGUMENT): a null raw, dark, flat or out; an unknown raw_dtype; H or W above 2^24; size
 * not in {3, 5, 7} or above H or W; dif or t_min not finite or out of range; unknown flag bits, or CLAMP without LOG; a float32 raw,
 * dark, flat, out or counts that is not 4-byte aligned, a uint16 raw that is not 2-byte aligned; out overlapping an input; more than
 * 2^31 - 1 tiles of NAF_FRAMES_TILE_H x NAF_FRAMES_TILE_W pixels over all views.  N H W == 0 returns NAF_OK without examining anything
 * else.  Element offsets are 64-bit.  The call takes the stream, allocates nothing and never synchronises. */
#define NAF_FRAMES_RAW_F32 0
#define NAF_FRAMES_RAW_U16 1
#define NAF_FRAMES_LOG 1u
#define NAF_FRAMES_CLAMP_NONNEG 2u
#define NAF_FRAMES_MAX_SIZE 7u
#define NAF_FRAMES_TILE_H 16u
#define NAF_FRAMES_TILE_W 64u
int naf_frames_condition(const void *raw, int raw_dtype, const float *dark, const float *flat, const uint8_t *bad, uint32_t N, uint32_t H,
                         uint32_t W, uint32_t size, float dif, float t_min, uint32_t flags, float *out, uint32_t *counts, void *stream);

/* A4  sinogram in-painting for metal artefact reduction: the pixels of a metal trace replaced, in every detector row of every view, by
 * linear interpolation between their nearest valid neighbours (LI-MAR, Kalender et al. 1987), optionally on the sinogram divided by
 * a prior's (NMAR, Meyer et al. 2010), in one launch (metal.py).  DESIGN.md section 32; the bitmap search and the per-pixel
 * arithmetic are csrc/inpaint_device.h.
 *   p, out  f32 [N, H, W] C-contiguous: N views, H detector rows (v), W detector columns (u)
 *   mask    u8 [N, H, W]: non-zero marks a pixel of the trace
 *   prior   f32 [N, H, W] or NULL: the forward projection of a prior volume;  eps  f32 > 0, finite (read only with a prior)
 *   counts  u32 [N, 2] (+=) or NULL
 * Per view i, row v and column u, every operation one IEEE fp32 operation in the order written, the divisions correctly rounded:
 *   1. g[u] = prior ? fmaxf(prior[i,v,u], eps) : 1,   q[u] = prior ? p[i,v,u] / g[u] : p[i,v,u]
 *   2. a pixel that is not masked: out gets the bits of p
 *   3. a masked pixel: L is the largest column below u of the same row and view that is not masked, R the smallest above u.
 *        both exist:    w = (float)(u - L) / (float)(R - L),  d = q[R] - q[L],  val = q[L] + w d
 *        only L (or R): val = q[L] (or q[R])
 *        out = prior ? val g[u] : val
 *        neither (the whole row is masked): out gets the bits of p
 *   4. counts[i, 0] += the pixels of view i that were replaced, counts[i, 1] += the masked pixels left as they were: summed within a
 *      workgroup and added with one integer atomic each, so equal inputs give equal counts.  The caller zeroes them.
 * Non-finite values are not special: they propagate as the arithmetic says.  Every output is a pure function of the inputs: equal
 * inputs give equal bits, the bits of a float32 numpy restatement (tests/_inpaint_oracle.py).
 * `out` may be p itself: a pixel that is not masked is only ever re-stored with its own bits, and a masked pixel is never read as a
 * neighbour (L and R are not masked, and q is read at L, R and u only), so no lane reads what another lane stores.  In place the
 * kernel skips the stores of the pixels it does not replace.  Any other overlap of `out` with p, mask or prior is refused.
 * Refused before any launch (NAF_ERR_INVALID_ARGUMENT): a null p, mask or out; W above NAF_INPAINT_MAX_W (the row's bitmap is held in
 * LDS); H above 2^24; N H above 2^31 - 1 (one workgroup per row); p, prior, out or counts not 4-byte aligned; a partial overlap; with a
 * prior, eps not finite or not above zero.  N H W == 0 returns NAF_OK without examining anything else.  Element offsets are 64-bit.
 * The call takes the stream, allocates nothing and never synchronises. */
#define NAF_INPAINT_MAX_W 16384u
int naf_inpaint_rows(const float *p, const uint8_t *mask, const float *prior, float eps, uint32_t N, uint32_t H, uint32_t W, float *out,
                     uint32_t *counts, void *stream);

/* A5  centre-of-rotation search (tomopy's find_center; Donath et al., J. Opt. Soc. Am. A 23, 2006): one slice back-projected from
 * filtered detector rows for K candidate offsets of the detector's column axis in one launch, and the two scores of every such slice
 * (center.py, reconstruct.find_center).  DESIGN.md section 34; the per-pixel arithmetic is csrc/center_device.h.
 *   q      f32 [S, N, W] C-contiguous: S slices, N views, W detector columns; filtered and FDK-weighted on the nominal geometry
 *          (naf_filter_rows).  Nothing is filtered here.
 *   trig   f32 [N, 2] = (cos a_i, sin a_i)
 *   cand   f32 [K]: candidate offsets in metres, added to ou
 *   f      f32 [S, K, n, n]: f[s, k, ix, iy] at x = (ix - (n - 1) / 2) dx + ox, y = (iy - (n - 1) / 2) dy + oy
 * The column axis is Rz(a) e_y and the source stands at DSO (cos a, sin a).  Per pixel and view, every operation one IEEE fp32
 * operation in the order written:
 *   t = y cos a - x sin a;   parallel: u* = t, w = 1;   cone: s = x cos a + y sin a, U = DSO - s, u* = DSD t / U, w = (DSO / U)^2
 *   base = (u* - ou) (1 / du) + (W / 2 - 0.5);   k = base - cand[k] / du
 *   f += w (q[floor k] + (k - floor k) (q[floor k + 1] - q[floor k]))   where 0 <= floor k <= W - 2, else nothing
 * Views are added in index order: equal inputs give equal bits.  No atomics.
 * Refused before any launch (NAF_ERR_INVALID_ARGUMENT): a null pointer; N < 1; W not in 1 .. NAF_CENTER_MAX_W; K not in 1 ..
 * NAF_CENTER_MAX_K; n above NAF_CENTER_MAX_SIZE; parallel not 0 or 1; a non-finite scalar; du, dx or dy not above zero; for a cone
 * beam DSO or DSD not above zero, or a slice whose corners reach the source's orbit; a pointer that is not 4-byte aligned; more
 * than 2^31 - 1 workgroups.  S n == 0 returns NAF_OK without examining anything else.
 *
 * naf_center_metrics: per slice s and candidate k, over the pixels within r (metres) of the slice's centre (the test is fp64:
 * ((ix - (n - 1) / 2) dx)^2 + ((iy - (n - 1) / 2) dy)^2 <= r^2),
 *   out[s, k, 0] = sum -min(f, 0)                                                     (negativity)
 *   out[s, k, 1] = sum |f[ix + 1, iy] - f[ix, iy]| + |f[ix, iy + 1] - f[ix, iy]|      (sharpness; both ends inside the circle)
 * f64 [S, K, 2], summed in fp64 in a fixed order (per-workgroup partials in `workspace`, then one pass in index order): equal
 * inputs give equal bits.  No atomics.  workspace: at least naf_center_metrics_workspace_bytes(S, K, n) bytes, 8-byte aligned.
 * Refused: a null pointer; n above NAF_CENTER_MAX_SIZE; dx, dy not finite or not above zero; r not finite or below zero; f not
 * 4-byte, out or workspace not 8-byte aligned; a workspace that is too small.  S K == 0 returns NAF_OK.
 * Both calls take the stream, allocate nothing and never synchronise. */
#define NAF_CENTER_MAX_W 16384u
#define NAF_CENTER_MAX_K 64u
#define NAF_CENTER_MAX_SIZE 4096u
#define NAF_CENTER_GROUP 8u
int naf_center_slices(const float *q, const float *trig, const float *cand, uint32_t S, uint32_t N, uint32_t W, uint32_t K, uint32_t n,
                      int parallel, float DSO, float DSD, float du, float ou, float dx, float dy, float ox, float oy, float *f,
                      void *stream);
size_t naf_center_metrics_workspace_bytes(uint32_t S, uint32_t K, uint32_t n);
int naf_center_metrics(const float *f, uint32_t S, uint32_t K, uint32_t n, float dx, float dy, float r, double *out, void *workspace,
                       size_t workspace_bytes, void *stream);

/* naf_center_slices_tilted: the same search for a tilted-axis (laminographic) parallel beam, where a candidate is an offset of the
 * detector's column axis and a tilt, and a slice is a height z (center.slices_tilted, reconstruct.find_center_tilted).
 * DESIGN.md section 35; the per-pixel arithmetic is csrc/center_tilted_device.h.  The scores are naf_center_metrics.
 *   q      f32 [N, H, W] C-contiguous on the device: whole filtered views (naf_filter_rows on the nominal geometry)
 *   trig   f32 [N, 2] = (cos a_i, sin a_i), on the device
 *   cand_host  f32 [K, 3] = (c_k / du, sin tau_k, cos tau_k) in HOST memory, the one array here that is: c_k the offset added
 *          to ou, in detector pixels; read before the call returns and passed to the kernel by value, so that a candidate can be
 *          refused without a device read
 *   z      f32 [S] on the device: the slices' heights in metres
 *   f      f32 [S, K, n, n] on the device, pixel centres as in naf_center_slices
 * The conventions are geometry.angle2pose's for mode "parallel": column axis (-sin a, cos a, 0), row axis (sin tau cos a,
 * sin tau sin a, -cos tau).  Per pixel, view and candidate, every operation one IEEE fp32 operation in the order written:
 *   t = y cos a - x sin a;   s = x cos a + y sin a;   base = (t - ou) (1 / du) + (W / 2 - 0.5);   k = base - cand_host[k][0]
 *   v = sin tau_k s - cos tau_k z;   r = (v - ov) (1 / dv) + (H / 2 - 0.5)
 *   acc += bilinear(q_i; r, k): linear along the columns in rows floor r and floor r + 1, then between them, where
 *          0 <= floor k <= W - 2 and 0 <= floor r <= H - 2, else nothing
 *   f = cos tau_k acc
 * Views are added in index order: equal inputs give equal bits.  No atomics.
 * Refused before any launch (NAF_ERR_INVALID_ARGUMENT): a null pointer; S < 1; N < 1; H not in 2 .. 2^24; W not in 2 ..
 * NAF_CENTER_MAX_W; K not in 1 .. NAF_CENTER_MAX_K; n above NAF_CENTER_MAX_SIZE; a non-finite scalar or candidate; du, dv, dx or dy
 * not above zero; a candidate whose sin^2 + cos^2 is further than 1e-3 from 1; a pointer that is not 4-byte aligned; more than
 * 2^31 - 1 workgroups.  n == 0 returns NAF_OK after these checks.  Takes the stream, allocates nothing and never synchronises. */
int naf_center_slices_tilted(const float *q, const float *trig, const float *cand_host, const float *z, uint32_t S, uint32_t N, uint32_t H,
                             uint32_t W, uint32_t K, uint32_t n, float du, float dv, float ou, float ov, float dx, float dy, float ox,
                             float oy, float *f, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* NAF_HIP_H */
