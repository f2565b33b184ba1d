// scatter_host.h -- host side of the binned gradient scatter: the launch plan (tile shape, buckets, record blocks), the workspace
// layout and the launch driver, shared by the training path (render_step.h, compiled in render_fused.hip) and the drop-in operator with a workspace
// (hash_encode.hip: naf_hash_encode_backward_ws).
#pragma once

#include <algorithm>

#include "naf_host.h"
#include "scatter_binned.h"
#include "scatter_v2.h"

namespace naf {

static inline bool per_level_launches(const naf_render_cfg *cfg) { return (cfg->flags & NAF_CFG_PER_LEVEL_LAUNCHES) != 0u; }

constexpr uint64_t kBinMinPoints = 1u << 13;             // measured: 128 rays x 192 samples 0.62 ms (atomics) vs 0.36 ms (binned) per step
constexpr size_t kBinBudgetBytes = (size_t)40 << 30;     // record buffer per pass (HBM is 288 GB): all 16 levels of a 65 536-ray
                                                         // step fit, so the reducer gets 1024 workgroups to balance over 256 CUs

// The canonical shape (two bf16 channels) takes the compact 8-byte records and the kernels of scatter_v2.h
static inline bool scatter_v2(const naf_render_cfg *cfg) {
    return cfg->mlp_precision == NAF_BF16 && cfg->C == 2u && (cfg->flags & NAF_CFG_SCATTER_PAIR12) == 0u;
}
// bytes of a pair record (scatter_binned.h): head + two corners x C values (fp32 in parity mode, bf16 packed in pairs otherwise)
static inline size_t record_bytes(const naf_render_cfg *cfg) {
    if (scatter_v2(cfg)) return sizeof(PairFx);
    return cfg->mlp_precision == NAF_F32 ? 4u * (1u + 2u * cfg->C) : 4u * (1u + 2u * ((cfg->C + 1u) / 2u));
}
// pass-1 tile shape, the host mirror of BinShape<Rec>
static inline uint32_t bin_threads(const naf_render_cfg *cfg) { return record_bytes(cfg) <= 12 ? 512u : 256u; }
static inline uint32_t bin_points_per_thread(const naf_render_cfg *cfg) { return record_bytes(cfg) <= 20 ? 2u : 1u; }
constexpr uint32_t kBigTileLog2Nb = 7u;                  // buckets per level from which pass 1 uses its 1024-thread shape

static inline bool make_bin_plan(const naf_render_cfg *cfg, uint64_t n_points, BinPlan *plan) {
    if (cfg->scatter_mode == NAF_SCATTER_ATOMIC || cfg->log2_hashmap_size == 0 || cfg->log2_hashmap_size > 28 || n_points == 0) return false;
    if (cfg->scatter_mode == NAF_SCATTER_AUTO && n_points < kBinMinPoints) return false;
    const uint64_t maxT = 1ull << cfg->log2_hashmap_size;
    uint32_t log2_nb = 6;
    while (((maxT >> log2_nb) * cfg->C * 8u) > (128u << 10)) ++log2_nb;         // reducer rows (64-bit) must fit LDS
    // NAF_CFG_MIN_BUCKETS: more, smaller buckets on request (a bucket keeps at least 64 rows)
    const uint32_t want_nb = 6u + ((cfg->flags & NAF_CFG_MIN_BUCKETS_MASK) >> NAF_CFG_MIN_BUCKETS_SHIFT);
    const uint32_t cap_nb = cfg->log2_hashmap_size >= 12u ? cfg->log2_hashmap_size - 6u : 6u;
    log2_nb = std::max(log2_nb, std::min(want_nb, cap_nb));
    const size_t rec = record_bytes(cfg);
    // Tables of 2^20 rows per level and more need 128 .. 512 buckets (the reducer's rows must fit the LDS), which cuts a
    // 1024-point tile into runs of 8 .. 32 records -- short, ragged reads in pass 2.  With 12-byte records a 2048-point
    // tile (ONE workgroup of 1024 threads per CU instead of two of 512: the same 16 waves) still fits the LDS.
    const bool big = rec <= 12 && log2_nb >= kBigTileLog2Nb;
    const uint32_t tile = bin_threads(cfg) * bin_points_per_thread(cfg) * (big ? 2u : 1u);
    plan->tile_points = tile;
    plan->n_tiles = (uint32_t)((n_points + tile - 1) / tile);
    plan->log2_nb = log2_nb;
    // A tile's block holds four pair records per point plus the second halves of unpaired pairs: 1.6 % on average, but ALL
    // pairs of a ray that keeps an x cell with index 63 mod 64 for its whole length (seen at T = 2^22, where 1.25x was not
    // always enough).  1.375x; a tile that still fills its block spills the excess to atomics (correct, counted).  More
    // would fit the LDS next to a second workgroup, but the larger allocation measured 2-3 % slower.  A multiple of 32
    // records: blocks start on 128-byte lines.
    plan->slots = std::min<uint32_t>(65504u, ((tile * 11u / 2u) + 31u) & ~31u);
    if ((cfg->flags & NAF_CFG_TEST_TINY_BLOCKS) != 0u) plan->slots = std::max(32u, tile & ~31u);      // a quarter of a tile's records fit
    // pass 2 reads a bucket's run of a tile with W lanes: W = the power of two >= 1.25 x the mean run length, at most a wave
    const uint32_t mean_run = std::max<uint32_t>(1u, (tile * 4u) >> log2_nb);
    plan->log2_w = 3u;
    while (plan->log2_w < 6u && (1u << plan->log2_w) < mean_run + mean_run / 4u) ++plan->log2_w;
    plan->max_local_rows = (uint32_t)((((maxT + (1ull << log2_nb) - 1) >> log2_nb) + 63u) & ~63ull);
    const size_t per_level = (size_t)plan->n_tiles * plan->slots * rec;
    plan->levels_per_pass = (uint32_t)std::min<size_t>(cfg->L, std::max<size_t>(1, kBinBudgetBytes / per_level));
    if (per_level_launches(cfg)) plan->levels_per_pass = 1;
    return true;
}

// Workgroups a reducer launch over `nl` levels splits each bucket's tiles between: 1 when buckets x levels give every CU a
// workgroup (one owner per row, sums formed in a fixed order: the table gradient is bit-reproducible -- this covers the four-level
// buckets of a data-parallel step, 64 x 4 = 256), more (with per-row fp32 atomics at the end, whose order is not fixed) only when a
// pass holds fewer than four levels' worth of buckets.
static inline uint32_t reducer_split(uint32_t NB, uint32_t nl) { return NB * nl >= 256u ? 1u : std::max(1u, std::min(16u, 1024u / (NB * nl))); }

// The binned scatter's part of a workspace (the training step's: render_step.h carve(); the drop-in's: hash_encode.hip), carved
// from `base` for `plan`.
struct BinRegions {
    unsigned char *regions;      // record blocks [level slot][tile][slots], bucket-sorted per tile
    uint32_t *counts;            // run words [level slot][bucket][tile] = start | length << 16
    uint32_t *overflow;          // contributions that fell back to atomics (diagnostic counters): [0] total, [1 + level] per level
    uint32_t *gmax;              // bit pattern of max |feature gradient| of the step (fixed-point scale), right behind overflow[33]
    size_t bytes;
};

static inline BinRegions carve_bin_regions(unsigned char *base, const naf_render_cfg *cfg, const BinPlan &plan) {
    const size_t n_runs = ((size_t)plan.levels_per_pass << plan.log2_nb) * plan.n_tiles;
    const size_t block_bytes = ((size_t)plan.levels_per_pass * plan.n_tiles * plan.slots * record_bytes(cfg) + 255) & ~(size_t)255;
    BinRegions r;
    r.regions = base;
    r.counts = (uint32_t *)(base + block_bytes);
    r.overflow = r.counts + n_runs;
    r.gmax = r.overflow + 33;
    r.bytes = block_bytes + (((n_runs + 33 + 1) * 4 + 255) & ~(size_t)255);
    return r;
}

// What a launch of pass 1 is given besides the arguments its record family adds
struct BinPass {
    const int32_t *offsets;
    float *grad_table;
    const BinRegions &w;
    uint32_t H, l0, nl;          // levels [l0, l0 + nl)
    const BinPlan &plan;
    const SlabReduce &job;
};

// The launches of the binned scatter over the levels [lv_begin, lv_end): pass 1 (scatter_bin*_kernel) bins the feature gradients
// into bucket-sorted records, pass 2 (scatter_reduce*_kernel) sums each bucket's records into its rows of grad_table.  The pass
// and bucket policy is the same for every record family; `F` supplies what is not:
//   Rec, kThreads, kPoints        the record and pass 1's tile shape (BinShape); kHasBig: whether the 1024-thread shape exists
//   kLvMany, kLvFew               levels per bin workgroup when tiles are plentiful / scarce
//   bin_kernel(plan, big, many)   the pass-1 instantiation; reduce_kernel(adam): the pass-2 one
//   bin_lds(plan)                 pass 1's dynamic LDS bytes
//   launch_bin(timed, k, grid, threads, lds, s, pass)   a pass-1 launch timed as `timed`, with the family's own arguments; launch_as()'s result
// `slab_job` (training steps): the deferred slab reduction, run by spare workgroups of the first pass-1 launch (StepExtras).
// `buckets` (data parallel): each bucket's event is recorded as soon as its rows are final.
template <typename F>
static int launch_binned_scatter(F &fam, const naf_render_cfg *cfg, const BinPlan &plan, const BinRegions &w, const int32_t *offsets,
                                 float *grad_table, uint32_t lv_begin, uint32_t lv_end, const naf_grad_buckets *buckets, hipStream_t s,
                                 const AdamTail *adam = nullptr, const SlabReduce *slab_job = nullptr) {
    constexpr uint32_t NT = F::kThreads, PTS = F::kPoints;
    const bool big = F::kHasBig && plan.tile_points == 2u * NT * PTS;
    if (!big && plan.tile_points != NT * PTS) return fail(NAF_ERR_LAUNCH, "binned scatter: plan / kernel tile mismatch");
    const uint32_t threads = big ? 2u * NT : NT;
    // levels per bin workgroup: all of them when there are enough tiles to fill the chip several times over (the sample
    // position is evaluated once per point, and stores drain behind the next level: 3.85 -> 3.53 ms at 65 536 rays),
    // fewer when tiles are scarce (1 024-ray steps: 0.093 -> 0.071 ms)
    const bool many = plan.n_tiles >= (big ? 768u : 1536u);
    const uint32_t LV = many ? F::kLvMany : F::kLvFew;
    const auto bin = fam.bin_kernel(plan, big, many);
    const auto red = fam.reduce_kernel(adam);
    const AdamTail tail = adam != nullptr ? *adam : AdamTail{};
    const uint32_t NB = 1u << plan.log2_nb;
    const uint32_t red_lds = plan.max_local_rows * cfg->C * 8u, bin_lds = fam.bin_lds(plan);
    if (int rc = raise_lds_limit(red, red_lds, "binned scatter: cannot raise dynamic LDS limit (reduce)")) return rc;
    if (int rc = raise_lds_limit(bin, bin_lds, "binned scatter: cannot raise dynamic LDS limit (bin)")) return rc;
    static const char *const bin_names[32] = NAF_LEVEL_NAMES("scatter_bin_kernel_L");
    static const char *const red_names[32] = NAF_LEVEL_NAMES("scatter_reduce_kernel_L");
    const bool per_level = per_level_launches(cfg);
    SlabReduce job{};
    if (slab_job != nullptr) job = *slab_job;
    // pass 1 over the levels [l0, l0 + nl): their records fill the region buffer from level slot 0
    // (both passes are timed under a level's own name on the per-level diagnostic path; a failed launch names the kernel)
    auto launch_bin = [&](uint32_t l0, uint32_t nl) -> int {
        const uint32_t spare = job.slabs != nullptr ? kSlabReduceBlocks : 0u;
        const int rc = fam.launch_bin(per_level ? level_name(bin_names, l0) : "scatter_bin_kernel", bin, dim3(plan.n_tiles + spare, (nl + LV - 1u) / LV), threads, bin_lds, s,
                                      BinPass{offsets, grad_table, w, cfg->H, l0, nl, plan, job});
        job = SlabReduce{};
        return rc;
    };
    // pass 2 over the level slots [ly0, ly0 + nl) of a bin pass that started at level l0
    auto launch_reduce = [&](uint32_t l0, uint32_t ly0, uint32_t nl) -> int {
        // keep >= ~1024 reducer workgroups in flight: with one or two levels per pass split each bucket's tiles.
        // (A reducer workgroup owns a CU's LDS, so 256 run at a time: 512 or more unsplit ones already come in full rounds.)
        const uint32_t n_split = reducer_split(NB, nl);
        if (adam != nullptr && n_split != 1u) return fail(NAF_ERR_LAUNCH, "binned scatter: the Adam tail needs unsplit reducer launches");
        return launch_as(per_level ? level_name(red_names, l0 + ly0) : "scatter_reduce_kernel", "scatter_reduce_kernel", red, dim3(NB, nl, n_split), dim3(1024), red_lds, s,
                         (const typename F::Rec *)w.regions, w.counts, offsets, grad_table, w.gmax, l0, ly0, cfg->H, plan, tail);
    };
    if (buckets != nullptr && !per_level && plan.levels_per_pass >= cfg->L && lv_begin == 0u && lv_end == cfg->L) {
        // data parallel, and the records of all levels fit one pass: bin ONCE (the sample position is evaluated once per
        // point and the stores of a level drain behind the next, exactly as in the single-GPU step), then finish the table
        // bucket by bucket -- each bucket's event fires as soon as its rows are final, and its all-reduce overlaps the
        // reduction of the buckets that follow.
        if (int rc = launch_bin(0u, cfg->L)) return rc;
        for (uint32_t b = 0; b < buckets->n_buckets; ++b) {
            if (int rc = launch_reduce(0u, buckets->level_begin[b], buckets->level_end[b] - buckets->level_begin[b])) return rc;
            if (buckets->ready[b] != nullptr && hipEventRecord((hipEvent_t)buckets->ready[b], s) != hipSuccess)
                return fail(NAF_ERR_LAUNCH, "render_train: cannot record a bucket event");
        }
        return NAF_OK;
    }
    for (uint32_t l0 = lv_begin; l0 < lv_end; l0 += plan.levels_per_pass) {
        const uint32_t nl = std::min(plan.levels_per_pass, lv_end - l0);
        if (int rc = launch_bin(l0, nl)) return rc;
        if (int rc = launch_reduce(l0, 0u, nl)) return rc;
    }
    return NAF_OK;
}

// ---- record families ---------------------------------------------------------------------------------------------------------
// (scatter_v2.h's, FxRecords, is declared in render_step.h, which render_fused.hip alone includes: a class that is no template instantiates its kernels in every
// translation unit that declares it.)
// scatter_binned.h: pair records of fp32 values, or of bf16 ones packed in pairs, from gradients whose (level l, point b) values sit
// at grad + (l * sl + b * sb) * C.  The training path (render_step.h: fp32 parity mode, shapes with C != 2,
// NAF_CFG_SCATTER_PAIR12) and the drop-in operator (hash_encode.hip: four levels per bin workgroup at every batch size, no Adam
// tail -- so that it instantiates no reducer with one).
template <typename FT, uint32_t C, typename Src, typename R, uint32_t kLvMany_, bool kAdamTail>
struct PairRecords {
    using Rec = R;
    static constexpr uint32_t kThreads = BinShape<Rec>::kThreads, kPoints = BinShape<Rec>::kPoints, kLvMany = kLvMany_, kLvFew = 4u;
    static constexpr bool kHasBig = sizeof(Rec) <= 12;                 // the 1024-thread shape of pass 1 (make_bin_plan)
    Src src;
    const void *grad;
    uint32_t B, sl, sb;

    auto bin_kernel(const BinPlan &, bool big, bool many) const {
        constexpr uint32_t NT = kThreads, PTS = kPoints;
        auto bin = many ? scatter_bin_kernel<FT, C, Src, Rec, NT, PTS, kLvMany> : scatter_bin_kernel<FT, C, Src, Rec, NT, PTS, kLvFew>;
        if constexpr (kHasBig) {
            if (big) bin = many ? scatter_bin_kernel<FT, C, Src, Rec, 2u * NT, PTS, kLvMany> : scatter_bin_kernel<FT, C, Src, Rec, 2u * NT, PTS, kLvFew>;
        }
        return bin;
    }
    auto reduce_kernel(const AdamTail *adam) const {
        if constexpr (kAdamTail) { if (adam != nullptr) return scatter_reduce_kernel<C, Rec, true>; }
        return scatter_reduce_kernel<C, Rec, false>;
    }
    uint32_t bin_lds(const BinPlan &plan) const { return (2u * (1u << plan.log2_nb) + 4u) * 4u + plan.slots * (uint32_t)sizeof(Rec); }
    template <typename K>
    int launch_bin(const char *timed, K bin, dim3 grid, uint32_t threads, uint32_t lds, hipStream_t s, const BinPass &p) const {
        return launch_as(timed, "scatter_bin_kernel", bin, grid, dim3(threads), lds, s, src, (const typename FT::store_t *)grad, p.offsets, p.grad_table, (Rec *)p.w.regions,
                         p.w.counts, p.w.overflow, B, p.H, p.l0, p.nl, p.plan, p.job, sl, sb);
    }
};

}  // namespace naf
