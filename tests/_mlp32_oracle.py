"""Float64 rehearsal of one training step through the 32-point MLP kernels, with its layouts, cases, probes, tolerances and faults
(not a test module).

mlp_forward_kernel<P, C, true> and mlp_backward_kernel<P, C> (csrc/mlp_kernels.h on csrc/field_mlp.h) serve the fp32 parity mode and
every bf16 shape with C != 2.  The arithmetic is that of tests/_mlp16_oracle.py, whose rehearse / step_reference / geometry /
table_gradient / ratios this module imports and does not restate: only the tile (32 points), the launch plan and the layouts differ.

ROUNDINGS.  mlp_backward_kernel read against _mlp16_oracle.backward_points, for P = PrecBF16 (P::pack converts to bf16, round to
nearest even; P = PrecF32 packs nothing, rnd = identity):
  * x0, h1, h2 are packed where they enter an MFMA (mlp_tile_forward: x0f = pack(x0), pack(h1), pack(h2)); the features arrive as bf16
    already, so pack(x0) is exact.  h3 is NOT packed: the output layer and dw3 += g4 h3 run on fp32 values.
  * G3 = (w3 g4) lrelu'(z3), G2 and G1 are packed once (g3f, g2f, g1f); the packed fragment feeds both the transpose image
    (P::tr_put -> P::tr_load -> the weight-gradient MFMAs) and the chain back through W2b^T, W1^T, W0^T.
  * the hidden layers' bias gradients are P::frag_sum of the tile READ BACK from the image: sums of the rounded G, as reduce_gradients
    forms them; db3 += g4 is not rounded.
  * dx = W2a^T G3 + W0^T G1 accumulates in fp32 and is rounded only by store_feat_slots (bf16 feature gradients), as rehearse() does.
  * padding lanes of a ragged tile take the features of the ray's last sample and gsig = 0: every product they enter is 0.

LAYOUTS.  f32: L 16 x C 2, fp32 table, mlp_precision F32, rnd = identity.  bf16-8x4 / bf16-4x8: bf16 table (rounded once, like the
engine's shadow copy), rnd = bf16_round; the 4 x 8 layout runs three cases only (LAYOUT_CASES).  C = 1 (L = 32) is LEFT OUT: its
levels from 20 up have scales 16 * 2^l - 1 of more than 29 significant bits, so x * scale + 0.5 evaluated in float64 and rounded once
(HashEncoderRef's stand-in for the kernels' fmaf) is no longer an exact product -- the reference would pick other cells than the
kernels (tests/test_hip_fused.py, test_fused_other_level_shapes_fp32_vs_oracle, says the same of the torch oracle) -- and the
bit-for-bit check against oracle/hash_ref.c that would be needed to include it has not been made.

PLAN (csrc/mlp_step_plan.h restated; tests/test_step_plan_cpu.py holds backward_slabs / forward_grid to it): the backward runs
backward_slabs(n) = min(ceil(n / 4), 512) workgroups of four waves, wave w takes rays w, w + 4 slabs, ... and prefetches the first
tile of its next ray during the last tile of this one; the four waves of a workgroup fold into slab w // 4; the forward runs
forward_grid(n) = min(ceil(n / 4), 2048) workgroups the same way.  A ray is ceil(S / 32) tiles.

| (rays, S)   | what it reaches |
|---|---|
| (1024, 192) | the YAML step: 256 slabs, one ray per wave, 6 full tiles |
| (300, 64)   | 75 full workgroups, 2 full tiles: nothing ragged |
| (37, 50)    | 10 slabs, the last workgroup holds one ray; 2 tiles, the second of 18 points |
| (1, 33)     | one workgroup with three idle waves; 2 tiles, the second of ONE point |
| (3, 70)     | one workgroup with one idle wave; 3 tiles, the last of 6 points |
| (24, 7)     | 6 slabs, one ragged tile of 7 points |
| (6, 1030)   | S > kMaxSamplesLds: sample_dist without the depth buffer; 33 tiles, the last of 6 points; two idle waves in slab 1 |
| (2100, 40)  | 512 slabs = 2 048 waves, 52 waves take a second ray (and prefetch its first tile from ray r + 2 048); ragged tile of 8 |
| (4500, 20)  | 404 waves take three rays, the others two; one ragged tile of 20 points |
| (8300, 20)  | 8 192 forward waves, 108 take a second ray; backward waves take four or five rays |

PROBES and PATTERNS as in _mlp16_oracle: `zero` (all weights 0: exact zeros), `probe` (at most 16 unequal weights: both ends of the
batch, either side of every multiple of 4 * slabs -- where a backward wave wraps -- and of 4 * forward_grid, either side of the last
slab boundary, random rays; the reference is over those rays plus 48 more for the line integrals), `dense` (n S <= 2^16).

TOLERANCES.  bf16 layouts keep TOL_ACC / TOL_LOSS / TOL_GRAD / TOL_TABLE of _mlp16_oracle.  The f32 tolerances are MEASURED
(tests/test_mlp32_oracle_cpu.py measures them again on every run): the rehearsal in float32 against itself in float64 on (37, 50)
dense, (300, 64) dense and (1024, 192) probe in the four summation orders of summation_orders(), the table gradient scattered with
fp32 adds in the same point order (the atomic scatter adds in fp32).  Tolerance = 8 x the worst figure of the class, rounded up to
one significant digit (8 x and not the usual 4 x: the kernel's expf / sqrtf are not correctly rounded and its MFMA chains add in a
tree no CPU order reproduces); each has to stay <= 1e-5.  See F32_MEASURED below for the figures.
"""
import collections
import functools
import math

import numpy as np
import torch

import _mlp16_oracle as O
from _mlp16_oracle import BLOCKS, DENSE_MAX_POINTS, bf16_round, identity, rel_l2      # noqa: F401  (re-exported for the test modules)
from oracle import hashgrid_ref

MAX_SLABS = 512                    # kBackwardBlocks
MAX_FORWARD_GRID = 2048            # kForwardBlocks
TILE = 32

Layout = collections.namedtuple("Layout", "L C table_dtype rnd")
LAYOUTS = {"f32": Layout(16, 2, torch.float32, identity),
           "bf16-8x4": Layout(8, 4, torch.bfloat16, bf16_round),
           "bf16-4x8": Layout(4, 8, torch.bfloat16, bf16_round)}
# the layouts of the head cases (OUTPUT HEADS below): the 16-point kernels' own (C = 2, bf16: _mlp16_oracle's plan and probes) beside two of the above
HEAD_LAYOUTS = dict(LAYOUTS, **{"bf16-16x2": Layout(16, 2, torch.bfloat16, bf16_round)})

CASES = ((1024, 192), (300, 64), (37, 50), (1, 33), (3, 70), (24, 7), (6, 1030), (2100, 40), (4500, 20), (8300, 20))
LAYOUT_CASES = {"f32": CASES, "bf16-8x4": CASES, "bf16-4x8": ((1024, 192), (37, 50), (2100, 40))}
MEASURE_CASES = ((37, 50, "dense"), (300, 64, "dense"), (1024, 192, "probe"))

# f32 layout: worst float32-against-float64 figure of each class over MEASURE_CASES x summation_orders() (one thread, see measure()),
# and the tolerance derived from it.  Gradient blocks: the worst of the eight.
#   acc    1.75e-7  (1024, 192) probe, waves   [4.2e-8 .. 1.75e-7 over the twelve runs]   -> 1.41e-6 -> 2e-6
#   loss   7.40e-8  (300, 64) dense, every order [1.6e-8 .. 7.4e-8]                         -> 5.93e-7 -> 6e-7
#   grad   3.90e-7  (300, 64) dense, waves (W2)  [7.2e-8 .. 3.9e-7]                         -> 3.12e-6 -> 4e-6
#   table  2.20e-7  (1024, 192) probe, waves    [1.16e-7 .. 2.2e-7]                         -> 1.76e-6 -> 2e-6
# (bf16 layouts, same runs, as fractions of the _mlp16_oracle tolerances they keep: acc 0.11, loss 0.02, gradient blocks 0.09,
#  table 0.13 with the stored bf16 flips left in -- tests/test_mlp32_oracle_cpu.py asserts a quarter.)
F32_MEASURED = {"acc": 1.76e-7, "loss": 7.41e-8, "grad": 3.90e-7, "table": 2.20e-7}


def derived_tolerance(worst):
    """8 x worst, rounded up to one significant digit."""
    v = 8.0 * worst
    e = math.floor(math.log10(v))
    return math.ceil(v / 10.0 ** e - 1e-9) * 10.0 ** e


F32_TOL = {k: derived_tolerance(v) for k, v in F32_MEASURED.items()}      # acc 2e-6, loss 6e-7, grad 4e-6, table 2e-6
F32_TOL_CEILING = 1e-5             # a twentieth of the 2e-4 the fp32 gradients are held to against the torch oracle


# ---- launch plan of mlp_step_plan.h, restated ------------------------------------------------------------------------------------------
def n_tiles(S):
    return (S + TILE - 1) // TILE


def backward_slabs(n_rays):
    return max(1, min((n_rays + 3) // 4, MAX_SLABS))


def forward_grid(n_rays):
    return max(1, min((n_rays + 3) // 4, MAX_FORWARD_GRID))


def wave_rays(n_rays, wave, n_waves):
    """The rays wave `wave` of `n_waves` takes, in its order."""
    return list(range(wave, n_rays, n_waves))


def slab_rays(n_rays, slab):
    """The rays whose sums fold into a slab: those of the four waves of workgroup `slab`."""
    waves = 4 * backward_slabs(n_rays)
    return [r for w in range(4 * slab, 4 * slab + 4) for r in wave_rays(n_rays, w, waves)]


def rays_per_wave(n_rays, n_waves):
    """(fewest, most) rays a wave takes."""
    return n_rays // n_waves, -(-n_rays // n_waves)


# ---- cases: probes, weights, reference rays -----------------------------------------------------------------------------------------------
def probe_rays(n, S, seed=5):
    """At most 16 rays: the first and last three, either side of every multiple of 4 * slabs and of 4 * forward_grid, either side of
    the last slab boundary, random ones up to 16."""
    bw, fw = 4 * backward_slabs(n), 4 * forward_grid(n)
    want = [0, 1, 2, n - 3, n - 2, n - 1]
    for e in list(range(bw, n, bw)) + list(range(fw, n, fw)) + [4 * (backward_slabs(n) - 1)]:
        want += [e - 1, e]
    out = sorted({r for r in want if 0 <= r < n})
    assert len(out) <= 16, (n, S, out)
    rng = np.random.default_rng(seed + n + S)
    for r in rng.permutation(n):
        if len(out) >= min(16, n):
            break
        if int(r) not in out:
            out.append(int(r))
    return sorted(out)


def patterns(n, S):
    return ("zero", "probe", "dense") if n * S <= DENSE_MAX_POINTS else ("zero", "probe")


def case_inputs(n, S):
    """rays [n, 8], t_rand [n, S], target [n] of _mlp16_oracle.case_inputs and this plan's probe rays; shared and read-only."""
    rays, t_rand, target, _ = O.case_inputs(n, S)
    return rays, t_rand, target, tuple(probe_rays(n, S))


def case_weight(n, S, pattern):
    """weight [n] fp32 as _mlp16_oracle.case_weight makes them, on this plan's probes: 'zero'; 'probe' (unequal values from
    [0.5, 1.5] / 16 on the probe rays, 0 elsewhere); 'dense' ([0.5, 1.5] / n)."""
    if pattern != "probe":
        return O.case_weight(n, S, pattern)
    g = torch.Generator().manual_seed(7 + n + S)
    u = 0.5 + torch.rand(n, generator=g)
    w = torch.zeros(n)
    idx = torch.tensor(probe_rays(n, S))
    w[idx] = u[idx] / 16
    return w


def reference_rays(n, S, pattern):
    """All rays (dense), or the probes plus 48 random rays for the line integrals."""
    if pattern == "dense":
        return list(range(n))
    probes = probe_rays(n, S)
    rng = np.random.default_rng(11 + n + S)
    extra = [int(r) for r in rng.permutation(n) if int(r) not in probes][:48]
    return sorted(probes + extra)


def oracle_net(layout, seed, log2T=12, act="sigmoid"):
    """The oracle twin of a layout's network with a random table, the table rounded once where the layout stores bf16."""
    lay = HEAD_LAYOUTS[layout]
    ref = O.oracle_net(seed, log2T=log2T, L=lay.L, C=lay.C, act=act)
    return ref if lay.table_dtype == torch.float32 else O.round_table_once(ref)


# ---- the reference of a case ------------------------------------------------------------------------------------------------------------------
_SWAP = list(range(4)) + list(range(8, 12)) + list(range(4, 8)) + list(range(12, 32))      # features 4..7 <-> 8..11


def reference(layout, ref, n, S, pattern, fault=None, **kw):
    """_mlp16_oracle.step_reference of a case in a layout's rounding (kw: dtype, order, sample_order, chunks, act, flip).  The fault key
    'swap_features' (fault_chunks_swapped) acts on the finished blocks; every other key is rehearse()'s."""
    fault = dict(fault or {})
    swap = fault.pop("swap_features", None)
    rays, t_rand, target, _ = case_inputs(n, S)
    out = O.step_reference(ref, rays, t_rand, target, case_weight(n, S, pattern), reference_rays(n, S, pattern), S,
                           rnd=LAYOUTS[layout].rnd, fault=fault or None, **kw)
    if swap is not None:
        b = list(out["blocks"])
        for l in range(3):
            if swap == "G":                                  # the A operand: output features, and the bias sums read from it
                b[2 * l], b[2 * l + 1] = b[2 * l][_SWAP], b[2 * l + 1][_SWAP]
            else:                                            # the B operands X0 / H1 / H2: input features
                cols = _SWAP if l < 2 else _SWAP + [32 + i for i in _SWAP]
                b[2 * l] = b[2 * l][:, cols]
        out["blocks"], out["packed"] = b, O.pack(b)
    return out


def table_gradient_f32(dx, n, S, pattern, ref, order=None):
    """The table gradient summed the way the atomic scatter sums it: fp32 adds of fp32 products, one point after the other in `order`."""
    rays, t_rand, _, _ = case_inputs(n, S)
    ids = torch.as_tensor(reference_rays(n, S, pattern))
    _, pts, _ = O.geometry(rays[ids], t_rand[ids], S)
    enc = ref.encoder
    x01 = ((pts + O.BOUND) / (2 * O.BOUND)).numpy().astype(np.float32)
    g = dx.float().numpy().reshape(-1, enc.num_levels, enc.level_dim)
    offs = enc.offsets.numpy()
    perm = np.arange(len(x01)) if order is None else np.asarray(order)
    acc = np.zeros((int(offs[-1]), enc.level_dim), np.float32)
    for lvl in range(enc.num_levels):
        rows, w = hashgrid_ref.corners(x01, lvl, offs, enc.base_resolution)
        for corner in range(rows.shape[1]):
            np.add.at(acc, rows[perm, corner], (w[perm, corner:corner + 1] * g[perm, lvl]).astype(np.float32))
    return acc


def summation_orders(n, S, pattern, ids=None):
    """name -> kwargs of rehearse(): the four orders the f32 tolerances are measured in.  'waves': the points in the order the
    backward's waves take them (wave w: rays w, w + 4 slabs, ..., waves in slab order), as partial sums of 32 consecutive points
    -- the kernel's tiles wherever S is a multiple of 32 -- added one after the other."""
    ids = reference_rays(n, S, pattern) if ids is None else list(ids)
    N = len(ids) * S
    g = torch.Generator().manual_seed(3 * n + S)
    waves = 4 * backward_slabs(n)
    by_wave = sorted(range(len(ids)), key=lambda i: (ids[i] % waves, ids[i] // waves))
    wave_order = torch.cat([torch.arange(i * S, (i + 1) * S) for i in by_wave])
    return {"natural": dict(),
            "shuffled-7": dict(order=torch.randperm(N, generator=g), sample_order=torch.randperm(S, generator=g), chunks=7),
            "reversed-3": dict(order=torch.arange(N - 1, -1, -1), sample_order=torch.arange(S - 1, -1, -1), chunks=3),
            "waves": dict(order=wave_order, chunks=-(-N // TILE))}


def rehearse_in_float32(layout, ref, n, S, pattern, **kw_all):
    """order name -> the float32 rehearsal of a case in that order (reference()'s dict).  One thread, so that the BLAS behind the
    partial products sums the same way wherever this runs.  f32 layout: the table gradient is scattered in fp32 too, in the same
    point order."""
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        out = {}
        for name, kw in summation_orders(n, S, pattern).items():
            got = reference(layout, ref, n, S, pattern, dtype=torch.float32, **kw, **kw_all)
            if layout == "f32":
                got["emb_g"] = table_gradient_f32(got["dx"], n, S, pattern, ref, kw.get("order"))
            out[name] = got
        return out
    finally:
        torch.set_num_threads(threads)


def figure_classes(r):
    """ratios()-style dict of figures -> the four classes (gradient blocks: the worst)."""
    return {"acc": r["acc"], "loss": r["loss"], "grad": max(r[k] for k in BLOCKS), "table": r["table"]}


def figures(got, want):
    """Every figure of the comparison as it is (not as a fraction of a tolerance): name -> relative error."""
    r = O.ratios(got, want)
    scale = {"acc": O.TOL_ACC, "loss": O.TOL_LOSS, "table": O.TOL_TABLE}
    return {k: v * scale.get(k, O.TOL_GRAD) for k, v in r.items()}


def ratios(layout, got, want, tol_table=None):
    """Every figure as a fraction of its tolerance in `layout`."""
    if layout != "f32":
        return O.ratios(got, want, **({} if tol_table is None else dict(tol_table=tol_table)))
    f = figures(got, want)
    tol = dict(F32_TOL, table=F32_TOL["table"] if tol_table is None else tol_table)
    return {k: v / tol.get(k, tol["grad"]) for k, v in f.items()}


def acc_tolerance(layout):
    return F32_TOL["acc"] if layout == "f32" else O.TOL_ACC


def numpy_dict(out):
    return {k: (v.double().numpy() if torch.is_tensor(v) and k != "rays" else v) for k, v in out.items()}


# ---- faults: what a subtly wrong 32-point kernel would compute ------------------------------------------------------------------------------
# Every builder returns the `fault` dict of reference() for the rays `ids` (sorted global ray numbers) of a case, or None where the
# case gives the fault nothing to act on.
def _local(ids):
    return {int(r): i for i, r in enumerate(ids)}


def _ray_count(ids, S, rays, value):
    loc = _local(ids)
    c, lc = torch.ones(len(ids), S), torch.ones(len(ids))
    for r in rays:
        if r in loc:
            c[loc[r]], lc[loc[r]] = value, value
    return c, lc


def fault_ray_dropped(S, ids, ray):
    """A wave never took a ray (its second, say): no sums, no loss share, no feature gradients."""
    c, lc = _ray_count(ids, S, [ray], 0.0)
    return dict(count=c, stored=c, loss_count=lc)


def fault_ray_twice(S, ids, ray):
    """A ray ran on two waves: sums and loss share count twice, the feature gradients are stored twice (same values)."""
    c, lc = _ray_count(ids, S, [ray], 2.0)
    return dict(count=c, loss_count=lc)


def fault_slab_skipped(n, S, ids, slab):
    """The reducer skipped a slab: sums and loss shares of its rays are gone, their feature gradients are not."""
    c, lc = _ray_count(ids, S, slab_rays(n, slab), 0.0)
    return dict(count=c, loss_count=lc)


def fault_weight_shifted(n, S, pattern, ids, shift):
    """weight[r] read at r + shift."""
    return O.fault_weight_shifted(case_weight(n, S, pattern), ids, shift)


def fault_loss_per_tile(S, ids):
    """loss_part added once per tile instead of once per ray."""
    return dict(loss_count=torch.full((len(ids),), float(n_tiles(S)))) if n_tiles(S) > 1 else None


def fault_padding_contributes(n, S, ids, tail_dist=False):
    """The padding lanes of a ragged last tile are not masked: each repeats the ray's last sample (the features the kernels load for
    them) with the distance of an interior sample.  tail_dist: with the last sample's own 1e-10 |d| (what buffered_dist / sample_dist
    return past the end: invisible, and harmless -- see tests/test_mlp32_oracle_cpu.py)."""
    pad = TILE * n_tiles(S) - S
    if pad == 0:
        return None
    rays = case_inputs(n, S)[0]
    idx = torch.as_tensor(list(ids))
    dn = rays[idx, 3:6].double().norm(dim=-1)
    step = (rays[idx, 7] - rays[idx, 6]).double() / max(S - 1, 1)
    d = (1e-10 if tail_dist else step) * dn
    er = torch.arange(len(ids)).repeat_interleave(pad)
    return dict(extra=(er, torch.full_like(er, S - 1), d.repeat_interleave(pad)))


def fault_next_ray_prefetch(n, S, ids):
    """The first tile of a wave's NEXT ray prefetched from ray r + 1 instead of r + n_waves: ray t >= n_waves runs its first tile on
    the features of ray t - n_waves + 1 (wherever both are among `ids`)."""
    waves = 4 * backward_slabs(n)
    loc = _local(ids)
    src_ray = torch.arange(len(ids))[:, None].repeat(1, S)
    hit = 0
    for t in ids:
        if t >= waves and t - waves + 1 in loc:
            src_ray[loc[t], :min(TILE, S)] = loc[t - waves + 1]
            hit += 1
    return dict(feature_source=(src_ray, torch.arange(S).repeat(len(ids), 1))) if hit else None


def fault_bias_half_lost(S, ids, rays=None):
    """The hidden layers' bias sums miss one lane half: P::tr_load gives lane half 1 the points 8..15 and 24..31 of every tile, and
    db += shfl_xor(db, 32) is what adds them."""
    s = torch.arange(S)
    lost = ((s % TILE) // 8) % 2 == 1
    if not bool(lost.any()):
        return None
    c = torch.ones(len(ids), S)
    rows = range(len(ids)) if rays is None else [_local(ids)[r] for r in rays]
    for i in rows:
        c[i, lost] = 0.0
    return dict(bias_count=c)


def fault_bias3_tile_lost(S, ids, ray, tile):
    """db3 misses one tile of one ray."""
    c = torch.ones(len(ids), S)
    c[_local(ids)[ray], TILE * tile:TILE * (tile + 1)] = 0.0
    return dict(bias3_count=c)


def fault_chunks_swapped(operand):
    """Two 8-byte chunks of the transposed read exchanged (chunk c of an image row holds features 4 c .. 4 c + 3): features 4..7 and
    8..11 of an operand swap.  operand 'G': the gradient tile -- rows of dW0 / dW1 / dW2 and entries of db0 / db1 / db2 permuted;
    'X': the input tiles X0 / H1 / H2 -- columns of dW0 / dW1 / dW2 permuted."""
    assert operand in ("G", "X")
    return dict(swap_features=operand)


# ---- OUTPUT HEADS ------------------------------------------------------------------------------------------------------------------------------
# The cases above restate the sigmoid head.  The other three heads of naf_render_cfg.last_activation (relu: LeakyReLU(0.01), tanh, none)
# run on a few cases per kernel family (tests/test_hip_mlp_heads_reference.py; tests/test_mlp_heads_oracle_cpu.py checks what follows
# without a GPU).  (rays, S, pattern) per layout; bf16-16x2 is _mlp16_oracle's plan: mlp16_train_kernel<12>, its 4-wave form on a ragged
# tile, the pair above the one-launch limit with a wave's second item, and a dense case; the 32-point kernels: a ragged tile, the
# one-point tile, a wave's second ray and its prefetched tile.
HEAD_ACTS = ("relu", "tanh", "none")
HEAD_CASES = {"bf16-16x2": ((1024, 192, "probe"), (700, 100, "probe"), (3100, 40, "probe"), (24, 7, "dense")),
              "f32": ((37, 50, "dense"), (1, 33, "dense"), (2100, 40, "probe")),
              "bf16-8x4": ((37, 50, "dense"), (1, 33, "dense"), (2100, 40, "probe"))}
HEAD_ZERO_CASE = (24, 7)
# Network seed per head (_naf_helpers.naf_pair and oracle_net give the same weights for a seed).  tanh and none keep 37, the seed of
# every sigmoid case: |z4| < 0.19 there, no point anywhere near tanh's saturation (the fraction of points with |y| > 0.99 is 0, so
# neither `scale` nor b3 had to move).  relu: see THE LEAKY HEAD'S DECISION.
HEAD_SEEDS = {"sigmoid": 37, "relu": 222, "tanh": 37, "none": 37}

# f32 layout, per head: worst float32-against-float64 figure of each class over MEASURE_CASES x summation_orders(), as F32_MEASURED
# (whose sigmoid figures stay as they are), and 8 x that rounded up to one digit.
#   relu  acc 2.203e-7 (37, 50) waves -> 2e-6 | loss 1.118e-7 (300, 64) shuffled-7 -> 9e-7 | grad 4.777e-7 (300, 64) waves -> 4e-6 | table 1.552e-7 -> 2e-6
#   tanh  acc 1.951e-7 (1024, 192) waves -> 2e-6 | loss 9.366e-8 (1024, 192) waves -> 8e-7 | grad 3.993e-7 (300, 64) waves -> 4e-6 | table 1.594e-7 -> 2e-6
#   none  acc 2.017e-7 (1024, 192) waves -> 2e-6 | loss 9.775e-8 (37, 50) shuffled-7 -> 8e-7 | grad 6.018e-7 (300, 64) waves -> 5e-6 | table 1.440e-7 -> 2e-6
# (smallest figure of a class over the twelve runs of a head: acc 3.6e-8, loss 7.7e-10, grad 7.1e-8, table 1.06e-7.)  tanh's gradient figure is
# that of the other heads: nothing saturates in these cases, see HEAD_SEEDS.
HEAD_F32_MEASURED = {"sigmoid": F32_MEASURED,
                     "relu": {"acc": 2.21e-7, "loss": 1.12e-7, "grad": 4.78e-7, "table": 1.56e-7},
                     "tanh": {"acc": 1.96e-7, "loss": 9.37e-8, "grad": 4.00e-7, "table": 1.60e-7},
                     "none": {"acc": 2.02e-7, "loss": 9.78e-8, "grad": 6.02e-7, "table": 1.45e-7}}
HEAD_F32_TOL = {act: {k: derived_tolerance(v) for k, v in m.items()} for act, m in HEAD_F32_MEASURED.items()}

# THE LEAKY HEAD'S DECISION.  z4 > 0 is a discontinuity of the leaky head's derivative: a weighted point that the kernel's fp32 z4 puts
# on the other side of 0 than the reference's moves a block by far more than any tolerance here.  Per precision, delta = 8 x the worst
# |z4(float32 rehearsal) - z4(float64 rehearsal)| over the relu cases x summation_orders() (worst figures below, rounded up to one
# digit like the tolerances); a weighted point with |z4| < delta is UNDECIDED.  The relu seed is chosen so that no f32 case and no
# f32 MEASURE_CASE has one and every bf16 case at most HEAD_MAX_UNDECIDED; for those the reference supplies both branches and the
# comparison takes the best combination (head_references / best_ratios), as _raymarch_oracle does for its thresholds.
#   f32 2.97e-8 at (300, 64) dense -> 3e-7;  bf16 1.53e-5 at bf16-16x2 (1024, 192) probe (a hidden activation on a bf16 rounding boundary) -> 2e-4
HEAD_Z4_MEASURED = {"f32": 3.0e-8, "bf16": 1.6e-5}
HEAD_DELTA = {k: derived_tolerance(v) for k, v in HEAD_Z4_MEASURED.items()}
HEAD_MAX_UNDECIDED = {"f32": 0, "bf16": 2}


def head_precision(layout):
    return "f32" if layout == "f32" else "bf16"


def head_inputs(layout, n, S, pattern):
    """-> rays, t_rand, target, weight (the batch's), reference rays of a head case, on the layout's plan and probes."""
    if layout == "bf16-16x2":
        rays, t_rand, target, _ = O.case_inputs(n, S)
        return rays, t_rand, target, O.case_weight(n, S, pattern), O.reference_rays(n, S, pattern)
    rays, t_rand, target, _ = case_inputs(n, S)
    return rays, t_rand, target, case_weight(n, S, pattern), reference_rays(n, S, pattern)


def head_reference(layout, ref, n, S, pattern, act, **kw):
    """_mlp16_oracle.step_reference of a head case in the layout's rounding (kw: rehearse()'s)."""
    rays, t_rand, target, weight, ids = head_inputs(layout, n, S, pattern)
    return O.step_reference(ref, rays, t_rand, target, weight, ids, S, rnd=HEAD_LAYOUTS[layout].rnd, act=act, **kw)


def head_rehearse_in_float32(layout, ref, n, S, pattern, act):
    """order name -> the float32 rehearsal of a head case in that order, as rehearse_in_float32 (which it is for the 32-point layouts)."""
    if layout != "bf16-16x2":
        return rehearse_in_float32(layout, ref, n, S, pattern, act=act)
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        ids = head_inputs(layout, n, S, pattern)[4]
        return {name: head_reference(layout, ref, n, S, pattern, act, dtype=torch.float32, **kw)
                for name, kw in summation_orders(n, S, pattern, ids).items()}
    finally:
        torch.set_num_threads(threads)


def undecided_points(layout, n, S, pattern, want):
    """-> (flat indices into the reference's n_ids * S points of the weighted points with |z4| < delta, the smallest |z4| / delta
    among the weighted points)."""
    _, _, _, weight, ids = head_inputs(layout, n, S, pattern)
    delta = HEAD_DELTA[head_precision(layout)]
    z = torch.as_tensor(want["z4"]).abs().double()
    live = (weight[torch.as_tensor(ids)] > 0)[:, None].expand_as(z)
    if not bool(live.any()):
        return [], float("inf")
    und = torch.nonzero((live & (z < delta)).reshape(-1)).reshape(-1).tolist()
    return und, float(z[live].min()) / delta


def head_references(layout, ref, n, S, pattern, act):
    """The references a kernel may match: one, or -- leaky head with k <= HEAD_MAX_UNDECIDED undecided points -- the 2^k combinations
    of their branches (the first is the reference's own)."""
    base = head_reference(layout, ref, n, S, pattern, act)
    if act != "relu":
        return [base]
    und, _ = undecided_points(layout, n, S, pattern, base)
    assert len(und) <= HEAD_MAX_UNDECIDED[head_precision(layout)], (layout, n, S, pattern, und)
    out = [base]
    for combo in range(1, 1 << len(und)):
        flip = torch.zeros(base["z4"].numel(), dtype=torch.bool)
        flip[[p for i, p in enumerate(und) if combo >> i & 1]] = True
        out.append(head_reference(layout, ref, n, S, pattern, act, flip=flip))
    return out


def head_tolerances(layout, act):
    """acc / loss / grad / table of a head in a layout: measured per head in f32, _mlp16_oracle's in every bf16 layout."""
    if layout == "f32":
        return HEAD_F32_TOL[act]
    return {"acc": O.TOL_ACC, "loss": O.TOL_LOSS, "grad": O.TOL_GRAD, "table": O.TOL_TABLE}


def head_ratios(layout, act, got, want):
    """Every figure as a fraction of the head's tolerance in `layout`."""
    tol = head_tolerances(layout, act)
    return {k: v / tol.get(k, tol["grad"]) for k, v in figures(got, want).items()}


def best_ratios(layout, act, got, wants):
    """head_ratios against the reference of `wants` that suits `got` best (smallest worst fraction)."""
    return min((head_ratios(layout, act, got, numpy_dict(w) if torch.is_tensor(w["acc"]) else w) for w in wants), key=lambda r: max(r.values()))
