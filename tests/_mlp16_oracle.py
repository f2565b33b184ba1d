"""Float64 rehearsal of one bf16 training step of the canonical NAF network, with its cases, probes and tolerances (not a test module).

The bf16 MLP kernels of csrc/mlp16_kernels.h (mlp16_forward_split_kernel, mlp16_backward_kernel, mlp16_train_kernel<4> / <12>, the
slab fold mlp16_fold_slab and slab_reduce_block of mlp_slabs.h) are "fp32 with bf16 MFMA operands": features, W0..W2, the hidden
activations and the gradient tiles G3, G2, G1 are rounded to bf16 (round to nearest even) where they enter an MFMA; the accumulation,
the output layer, the masks and the biases are not rounded.  rehearse() makes exactly those roundings and is exact elsewhere (float64),
so the kernels differ from it by fp32 summation order and by the rare operand that an fp32 reordering moves across a bf16 rounding
boundary -- and by nothing else.  tests/test_mlp16_oracle_cpu.py validates the rehearsal and the tolerances without a GPU,
tests/test_hip_mlp16_reference.py holds the kernels to them, tests/test_hip_fused.py runs its fp32 form (the emulation it always had).

WORK ITEMS.  backward16_parts / mlp_train_waves / n_slabs restate the launch plan of csrc/mlp_step_plan.h (tests/test_step_plan_cpu.py
holds them to it), tile_ranges the kernels' first_tile: a ray is cut into `parts`
ranges of 16-point tiles, item = ray * parts + part, four consecutive items (of one workgroup) fold into a slab, 768 workgroups of four
waves at most.  They serve only to PLACE probes and faults; the reference sums over points and knows nothing of items.

PROBES.  At training sizes a full reference is expensive and a lost item is 1e-3 of the gradient.  With weights that vanish off a few
probe rays the reference is a sum over those rays alone and one lost item among them is an error of order one; the zero pattern (all
weights 0) demands exact zeros; the dense pattern (small cases) sees an item of ANY ray counted or leaking.  The probe weights are
unequal, so a kernel that reads weight[r +- 1], weight[item] or weight[wave] cannot pass.
"""
import functools

import numpy as np
import torch

from _naf_helpers import crossing_rays
from oracle import render_ref as R
from oracle.hashgrid_ref import HashEncoderRef, hash_encode_backward
from oracle.network_ref import DensityNetworkRef

BOUND = 0.3
LEAK = 0.01
MAX_ITEM_WAVES = 3072              # 768 workgroups x 4 waves (kBackwardBlocks16), also the one-launch limit (NAF_MLP_TRAIN_MAX_RAYS)
MAX_SAMPLES_LDS = 1024             # kMaxSamplesLds

# tolerances: those of test_hip_fused.py::test_bf16_mode_backward_matches_a_bf16_rounding_emulation and its written rationale (fp32
# summation order; one 2^-9 flip among thousands of operands; a rounding in the wrong place would be ~4e-3), 3e-3 for bf16 records
TOL_ACC, TOL_LOSS, TOL_GRAD, TOL_TABLE, TOL_TABLE_BINNED = 2e-6, 1e-5, 2e-4, 2e-4, 3e-3
BLOCKS = ("W0", "b0", "W1", "b1", "W2", "b2", "w3", "b3")
BLOCK_SHAPES = ((32, 32), (32,), (32, 32), (32,), (32, 64), (32,), (1, 32), (1,))

# (n_rays, S): see the table in the docstring of test_hip_mlp16_reference.py
CASES = ((1024, 192), (256, 192), (300, 192), (700, 100), (1001, 75), (3072, 40), (3100, 40), (5000, 20), (6, 1030), (24, 7))
DENSE_MAX_POINTS = 1 << 16


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def bf16_round(t):
    """The nearest bf16 (ties to even) of every element, in the tensor's own dtype.  float64 values pass through fp32 first, as the
    kernels' operands do."""
    return t.float().bfloat16().to(t.dtype)


def identity(t):
    return t


# ---- launch plan of mlp_step_plan.h, restated -----------------------------------------------------------------------------------------
def n_tiles(S):
    return (S + 15) // 16


def backward16_parts(n_rays, S):
    return max(1, min(n_tiles(S), 12, MAX_ITEM_WAVES // max(n_rays, 1)))


def mlp_train_waves(n_rays, S):
    """Waves per workgroup of mlp16_train_kernel, 0: the step runs the forward / backward pair."""
    if n_rays == 0 or n_rays > MAX_ITEM_WAVES or S == 0 or S > MAX_SAMPLES_LDS // 2:
        return 0
    parts = backward16_parts(n_rays, S)
    return 4 if 4 % parts == 0 else 12 if 12 % parts == 0 else 0


def tile_ranges(S, parts, round_up=False):
    """first_tile(0 .. parts): part p owns the tiles [f[p], f[p + 1])."""
    t = n_tiles(S)
    return [-((-p * t) // parts) if round_up else p * t // parts for p in range(parts + 1)]


def n_slabs(n_rays, S):
    return max(1, min((n_rays * backward16_parts(n_rays, S) + 3) // 4, MAX_ITEM_WAVES // 4))


def item_points(n_rays, S, item):
    """-> (ray, first sample, end sample) of a work item."""
    parts = backward16_parts(n_rays, S)
    f = tile_ranges(S, parts)
    r, p = divmod(item, parts)
    return r, 16 * f[p], min(S, 16 * f[p + 1])


def slab_items(n_rays, S, slab):
    """The work items that fold into a slab: the four waves of workgroup `slab`, each with every item it takes."""
    items = n_rays * backward16_parts(n_rays, S)
    waves = 4 * n_slabs(n_rays, S)
    return [i for w in range(4 * slab, 4 * slab + 4) for i in range(w, items, waves)]


# ---- cases: rays, jitter, targets, probes, weights -------------------------------------------------------------------------------------
def probe_rays(n, S, seed=3):
    """At most 16 rays: the first three and the last three, the rays whose items sit on either side of every multiple of 3 072 items
    and of the last slab boundary, and random ones up to 16."""
    parts = backward16_parts(n, S)
    items = n * parts
    want = [0, 1, 2, n - 3, n - 2, n - 1]
    edges = list(range(MAX_ITEM_WAVES, items, MAX_ITEM_WAVES)) + [4 * (n_slabs(n, S) - 1)]
    for e in edges:
        want += [(e - 1) // parts, e // parts]
    out = sorted({r for r in want if 0 <= r < n})
    rng = np.random.default_rng(seed + n + S)
    for r in rng.permutation(n):
        if len(out) >= min(16, n):
            break
        if int(r) not in out:
            out.append(int(r))
    return sorted(out)


def patterns(n, S):
    return ("zero", "probe", "dense") if n * S <= DENSE_MAX_POINTS else ("zero", "probe")


@functools.lru_cache(maxsize=None)
def case_inputs(n, S):
    """rays [n, 8], t_rand [n, S], target [n] (fp32, CPU) and the probe rays of a case; shared and read-only."""
    rays = crossing_rays(n, seed=41 + n)
    g = torch.Generator().manual_seed(1000 + n + S)
    t_rand = torch.rand(n, S, generator=g)
    target = torch.rand(n, generator=g) * 0.2
    return rays, t_rand, target, tuple(probe_rays(n, S))


def case_weight(n, S, pattern):
    """weight [n] fp32: 'zero'; 'probe' (unequal values from [0.5, 1.5] / 16 on the probe rays, 0 elsewhere); 'dense' ([0.5, 1.5] / n)."""
    g = torch.Generator().manual_seed(7 + n + S)
    u = 0.5 + torch.rand(n, generator=g)
    if pattern == "zero":
        return torch.zeros(n)
    if pattern == "dense":
        return u / n
    if pattern != "probe":
        raise ValueError(pattern)
    w = torch.zeros(n)
    idx = torch.tensor(case_inputs(n, S)[3])
    w[idx] = u[idx] / 16
    return w


def reference_rays(n, S, pattern):
    """The rays the reference is computed over: all of them (dense) or the probes plus 48 random rays for the line integrals."""
    if pattern == "dense":
        return list(range(n))
    probes = list(case_inputs(n, S)[3])
    rng = np.random.default_rng(11 + n + S)
    extra = [int(r) for r in rng.permutation(n) if int(r) not in probes][:48]
    return sorted(probes + extra)


def oracle_net(seed, log2T=12, scale=0.5, L=16, C=2, act="sigmoid"):
    """The canonical network's oracle twin with a random table (for the CPU tests; the GPU tests take _naf_helpers.naf_pair's).
    L x C = 32: the level shape of the encoder (tests/_mlp32_oracle.py runs 8 x 4 and 4 x 8).  act: the output head (HEADS); the
    weights of a seed do not depend on it."""
    torch.manual_seed(seed)
    enc = HashEncoderRef(3, L, C, 16, log2T)
    enc.embeddings.data.uniform_(-scale, scale)
    return DensityNetworkRef(enc, bound=BOUND, num_layers=4, hidden_dim=32, skips=(2,), out_dim=1, last_activation=act)


def round_table_once(ref):
    """A bf16 table is rounded once, like the shadow copy the kernels gather from."""
    ref.encoder.embeddings.data.copy_(ref.encoder.embeddings.data.to(torch.bfloat16).float())
    return ref


# ---- the rehearsal ---------------------------------------------------------------------------------------------------------------------
def _leaky(h):
    return torch.where(h > 0, h, LEAK * h)


def _mask(h):
    return torch.where(h > 0, torch.ones_like(h), torch.full_like(h, LEAK))


def mlp_params(layers, rnd, dtype):
    """W0..W2 rounded where they enter an MFMA, the output layer and all biases as they are."""
    W = [rnd(l.weight.detach().to(dtype)) for l in layers[:3]]
    b = [l.bias.detach().to(dtype) for l in layers]
    return W, b, layers[3].weight.detach().to(dtype)


# The output head (naf_render_cfg.last_activation 0..3; "relu" is the reference's name for LeakyReLU(0.01), network.py) as last_act and
# last_act_grad of csrc/field_mlp.h write it.  float64: the reference.  float32: the kernel's own formula, the cancellation in
# 1 - y y included.
HEADS = ("sigmoid", "relu", "tanh", "none")


def head(z, act):
    """last_act in z's dtype."""
    if act == "sigmoid":
        return torch.sigmoid(z)
    if act == "relu":
        return _leaky(z)
    if act == "tanh":
        return torch.tanh(z)
    if act != "none":
        raise ValueError(act)
    return z


def head_grad(z, y, act, slope=LEAK, flip=None):
    """last_act_grad, THROUGH THE OUTPUT y as the kernels form it: y (1 - y), z > 0 ? 1 : 0.01, 1 - y y, 1.  slope: the leaky head's
    value for z <= 0 (fault injection); flip [N] bool: points whose z > 0 is decided the other way (the undecided points of
    tests/_mlp32_oracle.py's head cases)."""
    if act == "sigmoid":
        return y * (1 - y)
    if act == "relu":
        up = z > 0
        if flip is not None:
            up = up ^ flip.reshape(up.shape)
        return torch.where(up, torch.ones_like(z), torch.full_like(z, slope))
    if act == "tanh":
        return 1 - y * y
    if act != "none":
        raise ValueError(act)
    return torch.ones_like(z)


def forward_points(x, params, rnd, act="sigmoid", with_z=False):
    """x [N, 32]: the (rounded) features.  -> h1, h2, h3, sigma [N] (and z4 [N], the output unit before its head: with_z)."""
    W, b, w3 = params
    h1 = _leaky(x @ W[0].T + b[0])
    h2 = _leaky(rnd(h1) @ W[1].T + b[1])
    h3 = _leaky(torch.cat([x, rnd(h2)], -1) @ W[2].T + b[2])
    z4 = h3 @ w3.T + b[3]
    sig = head(z4, act).reshape(-1)
    return (h1, h2, h3, sig, z4.reshape(-1)) if with_z else (h1, h2, h3, sig)


def backward_points(x, gsig, params, rnd, act="sigmoid", slope=LEAK, flip=None):
    """Backward of points with features x [N, 32] and d loss / d sigma gsig [N] (the kernels recompute the forward from the features,
    sigma and its derivative with their own copy of `act`): the operands of the weight-gradient products and the feature gradients
    dx [N, 32] (unrounded).  slope, flip: see head_grad."""
    W, b, w3 = params
    h1, h2, h3, sig, z4 = forward_points(x, params, rnd, act, with_z=True)
    g4 = (gsig * head_grad(z4, sig, act, slope, flip)).reshape(-1, 1)
    G3 = rnd((w3 * g4) * _mask(h3))
    G2 = rnd((G3 @ W[2][:, 32:]) * _mask(h2))
    G1 = rnd((G2 @ W[1]) * _mask(h1))
    dx = G3 @ W[2][:, :32] + G1 @ W[0]
    return dict(g4=g4, h3=h3, G=(G1, G2, G3), inp=(x, rnd(h1), torch.cat([x, rnd(h2)], -1)), dx=dx)


def _sum_rows(t, order, chunks):
    """Sum over dim 0 in the given order, as `chunks` partial sums added at the end."""
    if order is not None:
        t = t[order]
    parts = [c.sum(0) for c in torch.chunk(t, chunks, 0)]
    return functools.reduce(lambda a, c: a + c, parts)


def _matmul_rows(a, b, order, chunks):
    """a.T @ b over dim 0 in the given order, as `chunks` partial products."""
    if order is not None:
        a, b = a[order], b[order]
    parts = [x.T @ y for x, y in zip(torch.chunk(a, chunks, 0), torch.chunk(b, chunks, 0))]
    return functools.reduce(lambda p, q: p + q, parts)


def reduce_gradients(bp, m=None, mb=None, mb3=None, order=None, chunks=1):
    """The eight gradient blocks (BLOCKS) from per-point operands.  m / mb / mb3 [N]: how often a point counts in every sum / in the
    hidden layers' bias sums / in db3 (fault injection; None: once).  Bias gradients are sums of the ROUNDED tiles, as the kernels add
    the bf16 operand they have just built (add_bf16x4)."""
    one = torch.ones_like(bp["g4"]) if m is None else m.reshape(-1, 1).to(bp["g4"].dtype)
    hb = one if mb is None else one * mb.reshape(-1, 1).to(one.dtype)
    ob = one if mb3 is None else one * mb3.reshape(-1, 1).to(one.dtype)
    out = []
    for l in range(3):
        out.append(_matmul_rows(bp["G"][l] * one, bp["inp"][l], order, chunks))
        out.append(_sum_rows(bp["G"][l] * hb, order, chunks))
    out.append(_sum_rows(bp["g4"] * one * bp["h3"], order, chunks).reshape(1, -1))
    out.append(_sum_rows(bp["g4"] * ob, order, chunks).reshape(1))
    return out


def pack(blocks):
    """The layout of net.packed_mlp(): per layer the weight, then the bias."""
    return torch.cat([b.reshape(-1) for b in blocks])


def unpack(flat):
    out, off = [], 0
    for shape in BLOCK_SHAPES:
        k = int(np.prod(shape))
        out.append(flat[off:off + k].reshape(shape))
        off += k
    assert off == flat.numel() == 4225
    return out


def rehearse(x, dist, target, weight, layers, rnd=bf16_round, dtype=torch.float64, fault=None, order=None, sample_order=None, chunks=1,
             act="sigmoid", flip=None):
    """One training step on rays with features x [n, S, 32] (encoder output, not yet rounded), sample distances dist [n, S], targets and
    weights [n].  acc comes from the rehearsal's own forward, dacc = 2 w (acc - target), loss = sum w (acc - target)^2.

    `order` (a permutation of the n * S points), `sample_order` (a permutation of a ray's S samples) and `chunks`: every sum over
    points / over the samples of a ray is formed in that order, as `chunks` partial sums added at the end.
    `fault`: dict of deviations a wrong kernel would make, see the fault_* builders.
    `act`: the output head (HEADS).  `flip` [n * S] bool: points whose leaky-head decision z4 > 0 the backward takes the other way.

    -> dict: acc [n], loss, dacc [n], blocks (list of 8), packed [4225], dx [n * S, 32] (rounded: stored as bf16), z4 [n, S]."""
    fault = fault or {}
    n, S, _ = x.shape
    params = mlp_params(layers, rnd, dtype)
    xr = rnd(x.to(dtype)).reshape(n * S, 32)
    dist = dist.to(dtype)
    target = target.to(dtype)
    weight = weight.to(dtype)
    fwd = forward_points(xr, params, rnd, act, with_z=True)
    sig, z4 = fwd[3].reshape(n, S), fwd[4].reshape(n, S)
    if "head_forward_items" in fault:                                     # work items whose forward got the default head (0: sigmoid)
        sig = sig.clone()
        for r, a, e in fault["head_forward_items"]:
            sig[r, a:e] = head(z4[r, a:e], "sigmoid")
    terms = sig * dist
    if sample_order is not None:
        terms = terms[:, sample_order]
    acc = functools.reduce(lambda a, c: a + c, [c.sum(-1) for c in torch.chunk(terms, chunks, -1)])
    err = acc - target
    w = fault.get("weight_read", weight).to(dtype)                       # a kernel that reads another ray's weight
    dacc = 2.0 * w * err
    loss = (fault.get("loss_count", torch.ones(n)).to(dtype) * w * err * err).sum()
    gsig = (dacc[:, None] * dist).reshape(-1)
    xb = xr
    if "feature_source" in fault:                                         # the backward of a point recomputed from another point's features:
        src = fault["feature_source"]                                     # sample numbers [n, S] of the same ray, or (rays [n, S], samples [n, S])
        src_ray, src_sample = src if isinstance(src, tuple) else (torch.arange(n)[:, None], src)
        xb = xr.reshape(n, S, 32)[src_ray, src_sample].reshape(n * S, 32)
    m = fault.get("count")
    m = None if m is None else m.reshape(-1).to(dtype)
    if "extra" in fault:                                                  # points that should contribute nothing (padding)
        er, es, ed = fault["extra"]
        xb = torch.cat([xb, xr.reshape(n, S, 32)[er, es]])
        gsig = torch.cat([gsig, dacc[er] * ed.to(dtype)])
        m = torch.cat([torch.ones(n * S, dtype=dtype) if m is None else m, torch.ones(len(er), dtype=dtype)])
    if flip is not None and flip.numel() != gsig.numel():
        raise ValueError("flip and extra points do not combine")
    # head_backward: the backward's own copy of `act` is another head's; head_slope: its leaky derivative for z4 <= 0 is not 0.01
    bp = backward_points(xb, gsig, params, rnd, fault.get("head_backward", act), fault.get("head_slope", LEAK), flip)

    def widen(v):
        if v is None or v.numel() == gsig.numel():
            return v
        return torch.cat([v.reshape(-1).to(dtype), torch.ones(gsig.numel() - v.numel(), dtype=dtype)])
    if order is not None and gsig.numel() != n * S:
        raise ValueError("order and extra points do not combine")
    blocks = reduce_gradients(bp, m, widen(fault.get("bias_count")), widen(fault.get("bias3_count")), order, chunks)
    dx = rnd(bp["dx"][:n * S])
    if "stored" in fault:                                                 # feature gradients that were never written
        dx = dx * fault["stored"].reshape(-1, 1).to(dtype)
    return dict(acc=acc, loss=loss, dacc=dacc, blocks=blocks, packed=pack(blocks), dx=dx, z4=z4)


def geometry(rays, t_rand, S):
    """Depths (the oracle's, fp32), points [n * S, 3] and sample distances [n, S] (float64 of the fp32 depths) of perturbed rays."""
    n = rays.shape[0]
    z = R.sample_depths(rays[:, 6:7], rays[:, 7:8], S, True, t_rand)
    pts = R.points_on_rays(rays, z, BOUND).reshape(-1, 3)
    dn = rays[:, 3:6].double().norm(dim=-1, keepdim=True)
    zd = z.double()
    dist = torch.cat([zd[:, 1:] - zd[:, :-1], torch.full((n, 1), 1e-10, dtype=torch.float64)], -1) * dn
    return z, pts, dist


def table_gradient(dx, pts, ref):
    """The table gradient: the scatter of the stored feature gradients (oracle.hashgrid_ref.hash_encode_backward, float64 sums; it
    takes the gradients as fp32, which holds every bf16 exactly)."""
    enc = ref.encoder
    xn = ((pts + BOUND) / (2 * BOUND)).numpy().astype(np.float32)
    offs = enc.offsets.numpy()
    return hash_encode_backward(dx.float().numpy(), xn, offs, enc.base_resolution, int(offs[-1]), enc.level_dim)


def step_reference(ref, rays, t_rand, target, weight, ray_ids, S, **kw):
    """rehearse() for the rays `ray_ids` of a batch (weight: the whole batch's), on the oracle encoder's features of the table as
    stored (kw: rehearse()'s, `act` among them).  -> the rehearsal's dict plus emb_g (the table gradient) and rays (ray_ids)."""
    ids = torch.as_tensor(list(ray_ids))
    with torch.no_grad():
        _, pts, dist = geometry(rays[ids], t_rand[ids], S)
        x = ref.encoder(pts, BOUND).reshape(len(ids), S, 32)
        out = rehearse(x, dist, target[ids], weight[ids], ref.layers, **kw)
        out["emb_g"] = table_gradient(out["dx"], pts, ref)
    out["rays"] = ids
    return out


def ratios(got, want, tol_table=TOL_TABLE):
    """Every figure of the comparison as a fraction of its tolerance: dict name -> ratio.  got / want: acc, loss, packed, emb_g
    (`want` may hold fewer rays: got['acc'] is then taken at want['rays']).  Exact zeros are the caller's business."""
    acc = np.asarray(got["acc"], np.float64)
    if "rays" in want and len(acc) != len(want["acc"]):
        acc = acc[np.asarray(want["rays"])]
    out = {"acc": rel_l2(acc, want["acc"]) / TOL_ACC}
    lw = float(want["loss"])
    out["loss"] = abs(float(got["loss"]) - lw) / max(abs(lw), 1e-300) / TOL_LOSS
    for name, a, b in zip(BLOCKS, unpack(torch.as_tensor(got["packed"]).double()), unpack(torch.as_tensor(want["packed"]).double())):
        out[name] = rel_l2(a.numpy(), b.numpy()) / TOL_GRAD
    out["table"] = rel_l2(got["emb_g"], want["emb_g"]) / tol_table
    return out


# ---- faults: what a subtly wrong kernel would compute ------------------------------------------------------------------------------------
# Every builder returns the `fault` dict of rehearse() for the rays `ids` (sorted global ray numbers) of a case (n, S); items and slabs
# are chosen by the caller among those that touch `ids`.
def _local(ids):
    return {int(r): i for i, r in enumerate(ids)}


def _count_items(n, S, ids, items, value):
    loc = _local(ids)
    c = torch.ones(len(ids), S)
    for it in items:
        r, a, e = item_points(n, S, it)
        if r in loc:
            c[loc[r], a:e] = value
    return c


def fault_item_dropped(n, S, ids, item):
    """A wave never ran its item: no sums, no feature gradients, and no loss share if it was the ray's first range."""
    c = _count_items(n, S, ids, [item], 0.0)
    f = dict(count=c, stored=c)
    if item % backward16_parts(n, S) == 0:
        lc = torch.ones(len(ids))
        lc[_local(ids)[item // backward16_parts(n, S)]] = 0.0
        f["loss_count"] = lc
    return f


def fault_slab_dropped(n, S, ids, slab):
    """The reducer skipped a slab: the sums and loss shares of its items are gone, the feature gradients are not."""
    parts = backward16_parts(n, S)
    items = slab_items(n, S, slab)
    lc = torch.ones(len(ids))
    loc = _local(ids)
    for it in items:
        if it % parts == 0 and it // parts in loc:
            lc[loc[it // parts]] = 0.0
    return dict(count=_count_items(n, S, ids, items, 0.0), loss_count=lc)


def fault_item_twice(n, S, ids, item):
    """An item ran on two waves: its sums (and loss share) count twice, its feature gradients are stored twice (same values)."""
    parts = backward16_parts(n, S)
    f = dict(count=_count_items(n, S, ids, [item], 2.0))
    if item % parts == 0:
        lc = torch.ones(len(ids))
        lc[_local(ids)[item // parts]] = 2.0
        f["loss_count"] = lc
    return f


def fault_weight_shifted(weight, ids, shift):
    """weight[r] read at r + shift (clamped to the batch)."""
    idx = (torch.as_tensor(list(ids)) + shift).clamp(0, weight.numel() - 1)
    return dict(weight_read=weight[idx])


def fault_loss_per_range(n, S, ids):
    """loss_part added once per tile range instead of once per ray."""
    return dict(loss_count=torch.full((len(ids),), float(backward16_parts(n, S))))


def fault_bias_group_lost(n, S, ids, item, group, layer3=False):
    """The fold lost a lane group's share of an item's bias sums: the hidden layers' biases miss the four points lane group `group` holds
    of every tile (tr16_get: points 4 g .. 4 g + 3), or -- layer3 -- db3 misses the item's 16-point tiles altogether (db3 lives in
    lane group 0 alone)."""
    loc = _local(ids)
    r, a, e = item_points(n, S, item)
    c = torch.ones(len(ids), S)
    s = torch.arange(a, e)
    if layer3:
        c[loc[r], s] = 0.0
        return dict(bias3_count=c)
    c[loc[r], s[(s % 16) // 4 == group]] = 0.0
    return dict(bias_count=c)


def fault_padding_contributes(n, S, ids, rays, tail_dist=False):
    """The padding lanes of a ragged last tile are not masked: each repeats the ray's last sample (the features the kernels load for
    them) with the distance of an interior sample -- what sample_dist's formula gives past the end of a ray whose depths go on.
    tail_dist: with the last sample's own 1e-10 |d| instead (see test_mlp16_oracle_cpu.py: invisible, and harmless)."""
    pad = 16 * n_tiles(S) - S
    idx = torch.as_tensor(list(ids))
    dn = rays[idx, 3:6].double().norm(dim=-1)
    step = (rays[idx, 7] - rays[idx, 6]).double() / max(S - 1, 1)
    d = (1e-10 if tail_dist else step) * dn
    er = torch.arange(len(ids)).repeat_interleave(pad)
    return dict(extra=(er, torch.full_like(er, S - 1), d.repeat_interleave(pad)))


def fault_first_tile_rounded_up(n, S, ids):
    """The prefetch of an item's first tile takes first_tile rounded up where the loop rounds down: wherever the two differ (uneven
    ranges) the first tile of the range runs on the NEXT tile's features (clamped to the ray's last sample)."""
    parts = backward16_parts(n, S)
    lo, hi = tile_ranges(S, parts), tile_ranges(S, parts, round_up=True)
    src = torch.arange(S).repeat(len(ids), 1)
    hit = 0
    for p in range(parts):
        if hi[p] != lo[p] and lo[p] < lo[p + 1]:
            a, e = 16 * lo[p], min(S, 16 * lo[p] + 16)
            src[:, a:e] = (torch.arange(a, e) + 16 * (hi[p] - lo[p])).clamp(max=S - 1)
            hit += 1
    return dict(feature_source=src) if hit else None


# ---- head faults: a kernel whose output head is not the one of the cfg ----------------------------------------------------------------------
def fault_head_backward(other):
    """The backward kernel got another head than the forward: sigma and its derivative recomputed with `other`."""
    return dict(head_backward=other)


def fault_head_slope(slope):
    """The leaky head's derivative for z4 <= 0 is `slope` (1: the identity's; 0: a plain ReLU's) where 0.01 belongs."""
    return dict(head_slope=float(slope))


def fault_head_forward_items(ids, ranges):
    """`ranges`: (global ray, first sample, end sample) of the work items or tiles whose forward took head 0."""
    loc = _local(ids)
    return dict(head_forward_items=[(loc[r], a, e) for r, a, e in ranges])
