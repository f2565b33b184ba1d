"""The output heads relu (LeakyReLU 0.01), tanh and none of every MLP kernel (last_act / last_act_grad / last_act16 of csrc/field_mlp.h
and csrc/field_mlp16.h, a run-time argument of each launch in csrc/render_step.h) against the float64 rehearsal with that head
(head / head_grad of tests/_mlp16_oracle.py; cases, seeds, tolerances and the leaky head's undecided points: OUTPUT HEADS in
tests/_mlp32_oracle.py; tests/test_mlp_heads_oracle_cpu.py derives them and shows that every head fault lands outside).  The sigmoid
head is what tests/test_hip_mlp16_reference.py and tests/test_hip_mlp32_reference.py restate; it returns here for saturation only.

Training steps run through NAFEngine.backward with the atomic scatter, as in those modules:
  * 16-point kernels (bf16 table, C = 2), flags = 0 and NAF_CFG_MLP_TWO_KERNELS: (1024, 192) probe -- mlp16_train_kernel<12> / the
    split forward and mlp16_backward_kernel; (700, 100) probe -- 4-wave workgroups, ragged tile; (3100, 40) probe -- above the
    one-launch limit, a wave's second item; (24, 7) dense; the zero pattern at (24, 7) with exact zeros;
  * 32-point kernels, f32 and bf16-8x4: (37, 50) dense, (1, 33) dense (the one-point tile), (2100, 40) probe (a wave's second ray and
    its prefetched tile).
Forward-only heads at (41, 17) and (41, 64), f32 and bf16, with NAF_CFG_FORWARD_FUSED where the shape has that kernel (bf16): the
per-sample sigma of naf_render_forward_samples and naf_field_forward on the same points against forward_points(..., act) at relative
L2 2e-6 (the sigmoid row's bar in tests/test_hip_raymarch_reference.py); optical_depth[:, -1] against acc, and acc bit-equal with and
without the per-sample outputs, with sigma negative for some samples (every one of these heads is, on these networks).
Saturation, sigmoid and tanh with b3 = +100 and -100 at (24, 7) dense in both precisions: y (1 - y) and 1 - y y formed from the fp32
output are exactly 0 at the limit (read from last_act_grad), so every gradient is an exact zero of either sign.

Tolerances: bf16 those of _mlp16_oracle (acc 2e-6, loss 1e-5, gradient blocks and table 2e-4); f32 measured per head
(_mlp32_oracle.HEAD_F32_TOL: acc 2e-6, loss 8e-7 .. 9e-7, gradient blocks 4e-6 .. 5e-6, table 2e-6).  Every case prints its worst
fraction of a tolerance; DESIGN.md section 2 has the figures measured on an MI355X."""
import functools

import numpy as np
import pytest
import torch

import _mlp32_oracle as M
import _raymarch_oracle as RM
from _naf_helpers import naf_pair

pytestmark = pytest.mark.gpu
O = M.O
SIGMA_TOL = 2e-6


def _abi():
    from neuralvolumetricreconstructionformedicalimages_amd import _abi
    return _abi


def _pair(layout, act, oracle):
    lay = M.HEAD_LAYOUTS[layout]
    return naf_pair(seed=M.HEAD_SEEDS[act], log2T=12, L=lay.L, C=lay.C, last_activation=act, oracle=oracle)


@functools.lru_cache(maxsize=None)
def _ref(layout, act):
    """The oracle twin; a bf16 table rounded once like the engine's shadow."""
    ref = _pair(layout, act, True)[1]
    return ref if M.HEAD_LAYOUTS[layout].table_dtype == torch.float32 else O.round_table_once(ref)


@functools.lru_cache(maxsize=None)
def _wants(layout, n, S, pattern, act):
    """The references of a case (more than one: the branch combinations of a relu case's undecided points); computed once, read-only."""
    return [M.numpy_dict(w) for w in M.head_references(layout, _ref(layout, act), n, S, pattern, act)]


def _step(layout, n, S, pattern, act, flags=0, b3=None):
    from neuralvolumetricreconstructionformedicalimages_amd.engine import NAFEngine
    A = _abi()
    lay = M.HEAD_LAYOUTS[layout]
    net = _pair(layout, act, False)[0]
    if b3 is not None:
        net.layers[3].bias.data.fill_(b3)
    rays, t_rand, target, weight, _ = M.head_inputs(layout, n, S, pattern)
    eng = NAFEngine(net, S, perturb=True, table_dtype=lay.table_dtype, mlp_precision=A.F32 if layout == "f32" else A.BF16, scatter_mode=1,
                    cfg_flags=flags)
    acc = eng.backward(rays.cuda(), target.cuda(), weight.cuda(), t_rand=t_rand.cuda())
    torch.cuda.synchronize()
    return dict(acc=acc.double().cpu().numpy(), loss=float(eng.loss.item()), packed=eng.mlp_g.cpu(), emb_g=eng.emb_g.float().cpu().numpy())


def _hold(label, layout, act, got, wants):
    r = M.best_ratios(layout, act, got, wants)
    order = sorted(r, key=r.get, reverse=True)
    print(f"heads {label}: worst {order[0]} {r[order[0]]:.3f} of its tolerance | " + " ".join(f"{k}={r[k]:.3f}" for k in order) +
          (f" | best of {len(wants)} branch combinations" if len(wants) > 1 else ""))
    assert r[order[0]] < 1.0, r


# ---- training steps -----------------------------------------------------------------------------------------------------------------------
_RUNS16 = [(act, n, S, p) for act in M.HEAD_ACTS for n, S, p in M.HEAD_CASES["bf16-16x2"]]


@pytest.mark.parametrize("two_kernels", [False, True], ids=["auto", "pair"])
@pytest.mark.parametrize("act,n,S,pattern", _RUNS16, ids=[f"{a}-{n}x{S}-{p}" for a, n, S, p in _RUNS16])
def test_16_point_step_matches_the_float64_rehearsal_of_its_head(act, n, S, pattern, two_kernels):
    got = _step("bf16-16x2", n, S, pattern, act, _abi().CFG_MLP_TWO_KERNELS if two_kernels else 0)
    _hold(f"bf16-16x2 {act} ({n}, {S}) {pattern} {'pair' if two_kernels else 'auto'}", "bf16-16x2", act, got, _wants("bf16-16x2", n, S, pattern, act))


@pytest.mark.parametrize("act", M.HEAD_ACTS)
def test_16_point_step_with_zero_weights_gives_exact_zeros(act):
    n, S = M.HEAD_ZERO_CASE
    got = _step("bf16-16x2", n, S, "zero", act)
    want = _wants("bf16-16x2", n, S, "dense", act)[0]
    ratio = M.rel_l2(got["acc"], want["acc"]) / O.TOL_ACC
    print(f"heads bf16-16x2 {act} ({n}, {S}) zero: acc {ratio:.3f} of its tolerance")
    assert got["loss"] == 0.0 and not got["packed"].any() and not got["emb_g"].any()                  # 0 x finite: no tolerance
    assert ratio < 1.0


_RUNS32 = [(layout, act, n, S, p) for layout in ("f32", "bf16-8x4") for act in M.HEAD_ACTS for n, S, p in M.HEAD_CASES[layout]]


@pytest.mark.parametrize("layout,act,n,S,pattern", _RUNS32, ids=[f"{l}-{a}-{n}x{S}-{p}" for l, a, n, S, p in _RUNS32])
def test_32_point_step_matches_the_float64_rehearsal_of_its_head(layout, act, n, S, pattern):
    _hold(f"{layout} {act} ({n}, {S}) {pattern}", layout, act, _step(layout, n, S, pattern, act), _wants(layout, n, S, pattern, act))


def test_the_relu_cases_meet_the_undecided_point_condition_on_these_networks():
    """tests/test_mlp_heads_oracle_cpu.py checks the condition on oracle_net's networks; these are naf_pair's (the same weights)."""
    for layout, cases in M.HEAD_CASES.items():
        for n, S, pattern in cases:
            und, nearest = M.undecided_points(layout, n, S, pattern, _wants(layout, n, S, pattern, "relu")[0])
            print(f"heads {layout} relu ({n}, {S}) {pattern}: {len(und)} undecided, smallest |z4| / delta {nearest:.3g}")
            assert len(und) <= M.HEAD_MAX_UNDECIDED[M.head_precision(layout)]


# ---- forward-only kernels ---------------------------------------------------------------------------------------------------------------
# Seeds of the forward cases.  The forward is continuous in z4, so the leaky head needs no seed without undecided points here, and
# HEAD_SEEDS' 222 leaves every one of these samples at z4 < 0: in f32 the relu cases take 29, which puts half of the samples on
# either branch.  In bf16 they keep 222, for a reason read off the reference alone (on_a_bf16_boundary): the oracle encoder sums a
# level's corners without fma, the kernels' encoder with (as oracle/hash_ref.c), so a reference feature within one fp32 ulp of a bf16
# rounding boundary may enter the MLP one bf16 step away.  Seed 29 has 1 such feature at (41, 17) and 5 at (41, 64), seed 222 none.
# One step of one feature is 3e-5 of one sigma; against |sigma| = 0.48 of a head centred on 0 that is 7e-5 relative L2, where the
# sigmoid row's |sigma| = 13 leaves the 2e-6 room for it.  Measured on an MI355X with seed 29 in bf16: 34.0 x the bar at (41, 17),
# 3.29 x at (41, 64), largest |difference| 3.28e-5 and 6.07e-6 at single samples, fused and two-kernel forward alike, f32 0.22.
# The leaky head's z4 > 0 branch in bf16 is held by the training steps above (19, 12, 2, 2 and 9, 2 weighted points).
FORWARD_SEEDS = {("relu", "f32"): 29}


@functools.lru_cache(maxsize=None)
def _forward_pair(act, prec):
    return naf_pair(seed=FORWARD_SEEDS.get((act, prec), M.HEAD_SEEDS[act]), last_activation=act, oracle=True)


def on_a_bf16_boundary(x):
    """How many fp32 features round to another bf16 when moved by one ulp either way."""
    up, down = torch.nextafter(x, torch.full_like(x, 10.0)), torch.nextafter(x, torch.full_like(x, -10.0))
    return int(((M.bf16_round(up) != M.bf16_round(x)) | (M.bf16_round(down) != M.bf16_round(x))).sum())


def _sigma_reference(act, rays, z, prec):
    """sigma of the float64 rehearsal with the head on the oracle encoder's features, as tests/test_hip_raymarch_reference.py."""
    ref = _forward_pair(act, prec)[1]
    rnd = M.identity if prec == "f32" else M.bf16_round
    with torch.no_grad():
        pts = O.R.points_on_rays(torch.from_numpy(rays), torch.from_numpy(z), O.BOUND).reshape(-1, 3)
        x = ref.encoder(pts, O.BOUND)
        sig = O.forward_points(rnd(x.double()), O.mlp_params(ref.layers, rnd, torch.float64), rnd, act)[3]
    return sig.numpy().reshape(z.shape), pts, on_a_bf16_boundary(x)


_FORWARD = [(act, prec, fused, S) for act in M.HEAD_ACTS for prec, fused in (("f32", False), ("bf16", False), ("bf16", True)) for S in (17, 64)]


@pytest.mark.parametrize("act,prec,fused_kernel,S", _FORWARD, ids=[f"{a}-{p}{'-fused' if f else ''}-41x{S}" for a, p, f, S in _FORWARD])
def test_forward_only_kernels_take_the_head(act, prec, fused_kernel, S):
    from neuralvolumetricreconstructionformedicalimages_amd import fused
    A = _abi()
    n = 41
    net = _forward_pair(act, prec)[0]
    rays = RM.make_rays(n, 19)
    t_rand = np.random.default_rng(S).random((n, S)).astype(np.float32)
    z = RM.sample(rays, t_rand, S, True, 0.3)[0]
    precision = A.F32 if prec == "f32" else A.BF16
    rd, td = torch.from_numpy(rays).cuda(), torch.from_numpy(t_rand).cuda()
    sg_ref, pts, boundary = _sigma_reference(act, rays, z, prec)
    saved = fused.forward_fused
    fused.forward_fused = fused_kernel
    try:
        assert bool(fused.render_cfg(net, S, True, precision, forward_only=True).flags & A.CFG_FORWARD_FUSED) == fused_kernel
        acc, sigma, tau = fused.render_samples(rd, net, S, True, t_rand=td, mlp_precision=precision)
        only = fused.render_samples(rd, net, S, True, t_rand=td, mlp_precision=precision, want_sigma=False, want_depth=False)[0]
        field = fused.field_query(net, pts.cuda(), mlp_precision=precision)
        torch.cuda.synchronize()
    finally:
        fused.forward_fused = saved
    sg, fq = sigma.cpu().numpy(), field.cpu().numpy().reshape(n, S)
    assert np.isfinite(sg).all() and (sg < 0).any() and (sg_ref < 0).any()
    if act == "relu" and prec == "f32":                                # both branches of the leaky head
        assert min(int((sg_ref > 0).sum()), int((sg_ref < 0).sum())) > sg.size // 4
    if act == "relu" and prec == "bf16":                               # see FORWARD_SEEDS
        assert boundary == 0
    assert torch.equal(only, acc)                                      # the per-sample outputs change no bit of acc
    f_sg, f_fq = M.rel_l2(sg, sg_ref) / SIGMA_TOL, M.rel_l2(fq, sg_ref) / SIGMA_TOL
    tau_ref, scale = RM.running_depth(sg, z, rays)
    f_acc = float((np.abs(acc.cpu().numpy() - tau_ref[:, -1]) / scale[:, -1]).max()) / RM.TOL_SUM
    f_last = float((np.abs(tau[:, -1].cpu().numpy().astype(np.float64) - acc.cpu().numpy()) / scale[:, -1]).max()) / RM.TOL_TAU
    print(f"heads forward {act} {prec}{' fused' if fused_kernel else ''} ({n}, {S}): sigma {f_sg:.3f}, field sigma {f_fq:.3f}, acc {f_acc:.3f}, "
          f"tau[-1] against acc {f_last:.3f} of their tolerances; largest |sigma difference| {np.abs(sg - sg_ref).max():.3g}, "
          f"{int((sg < 0).sum())} of {sg.size} sigma < 0, {boundary} reference features within an ulp of a bf16 boundary")
    assert f_sg < 1.0 and f_fq < 1.0 and f_acc < 1.0 and f_last < 1.0


# ---- saturation ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["f32", "bf16"])
@pytest.mark.parametrize("act", ["sigmoid", "tanh"])
def test_saturated_heads_give_the_limit_and_exact_zero_gradients(act, prec):
    """b3 = +-100 puts every z4 within 1 of +-100.  From the code: expf(-z) vanishes against 1 for z ~ +100, so the sigmoid is 1.0f
    and y (1 - y) = 0; tanhf(+-100) = +-1.0f and 1 - y y = 0.  The sigmoid of z ~ -100 is 1 / (1 + expf(100)) = 3.7e-44, an fp32
    subnormal: the MI355X returns +0 for it in every forward kernel (the division flushes the subnormal quotient), which is the limit's
    bits as well -- and were it kept, g4 = gsig y (1 - y) < 4e-3 x 1.1e-43 would still be below half the smallest subnormal.  Every
    gradient is therefore an exact zero of either sign in all four cases.  acc and loss are finite and inside the head's tolerances
    of the float64 reference, except the sigmoid's acc at -100: the reference's 3e-44 has no fp32 neighbour but 0, so acc is held
    to the exact 0 that sigma = 0 gives."""
    from neuralvolumetricreconstructionformedicalimages_amd import fused
    A = _abi()
    layout = "f32" if prec == "f32" else "bf16-16x2"
    n, S = 24, 7
    rays, t_rand, _, _, _ = M.head_inputs(layout, n, S, "dense")
    tol = M.head_tolerances(layout, act)
    for b3 in (100.0, -100.0):
        ref = M.oracle_net(layout, M.HEAD_SEEDS[act], act=act)
        assert all(torch.equal(a, b) for a, b in zip(ref.state_dict().values(), _ref(layout, act).state_dict().values()))
        ref.layers[3].bias.data.fill_(b3)
        want = M.numpy_dict(M.head_reference(layout, ref, n, S, "dense", act))
        assert float(np.abs(np.abs(want["z4"]) - 100.0).max()) < 1.0
        got = _step(layout, n, S, "dense", act, b3=b3)
        net = _pair(layout, act, False)[0]
        net.layers[3].bias.data.fill_(b3)
        sigma = fused.render_samples(rays.cuda(), net, S, True, t_rand=t_rand.cuda(), mlp_precision=A.F32 if prec == "f32" else A.BF16)[1]
        sg = sigma.cpu().numpy()
        limit = {("sigmoid", 100.0): 1.0, ("sigmoid", -100.0): 0.0, ("tanh", 100.0): 1.0, ("tanh", -100.0): -1.0}[act, b3]
        print(f"heads saturation {act} {prec} b3 = {b3:+.0f}: sigma in [{sg.min():.9g}, {sg.max():.9g}], acc[0] {got['acc'][0]:.9g}, loss {got['loss']:.9g}")
        assert np.isfinite(got["acc"]).all() and np.isfinite(got["loss"])
        assert (sg.view(np.uint32) == np.float32(limit).view(np.uint32)).all()                      # the limit's bits
        if (act, b3) == ("sigmoid", -100.0):
            assert 0.0 < float(want["acc"].max()) < 2.0 ** -140 and not got["acc"].any()
        else:
            f_acc = M.rel_l2(got["acc"], want["acc"]) / tol["acc"]
            print(f"heads saturation {act} {prec} b3 = {b3:+.0f}: acc {f_acc:.3f} of its tolerance")
            assert f_acc < 1.0
        f_loss = abs(got["loss"] - float(want["loss"])) / abs(float(want["loss"])) / tol["loss"]
        print(f"heads saturation {act} {prec} b3 = {b3:+.0f}: loss {f_loss:.3f} of its tolerance")
        assert f_loss < 1.0
        packed, emb_g = got["packed"].numpy(), got["emb_g"]
        assert np.isfinite(packed).all() and np.isfinite(emb_g).all() and not packed.any() and not emb_g.any()
