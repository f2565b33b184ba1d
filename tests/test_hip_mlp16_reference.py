"""The bf16 MLP step kernels (mlp16_forward_split_kernel, mlp16_backward_kernel, mlp16_train_kernel<4> / <12>, mlp16_fold_slab,
slab_reduce_block) against the float64 rehearsal of tests/_mlp16_oracle.py, at the work-item layouts a training step takes.

Every case runs through NAFEngine.backward (naf_render_train: the loss is formed in the kernel) on a bf16 table with the atomic
scatter (the table gradient is then a plain fp32 sum of the stored bf16 feature gradients), once as the step picks its kernels
(flags = 0) and once with NAF_CFG_MLP_TWO_KERNELS, so the one-launch kernel and the pair are each held to the reference on their own.

| (rays, S)   | what it reaches |
|---|---|
| (1024, 192) | chest step: 3 parts x 4 tiles, 12-wave workgroups, 768 slabs, the four-chain loop of the reducer |
| (256, 192)  | 12 parts, 3 072 items of one tile |
| (300, 192)  | parts = 10: the pair even without the flag; uneven ranges; rays straddle workgroups |
| (700, 100)  | 7 tiles in 4 parts (1-2-2-2), ragged last tile, 4-wave workgroups |
| (1001, 75)  | 5 tiles in 3 parts (1-2-2), ragged last workgroup and slab |
| (3072, 40)  | parts = 1, the largest one-launch step, ragged tile |
| (3100, 40)  | above the one-launch limit: 3 100 items on 3 072 waves, 28 waves take a second item (and prefetch its first tile) |
| (5000, 20)  | several items per wave, S = one full tile + 4 points |
| (6, 1030)   | S > kMaxSamplesLds: sample_dist without the depth buffer, 65 tiles in 12 parts |
| (24, 7)     | one ragged tile per ray, fewer items than one workgroup holds waves |

Weight patterns (per-ray weights are unequal wherever they are not zero): `zero` -- loss and every gradient are exactly 0, the line
integrals still match; `probe` -- at most 16 weighted rays (both ends of the batch, either side of every 3 072-item and of the last
slab boundary, random ones), reference over those rays alone; `dense` (n S <= 2^16) -- all rays weighted, full reference.

Tolerances (those of test_hip_fused.py's emulation test and its rationale; tests/test_mlp16_oracle_cpu.py shows what they leave to
spare and that each fault of its list lands outside): line integrals 2e-6 relative L2 on the probes + 48 random rays, loss 1e-5, each
of the eight gradient blocks 2e-4, table gradient 2e-4 (3e-3 through the binned scatter's bf16 records)."""
import functools

import pytest
import torch

import _mlp16_oracle as O
from _naf_helpers import naf_pair

pytestmark = pytest.mark.gpu

SEED = 37


@functools.lru_cache(maxsize=None)
def _ref():
    """The oracle twin, its table rounded once like the engine's bf16 shadow."""
    return O.round_table_once(naf_pair(seed=SEED, log2T=12)[1])


@functools.lru_cache(maxsize=None)
def _want(n, S, dense):
    """The reference of a case: computed once, shared by both kernel routes and (acc) by the zero pattern; read-only."""
    pattern = "dense" if dense else "probe"
    rays, t_rand, target, _ = O.case_inputs(n, S)
    return O.step_reference(_ref(), rays, t_rand, target, O.case_weight(n, S, pattern), O.reference_rays(n, S, pattern), S)


def _step(n, S, pattern, flags, scatter_mode=1):
    from neuralvolumetricreconstructionformedicalimages_amd.engine import NAFEngine
    net = naf_pair(seed=SEED, log2T=12, oracle=False)[0]
    rays, t_rand, target, _ = O.case_inputs(n, S)
    weight = O.case_weight(n, S, pattern)
    eng = NAFEngine(net, S, perturb=True, table_dtype=torch.bfloat16, scatter_mode=scatter_mode, cfg_flags=flags)
    acc = eng.backward(rays.cuda(), target.cuda(), weight.cuda(), t_rand=t_rand.cuda())
    torch.cuda.synchronize()
    return dict(acc=acc.double().cpu().numpy(), loss=float(eng.loss.item()), packed=eng.mlp_g.cpu(), emb_g=eng.emb_g.cpu().numpy())


def _flags(two_kernels):
    from neuralvolumetricreconstructionformedicalimages_amd import _abi
    return _abi.CFG_MLP_TWO_KERNELS if two_kernels else 0


_RUNS = [(n, S, p) for n, S in O.CASES for p in O.patterns(n, S)]


@pytest.mark.parametrize("two_kernels", [False, True], ids=["auto", "pair"])
@pytest.mark.parametrize("n,S,pattern", _RUNS, ids=[f"{n}x{S}-{p}" for n, S, p in _RUNS])
def test_bf16_training_step_matches_the_float64_rehearsal(n, S, pattern, two_kernels):
    got = _step(n, S, pattern, _flags(two_kernels))
    want = _want(n, S, pattern == "dense")
    if pattern == "zero":                                    # 0 x finite: no tolerance
        ratio = O.rel_l2(got["acc"][want["rays"].numpy()], want["acc"].numpy()) / O.TOL_ACC
        print(f"mlp16 ({n}, {S}) zero {'pair' if two_kernels else 'auto'}: acc {ratio:.3f} of its tolerance")
        assert got["loss"] == 0.0 and not got["packed"].any() and not got["emb_g"].any()
        assert ratio < 1.0
        return
    r = O.ratios(got, _numpy(want))
    worst = max(r, key=r.get)
    print(f"mlp16 ({n}, {S}) {pattern} {'pair' if two_kernels else 'auto'}: worst {worst} {r[worst]:.3f} of its tolerance | " +
          " ".join(f"{k}={v:.3f}" for k, v in r.items()))
    assert r[worst] < 1.0, r


def test_chest_step_through_the_binned_scatter():
    """(1024, 192) probe with the scatter left to choose (binned: the slab reduction then rides in spare workgroups of the scatter's
    first launch).  MLP figures as above; the table gradient to the 3e-3 that bf16 records are granted (test_hip_fused.py,
    test_binned_scatter_equals_atomic_scatter)."""
    n, S = 1024, 192
    got = _step(n, S, "probe", 0, scatter_mode=None)
    r = O.ratios(got, _numpy(_want(n, S, False)), tol_table=O.TOL_TABLE_BINNED)
    worst = max(r, key=r.get)
    print(f"mlp16 ({n}, {S}) probe binned: worst {worst} {r[worst]:.3f} of its tolerance | " + " ".join(f"{k}={v:.3f}" for k, v in r.items()))
    assert r[worst] < 1.0, r


def _numpy(out):
    return {k: (v.double().numpy() if torch.is_tensor(v) and k != "rays" else v) for k, v in out.items()}
