"""mlp16_train_kernel (MLP forward, loss and backward of a small bf16 training step in one launch) against the kernel pair it
replaces, which NAF_CFG_MLP_TWO_KERNELS keeps: BIT equality of everything a step leaves behind.

The bit rule holds by construction: the kernel hands its waves the work items of mlp16_backward_kernel one to one and folds the
same four consecutive items into each slab, the line integral of a ray is added in the order of the forward kernels, and the tile
arithmetic is the same code.  So nothing here has a tolerance.  Every case has at least 2^13 points (below that the table scatter
uses fp32 atomics, whose order is not reproducible from run to run whatever the MLP kernels do)."""
import pytest
import torch

from _naf_helpers import crossing_rays, naf_pair

pytestmark = pytest.mark.gpu

# (rays, samples, log2 table rows): chest_50's step (1 024 x 192: 12 tiles, three ranges of four per ray, 12-wave workgroups);
# 5 and 7 tiles with a ragged last tile (uneven ranges 1-2-2 and 2-2-3); a ragged last workgroup (1 001 rays); and the ray counts
# that give 1, 2, 4, 6 and 12 ranges per ray (4-wave workgroups for 1, 2, 4).
CASES = [(1024, 192, 19), (1024, 75, 16), (1024, 100, 16), (1001, 192, 16), (2048, 192, 16), (1536, 192, 16), (768, 64, 16),
         (512, 192, 16), (256, 192, 16)]


def _run(n, S, log2T, flags, steps, adam):
    from neuralvolumetricreconstructionformedicalimages_amd.engine import NAFEngine
    rays = crossing_rays(n, seed=41).cuda()
    target = torch.rand(n, generator=torch.Generator().manual_seed(5)).cuda() * 0.2
    weight = torch.full((n,), 1.0 / n, device="cuda")
    net, _ = naf_pair(seed=37, log2T=log2T, oracle=False)
    eng = NAFEngine(net, S, perturb=True, lr=3e-3, table_dtype=torch.bfloat16, fuse_table_adam=adam, cfg_flags=flags)
    out = []
    for step in range(steps):
        if adam:
            eng.train_step(rays, target, weight, ray_base=step * n)
        else:                                                # naf_render_train: the gradients themselves
            eng.backward(rays, target, weight, ray_base=step * n)
        out += [eng.acc[:n].clone(), eng.loss.clone()]
    torch.cuda.synchronize()
    out += [eng.emb.clone(), eng.emb_m.clone(), eng.emb_v.clone(), eng.emb_g.clone(), eng.mlp.clone(), eng.mlp_m.clone(), eng.mlp_v.clone(),
            eng.mlp_g.clone()]
    if eng.emb_lp is not None:
        out.append(eng.emb_lp.clone())
    return out


@pytest.mark.parametrize("steps", [1, 8])
@pytest.mark.parametrize("n,S,log2T", CASES)
def test_one_launch_step_equals_the_kernel_pair_bit_for_bit(n, S, log2T, steps):
    """naf_render_train_adam: line integrals and loss of every step, table (+ 16-bit shadow), MLP parameters and all moments."""
    from neuralvolumetricreconstructionformedicalimages_amd import _abi
    one = _run(n, S, log2T, 0, steps, True)
    two = _run(n, S, log2T, _abi.CFG_MLP_TWO_KERNELS, steps, True)
    assert len(one) == len(two)
    for i, (a, b) in enumerate(zip(one, two)):
        assert torch.equal(a, b), (i, float((a.float() - b.float()).abs().max()))
    assert float(one[0].abs().max()) > 0 and float(one[1]) > 0          # it rendered something and had a loss
    fresh = naf_pair(seed=37, log2T=log2T, oracle=False)[0]
    assert not torch.equal(one[2 * steps + 4], fresh.packed_mlp().detach().cuda())      # ... and trained the MLP


@pytest.mark.parametrize("n,S,log2T", CASES[:4])
def test_one_launch_gradients_equal_the_kernel_pair_bit_for_bit(n, S, log2T):
    """naf_render_train (no optimiser): the table gradient -- the scatter of dfeat -- and the MLP gradient."""
    from neuralvolumetricreconstructionformedicalimages_amd import _abi
    one = _run(n, S, log2T, 0, 1, False)
    two = _run(n, S, log2T, _abi.CFG_MLP_TWO_KERNELS, 1, False)
    for i, (a, b) in enumerate(zip(one, two)):
        assert torch.equal(a, b), (i, float((a.float() - b.float()).abs().max()))
    assert float(one[5].abs().max()) > 0 and float(one[9].abs().max()) > 0      # emb_g, mlp_g
