"""The profile names of a step (naf_profile_enable / naf_profile_collect): bench.py's per-kernel table and its rooflines key on them
(encode_kernel, scatter_bin_kernel, scatter_reduce_kernel, hash_backward_kernel, mlp_forward_kernel, mlp_backward_kernel, adam_kernel),
so a slip in a name would silently empty a column.  Each route below runs ONE training step (or one forward) between
profile_enable(True) and profile_collect() and is held to the whole {name: launches} dictionary.  The dictionaries were taken from
the library as it stood before the step's launches moved to naf_host.h's launch() / launch_as(), and read against
csrc/render_step.h, scatter_host.h and encode_kernel.h; nothing here looks at a time.

Shapes: L = 16, H = 16, C = 2, table 2^12, 64 samples per ray; 16 rays are 1 024 points (below kBinMinPoints: the atomic scatter),
128 rays exactly 2^13 (the binned scatter).  The 16-point bf16 kernels are timed under the aggregate names on purpose:
mlp16_forward_split_kernel and mlp16_forward_kernel as mlp_forward_kernel, mlp16_backward_kernel as mlp_backward_kernel,
mlp16_train_kernel as mlp_train_kernel.  levels_gather_kernel is reached through test_hip_levels.py's single-process helper
(two virtual ranks, no process group)."""
import pytest
import torch

from test_hip_levels import _batch, _levels_step, _make

pytestmark = pytest.mark.gpu

S = 64


def _levels(prefix):
    return {f"{prefix}{l:02d}": 1 for l in range(16)}


def _engine(table=torch.bfloat16, **kw):
    from neuralvolumetricreconstructionformedicalimages_amd.engine import NAFEngine
    return NAFEngine(_make(log2T=12), S, perturb=True, lr=1e-2, table_dtype=table, seed=5, **kw)


def _train(n_rays, **kw):
    def run():
        eng = _engine(**kw)
        rays, target, mask = _batch(n_rays, S)
        weight = mask.float() / mask.float().sum()
        return lambda: eng.train_step(rays, target, weight)
    return run


def _fused_forward():
    from neuralvolumetricreconstructionformedicalimages_amd import _abi, fused
    net = _make(log2T=12)
    rays = _batch(16, S)[0]

    def step():
        with torch.no_grad(), fused.scatter_mode(_abi.SCATTER_AUTO, flags=_abi.CFG_FORWARD_FUSED):
            fused.fused_render(rays, net, S, True, mlp_precision=_abi.BF16)
    return step


def _levels_gather():
    from neuralvolumetricreconstructionformedicalimages_amd import _abi
    eng = _engine()
    eng._levels_flags = _abi.CFG_LEVELS_GATHER_PASS
    rays, target, mask = _batch(128, S)
    weight = mask.float() / mask.float().sum()
    return lambda: _levels_step(eng, 2, rays, target, weight)


PER_LEVEL, TWO_KERNELS, ATOMIC = 1, 65536, 1        # _abi.CFG_PER_LEVEL_LAUNCHES, _abi.CFG_MLP_TWO_KERNELS, _abi.SCATTER_ATOMIC

ROUTES = {
    # the encoder, both MLP passes in one launch, the slab reduction (with the MLP's Adam), the atomic scatter, the table's Adam
    "bf16_1024_points": (_train(16), {
        "encode_kernel": 1, "mlp_train_kernel": 1, "mlp_grad_reduce_kernel": 1, "hash_backward_kernel": 1, "adam_kernel": 1}),
    "bf16_1024_points_two_mlp_kernels": (_train(16, cfg_flags=TWO_KERNELS), {
        "encode_kernel": 1, "mlp_forward_kernel": 1, "mlp_backward_kernel": 1, "mlp_grad_reduce_kernel": 1, "hash_backward_kernel": 1,
        "adam_kernel": 1}),
    # 8-byte records: the slab reduction rides on pass 1, the table's Adam on the reducer
    "bf16_8192_points": (_train(128), {
        "encode_kernel": 1, "mlp_train_kernel": 1, "scatter_bin_kernel": 1, "scatter_reduce_kernel": 1}),
    "bf16_8192_points_per_level": (_train(128, cfg_flags=PER_LEVEL), {
        **_levels("encode_kernel_L"), "mlp_train_kernel": 1, "mlp_grad_reduce_kernel": 1, **_levels("scatter_bin_kernel_L"),
        **_levels("scatter_reduce_kernel_L"), "adam_kernel": 1}),
    "bf16_8192_points_per_level_atomic": (_train(128, cfg_flags=PER_LEVEL, scatter_mode=ATOMIC), {
        **_levels("encode_kernel_L"), "mlp_train_kernel": 1, "mlp_grad_reduce_kernel": 1, **_levels("hash_backward_kernel_L"),
        "adam_kernel": 1}),
    # fp32 parity mode: the 32-point MLP kernels, the PairRecords family
    "fp32_8192_points": (_train(128, table=torch.float32), {
        "encode_kernel": 1, "mlp_forward_kernel": 1, "mlp_backward_kernel": 1, "scatter_bin_kernel": 1, "scatter_reduce_kernel": 1}),
    "fused_forward": (_fused_forward, {"fused_forward_kernel": 1}),
    # two virtual ranks of eight levels: two encodes, two MLP steps, then per owner the gather pass and the binned scatter; the MLP's Adam
    "levels_gather_pass": (_levels_gather, {
        "encode_kernel": 2, "mlp_train_kernel": 2, "mlp_grad_reduce_kernel": 2, "levels_gather_kernel": 2, "scatter_bin_kernel": 2,
        "scatter_reduce_kernel": 2, "adam_kernel": 1}),
}


@pytest.mark.parametrize("route", list(ROUTES))
def test_a_step_is_profiled_under_the_names_bench_reads(route):
    from neuralvolumetricreconstructionformedicalimages_amd import _abi
    make, want = ROUTES[route]
    step = make()
    torch.cuda.synchronize()
    _abi.profile_enable(True)
    try:
        step()
        torch.cuda.synchronize()
        got = {name: launches for name, (launches, _) in _abi.profile_collect().items()}
    finally:
        _abi.profile_enable(False)
    print(route, got)
    assert got == want
