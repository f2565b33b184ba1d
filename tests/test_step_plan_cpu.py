"""The launch plan of the step's MLP kernels (csrc/mlp_step_plan.h, which the host drivers of csrc/render_step.h call for every such
decision) held to its restatement in tests/_mlp16_oracle.py and to the invariants the kernel comments rely on.  The plan is printed
by tools/step_plan_host_check.cpp, built once for the host with AddressSanitizer and UBSan and run as a process of its own.

Grid: n_rays 0, every value 1 .. 3 100, 4 096, 65 536 and floor(2^31 / 192); n_samples 1, 2, 7, 15, 16, 17, 50, 63, 64, 65, 192,
200, 511, 512, 513, 1 024, 1 025; flags none, NAF_CFG_MLP_TWO_KERNELS, NAF_CFG_BACKWARD_ONE_WAVE_PER_SIMD.

The forward under NAF_CFG_MLP_TWO_KERNELS: that flag keeps the kernel PAIR, whose forward is mlp16_forward_split_kernel (naf_hip.h;
tests/test_hip_mlp16_reference.py forces the pair with it to hold that kernel to float64), so the split condition is the unflagged
one.  Only NAF_CFG_BACKWARD_ONE_WAVE_PER_SIMD ("no mlp16_forward_split_kernel, no mlp16_train_kernel") turns the split off."""
import os

import pytest

import _host_check
import _mlp16_oracle as O

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TWO_KERNELS, ONE_WAVE_PER_SIMD = 65536, 128          # include/naf_hip.h
N_RAYS = list(range(0, 3101)) + [4096, 65536, (1 << 31) // 192]
N_SAMPLES = (1, 2, 7, 15, 16, 17, 50, 63, 64, 65, 192, 200, 511, 512, 513, 1024, 1025)


D = _host_check.load("step_plan")
pytestmark = _host_check.needs_compiler


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    """caps, {flags: {(n_rays, S): Plan}}: the program built and run once over the whole grid."""
    workdir = str(tmp_path_factory.mktemp("step_plan_host_check"))
    cases = [(flags, n, S) for flags in (0, TWO_KERNELS, ONE_WAVE_PER_SIMD) for n in N_RAYS for S in N_SAMPLES]
    caps, out = D.plan(D.build(workdir), workdir, cases)
    by_flags = {0: {}, TWO_KERNELS: {}, ONE_WAVE_PER_SIMD: {}}
    for (flags, n, S), p in zip(cases, out):
        by_flags[flags][n, S] = p
    return caps, by_flags


def test_flags_and_constants_are_the_headers():
    text = open(os.path.join(REPO, "include", "naf_hip.h")).read()
    assert f"#define NAF_CFG_MLP_TWO_KERNELS {TWO_KERNELS}u" in text and f"#define NAF_CFG_BACKWARD_ONE_WAVE_PER_SIMD {ONE_WAVE_PER_SIMD}u" in text


def test_the_oracles_restatement_is_the_plan(plans):
    """parts, train waves and slabs of every case equal _mlp16_oracle's; so do the constants the oracle restates."""
    caps, by_flags = plans
    assert (caps.backward16 * 4, caps.train_max_rays, caps.max_samples_lds) == (O.MAX_ITEM_WAVES, O.MAX_ITEM_WAVES, O.MAX_SAMPLES_LDS)
    for (n, S), p in by_flags[0].items():
        assert (p.parts, p.train_waves, p.slabs16) == (O.backward16_parts(n, S), O.mlp_train_waves(n, S), O.n_slabs(n, S)), (n, S, p)


def test_the_32_point_restatement_is_the_plan(plans):
    """slabs and forward grid of the 32-point kernels equal _mlp32_oracle's at every batch size of the grid and under either flag (the
    32-point plan looks at neither), and so do the caps it restates."""
    import _mlp32_oracle as M
    caps, by_flags = plans
    assert (caps.backward, caps.forward, caps.max_samples_lds) == (M.MAX_SLABS, M.MAX_FORWARD_GRID, O.MAX_SAMPLES_LDS)
    for table in by_flags.values():
        for (n, S), p in table.items():
            assert (p.slabs32, p.forward_grid32) == (M.backward_slabs(n), M.forward_grid(n)), (n, S, p)


def test_forward_splits_exactly_below_2048_rays_with_4_to_32_tiles(plans):
    _, by_flags = plans
    for (n, S), p in by_flags[0].items():
        assert bool(p.splits) == (n < 2048 and S <= 512 and -(-S // 16) >= 4), (n, S)


def test_diagnostic_flags_keep_the_kernel_pair(plans):
    """Either flag: no one-launch kernel.  ONE_WAVE_PER_SIMD: no split forward either, and parts aim at 1 024 waves.  TWO_KERNELS:
    the pair as the unflagged plan would run it (see the module docstring), same parts and slabs."""
    _, by_flags = plans
    for key, p in by_flags[ONE_WAVE_PER_SIMD].items():
        n, S = key
        assert p.train_waves == 0 and p.train_grid == 0 and not p.splits, key
        assert p.parts == max(1, min(-(-S // 16), 12, 1024 // max(n, 1))), key
    for key, p in by_flags[TWO_KERNELS].items():
        assert p.train_waves == 0 and p.train_grid == 0, key
        assert p._replace(train_waves=0, train_grid=0) == by_flags[0][key]._replace(train_waves=0, train_grid=0), key


def test_every_grid_is_between_one_and_its_cap(plans):
    caps, by_flags = plans
    for flags, table in by_flags.items():
        for key, p in table.items():
            assert 1 <= p.split_grid <= caps.forward_split and 1 <= p.forward_grid16 <= caps.forward and 1 <= p.forward_grid32 <= caps.forward, key
            assert 1 <= p.slabs16 <= caps.backward16 and 1 <= p.slabs32 <= caps.backward, key
            assert 1 <= p.parts <= 12, key
            if p.train_waves:
                assert 1 <= p.train_grid <= caps.backward16, key


def test_one_launch_invariants(plans):
    """What mlp16_train_kernel's comments rely on: whole rays per workgroup (w % parts == 0), one work item per wave
    (n_rays * parts <= 3 072 and the grid's waves cover the items), whole slabs per workgroup, and the grid's slabs cover the count."""
    _, by_flags = plans
    seen = set()
    for (n, S), p in by_flags[0].items():
        w = p.train_waves
        if w == 0:
            continue
        seen.add(w)
        assert w in (4, 12) and w % p.parts == 0 and n * p.parts <= 3072, (n, S, p)
        assert p.train_grid * w >= n * p.parts and p.train_grid * (w // 4) >= p.slabs16, (n, S, p)
        assert 1 <= S <= 512 and 1 <= n <= 3072, (n, S)
    assert seen == {4, 12}
