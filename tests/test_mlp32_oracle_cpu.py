"""The float64 rehearsal of a training step through the 32-point MLP kernels (tests/_mlp32_oracle.py) checked without a GPU:

(a) every case reaches the launch layout its row of the case table claims (the plan functions themselves are held to
    csrc/mlp_step_plan.h by tests/test_step_plan_cpu.py);
(b) the tolerances are measured, not chosen: the rehearsal in float32 in four summation orders against itself in float64.  f32
    layout: 8 x every figure stays inside the tolerance of its class, each tolerance is 8 x the recorded worst figure rounded up to
    one digit and at most 1e-5.  bf16 layouts: every figure within a quarter of the _mlp16_oracle tolerances they keep;
(c) every fault of the list, injected into the rehearsal of a case and pattern tests/test_hip_mlp32_reference.py runs, lands outside
    at least one tolerance in every layout it applies to; the zero pattern gives exact zeros.
"""
import functools

import numpy as np
import pytest
import torch

import _mlp16_oracle as O
import _mlp32_oracle as M

SEED = 37


@functools.lru_cache(maxsize=None)
def _net(layout):
    return M.oracle_net(layout, SEED)


@functools.lru_cache(maxsize=None)
def _clean(layout, n, S, pattern):
    return M.numpy_dict(M.reference(layout, _net(layout), n, S, pattern))


def test_every_case_reaches_what_the_case_table_says():
    """n -> (slabs, fewest and most rays per backward wave, fewest and most per forward wave); S -> (tiles, points of the last)."""
    rays = {1024: (256, (1, 1), (1, 1)), 300: (75, (1, 1), (1, 1)), 37: (10, (0, 1), (0, 1)), 1: (1, (0, 1), (0, 1)), 3: (1, (0, 1), (0, 1)),
            24: (6, (1, 1), (1, 1)), 6: (2, (0, 1), (0, 1)), 2100: (512, (1, 2), (1, 1)), 4500: (512, (2, 3), (1, 1)), 8300: (512, (4, 5), (1, 2))}
    samples = {192: (6, 32), 64: (2, 32), 50: (2, 18), 33: (2, 1), 70: (3, 6), 7: (1, 7), 1030: (33, 6), 40: (2, 8), 20: (1, 20)}
    assert {n for n, _ in M.CASES} == set(rays) and {S for _, S in M.CASES} == set(samples)
    for n, S in M.CASES:
        slabs = M.backward_slabs(n)
        assert (slabs, M.rays_per_wave(n, 4 * slabs), M.rays_per_wave(n, 4 * M.forward_grid(n))) == rays[n], n
        assert (M.n_tiles(S), S - 32 * (M.n_tiles(S) - 1)) == samples[S], S
        probes = M.probe_rays(n, S)
        assert len(probes) == min(16, n) and {r for r in (0, 1, 2, n - 3, n - 2, n - 1) if 0 <= r < n} <= set(probes)
        assert sorted(r for s in range(slabs) for r in M.slab_rays(n, s)) == list(range(n))              # every ray in exactly one slab
    assert 1030 > O.MAX_SAMPLES_LDS
    assert sum(len(M.wave_rays(2100, w, 2048)) == 2 for w in range(2048)) == 52                          # 52 waves take a second ray
    assert sum(len(M.wave_rays(4500, w, 2048)) == 3 for w in range(2048)) == 404
    assert sum(len(M.wave_rays(8300, w, 8192)) == 2 for w in range(8192)) == 108                         # the forward's waves wrap
    assert M.slab_rays(37, 9) == [36] and M.slab_rays(1, 0) == [0] and M.slab_rays(3, 0) == [0, 1, 2] and M.slab_rays(6, 1) == [4, 5]
    assert M.slab_rays(2100, 0) == [0, 2048, 1, 2049, 2, 2050, 3, 2051] and M.slab_rays(2100, 13) == [52, 53, 54, 55]
    assert {2047, 2048} <= set(M.probe_rays(2100, 40)) and {2047, 2048, 4095, 4096} <= set(M.probe_rays(4500, 20))
    assert {2047, 2048, 4095, 4096, 6143, 6144, 8191, 8192, 2043, 2044} <= set(M.probe_rays(8300, 20))    # both wraps, last slab
    assert set(M.LAYOUT_CASES["bf16-4x8"]) <= set(M.CASES) and M.LAYOUT_CASES["f32"] == M.LAYOUT_CASES["bf16-8x4"] == M.CASES


def test_f32_tolerances_are_eight_times_the_recorded_figures_and_below_the_ceiling():
    assert M.F32_TOL == pytest.approx({"acc": 2e-6, "loss": 6e-7, "grad": 4e-6, "table": 2e-6}, rel=1e-12)
    for k, worst in M.F32_MEASURED.items():
        tol = M.F32_TOL[k]
        assert 8 * worst <= tol <= M.F32_TOL_CEILING, k
        digit = tol / 10.0 ** np.floor(np.log10(tol))
        assert abs(digit - round(digit)) < 1e-9 and (round(digit) - 1) * tol / round(digit) < 8 * worst, k      # one digit, rounded UP


@pytest.mark.parametrize("n,S,pattern", M.MEASURE_CASES)
@pytest.mark.parametrize("layout", list(M.LAYOUTS))
def test_float32_rehearsal_in_four_summation_orders(layout, n, S, pattern):
    """(b) natural; a random permutation of the points in 7 chunks; reversed samples in 3 chunks; 32-point partial sums in the
    backward's wave order.  f32: 8 x every figure is inside its class's tolerance (the table gradient scattered with fp32 adds in the
    same order, as the atomic scatter adds).  bf16: every figure below a quarter of its tolerance.  The bf16 feature gradients are
    STORED as bf16, so a value on a rounding boundary is stored one bf16 step away after a reordering (at most 2 in 1 000 values
    here); unlike at the 112 points of _mlp16_oracle's smallest case those flips stay inside the quarter at these sizes, so the table
    figure is asserted with them left in."""
    want = _clean(layout, n, S, pattern)
    worst = {}
    for name, got in M.rehearse_in_float32(layout, _net(layout), n, S, pattern).items():
        f = M.figure_classes(M.figures(M.numpy_dict(got), want))
        print(f"{layout} ({n}, {S}) {pattern} {name}: " + " ".join(f"{k}={v:.3g}" for k, v in f.items()))
        for k, v in f.items():
            worst[k] = max(worst.get(k, 0.0), v)
        if layout != "f32":
            flips = int((got["dx"].double().numpy() != want["dx"]).sum())
            assert flips <= max(1, want["dx"].size // 500), (name, flips)
    if layout == "f32":
        for k, v in worst.items():
            assert 8 * v <= M.F32_TOL[k], (k, v)
    else:
        tol = {"acc": O.TOL_ACC, "loss": O.TOL_LOSS, "grad": O.TOL_GRAD, "table": O.TOL_TABLE}
        for k, v in worst.items():
            assert v < 0.25 * tol[k], (k, v)


# ---- (c) fault injection -----------------------------------------------------------------------------------------------------------------
def _fault_list():
    """(name, n, S, pattern, builder(ids) -> fault dict or None)."""
    out = []
    add = lambda name, n, S, p, build: out.append((name, n, S, p, build))                                  # noqa: E731
    # a ray dropped: a wave's second and third ray, a ray of a dense case; a ray run twice
    add("ray-dropped-second", 2100, 40, "probe", lambda ids: M.fault_ray_dropped(40, ids, 2048))
    add("ray-dropped-third", 4500, 20, "probe", lambda ids: M.fault_ray_dropped(20, ids, 4096))
    add("ray-dropped-dense", 37, 50, "dense", lambda ids: M.fault_ray_dropped(50, ids, 17))
    add("ray-dropped-idle-waves", 3, 70, "dense", lambda ids: M.fault_ray_dropped(70, ids, 2))
    add("ray-twice-boundary", 2100, 40, "probe", lambda ids: M.fault_ray_twice(40, ids, 2047))
    add("ray-twice-dense", 37, 50, "dense", lambda ids: M.fault_ray_twice(50, ids, 36))
    add("ray-twice-last", 1024, 192, "probe", lambda ids: M.fault_ray_twice(192, ids, 1023))
    # a slab skipped by the reducer: the last one, the ragged last one, the first of 512 (eight rays)
    add("slab-skipped-last", 1024, 192, "probe", lambda ids: M.fault_slab_skipped(1024, 192, ids, 255))
    add("slab-skipped-ragged", 37, 50, "dense", lambda ids: M.fault_slab_skipped(37, 50, ids, 9))
    add("slab-skipped-first", 2100, 40, "probe", lambda ids: M.fault_slab_skipped(2100, 40, ids, 0))
    add("slab-skipped-last-of-512", 8300, 20, "probe", lambda ids: M.fault_slab_skipped(8300, 20, ids, 511))
    add("slab-skipped-second", 6, 1030, "dense", lambda ids: M.fault_slab_skipped(6, 1030, ids, 1))
    # weight[r] read at r +- 1
    for shift in (-1, 1):
        for n, S, p in ((1024, 192, "probe"), (37, 50, "dense"), (2100, 40, "probe"), (8300, 20, "probe"), (3, 70, "dense")):
            add(f"weight-shift{shift:+d}", n, S, p, lambda ids, n=n, S=S, p=p, shift=shift: M.fault_weight_shifted(n, S, p, ids, shift))
    # loss_part once per tile
    for n, S, p in ((1024, 192, "probe"), (37, 50, "dense"), (2100, 40, "probe"), (6, 1030, "dense"), (1, 33, "dense")):
        add("loss-per-tile", n, S, p, lambda ids, S=S: M.fault_loss_per_tile(S, ids))
    # the padding lanes of a ragged tile contributing
    for n, S, p in ((37, 50, "dense"), (2100, 40, "probe"), (24, 7, "dense"), (6, 1030, "dense"), (1, 33, "dense"), (3, 70, "dense"),
                    (4500, 20, "probe")):
        add("padding", n, S, p, lambda ids, n=n, S=S: M.fault_padding_contributes(n, S, ids))
    # the first tile of a wave's next ray prefetched from ray r + 1
    for n, S in ((2100, 40), (4500, 20), (8300, 20)):
        add("next-ray-prefetch", n, S, "probe", lambda ids, n=n, S=S: M.fault_next_ray_prefetch(n, S, ids))
    # one lane half's points missing from the hidden layers' bias sums; db3 missing for one tile
    add("bias-half", 1024, 192, "probe", lambda ids: M.fault_bias_half_lost(192, ids))
    add("bias-half-one-ray", 37, 50, "dense", lambda ids: M.fault_bias_half_lost(50, ids, rays=[20]))
    add("bias-half-second-ray", 2100, 40, "probe", lambda ids: M.fault_bias_half_lost(40, ids, rays=[2048]))
    add("bias3-tile", 1024, 192, "probe", lambda ids: M.fault_bias3_tile_lost(192, ids, 1023, 5))
    add("bias3-ragged-tile", 37, 50, "dense", lambda ids: M.fault_bias3_tile_lost(50, ids, 0, 1))
    add("bias3-tile-second-ray", 2100, 40, "probe", lambda ids: M.fault_bias3_tile_lost(40, ids, 2048, 0))
    # two chunks of the transposed read exchanged, in the gradient operand and in the input operands
    for operand in ("G", "X"):
        for n, S, p in ((1024, 192, "probe"), (37, 50, "dense"), (2100, 40, "probe")):
            add(f"chunks-swapped-{operand}", n, S, p, lambda ids, operand=operand: M.fault_chunks_swapped(operand))
    return out


_FAULTS = [(layout,) + f for layout in M.LAYOUTS for f in _fault_list() if (f[1], f[2]) in M.LAYOUT_CASES[layout]]


def test_every_fault_kind_is_injected_in_every_layout():
    kinds = {f[0].split("-")[0] for f in _fault_list()}
    assert kinds == {"ray", "slab", "weight", "loss", "padding", "next", "bias", "bias3", "chunks"}
    for layout in M.LAYOUTS:
        assert {f[1].split("-")[0] for f in _FAULTS if f[0] == layout} == kinds, layout
        assert {"ray-dropped", "ray-twice"} <= {"-".join(f[1].split("-")[:2]) for f in _FAULTS if f[0] == layout}


@pytest.mark.parametrize("layout,name,n,S,pattern,build", _FAULTS, ids=[f"{f[0]}-{f[1]}-{f[2]}x{f[3]}-{f[4]}" for f in _FAULTS])
def test_every_injected_fault_lands_outside_the_tolerances(layout, name, n, S, pattern, build):
    """(c) a ray dropped or run twice, a slab skipped, weight[r +- 1], the loss once per tile, unmasked padding lanes with an interior
    sample's distance, the next ray's first tile from ray r + 1, a lane half missing from the bias sums, db3 missing for a tile, two
    chunks of the transposed read exchanged: each moves at least one asserted figure past its tolerance.  (The swap is a fault of
    PrecBF16::tr_load alone; it is injected in the f32 layout as well, where the same permutation of PrecF32's image would show.)

    The one variant that does not, by construction of the renderer: padding lanes that contribute with the distance of the ray's
    LAST sample -- see test_padding_with_the_last_samples_distance_is_below_every_tolerance."""
    fault = build(M.reference_rays(n, S, pattern))
    assert fault is not None, "the case gives this fault nothing to act on"
    r = M.ratios(layout, M.numpy_dict(M.reference(layout, _net(layout), n, S, pattern, fault=fault)), _clean(layout, n, S, pattern))
    worst = max(r, key=r.get)
    print(f"{layout} {name} ({n}, {S}) {pattern}: worst {worst} = {r[worst]:.3g} x tolerance")
    assert r[worst] > 1.0, r


@pytest.mark.parametrize("layout", list(M.LAYOUTS))
def test_padding_with_the_last_samples_distance_is_below_every_tolerance(layout):
    """buffered_dist / sample_dist return 1e-10 |d| for every s >= S - 1, so a padding lane that were NOT masked would contribute what
    the last sample itself contributes: 1e-10 of an interior sample's share.  No tolerance can see it and no result depends on it."""
    n, S = 37, 50
    fault = M.fault_padding_contributes(n, S, M.reference_rays(n, S, "dense"), tail_dist=True)
    r = M.ratios(layout, M.numpy_dict(M.reference(layout, _net(layout), n, S, "dense", fault=fault)), _clean(layout, n, S, "dense"))
    assert max(r.values()) < 1e-2, r


@pytest.mark.parametrize("layout", list(M.LAYOUTS))
def test_zero_weights_give_exact_zeros_in_the_rehearsal(layout):
    out = M.reference(layout, _net(layout), 24, 7, "zero")
    assert float(out["loss"]) == 0.0 and not out["packed"].any() and not np.any(out["emb_g"]) and float(out["acc"].abs().min()) > 0
    assert len(out["rays"]) == 24 and not torch.count_nonzero(out["dx"])
