"""The output heads of the float64 rehearsal (head / head_grad of tests/_mlp16_oracle.py, the head cases of tests/_mlp32_oracle.py)
checked without a GPU:

(a) for each of the four heads the rehearsal with the identity for a rounding function IS the network: autograd through
    oracle.network_ref in float64 on the same features, line integrals, loss and all eight gradient blocks to 1e-12;
(b) the f32 tolerances of relu, tanh and none are measured per head by the rule of _mlp32_oracle (8 x the worst float32-against-
    float64 figure over MEASURE_CASES x summation_orders(), one digit, at most 1e-5; the sigmoid figures stay); the bf16 layouts keep
    _mlp16_oracle's tolerances, and the float32 rehearsal of every head case stays inside a quarter of them (table: inside);
(c) the leaky head's decision z4 > 0: delta is measured per precision, and every relu case has no undecided weighted point in f32
    and at most two in bf16 (printed per case with the smallest |z4| / delta);
(d) every head fault -- the backward with another head's derivative, the leaky slope 1 or 0, one 16-point item whose forward took
    head 0 -- lands outside the tolerance of EACH figure it can touch, in f32, bf16 16 x 2 and bf16 8 x 4.
"""
import functools

import numpy as np
import pytest
import torch

import _mlp16_oracle as O
import _mlp32_oracle as M

LAYOUTS = ("f32", "bf16-16x2", "bf16-8x4")
GRAD_FIGURES = O.BLOCKS + ("table",)


@functools.lru_cache(maxsize=None)
def _net(layout, act):
    return M.oracle_net(layout, M.HEAD_SEEDS[act], act=act)


@functools.lru_cache(maxsize=None)
def _clean(layout, n, S, pattern, act):
    return M.head_reference(layout, _net(layout, act), n, S, pattern, act)


@functools.lru_cache(maxsize=None)
def _float32(layout, n, S, pattern, act):
    return M.head_rehearse_in_float32(layout, _net(layout, act), n, S, pattern, act)


def test_head_cases_are_cases_of_the_reference_modules_and_the_seeds_give_one_network():
    assert set(M.HEAD_CASES) == set(LAYOUTS) and set(M.HEAD_ACTS) | {"sigmoid"} == set(O.HEADS) == set(M.HEAD_SEEDS)
    assert {c[:2] for c in M.HEAD_CASES["bf16-16x2"]} <= set(O.CASES) and M.HEAD_ZERO_CASE in O.CASES
    for layout in ("f32", "bf16-8x4"):
        assert {c[:2] for c in M.HEAD_CASES[layout]} <= set(M.LAYOUT_CASES[layout])
    assert (O.mlp_train_waves(1024, 192), O.mlp_train_waves(700, 100), O.mlp_train_waves(3100, 40), O.mlp_train_waves(24, 7)) == (12, 4, 0, 4)
    a, b = O.oracle_net(5, act="tanh"), O.oracle_net(5)                  # the head changes no weight
    assert all(torch.equal(x, y) for x, y in zip(a.state_dict().values(), b.state_dict().values())) and a.last_activation == "tanh"


# ---- (a) the restatement against autograd -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("act", O.HEADS)
def test_rehearsal_without_rounding_is_autograd_through_the_oracle_network(act):
    """(37, 50) dense, float64, rnd = identity: acc, loss and the eight gradient blocks against torch autograd through
    oracle.network_ref.mlp_forward with the same head, 1e-12 relative L2.  head_grad goes through the OUTPUT (y (1 - y), 1 - y y);
    autograd does not: the two agree in float64, which is what makes the float64 rehearsal the reference."""
    from oracle.network_ref import mlp_forward
    n, S = 37, 50
    ref = M.oracle_net("f32", M.HEAD_SEEDS[act], act=act).double()
    rays, t_rand, target, weight, ids = M.head_inputs("f32", n, S, "dense")
    assert ids == list(range(n)) and ref.last_activation == act
    _, pts, dist = O.geometry(rays, t_rand, S)
    with torch.no_grad():
        feat = ref.encoder(pts, O.BOUND)
    assert feat.dtype == torch.float64
    sig = mlp_forward(feat, [l.weight for l in ref.layers], [l.bias for l in ref.layers], (2,), act).reshape(n, S)
    acc = (sig * dist).sum(-1)
    loss = (weight.double() * (acc - target.double()) ** 2).sum()
    loss.backward()
    got = O.rehearse(feat.reshape(n, S, 32), dist, target, weight, ref.layers, rnd=O.identity, dtype=torch.float64, act=act)
    figures = {"acc": O.rel_l2(got["acc"].numpy(), acc.detach().numpy()),
               "loss": abs(float(got["loss"]) - float(loss.detach())) / abs(float(loss.detach()))}
    for name, a, b in zip(O.BLOCKS, got["blocks"], [p.grad for l in ref.layers for p in (l.weight, l.bias)]):
        assert a.shape == b.shape
        figures[name] = O.rel_l2(a.numpy(), b.numpy())
    print(f"{act}: " + " ".join(f"{k}={v:.2g}" for k, v in figures.items()))
    assert max(figures.values()) < 1e-12, figures


def test_head_and_head_grad_are_the_kernels_formulas():
    z = torch.tensor([-2.0, -1e-3, 0.0, 1e-3, 3.0], dtype=torch.float64)
    assert torch.equal(O.head(z, "relu"), torch.where(z > 0, z, 0.01 * z)) and torch.equal(O.head(z, "none"), z)
    assert torch.equal(O.head_grad(z, O.head(z, "relu"), "relu"), torch.tensor([0.01, 0.01, 0.01, 1.0, 1.0], dtype=torch.float64))   # z = 0: 0.01
    assert torch.equal(O.head_grad(z, z, "none"), torch.ones_like(z))
    y = O.head(z, "tanh")
    assert torch.equal(O.head_grad(z, y, "tanh"), 1 - y * y)
    flip = torch.tensor([False, True, False, False, False])
    assert torch.equal(O.head_grad(z, z, "relu", flip=flip), torch.tensor([0.01, 1.0, 0.01, 1.0, 1.0], dtype=torch.float64))
    # the limits of test_hip_mlp_heads_reference.py's saturation cases, in the kernels' own precision: y (1 - y) and 1 - y y are 0
    big = torch.tensor([100.0, -100.0])
    assert torch.equal(O.head(big, "tanh"), torch.tensor([1.0, -1.0])) and not O.head_grad(big, O.head(big, "tanh"), "tanh").any()
    s = O.head(big, "sigmoid")
    assert float(s[0]) == 1.0 and 0.0 <= float(s[1]) < 2.0 ** -126 and float(O.head_grad(big, s, "sigmoid")[0]) == 0.0


# ---- (b) tolerances --------------------------------------------------------------------------------------------------------------------
def test_f32_head_tolerances_are_eight_times_the_recorded_figures_and_below_the_ceiling():
    assert M.HEAD_F32_MEASURED["sigmoid"] is M.F32_MEASURED and M.HEAD_F32_TOL["sigmoid"] == M.F32_TOL      # not re-derived
    for act in M.HEAD_ACTS:
        for k, worst in M.HEAD_F32_MEASURED[act].items():
            tol = M.HEAD_F32_TOL[act][k]
            assert 8 * worst <= tol <= M.F32_TOL_CEILING, (act, k)
            digit = tol / 10.0 ** np.floor(np.log10(tol))
            assert abs(digit - round(digit)) < 1e-9 and (round(digit) - 1) * tol / round(digit) < 8 * worst, (act, k)
    for k, worst in M.HEAD_Z4_MEASURED.items():
        assert 8 * worst <= M.HEAD_DELTA[k] < 1.25 * 8 * worst + 1e-12 or M.HEAD_DELTA[k] == M.derived_tolerance(worst), k
    assert M.head_tolerances("bf16-8x4", "tanh") == M.head_tolerances("bf16-16x2", "relu") == \
        {"acc": O.TOL_ACC, "loss": O.TOL_LOSS, "grad": O.TOL_GRAD, "table": O.TOL_TABLE}


@pytest.mark.parametrize("n,S,pattern", M.MEASURE_CASES)
@pytest.mark.parametrize("act", M.HEAD_ACTS)
def test_f32_tolerances_are_measured_per_head(act, n, S, pattern):
    """The float32 rehearsal (the kernel's own formulas: 1 - y y formed from the fp32 output) in the four summation orders against
    float64: 8 x every figure stays inside the head's tolerance of its class.  relu: the case has no undecided point, so no order
    takes a decision the other way (asserted in (c))."""
    want = M.numpy_dict(_clean("f32", n, S, pattern, act))
    worst = {}
    for name, got in _float32("f32", n, S, pattern, act).items():
        f = M.figure_classes(M.figures(M.numpy_dict(got), want))
        print(f"f32 {act} ({n}, {S}) {pattern} {name}: " + " ".join(f"{k}={v:.4g}" for k, v in f.items()))
        for k, v in f.items():
            worst[k] = max(worst.get(k, 0.0), v)
    for k, v in worst.items():
        assert 8 * v <= M.HEAD_F32_TOL[act][k], (k, v)


_BF16_CASES = [(layout,) + c for layout in LAYOUTS[1:] for c in M.HEAD_CASES[layout]]


@pytest.mark.parametrize("layout,n,S,pattern", _BF16_CASES, ids=[f"{c[0]}-{c[1]}x{c[2]}-{c[3]}" for c in _BF16_CASES])
@pytest.mark.parametrize("act", M.HEAD_ACTS)
def test_bf16_layouts_keep_their_tolerances_for_every_head(act, layout, n, S, pattern):
    """The float32 rehearsal of every bf16 head case in the four summation orders: every figure inside a quarter of the tolerance
    _mlp16_oracle grants, the table gradient inside the tolerance itself (the stored bf16 flips of tests/test_mlp16_oracle_cpu.py:
    0.69 at the 112 points of (24, 7), whichever head).  relu: against the best of the references of the undecided points."""
    wants = M.head_references(layout, _net(layout, act), n, S, pattern, act)
    for name, got in _float32(layout, n, S, pattern, act).items():
        r = M.best_ratios(layout, act, M.numpy_dict(got), wants)
        print(f"{layout} {act} ({n}, {S}) {pattern} {name}: " + " ".join(f"{k}={v:.3f}" for k, v in r.items()))
        assert max(v for k, v in r.items() if k != "table") < 0.25 and r["table"] < 1.0, (name, r)


def test_no_tanh_case_has_a_saturated_point():
    """Recorded beside HEAD_SEEDS: with the seed and table scale of the sigmoid cases |y| stays far below 0.99 in every tanh case, so
    the tolerance of 1 - y y is measured where it does not cancel; saturation itself is the GPU module's +-100 cases."""
    for layout in LAYOUTS:
        for n, S, pattern in M.HEAD_CASES[layout] + (M.MEASURE_CASES if layout == "f32" else ()):
            z = _clean(layout, n, S, pattern, "tanh")["z4"]
            assert float((torch.tanh(z).abs() > 0.99).double().mean()) == 0.0 and float(z.abs().max()) < 0.5, (layout, n, S)


# ---- (c) the leaky head's decision -----------------------------------------------------------------------------------------------------------
_RELU_CASES = [(layout,) + c for layout in LAYOUTS for c in M.HEAD_CASES[layout] + (M.MEASURE_CASES if layout == "f32" else ())]
_RELU_CASES = sorted(set(_RELU_CASES), key=_RELU_CASES.index)


@pytest.mark.parametrize("layout,n,S,pattern", _RELU_CASES, ids=[f"{c[0]}-{c[1]}x{c[2]}-{c[3]}" for c in _RELU_CASES])
def test_relu_cases_meet_the_undecided_point_condition(layout, n, S, pattern):
    """delta (HEAD_DELTA) covers 8 x the worst |z4(float32) - z4(float64)| of the case over the summation orders; the weighted points
    with |z4| < delta are none in f32 and at most two in a bf16 layout.  Both branches of the head are taken among the weighted points
    of every case of more than 1 000 of them."""
    prec = M.head_precision(layout)
    want = _clean(layout, n, S, pattern, "relu")
    dz = max(float((got["z4"].double() - want["z4"]).abs().max()) for got in _float32(layout, n, S, pattern, "relu").values())
    und, nearest = M.undecided_points(layout, n, S, pattern, want)
    _, _, _, weight, ids = M.head_inputs(layout, n, S, pattern)
    z = want["z4"][weight[torch.as_tensor(ids)] > 0]
    up, down = int((z > 0).sum()), int((z <= 0).sum())
    print(f"{layout} relu ({n}, {S}) {pattern}: {len(und)} undecided of {z.numel()} weighted points ({up} with z4 > 0, {down} with z4 <= 0), "
          f"smallest |z4| / delta {nearest:.3g}, worst |z4 (float32) - z4 (float64)| {dz:.3g} = {8 * dz / M.HEAD_DELTA[prec]:.3f} of delta / 8")
    assert 8 * dz <= M.HEAD_DELTA[prec]
    assert len(und) <= M.HEAD_MAX_UNDECIDED[prec]
    assert len(M.head_references(layout, _net(layout, "relu"), n, S, pattern, "relu")) == 1 << len(und)
    assert down > 0 and (up > 0 or z.numel() < 1000)


def test_the_better_of_the_branch_combinations_is_taken():
    """A 'kernel' that decides one point the other way is outside against the reference's own branch and matches the combination
    that flips it."""
    layout, n, S, pattern = "bf16-8x4", 37, 50, "dense"
    ref, base = _net(layout, "relu"), _clean(layout, n, S, pattern, "relu")
    flip = torch.zeros(base["z4"].numel(), dtype=torch.bool)
    flip[int(base["z4"].reshape(-1).abs().argmin())] = True
    other = M.head_reference(layout, ref, n, S, pattern, "relu", flip=flip)
    assert max(M.head_ratios(layout, "relu", M.numpy_dict(other), M.numpy_dict(base)).values()) > 1.0
    assert max(M.best_ratios(layout, "relu", M.numpy_dict(other), [base, other]).values()) == 0.0


# ---- (d) head faults ----------------------------------------------------------------------------------------------------------------------------
def _probe_item(layout):
    """(n, S, pattern, range) of one 16-point piece of a probe ray: a work item of the 16-point plan (the last ray's last tile range,
    cut to 16 points), the first half tile of a wave's SECOND ray in the 32-point plan."""
    if layout == "bf16-16x2":
        n, S = 1024, 192
        r, a, e = O.item_points(n, S, n * O.backward16_parts(n, S) - 1)
        return n, S, "probe", (r, e - 16, e)
    return 2100, 40, "probe", (2048, 0, 16)


def _fault_list():
    """(name, head, case of the layout or None for the probe item's, builder(layout, ids) -> fault, figures that have to land outside)."""
    out = []
    for act, other in (("tanh", "sigmoid"), ("relu", "none"), ("none", "tanh"), ("none", "relu"), ("tanh", "none")):
        out.append((f"{other}-derivative-under-{act}", act, lambda layout, ids, other=other: O.fault_head_backward(other), GRAD_FIGURES))
    for slope in (1, 0):
        out.append((f"leaky-slope-{slope}", "relu", lambda layout, ids, slope=slope: O.fault_head_slope(slope), GRAD_FIGURES))
    for act in M.HEAD_ACTS:
        out.append((f"item-with-head-0-under-{act}", act, lambda layout, ids: O.fault_head_forward_items(ids, [_probe_item(layout)[3]]), ("acc", "loss")))
    return out


def _fault_cases(layout, figures):
    if figures == ("acc", "loss"):
        return [_probe_item(layout)[:3]]
    return [M.HEAD_CASES[layout][0], M.HEAD_CASES[layout][-1]] if layout == "bf16-16x2" else [M.HEAD_CASES[layout][0], M.HEAD_CASES[layout][2]]


_FAULTS = [(layout, name, act) + case + (build, figs) for layout in LAYOUTS for name, act, build, figs in _fault_list() for case in _fault_cases(layout, figs)]


@pytest.mark.parametrize("layout,name,act,n,S,pattern,build,figs", _FAULTS, ids=[f"{f[0]}-{f[1]}-{f[3]}x{f[4]}-{f[5]}" for f in _FAULTS])
def test_every_head_fault_lands_outside_every_tolerance_it_can_touch(layout, name, act, n, S, pattern, build, figs):
    """A backward that got another head (sigmoid's derivative under tanh, the identity's under relu, ...), a leaky derivative of slope
    1 or 0 for z4 <= 0, one 16-point item of a probe ray whose forward took head 0: EVERY one of the eight gradient blocks and the
    table gradient (derivative faults), the line integrals AND the loss (the forward fault) land outside the head's tolerance."""
    ref = _net(layout, act)
    fault = build(layout, M.head_inputs(layout, n, S, pattern)[4])
    r = M.head_ratios(layout, act, M.numpy_dict(M.head_reference(layout, ref, n, S, pattern, act, fault=fault)),
                      M.numpy_dict(_clean(layout, n, S, pattern, act)))
    least = min(figs, key=r.get)
    print(f"{layout} {name} ({n}, {S}) {pattern}: least moved {least} = {r[least]:.3g} x tolerance")
    assert r[least] > 1.0, r
    if figs == ("acc", "loss"):                                            # the item is on a weighted ray and is 16 points
        rg = _probe_item(layout)[3]
        assert rg[2] - rg[1] == 16 and float(M.head_inputs(layout, n, S, pattern)[3][rg[0]]) > 0


@pytest.mark.parametrize("act", M.HEAD_ACTS)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_zero_weights_give_exact_zeros_for_every_head(layout, act):
    n, S = M.HEAD_ZERO_CASE
    out = M.head_reference(layout, _net(layout, act), n, S, "zero", act)
    assert float(out["loss"]) == 0.0 and not out["packed"].any() and not np.any(out["emb_g"]) and not torch.count_nonzero(out["dx"])
    assert float(out["acc"].abs().min()) > 0
