"""Where the tolerances of tests/_raymarch_oracle.py come from, and that they tell a wrong kernel from a right one -- no GPU.

Each kernel's arithmetic is restated in float32 (`*_f32` of the oracle module) in three summation orders -- sequential, the kernel's
own shuffle tree with its per-chunk carry, reversed -- and compared with the float64 oracle on the cases the GPU module runs.  A
tolerance is 8 x the worst of those figures, rounded up to one digit, and at most its cap (depths 3e-6 m, weights 1e-6 of the
largest, integrals and tau 2e-6 of sum|sigma dist| of the prefix).  Then each fault of the list below is injected into the
float32 restatement and has to land outside the tolerance in every case it can touch.

Measured when the module was added (worst over cases and orders; printed by the tests):
  cdf 1.4e-7 in the kernel's order (1.8e-6 sequential at second_max_trip, 2.7e-6 for the sequential sum of a constant ray, kept out:
  see _resample_figures); depths 2.1e-7 m in the kernel's order, 7.3e-7 m reversed (lds_64k); weights 1.0e-7; integrals 1.1e-7 and
  tau 1.7e-7 of the prefix's sum|sigma dist|; grad_sigma 1.6e-7 relative.
Resampling cases: no ray of any case is skipped; 3 of the 101 rays of first_carry_spike (3.0 %) have an undecided sample and none
elsewhere (caps: 2 % skipped, 5 % undecided, none for the hand-built u)."""
import functools

import numpy as np
import pytest

import _raymarch_oracle as O

ORDERS = ("seq", "tree", "rev")
CPU_CASES = [c for c in O.RESAMPLE_CASES]


@functools.lru_cache(maxsize=None)
def _case(name):
    case = next(c for c in O.RESAMPLE_CASES if c[0] == name)
    rays, t_rand, sigma, u = O.resample_inputs(case)
    _, n, S, NF, _, det = case
    z = O.sample(rays, t_rand, S, True, 0.3)[0]
    return dict(case=case, z=z, sigma=sigma, u=u, NF=NF, det=det, ref=O.resample(sigma, z, u, NF, det))


def _depth_error(ref, fine):
    """Per fine sample: distance to the nearest admissible depth (the oracle's own, or a candidate's)."""
    err = np.abs(fine.astype(np.float64) - ref["fine"])
    for (r, j), vals in ref["cands"].items():
        err[r, j] = min([err[r, j]] + [abs(float(fine[r, j]) - v) for v in vals])
    return err


def _round_up_one_digit(x):
    e = np.floor(np.log10(x))
    return np.ceil(x / 10 ** e - 1e-9) * 10 ** e


def _holds(name, worst, tol, cap=None, tree=None):
    """tolerance = 8 x worst rounded up to one digit, or the cap where that is lower; the kernel's own order stays 8 x inside it."""
    want = _round_up_one_digit(8 * worst)
    print(f"raymarch oracle: {name}: worst fp32-vs-fp64 {worst:.3g}, x 8 rounded up {want:.1g}, tolerance {tol:.1g}"
          + (f", cap {cap:.1g}" if cap else "") + (f", the kernel's order {tree:.3g}" if tree is not None else ""))
    if cap is None or want <= cap:
        assert 8 * worst <= tol <= 1.0000001 * want, (name, worst, tol)
    else:
        assert tol == cap and 8 * tree <= tol, (name, worst, tree, tol)


@functools.lru_cache(maxsize=None)
def _resample_figures():
    worst = dict(cdf=0.0, depth=0.0, weight=0.0)
    where = {}
    for case in CPU_CASES:
        c = _case(case[0])
        for order in ORDERS:
            if order == "rev" and case[2] > 300 and case[1] > 100:
                continue                                                   # the O(S^2) order on 4 100 x 257: the small cases cover it
            got = O.resample_f32(c["sigma"], c["z"], c["u"], c["NF"], c["det"], order)
            cdf_err, depth_err = np.abs(got["cdf"] - c["ref"]["cdf"]).max(-1), _depth_error(c["ref"], got["fine"]).max(-1)
            if order != "tree":
                # equal addends round the same way every time: a sequential fp32 sum of a constant ray's S - 2 equal terms drifts
                # linearly (2.7e-6 of cdf at 193 intervals) where the kernel's tree stays at 6e-8.  That figure belongs to the
                # order, not to fp32, and 8 x it would let a kernel pass that sums a constant row one term at a time; it is
                # printed and kept out of the tolerance.
                flat = (c["ref"]["weights"][:, 1:] == 0).all(-1)
                if flat.any():
                    worst["constant_ray_cdf"] = max(worst.get("constant_ray_cdf", 0.0), float(cdf_err[flat].max()))
                    cdf_err, depth_err = cdf_err[~flat], depth_err[~flat]
                if cdf_err.size == 0:
                    continue
            figs = dict(cdf=cdf_err.max(), depth=depth_err.max(),
                        weight=np.abs(got["weights"] - c["ref"]["weights"]).max() / c["ref"]["weights"].max())
            for k, v in figs.items():
                if v > worst[k]:
                    worst[k], where[k] = float(v), (case[0], order)
                if order == "tree":
                    worst["tree_" + k] = max(worst.get("tree_" + k, 0.0), float(v))
    return worst, where


def test_resampling_tolerances_are_measured_and_within_their_caps():
    worst, where = _resample_figures()
    print("raymarch oracle: worst at", where, "| sequential and reversed sums of a constant ray, not counted: cdf", worst.get("constant_ray_cdf"))
    # DELTA is taken from the kernel's own order: the sequential and reversed sums of 255 .. 1 022 terms err by up to 1.8e-6, and a
    # delta of 8 x that would leave every ray of the S = 1 024 case undecided.  The smaller delta admits fewer alternatives: it is
    # the stricter choice, and the other orders still have to match through it (test_exclusion_cap_holds_from_the_oracle_alone).
    print(f"raymarch oracle: cdf, all orders: worst {worst['cdf']:.3g}")
    _holds("cdf in the kernel's order (DELTA)", worst["tree_cdf"], O.DELTA)
    _holds("resampled depths", worst["depth"], O.TOL_DEPTH, O.CAPS["depth"], worst["tree_depth"])
    _holds("weights", worst["weight"], O.TOL_WEIGHT, O.CAPS["weight"], worst["tree_weight"])


@pytest.mark.parametrize("case", CPU_CASES, ids=[c[0] for c in CPU_CASES])
def test_exclusion_cap_holds_from_the_oracle_alone(case):
    c = _case(case[0])
    skipped, undecided = O.exclusion(c["ref"])
    print(f"raymarch oracle: {case[0]}: {skipped:.3%} of the rays skipped, {undecided:.3%} with an undecided sample")
    assert skipped <= 0.02 and undecided <= 0.05
    # the kernel's arithmetic in every order matches by the combination rule (reversed: O(S^2), left out on 4 100 x 257)
    for order in ORDERS if case[1] * case[2] < 200000 else ("seq", "tree"):
        got = O.resample_f32(c["sigma"], c["z"], c["u"], c["NF"], c["det"], order)
        m = O.match_rows(c["ref"], got["row"])
        assert not m["failed"], (order, m["failed"][:3])
        assert O.contains_coarse(got["row"], c["z"])


def _hand_built(which):
    """Hand-built u on S = 4 with two intervals of equal weight (cdf = 0, 0.5, 1) and on a 67-sample walk."""
    rays = O.make_rays(6, 91)
    if which == "equal":
        S = 4
        sigma = np.tile(np.array([0.0, 0.25, 0.5, 0.25], O.f32), (6, 1)) * np.arange(1, 7, dtype=O.f32)[:, None]
        sigma[:] = np.array([0.0, 0.25, 0.5, 0.25], O.f32)          # equal steps on every ray: the call's maximum is that step
    else:
        S = 67
        sigma = O.make_sigma("walk", 6, S, 17)
    below_one = np.nextafter(O.f32(1.0), O.f32(0.0))
    u = np.tile(np.array([0.0, 0.5, below_one, 0.25, 0.75], O.f32), (6, 1))
    z = O.sample(rays, np.random.default_rng(4).random((6, S)).astype(O.f32), S, True, 0.3)[0]
    return rays, z, sigma, u


@pytest.mark.parametrize("which", ["equal", "walk"])
def test_hand_built_u_has_no_undecided_sample(which):
    rays, z, sigma, u = _hand_built(which)
    ref = O.resample(sigma, z, u, u.shape[1], False)
    assert O.exclusion(ref) == (0.0, 0.0)
    if which == "equal":
        np.testing.assert_array_equal(ref["cdf"], np.tile([0.0, 0.5, 1.0], (6, 1)))       # exactly representable entries
        np.testing.assert_allclose(ref["fine"][:, 1], ref["mid"][:, 1], rtol=0, atol=1e-15)  # u on the entry: the bin edge itself
    for order in ORDERS:
        got = O.resample_f32(sigma, z, u, u.shape[1], False, order)
        assert not O.match_rows(ref, got["row"])["failed"]


# ---- faults ---------------------------------------------------------------------------------------------------------------------------
def _row_fails(c, fault, order="tree"):
    got = O.resample_f32(c["sigma"], c["z"], c["u"], c["NF"], c["det"], order, fault)
    wrong_w = np.abs(got["weights"] - c["ref"]["weights"]).max() / c["ref"]["weights"].max()
    m = O.match_rows(c["ref"], got["row"])
    return bool(m["failed"]) or not (wrong_w <= O.TOL_WEIGHT)


def _touches(case, fault):
    _, n, S, NF, pattern, det = case
    P = 2
    while P < S + NF:
        P *= 2
    cdf_matters = not (det and NF <= 2)                       # deterministic u = 0 and u = 1: the first and last bin edge whatever the cdf
    return dict(
        carry_dropped=S - 2 > 64 and cdf_matters,
        carry_lane62=S - 2 > 64 and pattern != "spike" and cdf_matters,       # lane 63 of a spike's chunk holds a flat interval: 5e-6 of cdf
        no_eps=pattern in ("spike", "constant", "one_constant"),       # where some weight is small next to 1e-5; one interval (S = 3) has pdf 1 either way
        last_in_total=pattern != "spike" and cdf_matters,                    # a spike's last interval is flat: 2.5e-6 of the total
        max_per_ray=pattern in ("walk", "one_constant") and n > 1,
        no_floor=pattern == "constant",                        # a call whose largest difference is 0
        finite_pad=P > S + NF, sort_pair=True, truncated=P // 2 < S + NF,
    )[fault]


_ROW_FAULTS = ("carry_dropped", "carry_lane62", "no_eps", "last_in_total", "max_per_ray", "no_floor", "finite_pad", "sort_pair", "truncated")
_SMALL = [c for c in CPU_CASES if c[1] * c[2] < 20000]


@pytest.mark.parametrize("fault", _ROW_FAULTS)
def test_each_resampling_fault_lands_outside_the_tolerance(fault):
    touched = [c for c in _SMALL if _touches(c, fault)]
    assert touched
    for case in touched:
        if fault == "no_eps" and case[4] == "constant":
            # weights 0 and no term: 0 / 0, a row of NaN
            assert _row_fails(_case(case[0]), fault), case[0]
            continue
        assert _row_fails(_case(case[0]), fault), (fault, case[0])


def test_the_first_carry_case_alone_tells_the_carry_faults():
    """S = 66 (64 intervals, one full chunk) takes no carry: both carry faults pass it; S = 67 does not."""
    for fault in ("carry_dropped", "carry_lane62"):
        assert not _row_fails(_case("one_chunk"), fault)
        assert _row_fails(_case("first_carry"), fault)


def test_a_left_sided_search_shows_next_to_a_flat_interval():
    """Across an entry between ordinary intervals the depth is continuous, so either side of the search gives the same depth (u = 0,
    0.5 and 1 of the hand-built rows included).  It is not below a flat interval (denom < 1e-5 -> 1): u exactly on the flat
    interval's lower entry has to come out at that entry's bin edge; searched from the left it lands a whole bin lower ...  The
    entry is taken from the float32 restatement, so that u sits on it bit for bit."""
    rays = O.make_rays(4, 3)
    S = 12
    sigma = np.zeros((4, S), O.f32)
    sigma[:, 3] = 1.0                                                    # intervals 2 and 3 carry the weight, the rest are flat
    z = O.sample(rays, np.random.default_rng(2).random((4, S)).astype(O.f32), S, True, 0.3)[0]
    probe = O.resample_f32(sigma, z, np.zeros((4, 1), O.f32), 1, False)
    u = probe["cdf"][:, 6:7].copy()                                      # entry 6: the flat interval 5 below it, the flat 6 above
    ref = O.resample(sigma, z, u, 1, False)
    right = O.resample_f32(sigma, z, u, 1, False)
    left = O.resample_f32(sigma, z, u, 1, False, fault="left_search")
    np.testing.assert_allclose(right["fine"][:, 0], ref["mid"][:, 6], rtol=0, atol=O.TOL_DEPTH)
    assert (np.abs(left["fine"][:, 0].astype(np.float64) - ref["mid"][:, 6]) > 100 * O.TOL_DEPTH).all()
    # the oracle itself sees u within DELTA of that entry and offers both depths: such a sample is undecided by construction,
    # which is why the GPU module's hand-built u stay on entries between ordinary intervals
    assert len(ref["alts"]) == 4


@functools.lru_cache(maxsize=None)
def _integrate_figures():
    worst = dict(acc=0.0, tau=0.0, grad=0.0)
    for S in O.INTEGRATE_S:
        rays, z, sigma, grad = O.integrate_inputs(37, S)
        acc, scale = O.integrate(sigma, z, rays)
        tau, tscale = O.running_depth(sigma, z, rays)
        gs = O.integrate_adjoint(grad, z, rays)
        live = scale > 0
        for order in ORDERS:
            got = O.integrate_f32(sigma, z, rays, order)
            assert (got[~live] == 0).all()                                # the all-zero ray: an exact 0
            worst["acc"] = max(worst["acc"], float((np.abs(got - acc)[live] / scale[live]).max()))
            for W in (16, 32):
                t32 = O.running_depth_f32(sigma, z, rays, order, W)
                worst["tau"] = max(worst["tau"], float((np.abs(t32 - tau)[live] / tscale[live]).max()))
        g32 = O.integrate_adjoint_f32(grad, z, rays)
        worst["grad"] = max(worst["grad"], float((np.abs(g32 - gs) / np.abs(gs)).max()))
    return worst


def test_integral_tolerances_are_measured_and_within_their_caps():
    worst = _integrate_figures()
    _holds("line integrals", worst["acc"], O.TOL_SUM, O.CAPS["sum"])
    _holds("running depth", worst["tau"], O.TOL_TAU, O.CAPS["sum"])
    _holds("grad_sigma", worst["grad"], O.TOL_GRAD)


@pytest.mark.parametrize("fault", ["last_dist_zero", "last_dist_prev"])
@pytest.mark.parametrize("S", O.INTEGRATE_S)
def test_a_wrong_last_distance_lands_outside_the_tolerance(fault, S):
    """The last sample's 1e-10 |d| is below the integral's tolerance wherever another sample carries weight, so the forward sum tells
    `last_dist_prev` only; grad_sigma[:, -1] = grad_acc 1e-10 |d| tells both.  S = 1 has no previous distance: the fault cannot
    touch it."""
    rays, z, sigma, grad = O.integrate_inputs(37, S)
    if fault == "last_dist_prev" and S == 1:
        return
    gs = O.integrate_adjoint(grad, z, rays)
    g32 = O.integrate_adjoint_f32(grad, z, rays, fault)
    assert (np.abs(g32 - gs)[:, -1] > O.TOL_GRAD * np.abs(gs[:, -1])).all()
    if fault == "last_dist_prev":
        acc, scale = O.integrate(sigma, z, rays)
        live = (scale > 0) & (np.abs(sigma[:, -1]) > 0.05)
        got = O.integrate_f32(sigma, z, rays, "tree", fault)
        assert (np.abs(got - acc)[live] > O.TOL_SUM * scale[live]).all()


@pytest.mark.parametrize("W", [16, 32])
@pytest.mark.parametrize("fault", ["tau_carry_w2", "tau_restart"])
def test_a_wrong_tile_carry_lands_outside_the_tolerance(W, fault):
    for S in (15, 16, 17, 33, 64, 65, 100):
        rays, z, _, _ = O.integrate_inputs(41, S, seed=9)
        sigma = (0.2 + 0.8 * np.random.default_rng(S).random((41, S))).astype(O.f32)      # a sigmoid's range: every term counts
        tau, scale = O.running_depth(sigma, z, rays)
        got = O.running_depth_f32(sigma, z, rays, "tree", W, fault)
        bad = np.abs(got - tau) > O.TOL_TAU * scale
        if S <= W:
            assert not bad.any()                                           # one tile: no carry to get wrong
        else:
            assert bad[:, W:].all(-1).all() if fault == "tau_restart" else bad[:, W:].any(-1).all(), (S, W)
    # relative L2 at 1e-2, the earlier bar, passes one term lost from one prefix of one ray
    rays, z, _, _ = O.integrate_inputs(41, 100, seed=9)
    sigma = (0.2 + 0.8 * np.random.default_rng(0).random((41, 100))).astype(O.f32)
    tau, scale = O.running_depth(sigma, z, rays)
    lost = tau.copy()
    lost[7, 50] -= (tau[7, 50] - tau[7, 49])
    assert np.linalg.norm(lost - tau) / np.linalg.norm(tau) < 1e-2 and abs(lost - tau)[7, 50] > O.TOL_TAU * scale[7, 50]


def test_a_dropped_grid_stride_tail_is_seen():
    """Elements past the first trip of a capped grid keep the guard value (NaN).  The cut arrays go through the very comparisons the
    GPU module makes -- array_equal for the sampler, sum_fraction < 1 for the integrals, the flag of the range check -- and fail them;
    the whole arrays pass."""
    n, S = 8200, 257
    rays = O.make_rays(n, 1)
    z = O.sample(rays, None, S, False, 0.3)[0]
    assert np.array_equal(z.copy(), z) and not np.array_equal(O.grid_tail_dropped(z, 8192 * 256).astype(O.f32), z)
    assert O.grid_tail_dropped(z, 8192 * 256)[-1, -1] != z[-1, -1]                            # the last ray's last sample by itself
    n = 32768 + 7
    rays, z, sigma, grad = O.integrate_inputs(n, 2)
    acc, scale = O.integrate(sigma, z, rays)
    got = O.integrate_f32(sigma, z, rays)
    assert O.sum_fraction(got, acc, scale, O.TOL_SUM) < 1.0
    assert not O.sum_fraction(O.grid_tail_dropped(got, 32768), acc, scale, O.TOL_SUM) < 1.0
    gs, g32 = O.integrate_adjoint(grad, z, rays), O.integrate_adjoint_f32(grad, z, rays)
    assert float((np.abs(g32 - gs) / np.abs(gs)).max()) / O.TOL_GRAD < 1.0
    assert not float((np.abs(O.grid_tail_dropped(g32, 8192 * 256 // 32) - gs) / np.abs(gs)).max()) / O.TOL_GRAD < 1.0
    # the range check: a value out of range in the last element of the second trip only
    x = np.zeros(2097152 + 5, O.f32)
    x[-1] = 1.0
    assert O.normalize(x, 0.3)[1] is True and O.normalize_f32(x, 0.3)[0] is True and O.normalize_f32(x[:2097152], 0.3)[0] is False


# ---- encoder range check -----------------------------------------------------------------------------------------------------------
def _normalize_cases():
    f = O.f32
    size = f(0.3)
    up, down = np.nextafter(size, f(1)), np.nextafter(size, f(0))
    g = np.random.default_rng(0)
    inside = (g.random(65) * 2 - 1).astype(f) * down
    return size, {
        "all_negative": -np.abs(inside) - f(1e-6),
        "zeros": np.array([-0.0, 0.0, -0.0], f),
        "denormal": np.array([1e-45, -1e-45, 0.1], f),
        "exactly_size": np.array([-size, size, 0.0], f),
        "one_ulp_above": np.array([0.0, up], f), "one_ulp_below": np.array([-up, 0.0], f),
        "inf": np.array([0.0, np.inf], f), "minus_inf": np.array([-np.inf, 0.0], f),
        "nan_last": np.concatenate([inside, [np.nan]]).astype(f), "nan_first": np.concatenate([[np.nan], inside]).astype(f),
        "nan_alone": np.array([np.nan], f),
    }


def test_normalize_oracle_and_its_faults():
    size, cases = _normalize_cases()
    flags = {k: O.normalize(v, size)[1] for k, v in cases.items()}
    assert flags == dict(all_negative=False, zeros=False, denormal=False, exactly_size=False, one_ulp_above=True, one_ulp_below=True,
                         inf=True, minus_inf=True, nan_last=True, nan_first=True, nan_alone=True)
    for name, x in cases.items():
        out01, flag, mn, mx = O.normalize(x, size)
        got = O.normalize_f32(x, size)
        assert got[0] == flag
        if mn is None:
            assert got[1:] == (O.INT32_MAX, O.INT32_MIN)
        else:
            assert O.unordered_float(got[1]) == mn and O.unordered_float(got[2]) == mx
        want = ((x.astype(np.float64) + float(size)) / (2 * float(size)))
        with np.errstate(invalid="ignore"):
            assert (np.abs(out01 - want)[~np.isnan(x) & np.isfinite(x)] <= 2.0 ** -23).all()      # fp32 add and divide: within 2 ulp of 1
    # without the sign fold negative values order backwards: every case with two different negative values (or a negative
    # minimum next to a positive maximum, which still orders) -- all_negative is the one that cannot pass
    x = cases["all_negative"]
    bad = O.normalize_f32(x, size, "no_sign_fold")
    assert O.unordered_float(bad[1]) != float(x.min()) or O.unordered_float(bad[2]) != float(x.max())
    # the fault the GPU module found: fminf / fmaxf drop a NaN, so a range test on the reduced min / max never sees it
    for name in ("nan_last", "nan_first", "nan_alone"):
        assert O.normalize_f32(cases[name], size, "nan_lost")[0] is False and flags[name] is True


def test_ordered_int_orders_like_the_floats():
    v = np.array([-np.inf, -1.0, -1e-45, -0.0, 0.0, 1e-45, 0.3, np.inf], O.f32)
    o = O.ordered_int(v)
    assert (np.diff(o) > 0).all()
    assert [O.unordered_float(i) for i in o] == [float(x) for x in v]


def test_sampler_restatement_matches_torch_linspace_and_the_oracle():
    torch = pytest.importorskip("torch")
    from oracle import render_ref as R
    for S in (2, 3, 65, 257, 1024):
        np.testing.assert_array_equal(O.lin_t(S), torch.linspace(0, 1, S).numpy())
    rays = O.make_rays(11, 5)
    for S in (2, 65):
        tr = np.random.default_rng(S).random((11, S)).astype(O.f32)
        for perturb in (False, True):
            z, pts = O.sample(rays, tr, S, perturb, 0.3)
            rt = torch.from_numpy(rays)
            z_ref = R.sample_depths(rt[:, 6:7], rt[:, 7:], S, perturb, torch.from_numpy(tr))
            assert np.array_equal(z, z_ref.numpy()) and np.array_equal(pts, R.points_on_rays(rt, z_ref, 0.3).numpy())
