"""The CGLS vector kernels on the GPU (naf_cgls_wdot / naf_cgls_residual_step / naf_cgls_direction_step, cgls_kernels.py) against the
float64 forms of tests/_cgls_oracle.py, and `reconstruct.cgls` end to end against the float64 `cgls_operators` over the projector
oracles, on the 16^3 FDK rehearsal scan.  DESIGN.md section 19.

The solver bound.  CG amplifies the rounding of its operators, so no bound on the distance to the float64 iteration is derived.
It is measured instead, without any of the new kernels: `cgls_operators` in float32 over `projector.project_scan` and
`sart.backproject_scan` (array code on existing kernels) differs from the float64 oracle after 8 iterations by FLOAT32_SPREAD, of
the largest voxel (the volume) and of the first norm (the norms), as measured on an MI355X; the kernel solver is allowed 4 x
that, the house margin of DESIGN.md section 14.  `test_solver_matches_float64` prints today's spread next to the constant."""
import functools
import math

import numpy as np
import pytest
import torch

import _cgls_oracle as C

pytestmark = pytest.mark.gpu

# (mode, weighted) -> (max |x32 - x64| / max |x64|, max |norm32 - norm64| / norm64[0]) of the float32 composition after 8 iterations,
# measured on an MI355X: the largest of four scatter runs and two gather runs per case (the scatter's atomics move the last digits)
FLOAT32_SPREAD = {
    ("cone", False): (9.882e-07, 3.653e-08),
    ("cone", True): (9.563e-07, 3.813e-08),
    ("parallel", False): (1.461e-06, 4.567e-08),
    ("parallel", True): (1.476e-06, 4.583e-08),
}
MARGIN = 4.0


def _dev(a):
    return torch.tensor(np.ascontiguousarray(a), device="cuda")


def _workspace(n, n_iter=4):
    from neuralvolumetricreconstructionformedicalimages_amd import cgls_kernels as K
    return K.Workspace(n, n_iter, "cuda")


def _set(ws, gamma, delta, gamma_next, k, stopped=0):
    from neuralvolumetricreconstructionformedicalimages_amd import cgls_kernels as K
    ws.reset()
    values = torch.zeros(4, dtype=torch.float64)
    values[K.SLOT_GAMMA[k & 1]], values[K.SLOT_GAMMA[(k + 1) & 1]], values[K.SLOT_DELTA], values[K.SLOT_STOPPED] = \
        gamma, gamma_next, delta, stopped
    ws.scalars[:4] = values.cuda()


@pytest.mark.parametrize("n", C.SIZES)
def test_wdot_matches_float64_and_returns_the_same_bits(n):
    """sum w a^2 within (n + 2) 2^-53 of the correctly rounded float64 sum, with and without w, into each slot; two calls and an
    unaligned copy of the inputs (the element path) return the same bits; a NaN input gives NaN."""
    from neuralvolumetricreconstructionformedicalimages_amd import cgls_kernels as K
    r, _, w, _, _, _ = C.step_inputs(n)
    a = _dev(r)
    ws = _workspace(n)
    shifted_a, shifted_w = torch.empty(n + 1, device="cuda")[1:], torch.empty(n + 1, device="cuda")[1:]
    shifted_a.copy_(a)
    shifted_w.copy_(_dev(w))
    for weights, slot in ((None, K.SLOT_GAMMA[0]), (w, K.SLOT_DELTA), (None, K.SLOT_GAMMA[1])):
        want = C.wsum(r, weights)
        wd = None if weights is None else _dev(weights)
        got = []
        for arrays in ((a, wd), (a, wd), (shifted_a, None if wd is None else shifted_w)):
            ws.reset()
            K.wdot(*arrays, slot, ws)
            got.append(ws.scalars.cpu())
        value = float(got[0][slot])
        print(f"n {n} slot {slot} w {weights is not None}: sum {value:.17e}, float64 {want:.17e}, bound {C.wsum_bound(n, want):.3e}")
        assert abs(value - want) <= C.wsum_bound(n, want)
        assert torch.equal(got[0], got[1]) and torch.equal(got[0], got[2])
        others = got[0].clone()
        others[slot] = 0
        assert int((others != 0).sum()) == 0                              # nothing but the slot was written
    bad = a.clone()
    bad[n // 2] = float("nan")
    K.wdot(bad, _dev(w), K.SLOT_DELTA, ws)
    assert math.isnan(float(ws.scalars[K.SLOT_DELTA]))


@pytest.mark.parametrize("n", C.SIZES)
def test_residual_step_matches_float64(n):
    from neuralvolumetricreconstructionformedicalimages_amd import cgls_kernels as K
    r0, q0, w0, _, _, _ = C.step_inputs(n)
    ws = _workspace(n)
    worst = 0.0
    for k, (gamma, delta, gamma_next) in enumerate(C.LIVE_SCALARS):
        for weights in (w0, None):
            r, q, y = _dev(r0), _dev(q0), torch.full((n,), 7.0, device="cuda")
            w = None if weights is None else _dev(weights)
            _set(ws, gamma, delta, gamma_next, k)
            assert K.residual_step(r, q, w, y, k, ws) is y
            want_r, want_y = C.residual_step(r0, q0, weights, gamma, delta)
            got_r, got_y = r.cpu().numpy(), y.cpu().numpy()
            bound_r, bound_y = C.residual_bounds(q0, weights, gamma, delta, got_r, got_y)
            worst = max(worst, float((np.abs(got_r - want_r) / bound_r).max()), float((np.abs(got_y - want_y) / np.maximum(bound_y, 1e-300)).max()))
            assert np.all(np.abs(got_r - want_r) <= bound_r) and np.all(np.abs(got_y - want_y) <= bound_y)
            if weights is not None:
                assert (got_y[weights == 0] == 0).all()
            assert torch.equal(q, _dev(q0))
            scalars = ws.scalars.cpu()
            total = C.wsum(r0, weights)
            assert abs(float(scalars[K.HISTORY + k]) - total) <= C.wsum_bound(n, total)             # of the r it was given
            assert float(scalars[K.SLOT_STOPPED]) == 0 and float(scalars[K.SLOT_DELTA]) == delta
            assert float(scalars[K.SLOT_GAMMA[k & 1]]) == gamma
    print(f"n {n}: worst |. - float64| / bound over r and y = {worst:.3e}")


@pytest.mark.parametrize("n", C.SIZES)
def test_direction_step_matches_float64(n):
    from neuralvolumetricreconstructionformedicalimages_amd import cgls_kernels as K
    _, _, _, x0, p0, s0 = C.step_inputs(n)
    ws = _workspace(n)
    worst = 0.0
    for k, (gamma, delta, gamma_next) in enumerate(C.LIVE_SCALARS):
        x, p, s = _dev(x0), _dev(p0), _dev(s0)
        _set(ws, gamma, delta, gamma_next, k)
        before = ws.scalars.cpu()
        assert K.direction_step(x, p, s, k, ws) is x
        want_x, want_p = C.direction_step(x0, p0, s0, gamma, delta, gamma_next)
        got_x, got_p = x.cpu().numpy(), p.cpu().numpy()
        bound_x, bound_p = C.fma_bound(gamma / delta, p0, got_x), C.fma_bound(gamma_next / gamma, p0, got_p)
        worst = max(worst, float((np.abs(got_x - want_x) / bound_x).max()), float((np.abs(got_p - want_p) / bound_p).max()))
        assert np.all(np.abs(got_x - want_x) <= bound_x) and np.all(np.abs(got_p - want_p) <= bound_p)
        assert torch.equal(s, _dev(s0)) and torch.equal(ws.scalars.cpu(), before)
    print(f"n {n}: worst |. - float64| / bound over x and p = {worst:.3e}")


@pytest.mark.parametrize("n", (1, 65, 300001))
def test_breakdown_and_stop_leave_everything_as_it_is(n):
    """delta = 0 (and every other scalar that is not > 0, NaN included) and a stop mark set earlier: r, x and p come back bit for
    bit even where q and s are not finite, y = w r, and the stop mark is this iteration or stays the earlier one."""
    from neuralvolumetricreconstructionformedicalimages_amd import cgls_kernels as K
    r0, q0, w0, x0, p0, s0 = C.step_inputs(n)
    q0, s0 = q0.copy(), s0.copy()
    q0[0], s0[n // 2] = np.inf, np.nan
    ws = _workspace(n, 6)
    k = 3
    cases = [(scalars, 0, k) for scalars in C.DEAD_SCALARS] + [(C.LIVE_SCALARS[0], 2, 1)]        # (scalars, mark set, stopped_at)
    for (gamma, delta, gamma_next), mark, stopped_at in cases:
        for weights in (w0, None):
            r, q, y = _dev(r0), _dev(q0), torch.full((n,), 7.0, device="cuda")
            x, p, s = _dev(x0), _dev(p0), _dev(s0)
            w = None if weights is None else _dev(weights)
            _set(ws, gamma, delta, gamma_next, k, stopped=mark)
            K.residual_step(r, q, w, y, k, ws)
            assert ws.stopped_at() == stopped_at
            K.direction_step(x, p, s, k, ws)
            assert torch.equal(r, _dev(r0)) and torch.equal(x, _dev(x0)) and torch.equal(p, _dev(p0))
            assert torch.equal(y, _dev(r0 if weights is None else weights * r0))
            assert ws.stopped_at() == stopped_at
    # the direction step alone on a breakdown that no residual step has marked yet
    x, p, s = _dev(x0), _dev(p0), _dev(s0)
    _set(ws, 2.0, 0.0, 1.5, k)
    K.direction_step(x, p, s, k, ws)
    assert torch.equal(x, _dev(x0)) and torch.equal(p, _dev(p0)) and ws.stopped_at() is None


def test_wrapper_refusals(monkeypatch):
    from neuralvolumetricreconstructionformedicalimages_amd import _abi, cgls_kernels as K
    a, b, c, d = (torch.zeros(8, device="cuda") for _ in range(4))
    ws = _workspace(8, 2)
    with monkeypatch.context() as m:                                       # refused before the library is reached
        m.setattr(_abi, "lib", lambda: pytest.fail("the library was called"))
        with pytest.raises(RuntimeError, match="no CPU path"):
            K.wdot(a.cpu(), None, 0, ws)
        with pytest.raises(TypeError, match="float32"):
            K.wdot(a.double(), None, 0, ws)
        with pytest.raises(ValueError, match="slot"):
            K.wdot(a, None, 3, ws)
        with pytest.raises(ValueError, match="shape"):
            K.wdot(a, torch.zeros(7, device="cuda"), 0, ws)
        with pytest.raises(ValueError, match="up to 8 elements"):
            K.wdot(torch.zeros(9, device="cuda"), None, 0, ws)
        with pytest.raises(TypeError, match="Workspace"):
            K.wdot(a, None, 0, None)
        with pytest.raises(ValueError, match="y must not be q"):
            K.residual_step(a, b, None, b, 0, ws)
        with pytest.raises(ValueError, match="y must not be q"):
            K.residual_step(a, b, None, a, 0, ws)
        with pytest.raises(ValueError, match="k must be in"):
            K.residual_step(a, b, c, d, 2, ws)
        with pytest.raises(ValueError, match="must not overlap"):
            K.direction_step(a, a, c, 0, ws)
        with pytest.raises(ValueError, match="contiguous"):
            K.direction_step(a, torch.zeros(8, 2, device="cuda")[:, 0], c, 0, ws)
    empty = torch.zeros(0, device="cuda")
    K.wdot(empty, None, 0, ws)
    assert int((ws.scalars != 0).sum()) == 0


# ---- the solver -------------------------------------------------------------------------------------------------------------------
def _weights(c, weighted):
    return _dev(c["w"]) if weighted else None


@functools.lru_cache(maxsize=None)
def _solve(mode, weighted, deterministic):
    from neuralvolumetricreconstructionformedicalimages_amd import cgls
    c = C.scan_case(mode)
    info = {}
    x, norms = cgls(_dev(c["b"]), c["geo"], c["angles"], n_iter=C.SCAN_ITERS, weights=_weights(c, weighted), nonneg=False,
                    deterministic=deterministic, info=info)
    return x, norms, info


def _float32_composition(mode, weighted, deterministic):
    """`cgls_operators` in float32 over the existing projector pair: none of the new kernels."""
    from neuralvolumetricreconstructionformedicalimages_amd import projector, sart
    from neuralvolumetricreconstructionformedicalimages_amd.reconstruct import cgls_operators
    c = C.scan_case(mode)
    geo, angles = c["geo"], c["angles"]
    method = "gather" if deterministic else "scatter"
    return cgls_operators(lambda x: projector.project_scan(x, geo, angles),
                          lambda y: sart.backproject_scan(y.contiguous(), geo, angles, method=method),
                          _dev(c["b"]), C.SCAN_ITERS, weights=_weights(c, weighted), nonneg=False)


def _spread(x, norms, x64, norms64):
    dx = float(np.abs(x.cpu().numpy().astype(np.float64) - x64).max() / np.abs(x64).max())
    dn = max(abs(a - b) for a, b in zip(norms, norms64)) / norms64[0]
    return dx, dn


@pytest.mark.parametrize("deterministic", [False, True], ids=["scatter", "gather"])
@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "weighted"])
@pytest.mark.parametrize("mode", ["cone", "parallel"])
def test_solver_matches_float64(mode, weighted, deterministic):
    x64, norms64 = C.scan_solution(mode, weighted)
    x, norms, info = _solve(mode, weighted, deterministic)
    assert x.dtype == torch.float32 and tuple(x.shape) == x64.shape and len(norms) == C.SCAN_ITERS and info == {"stopped_at": None}
    dx, dn = _spread(x, norms, x64, norms64)
    today = _spread(*_float32_composition(mode, weighted, deterministic), x64, norms64)
    allowed = FLOAT32_SPREAD[(mode, weighted)]
    print(f"{mode} weighted {weighted} {'gather' if deterministic else 'scatter'}: kernels {dx:.3e} of max |x|, norms {dn:.3e} of "
          f"norms[0]; float32 composition today {today[0]:.3e}, {today[1]:.3e}, recorded {allowed[0]:.3e}, {allowed[1]:.3e}; "
          f"norms {norms[0]:.5e} -> {norms[-1]:.5e}")
    assert dx <= MARGIN * allowed[0] and dn <= MARGIN * allowed[1]
    assert all(b <= a for a, b in zip(norms, norms[1:]))


@pytest.mark.parametrize("mode", ["cone", "parallel"])
def test_deterministic_runs_return_the_same_bits_and_ignore_masked_rays(mode):
    """Two deterministic runs: the same volume and norms bit for bit.  And 1e3 written into the projections inside the zero-weight
    patches changes no bit either: a zero weight leaves the ray out."""
    from neuralvolumetricreconstructionformedicalimages_amd import cgls
    c = C.scan_case(mode)
    x, norms, _ = _solve(mode, True, True)
    again, norms_again = cgls(_dev(c["b"]), c["geo"], c["angles"], n_iter=C.SCAN_ITERS, weights=_weights(c, True), nonneg=False,
                              deterministic=True)
    assert torch.equal(x, again) and norms == norms_again
    spoiled = c["b"].copy()
    spoiled[c["patch"]] = 1e3
    masked, norms_masked = cgls(_dev(spoiled), c["geo"], c["angles"], n_iter=C.SCAN_ITERS, weights=_weights(c, True), nonneg=False,
                                deterministic=True)
    assert torch.equal(x, masked) and norms == norms_masked


def test_breakdown_options_and_refusals():
    from neuralvolumetricreconstructionformedicalimages_amd import cgls
    c = C.scan_case("parallel")
    geo, angles, b = c["geo"], c["angles"], _dev(c["b"])
    info, calls = {}, []
    x, norms = cgls(torch.zeros_like(b), geo, angles, n_iter=5, info=info)
    assert int((x != 0).sum()) == 0 and norms == [0.0] and info == {"stopped_at": 0}
    x, norms = cgls(torch.zeros_like(b), geo, angles, n_iter=5, weights=_weights(c, True), info=info, deterministic=True,
                    callback=lambda k, x, n: calls.append(k))
    assert bool(torch.isfinite(x).all()) and int((x != 0).sum()) == 0 and norms == [0.0] and info == {"stopped_at": 0} and calls == []
    # callback, nonneg and x0: the callback sees every iteration's norm; the clamp is applied once at the end; x0 is left alone
    free, norms_free, _ = _solve("parallel", False, True)
    seen = []
    clamped, norms = cgls(b, geo, angles, n_iter=C.SCAN_ITERS, deterministic=True, callback=lambda k, x, n: seen.append((k, n)))
    assert float(free.min()) < 0 and torch.equal(clamped, free.clamp(min=0)) and norms == list(norms_free)
    assert [k for k, _ in seen] == list(range(C.SCAN_ITERS)) and [n for _, n in seen] == norms
    x0 = free.clamp(min=0)
    keep = x0.clone()
    warm, warm_norms = cgls(b, geo, angles, n_iter=1, x0=x0)
    assert torch.equal(x0, keep) and warm is not x0 and warm_norms[0] < norms[0]
    same, none = cgls(b, geo, angles, n_iter=0, x0=x0)
    assert torch.equal(same, x0) and same is not x0 and none == []
    with pytest.raises(RuntimeError, match="no CPU path"):
        cgls(b.cpu(), geo, angles)
    with pytest.raises(ValueError, match="n_iter"):
        cgls(b, geo, angles, n_iter=-1)
    with pytest.raises(ValueError, match="weights must be float32"):
        cgls(b, geo, angles, weights=torch.ones(b.shape[0], b.shape[1], b.shape[2] - 1, device="cuda"))
    for bad in (-1.0, float("nan"), float("inf")):
        w = torch.ones_like(b)
        w[1, 2, 3] = bad
        with pytest.raises(ValueError, match=">= 0 and finite"):
            cgls(b, geo, angles, weights=w)
    with pytest.raises(ValueError, match="nVoxel"):
        cgls(b, geo, angles, x0=torch.zeros(16, 16, 15, device="cuda"))


def test_ray_length_weights_and_sirt_side_by_side():
    """Printed, not asserted: with R = 1 / (A 1) the objective is SIRT's, but the two Krylov spaces differ, so there is no theorem
    that orders the two residuals.  What is asserted is the helper itself."""
    from neuralvolumetricreconstructionformedicalimages_amd import cgls, projector, sirt
    from neuralvolumetricreconstructionformedicalimages_amd.reconstruct import pwls_weights, ray_length_weights
    c = C.scan_case("cone")
    geo, angles, b = c["geo"], c["angles"], _dev(c["b"])
    R = ray_length_weights(geo, angles, "cuda")
    row = projector.project_scan(torch.ones(c["dims"], device="cuda"), geo, angles)
    assert R.shape == b.shape and R.dtype == torch.float32
    assert torch.equal(R[row > 0], 1.0 / row[row > 0]) and int((R[row <= 0] != 0).sum()) == 0 and int((row > 0).sum()) > 0
    assert torch.equal(pwls_weights(b), torch.exp(-b))
    _, norms = cgls(b, geo, angles, n_iter=9, weights=R)
    _, sirt_norms = sirt(b, geo, angles, n_iter=9)
    print(f"||b - A x||_R after 8 iterations: CGLS {norms[8]:.5e}, SIRT {sirt_norms[8]:.5e} (start {norms[0]:.5e} and {sirt_norms[0]:.5e})")
    assert abs(norms[0] - sirt_norms[0]) <= 1e-5 * sirt_norms[0]
