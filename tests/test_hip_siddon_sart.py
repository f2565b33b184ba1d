"""The OS-SART subset step on the Siddon pair on the GPU (naf_sart_residual_scan_siddon / naf_sart_backproject_scan_siddon,
sart.py and reconstruct.py kind="siddon"; include/naf_hip.h P8): the residual kernel bit for bit against the
forward kernel, the paired transpose against the triples of tests/_siddon_transpose_oracle.py and their per-voxel bound, and
`os_sart` / `fista_tv` on the pair against their float64 and operator forms."""
import numpy as np
import pytest
import torch

import _siddon_oracle as S
import _siddon_sart_oracle as Q
import _siddon_transpose_oracle as T

pytestmark = pytest.mark.gpu

VIEW_LISTS = ([5, 0, 3], None)
PER_VIEW = 24 * 24


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _listed(views):
    return list(range(len(S.SCAN_ANGLES))) if views is None else views


@pytest.fixture(scope="module")
def scans():
    """mode -> (geo, rays of the whole scan as the kernels make them [8 * 576, 8], {view list: triples of its rays in list order})."""
    from neuralvolumetricreconstructionformedicalimages_amd.geometry import ConeGeometry, RayGenerator
    out = {}
    for mode in ("cone", "parallel"):
        geo = ConeGeometry(S.scan_geometry(mode))
        gen = RayGenerator(geo, S.SCAN_ANGLES, "cuda")
        rays = torch.cat([gen.rays_for_projection(i) for i in range(len(S.SCAN_ANGLES))]).cpu().numpy()
        by_view = rays.reshape(len(S.SCAN_ANGLES), PER_VIEW, 8)
        triples = {str(v): T.walk_triples(S.DIMS, geo.dVoxel, by_view[_listed(v)].reshape(-1, 8)) for v in VIEW_LISTS}
        out[mode] = (geo, rays, triples)
    return out


@pytest.mark.parametrize("mode", ["cone", "parallel"])
def test_residual_kernel(scans, mode):
    """5. r = b - A x and y = r / (A 1) are each one IEEE operation on the forward kernel's own bits, so both are held bit for bit
    (the expected values are formed on the host in float32 numpy); against float64, r stays within P6's bound plus the rounding
    of the subtraction, u (|r64| + bound)."""
    from neuralvolumetricreconstructionformedicalimages_amd import projector, sart
    geo, rays, _ = scans[mode]
    rng = np.random.default_rng(51)
    x = S.volume(S.DIMS, seed=12)
    b = rng.standard_normal((8, 24, 24)).astype(np.float32)
    xd, bd = _dev(x), _dev(b)
    Ax = projector.project_scan(xd, geo, S.SCAN_ANGLES, kind="siddon").cpu().numpy()
    row = projector.project_scan(torch.ones_like(xd), geo, S.SCAN_ANGLES, kind="siddon").cpu().numpy()
    want64, bound = S.project_rays(x, geo.dVoxel, rays)
    for views in VIEW_LISTS:
        v = _listed(views)
        y, r = sart.residual_scan(xd, bd, geo, S.SCAN_ANGLES, views, kind="siddon")
        assert tuple(y.shape) == tuple(r.shape) == (len(v), 24, 24) and y.dtype == r.dtype == torch.float32
        assert torch.equal(bd, _dev(b))                                            # `projections` is only read
        y, r = y.cpu().numpy(), r.cpu().numpy()
        want_r = (b[v] - Ax[v]).astype(np.float32)
        hit = row[v] > 0
        with np.errstate(divide="ignore", invalid="ignore"):
            want_y = np.where(hit, (want_r / row[v]).astype(np.float32), np.float32(0))
        assert np.array_equal(_bits(r), _bits(want_r)) and np.array_equal(_bits(y), _bits(want_y))
        assert 100 < int((~hit).sum()) < hit.size - 100                            # rays that miss: y = 0 and r = b exactly
        assert np.array_equal(_bits(r[~hit]), _bits(b[v][~hit])) and not y[~hit].any() and not Ax[v][~hit].any()
        y_only, none = sart.residual_scan(xd, bd, geo, S.SCAN_ANGLES, views, want_r=False, kind="siddon")
        again, again_r = sart.residual_scan(xd, bd, geo, S.SCAN_ANGLES, views, kind="siddon")
        assert none is None and np.array_equal(_bits(y_only.cpu().numpy()), _bits(y))
        assert np.array_equal(_bits(again.cpu().numpy()), _bits(y)) and np.array_equal(_bits(again_r.cpu().numpy()), _bits(r))
        r64 = b[v].astype(np.float64).reshape(-1) - want64.reshape(8, PER_VIEW)[v].reshape(-1)
        allowed = bound.reshape(8, PER_VIEW)[v].reshape(-1)
        allowed = allowed + S.U * (np.abs(r64) + allowed)
        use = float((np.abs(r.reshape(-1).astype(np.float64) - r64) / allowed).max())
        print(f"{mode}, views {views}: {int((~hit).sum())} of {hit.size} rays miss; r against float64 uses {use:.3f} of the bound")
        assert use <= 1.0
    # it is another residual than the interpolated pair's
    assert not torch.equal(sart.residual_scan(xd, bd, geo, S.SCAN_ANGLES)[0], sart.residual_scan(xd, bd, geo, S.SCAN_ANGLES, kind="siddon")[0])


@pytest.mark.parametrize("mode", ["cone", "parallel"])
def test_paired_transpose(scans, mode):
    """6. y of mixed signs with exact zeros planted, non-zero starts in both volumes: num within the per-voxel bound, den within the
    same bound for y = 1, untouched voxels bit-equal to the start; from a zeroed den, every voxel crossed by a ray whose y is 0 is
    strictly positive; den=None against projector.backproject_scan(kind="siddon") of the gathered views within twice the bound
    (atomic order only, as tests/test_hip_siddon_transpose.py::test_scan_equals_rays allows)."""
    from neuralvolumetricreconstructionformedicalimages_amd import projector, sart
    geo, _, triples = scans[mode]
    num0, den0 = T.start_volume(S.DIMS, 22), T.start_volume(S.DIMS, 23)
    for views in VIEW_LISTS:
        v, t = _listed(views), triples[str(views)]
        y = Q.planted_values(len(v) * PER_VIEW)
        (want_n, bound_n, m_n), (want_d, bound_d, m_d) = Q.pair_bounds(t, y, num0, den0)
        yd = _dev(y.reshape(len(v), 24, 24))
        num, den = _dev(num0).clone(), _dev(den0).clone()
        assert sart.backproject_scan(yd, geo, S.SCAN_ANGLES, views, num=num, den=den, kind="siddon") is num
        num, den = num.cpu().numpy().reshape(-1), den.cpu().numpy().reshape(-1)
        use_n, use_d = float(T.use(num, want_n, bound_n).max()), float(T.use(den, want_d, bound_d).max())
        assert np.array_equal(_bits(num[m_n == 0]), _bits(num0.reshape(-1)[m_n == 0]))
        assert np.array_equal(_bits(den[m_d == 0]), _bits(den0.reshape(-1)[m_d == 0]))
        assert int(m_d.sum()) > int(m_n.sum()) > 1000
        # the chord lengths of the rays with y == 0 reach den
        zeroed = torch.zeros(S.DIMS, device="cuda")
        sart.backproject_scan(yd, geo, S.SCAN_ANGLES, views, num=_dev(num0).clone(), den=zeroed, kind="siddon")
        crossed = np.zeros(t["n_voxels"], dtype=bool)
        crossed[t["offset"][(t["a"] > 0) & (y[t["ray"]] == 0)]] = True
        assert int(crossed.sum()) > 100 and (zeroed.cpu().numpy().reshape(-1)[crossed] > 0).all()
        # without den the numerator is P7's
        alone = sart.backproject_scan(yd, geo, S.SCAN_ANGLES, views, num=_dev(num0).clone(), kind="siddon").cpu().numpy().reshape(-1)
        full = np.zeros((8, 24, 24), dtype=np.float32)
        rest = [i for i in range(8) if i not in v]
        full[v] = y.reshape(len(v), 24, 24)
        assert not full[rest].any()
        p7 = projector.backproject_scan(_dev(full), geo, S.SCAN_ANGLES, out=_dev(num0).clone(), kind="siddon").cpu().numpy().reshape(-1)
        assert (np.abs(alone.astype(np.float64) - p7.astype(np.float64)) <= 2 * bound_n).all()
        use_alone = float(T.use(alone, want_n, bound_n).max())
        print(f"{mode}, views {views}: num uses {use_n:.3f} of the bound, den {use_d:.3f}, num without den {use_alone:.3f}; "
              f"{int(m_n.sum())} terms to num, {int(m_d.sum())} to den")
        assert max(use_n, use_d, use_alone) <= 1.0


@pytest.mark.parametrize("mode", ["cone", "parallel"])
def test_adjoint_identity(scans, mode):
    """6, last item.  sum num x against sum y (A x) in float64 for positive x and y (the allowance of DESIGN.md section 21 and
    tests/test_hip_siddon_transpose.py::test_adjoint_identity is relative to a sum without cancellation):
    1.001 u (K_max + 2 + m_max + 1)."""
    from neuralvolumetricreconstructionformedicalimages_amd import projector, sart
    geo, _, triples = scans[mode]
    t = triples["None"]
    rng = np.random.default_rng(31)
    x = rng.uniform(0.1, 1.0, S.DIMS).astype(np.float32)
    y = rng.uniform(0.1, 1.0, (8, 24, 24)).astype(np.float32)
    Ax = projector.project_scan(_dev(x), geo, S.SCAN_ANGLES, kind="siddon").cpu().numpy().astype(np.float64)
    den = torch.zeros(S.DIMS, device="cuda")
    num = sart.backproject_scan(_dev(y), geo, S.SCAN_ANGLES, None, den=den, kind="siddon").cpu().numpy().astype(np.float64)
    lhs, rhs = float((Ax * y).sum()), float((x * num).sum())
    m = np.bincount(t["offset"][t["a"] > 0], minlength=t["n_voxels"])
    allowed = 1.001 * S.U * (int(t["steps"].max()) + 2 + int(m.max()) + 1)
    print(f"{mode}: <Ax, y> {lhs:.9e}, <x, num> {rhs:.9e}, relative difference {abs(lhs - rhs) / lhs:.3e}, allowed {allowed:.3e}")
    assert lhs > 0 and abs(lhs - rhs) <= allowed * lhs
    # and the column sums against the row sums: <A 1, 1> = <1, A^T 1>
    rows = projector.project_scan(torch.ones(S.DIMS, device="cuda"), geo, S.SCAN_ANGLES, kind="siddon").double().sum().item()
    cols = den.double().sum().item()
    assert abs(rows - cols) <= allowed * rows


@pytest.fixture(scope="module")
def phantom():
    """The 32^3 phantom of _siddon_oracle.orientation_case, 8 views of 24 x 24, the data made by project_scan(kind="siddon"), the
    float64 operators of the triples of the kernels' own rays, and the float64 OS-SART of 20 iterations, made once."""
    from neuralvolumetricreconstructionformedicalimages_amd import projector
    from neuralvolumetricreconstructionformedicalimages_amd.geometry import RayGenerator
    from neuralvolumetricreconstructionformedicalimages_amd.reconstruct import os_sart_operators, subset_order
    _, geo, vol, _, _, angles = S.orientation_case()
    b = projector.project_scan(_dev(vol), geo, angles, kind="siddon")
    gen = RayGenerator(geo, angles, "cuda")
    rays = torch.cat([gen.rays_for_projection(i) for i in range(len(angles))]).cpu().numpy()
    ops = Q.phantom_operators(rays, vol.shape, geo.dVoxel)
    subsets = [list(s) for s in subset_order(angles, len(angles))]
    x64, norms64 = os_sart_operators(ops.A, ops.AT, b.cpu().numpy().astype(np.float64), subsets, 20)
    return {"geo": geo, "angles": angles, "vol": vol, "b": b, "x64": x64, "norms64": norms64, "cache": {}}


def _os_sart_20(phantom):
    from neuralvolumetricreconstructionformedicalimages_amd import os_sart
    if "x" not in phantom["cache"]:
        phantom["cache"]["x"] = os_sart(phantom["b"], phantom["geo"], phantom["angles"], n_iter=20, kind="siddon")
    return phantom["cache"]["x"]


def test_os_sart_end_to_end_against_float64(phantom):
    """7. 20 iterations, one view per subset, against `os_sart_operators` in float64 on the triples: the two conditions of
    tests/test_hip_sart.py::test_os_sart_end_to_end_against_float64 (tests/test_hip_sart.py:203 and :204)."""
    vol, x64, norms64 = phantom["vol"], phantom["x64"], phantom["norms64"]
    x, norms = _os_sart_20(phantom)
    assert tuple(x.shape) == vol.shape and x.dtype == torch.float32 and float(x.min()) >= 0 and len(norms) == 20
    got = x.cpu().numpy().astype(np.float64)
    p, p64 = Q.psnr_3d(got, vol), Q.psnr_3d(x64, vol)
    rel = [abs(a - c) / c for a, c in zip(norms, norms64)]
    print(f"psnr_3d {p:.3f} dB (float64 {p64:.3f} dB); relative L2 distance to float64 {np.linalg.norm(got - x64) / np.linalg.norm(x64):.3e}; "
          f"norms {norms[0]:.6e} -> {norms[-1]:.6e}, largest relative norm difference {max(rel):.3e}, first {rel[0]:.3e}")
    assert abs(p - p64) <= 0.1
    assert rel[0] <= 1e-5


def test_one_subset_of_all_views_against_sirt(phantom):
    """8. 5 iterations: psnr_3d within 0.1 dB of sirt(kind="siddon") (tests/test_hip_sart.py:215).  R has the same bits in both;
    what is left is the atomic order and the form of the update."""
    from neuralvolumetricreconstructionformedicalimages_amd import os_sart, sirt
    geo, angles, vol, b = (phantom[k] for k in ("geo", "angles", "vol", "b"))
    x, norms = os_sart(b, geo, angles, n_iter=5, n_subsets=1, kind="siddon")
    want, want_norms = sirt(b, geo, angles, n_iter=5, kind="siddon")
    p, p_sirt = Q.psnr_3d(x.cpu().numpy(), vol), Q.psnr_3d(want.cpu().numpy(), vol)
    print(f"one subset vs sirt, 5 iterations: psnr_3d {p:.4f} vs {p_sirt:.4f} dB, max abs difference "
          f"{float((x - want).abs().max()):.3e} (max of volume {float(want.max()):.3e}), norms {norms[-1]:.6e} vs {want_norms[-1]:.6e}")
    assert abs(p - p_sirt) <= 0.1


def test_without_the_weight_cache_and_two_subsets(phantom):
    """9. weight_cache_bytes=0 against the cached run at 20 iterations: within 0.01 dB; two sequential subsets beat SIRT at 5."""
    from neuralvolumetricreconstructionformedicalimages_amd import os_sart, sirt
    geo, angles, vol, b = (phantom[k] for k in ("geo", "angles", "vol", "b"))
    x, _ = _os_sart_20(phantom)
    uncached, norms = os_sart(b, geo, angles, n_iter=20, weight_cache_bytes=0, kind="siddon")
    p, p_un = Q.psnr_3d(x.cpu().numpy(), vol), Q.psnr_3d(uncached.cpu().numpy(), vol)
    print(f"cached {p:.4f} dB, uncached {p_un:.4f} dB, max abs difference {float((x - uncached).abs().max()):.3e}")
    assert abs(p - p_un) <= 0.01 and len(norms) == 20
    two, _ = os_sart(b, geo, angles, n_iter=5, n_subsets=2, order="sequential", kind="siddon")
    one, _ = sirt(b, geo, angles, n_iter=5, kind="siddon")
    p_two, p_one = Q.psnr_3d(two.cpu().numpy(), vol), Q.psnr_3d(one.cpu().numpy(), vol)
    print(f"5 iterations: two sequential subsets {p_two:.3f} dB, sirt {p_one:.3f} dB")
    assert p_two > p_one


# tests/test_hip_tvprox.py:27 (FISTA_REL_BOUND = MARGIN * 6.01e-7 / 0.778, MARGIN = 4 at :22): the fp32-against-fp64 spread of
# `fista_tv_operators` relative to the volume's largest value, x 4; applied as in tests/test_hip_tvprox.py:345
FISTA_REL_BOUND = 4 * 6.01e-7 / 0.778


def test_fista_tv_is_the_operator_form(phantom):
    """10. 30 iterations, 20 dual iterations (tests/test_hip_tvprox.py::test_fista_tv_is_the_operator_form) against
    `fista_tv_operators` over project_scan / backproject_scan(kind="siddon") with R = ray_length_weights(kind="siddon")."""
    from neuralvolumetricreconstructionformedicalimages_amd import fista_tv, fista_tv_operators, projector, reconstruct, tv
    geo, angles, b = (phantom[k] for k in ("geo", "angles", "b"))
    x, norms = fista_tv(b, geo, angles, n_iter=30, tv_iters=20, kind="siddon")
    state = {}

    def prox(z, t, nonneg):
        out, state["dual"] = tv.tv_prox(z, t, 20, nonneg, dual=state.get("dual"), return_dual=True)
        return out

    A = lambda v: projector.project_scan(v, geo, angles, kind="siddon")                      # noqa: E731
    AT = lambda y: projector.backproject_scan(y, geo, angles, kind="siddon")                 # noqa: E731
    want, want_norms = fista_tv_operators(A, AT, b, 30, prox, reconstruct.DEFAULT_FISTA_TV_LAMBDA)
    # the operator form's R is 1 / (A 1) of the forward kernel: the weights ray_length_weights(kind="siddon") returns
    R = reconstruct.ray_length_weights(geo, angles, "cuda", kind="siddon")
    assert torch.equal(R, reconstruct._inverse_where_positive(A(torch.ones_like(x)), torch))
    err, top = float((x - want).abs().max()), float(want.max())
    print(f"fista_tv(kind='siddon') against the operator form after 30 iterations: max abs difference {err:.3e} of a largest value "
          f"{top:.3e} (bound {FISTA_REL_BOUND * top:.3e}); norms {norms[0]:.6e} -> {norms[-1]:.6e} against {want_norms[0]:.6e} -> "
          f"{want_norms[-1]:.6e}")
    assert tuple(x.shape) == tuple(int(v) for v in geo.nVoxel) and x.dtype == torch.float32 and float(x.min()) >= 0 and len(norms) == 30
    assert err <= FISTA_REL_BOUND * top


def test_refusals(phantom):
    """11. What the Siddon pair cannot do raises ValueError, before anything is launched."""
    from neuralvolumetricreconstructionformedicalimages_amd import fista_tv, os_sart, sart
    geo, angles, b = (phantom[k] for k in ("geo", "angles", "b"))
    x = torch.zeros(tuple(int(v) for v in geo.nVoxel), device="cuda")
    for solver in (os_sart, fista_tv):
        with pytest.raises(ValueError, match="deterministic"):
            solver(b, geo, angles, n_iter=1, kind="siddon", deterministic=True)
        with pytest.raises(ValueError, match="bogus"):
            solver(b, geo, angles, n_iter=1, kind="bogus")
    with pytest.raises(ValueError, match="gather"):
        sart.backproject_scan(b, geo, angles, kind="siddon", method="gather")
    with pytest.raises(ValueError, match="bogus"):
        sart.backproject_scan(b, geo, angles, kind="bogus")
    with pytest.raises(ValueError, match="bogus"):
        sart.residual_scan(x, b, geo, angles, kind="bogus")
    num = torch.zeros_like(x)
    with pytest.raises(ValueError, match="two volumes"):
        sart.backproject_scan(b, geo, angles, num=num, den=num, kind="siddon")
