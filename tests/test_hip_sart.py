"""The OS-SART subset kernels on the GPU (naf_sart_residual_scan / naf_sart_backproject_scan / naf_sart_update, sart.py) against
the float64 oracles of tests/_sart_oracle.py and the torch expression, and `reconstruct.os_sart` end to end against the float64
`os_sart_operators`, `sirt` and itself without the weight cache."""
import functools

import numpy as np
import pytest
import torch

import _backproject_oracle as B
import _sart_oracle as S
import _tv_oracle as T
from test_hip_projector import _geometry

pytestmark = pytest.mark.gpu

BOUND = 1e-5                   # the forward and transpose tests': max abs error <= 1e-5 x max |result|

# name -> (scanner dict, angles, view list or None).  The three dense-matrix geometries of the back-projector tests (detector 10 x 8,
# two views, every ray of the first two hits the volume) and the seven-view scans with partial tiles at both detector edges.
SEVEN = np.linspace(0.1, 3.0, 7)
KERNEL_CASES = {f"{mode}-{tilt}-{'x'.join(map(str, dims))}": (lambda mode=mode, tilt=tilt, dims=dims: B.case_geometry(mode, tilt, dims),
                                                               B.CASE_ANGLES, None) for mode, tilt, dims in B.CASES}
for _mode, _tilt in (("cone", 0), ("parallel", 29)):
    for _views in ([5, 0, 3], None):
        KERNEL_CASES[f"{_mode}-{_tilt}-seven-{'list' if _views else 'all'}"] = (
            lambda mode=_mode, tilt=_tilt: dict(_geometry(mode, tilt), nDetector=[37, 21]), SEVEN, _views)
ALL_HIT = {f"{mode}-{tilt}-{'x'.join(map(str, dims))}" for mode, tilt, dims in B.CASES[:2]}


@functools.lru_cache(maxsize=None)
def _case(name):
    """Inputs and float64 references of a kernel case, made once and shared by the tests (read only)."""
    from neuralvolumetricreconstructionformedicalimages_amd.geometry import ConeGeometry
    make, angles, views = KERNEL_CASES[name]
    geo = ConeGeometry(make())
    angles = np.asarray(angles, dtype=np.float64)
    dims = tuple(int(v) for v in geo.nVoxel)
    N, H, W = len(angles), int(geo.nDetector[1]), int(geo.nDetector[0])
    listed = list(range(N)) if views is None else views
    rng = np.random.default_rng(len(name))
    x = rng.uniform(0.1, 1.1, dims).astype(np.float32)
    b = rng.uniform(0.0, 2.0, (N, H, W)).astype(np.float32)
    y = rng.uniform(0.5, 1.5, (len(listed), H, W)).astype(np.float32)
    rays = S.view_rays(geo, angles, listed)
    case = dict(geo=geo, angles=angles, dims=dims, views=views, listed=listed, x=x, b=b, y=y, rays=rays,
                residual=S.residual(x, b[listed], rays, geo), backprojection=S.backprojection(y, rays, geo, dims))
    for v in (x, b, y, rays, *case["residual"], *case["backprojection"]):
        v.setflags(write=False)
    return case


def _dev(a):
    return torch.tensor(a, device="cuda")


@pytest.mark.parametrize("name", list(KERNEL_CASES))
def test_residual_kernel_matches_float64(name):
    """Per pixel |r - r64| <= 1e-5 max|A64 x| + 2^-23 |b| (the forward test's bound plus the rounding of b - A x) and
    |y - y64| <= (1e-5 max|A64 x| + 3 x 2^-24 (|b| + |A64 x|)) / len (the subtraction, the division, and len itself); on a miss
    y = 0 and r = b exactly.  `projections` is left as it is and r = NULL gives the same y."""
    from neuralvolumetricreconstructionformedicalimages_amd import sart
    c = _case(name)
    r64, y64, ax64, length = c["residual"]
    hit = length > 0
    print(f"{name}: {int(hit.sum())} hits, {int((~hit).sum())} misses")
    assert hit.sum() >= 100 and (name in ALL_HIT or (~hit).sum() >= 10), "hits and misses must both be there"
    x, b = _dev(c["x"]), _dev(c["b"])
    y, r = sart.residual_scan(x, b, c["geo"], c["angles"], c["views"])
    assert y.shape == r.shape == c["y"].shape and y.dtype == r.dtype == torch.float32
    assert torch.equal(b, _dev(c["b"]))
    y_only, none = sart.residual_scan(x, b, c["geo"], c["angles"], c["views"], want_r=False)
    assert none is None and torch.equal(y_only, y)
    y, r = y.cpu().numpy().reshape(-1).astype(np.float64), r.cpu().numpy().reshape(-1).astype(np.float64)
    bs = c["b"][c["listed"]].reshape(-1).astype(np.float64)
    scale = np.abs(ax64).max()
    bound_r = BOUND * scale + 2.0 ** -23 * np.abs(bs)
    bound_y = (BOUND * scale + 3 * 2.0 ** -24 * (np.abs(bs) + np.abs(ax64)))[hit] / length[hit]
    ratio_r = (np.abs(r - r64) / bound_r).max()
    ratio_y = (np.abs(y - y64)[hit] / bound_y).max()
    print(f"{name}: worst |r - r64| / bound = {ratio_r:.3e}, worst |y - y64| / bound = {ratio_y:.3e}")
    assert (y[~hit] == 0).all() and (r[~hit] == bs[~hit]).all()
    assert ratio_r <= 1 and ratio_y <= 1


@pytest.mark.parametrize("name", list(KERNEL_CASES))
def test_paired_backprojection_matches_float64(name):
    from neuralvolumetricreconstructionformedicalimages_amd import projector, sart
    c = _case(name)
    num64, den64 = c["backprojection"]
    y = _dev(c["y"])
    den = torch.zeros(c["dims"], device="cuda")
    num = sart.backproject_scan(y, c["geo"], c["angles"], c["views"], den=den)
    assert num.shape == c["dims"] and num.dtype == torch.float32
    for what, got, want in (("num", num, num64), ("den", den, den64)):
        got = got.cpu().numpy()
        err, scale = np.abs(got - want).max(), np.abs(want).max()
        print(f"{name}: {what} max abs err / max = {err / scale:.3e}, zero voxels {(want == 0).sum()}")
        assert (got[want == 0] == 0).all()
        assert err <= BOUND * scale, (what, err, scale)
    # den = NULL: the numerator alone, which is backproject_scan of the gathered views
    alone = sart.backproject_scan(y, c["geo"], c["angles"], c["views"])
    gathered = projector.backproject_scan(y, c["geo"], c["angles"][c["listed"]])
    tol = 2 * BOUND * float(np.abs(num64).max())
    err = float((alone - gathered).abs().max())
    print(f"{name}: den = NULL vs backproject_scan of the gathered views {err / tol * 2 * BOUND:.3e} of max")
    assert err <= tol and float((alone - num).abs().max()) <= tol
    # Both outputs accumulate into non-zero starts: the slack of test_hip_backproject.test_scan_equals_rays_and_accumulates.  `out`
    # is an fp32 sum of start and a voxel's T positive terms in some order, `fresh` the T terms alone and start + fresh one more
    # rounding, so the two sides differ by at most (2 T + 2) x 2^-24 x (start + fresh) to first order; T is counted by the oracle
    # (+ 2 for a sample on a cell face that falls into the neighbouring cell in fp32).
    terms = _dev(B.backproject_rays(None, c["geo"].dVoxel, c["rays"], c["dims"], c["geo"].accuracy, count_terms=True))
    gen = torch.Generator(device="cuda").manual_seed(5)
    start_num = torch.rand(c["dims"], device="cuda", generator=gen) * num.max()
    start_den = torch.rand(c["dims"], device="cuda", generator=gen) * den.max()
    out_num, out_den = start_num.clone(), start_den.clone()
    assert sart.backproject_scan(y, c["geo"], c["angles"], c["views"], num=out_num, den=out_den) is out_num
    for what, out, start, fresh in (("num", out_num, start_num, num), ("den", out_den, start_den, den)):
        want = start + fresh
        slack = (2 * (terms + 2) + 2) * 2.0 ** -24 * want.double() * (1 + 1e-3)
        excess = ((out - want).abs().double() - slack).max()
        print(f"{name}: {what} terms per voxel up to {int(terms.max())}, accumulate error {float((out - want).abs().max()):.3e} "
              f"(max of out {float(out.max()):.3e})")
        assert float(excess) <= 0
        assert float((out - start).max()) > 0.5 * float(fresh.max())


def _update_reference(x, num, den, relax, nonneg, reciprocal):
    c = den if reciprocal else torch.where(den > 0, 1.0 / den, torch.zeros_like(den))
    out = x + relax * (c * num)
    return torch.clamp(out, 0, None) if nonneg else out


@pytest.mark.parametrize("shape", [(1,), (63,), (64,), (65,), (4099,), (8, 9, 7)])
def test_update_kernel_is_the_torch_expression(shape):
    """Same bits as x + relax * (c * num), c = where(den > 0, 1 / den, 0), clamp, evaluated by torch on the device; num comes back
    zero and den is zeroed only when asked; an unaligned base, on all three arrays or on one, changes no bit."""
    from neuralvolumetricreconstructionformedicalimages_amd import sart
    n = int(np.prod(shape))
    gen = torch.Generator(device="cuda").manual_seed(n)
    x0 = torch.rand(shape, device="cuda", generator=gen)
    num0 = torch.randn(shape, device="cuda", generator=gen) * 3
    den0 = torch.rand(shape, device="cuda", generator=gen) + 0.05
    den0.view(-1)[::3] = 0.0                                              # zeros, positives and one negative
    den0.view(-1)[n // 2] = -0.5 if n > 1 else 0.7
    relax = 0.7

    def shifted(t, by):
        buf = torch.empty(n + 1, device="cuda")
        buf[by:by + n] = t.reshape(-1)
        return buf[by:by + n].view(shape)

    for nonneg in (True, False):
        for reciprocal in (False, True):
            want = _update_reference(x0, num0, den0, relax, nonneg, reciprocal)
            if nonneg and n > 60:
                assert int((want == 0).sum()) > 0 and int((want > 0).sum()) > 0           # the clamp is at work
            for zero_den in ((False,) if reciprocal else (False, True)):
                results = []
                for offsets in ((0, 0, 0), (1, 1, 1), (1, 0, 0), (0, 0, 0)):
                    x, num, den = (shifted(t, by) for t, by in zip((x0, num0, den0), offsets))
                    assert sart.update(x, num, den, relax, nonneg, den_is_reciprocal=reciprocal, zero_den=zero_den) is x
                    assert int((num != 0).sum()) == 0
                    assert torch.equal(den, torch.zeros_like(den) if zero_den else den0)
                    results.append(x)
                wrong = int((results[0] != want).sum())
                if wrong:
                    host_c = (1.0 / den0.cpu()).cuda()
                    print(f"{shape} nonneg {nonneg} reciprocal {reciprocal}: {wrong} of {n} elements differ from torch, max "
                          f"{float((results[0] - want).abs().max()):.3e}; torch's device 1 / den differs from the host's in "
                          f"{int((host_c != 1.0 / den0).sum())} elements")
                assert all(torch.equal(r, want) for r in results)


@functools.lru_cache(maxsize=None)
def _pocs():
    """The rehearsal case on the device and its float64 OS-SART (one view per subset, order 0, 2, 1, 3, 20 iterations), once."""
    from neuralvolumetricreconstructionformedicalimages_amd.reconstruct import os_sart_operators
    A, AT, b, x_true, (geo, _), _ = S.pocs_operators()
    x64, norms64 = os_sart_operators(A, AT, b, S.SART_SUBSETS, 20)
    return geo, _dev(b.astype(np.float32)), x_true, x64, norms64


@functools.lru_cache(maxsize=None)
def _pocs_gpu():
    from neuralvolumetricreconstructionformedicalimages_amd import os_sart
    geo, b, _, _, _ = _pocs()
    return os_sart(b, geo, T.POCS_ANGLES, n_iter=20)


def test_os_sart_end_to_end_against_float64():
    from neuralvolumetricreconstructionformedicalimages_amd.reconstruct import subset_order
    geo, b, x_true, x64, norms64 = _pocs()
    assert [list(s) for s in subset_order(T.POCS_ANGLES, 4)] == S.SART_SUBSETS
    x, norms = _pocs_gpu()
    assert x.shape == T.POCS_DIMS and x.dtype == torch.float32 and float(x.min()) >= 0 and len(norms) == 20
    got = x.cpu().numpy().astype(np.float64)
    p, p64 = T.psnr_3d(got, x_true), T.psnr_3d(x64, x_true)
    rel = [abs(a - c) / c for a, c in zip(norms, norms64)]
    print(f"psnr_3d {p:.3f} dB (float64 {p64:.3f} dB); relative L2 distance to float64 {np.linalg.norm(got - x64) / np.linalg.norm(x64):.3e}; "
          f"norms {norms[0]:.6e} -> {norms[-1]:.6e}, largest relative norm difference {max(rel):.3e}, first {rel[0]:.3e}")
    assert abs(p64 - S.POCS_PSNR[20][1]) <= 0.01
    assert abs(p - p64) <= 0.1
    assert rel[0] <= 1e-5


def test_one_subset_of_all_views_against_sirt():
    from neuralvolumetricreconstructionformedicalimages_amd import os_sart, sirt
    geo, b, x_true, _, _ = _pocs()
    x, norms = os_sart(b, geo, T.POCS_ANGLES, n_iter=5, n_subsets=1)
    want, want_norms = sirt(b, geo, T.POCS_ANGLES, n_iter=5)
    p, p_sirt = T.psnr_3d(x.cpu().numpy(), x_true), T.psnr_3d(want.cpu().numpy(), x_true)
    print(f"one subset vs sirt, 5 iterations: psnr_3d {p:.4f} vs {p_sirt:.4f} dB, max abs difference "
          f"{float((x - want).abs().max()):.3e} (max of volume {float(want.max()):.3e}), norms {norms[-1]:.6e} vs {want_norms[-1]:.6e}")
    assert abs(p - p_sirt) <= 0.1


def test_without_the_weight_cache_and_two_subsets():
    from neuralvolumetricreconstructionformedicalimages_amd import os_sart, sirt
    geo, b, x_true, _, _ = _pocs()
    x, _ = _pocs_gpu()
    uncached, norms = os_sart(b, geo, T.POCS_ANGLES, n_iter=20, weight_cache_bytes=0)
    p, p_un = T.psnr_3d(x.cpu().numpy(), x_true), T.psnr_3d(uncached.cpu().numpy(), x_true)
    print(f"cached {p:.4f} dB, uncached {p_un:.4f} dB, max abs difference {float((x - uncached).abs().max()):.3e}")
    assert abs(p - p_un) <= 0.01 and len(norms) == 20
    two, _ = os_sart(b, geo, T.POCS_ANGLES, n_iter=5, n_subsets=2, order="sequential")
    one, _ = sirt(b, geo, T.POCS_ANGLES, n_iter=5)
    p_two, p_one = T.psnr_3d(two.cpu().numpy(), x_true), T.psnr_3d(one.cpu().numpy(), x_true)
    print(f"5 iterations: two sequential subsets {p_two:.3f} dB, sirt {p_one:.3f} dB")
    assert p_two > p_one


def test_refusals(monkeypatch):
    from neuralvolumetricreconstructionformedicalimages_amd import os_sart, sart
    geo, b, _, _, _ = _pocs()
    angles = T.POCS_ANGLES
    x = torch.zeros(T.POCS_DIMS, device="cuda")
    y = torch.ones(2, 24, 24, device="cuda")
    with pytest.raises(RuntimeError, match="no CPU path"):
        os_sart(b.cpu(), geo, angles, n_iter=1)
    with pytest.raises(RuntimeError, match="no CPU path"):
        sart.residual_scan(x.cpu(), b, geo, angles)
    with pytest.raises(RuntimeError, match="no CPU path"):
        sart.residual_scan(x, b.cpu(), geo, angles)
    with pytest.raises(RuntimeError, match="no CPU path"):
        sart.backproject_scan(y.cpu(), geo, angles, [0, 1])
    with pytest.raises(RuntimeError, match="no CPU path"):
        sart.update(x, x.cpu(), x.clone())
    from neuralvolumetricreconstructionformedicalimages_amd import _abi
    with monkeypatch.context() as m:                                       # refused before any launch: the library is not reached
        m.setattr(_abi, "lib", lambda: pytest.fail("the library was called"))
        for call in (lambda: sart.residual_scan(x, b, geo, angles, [0, 4]), lambda: sart.backproject_scan(y, geo, angles, [4, 0]),
                     lambda: sart.residual_scan(x, b, geo, angles, [-1])):
            with pytest.raises(ValueError, match="view index out of range"):
                call()
    with pytest.raises(ValueError, match="projections must be float32"):
        sart.residual_scan(x, b[:, :, :23].contiguous(), geo, angles)
    with pytest.raises(ValueError, match="projections must be float32"):
        sart.residual_scan(x, b.double(), geo, angles)
    with pytest.raises(ValueError, match="nVoxel"):
        sart.residual_scan(torch.zeros(16, 16, 15, device="cuda"), b, geo, angles)
    with pytest.raises(ValueError, match="y must be float32"):
        sart.residual_scan(x, b, geo, angles, [0, 1], y=torch.zeros(3, 24, 24, device="cuda"))
    with pytest.raises(ValueError, match="y must be float32"):
        sart.backproject_scan(y, geo, angles, [0, 1, 2])
    with pytest.raises(ValueError, match="contiguous"):
        sart.backproject_scan(torch.ones(2, 24, 24, device="cuda").transpose(1, 2), geo, angles, [0, 1])
    with pytest.raises(ValueError, match="den must be"):
        sart.backproject_scan(y, geo, angles, [0, 1], den=torch.zeros(16, 16, 15, device="cuda"))
    with pytest.raises(ValueError, match="two volumes"):
        sart.backproject_scan(y, geo, angles, [0, 1], num=x, den=x)
    with pytest.raises(TypeError, match="float32"):
        sart.update(x, x.clone().double(), x.clone())
    with pytest.raises(ValueError, match="shape"):
        sart.update(x, torch.zeros(16, 16, 15, device="cuda"), x.clone())
    with pytest.raises(ValueError, match="zero_den"):
        sart.update(x, x.clone(), x.clone(), den_is_reciprocal=True, zero_den=True)
    with pytest.raises(ValueError, match="n_subsets"):
        os_sart(b, geo, angles, n_iter=1, n_subsets=5)
    with pytest.raises(ValueError, match="relax"):
        os_sart(b, geo, angles, n_iter=1, relax=0.0)
    with pytest.raises(ValueError, match="nVoxel"):
        os_sart(b, geo, angles, n_iter=1, x0=torch.zeros(16, 16, 15, device="cuda"))
    x0 = torch.full(T.POCS_DIMS, 0.1, device="cuda")
    out, norms = os_sart(b, geo, angles, n_iter=1, x0=x0)
    assert torch.equal(x0, torch.full(T.POCS_DIMS, 0.1, device="cuda")) and out is not x0 and len(norms) == 1
    assert float((out - x0).abs().max()) > 0
    out, norms = os_sart(b, geo, angles, n_iter=0, x0=x0)
    assert torch.equal(out, x0) and out is not x0 and norms == []
    empty_y, empty_r = sart.residual_scan(x, b, geo, angles, [])
    assert empty_y.shape == empty_r.shape == (0, 24, 24)
    keep = torch.full(T.POCS_DIMS, 2.0, device="cuda")
    assert torch.equal(sart.backproject_scan(empty_y, geo, angles, [], num=keep), torch.full_like(keep, 2.0))
