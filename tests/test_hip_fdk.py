"""`reconstruct.fdk` on the GPU against its float64 rehearsal (tests/_filter_oracle.py `fdk_rehearsal`: the same `fdk_operators`
over the float64 convolution and the float64 back-projector), at the rehearsal's coarse size; DESIGN.md section 15.

Error bound per voxel.  The GPU volume is A^T_gpu(y_gpu), the rehearsal's A^T(y).  tests/test_hip_backproject.py holds the kernel
to 1e-5 max|A^T y| of the float64 scatter for y >= 0; by linearity on y = y+ - y- that is 2e-5 max A^T|y| here, where the filtered
projections change sign.  y_gpu differs from y by at most `filter_bound` per element, and A^T has no negative entry, so that
difference reaches a voxel as at most A^T(filter_bound).  The asserted bound is the sum of the two."""
import numpy as np
import pytest
import torch

import _filter_oracle as F

pytestmark = pytest.mark.gpu

N = F.REHEARSAL_SIZES[0]


@pytest.fixture(scope="module", params=["cone", "parallel"])
def case(request):
    from neuralvolumetricreconstructionformedicalimages_amd import fdk
    r = F.fdk_rehearsal(N, request.param)
    b = torch.tensor(r["b"], device="cuda")
    x = fdk(b, r["geo"], r["angles"])
    return request.param, r, b, x


def test_volume_matches_the_rehearsal(case):
    mode, r, b, x = case
    assert x.dtype == torch.float32 and tuple(x.shape) == (N, N, N) and x.device == b.device
    got = x.cpu().numpy().astype(np.float64)
    e_filter = F.filter_bound(r["b"], *r["weights"])
    bound = 2e-5 * float(r["AT"](np.abs(r["y"])).max()) + r["AT"](e_filter)
    err = np.abs(got - r["x"])
    print(f"{mode} {N}^3: max |x - float64| {err.max():.3e} of max |x| {np.abs(r['x']).max():.3f}; bound {bound.min():.3e} .. "
          f"{bound.max():.3e}, worst ratio {(err / bound).max():.4f}")
    assert np.all(err <= bound)


def test_psnr_parity_and_rho(case):
    from neuralvolumetricreconstructionformedicalimages_amd.utils import get_psnr_3d
    mode, r, _, x = case
    got = x.cpu().numpy()
    psnr = float(get_psnr_3d(got, r["truth"]))
    rho = float(got[F.ball_interior(r["geo"])].astype(np.float64).mean())
    print(f"{mode} {N}^3: psnr_3d {psnr:.4f} dB (float64 {r['psnr']:.4f}), rho {rho:.6f} (float64 {r['rho']:.6f})")
    assert abs(psnr - r["psnr"]) <= 0.1


def test_fdk_start_lowers_sirt_first_residual(case):
    from neuralvolumetricreconstructionformedicalimages_amd import sirt
    mode, r, b, x = case
    _, cold = sirt(b, r["geo"], r["angles"], n_iter=1)
    _, warm = sirt(b, r["geo"], r["angles"], n_iter=1, x0=x.clamp(min=0))
    print(f"{mode} {N}^3: SIRT residual_norms[0] from zeros {cold[0]:.5e}, from the clamped FDK volume {warm[0]:.5e}")
    assert warm[0] < cold[0]


def test_options_and_refusals():
    from neuralvolumetricreconstructionformedicalimages_amd import fdk
    from neuralvolumetricreconstructionformedicalimages_amd.geometry import ConeGeometry
    r = F.fdk_rehearsal(N, "cone")
    b = torch.tensor(r["b"], device="cuda")
    before = b.clone()
    x = fdk(b, r["geo"], r["angles"])
    assert torch.equal(b, before)                                      # the projections are not filtered in place
    clamped = fdk(b, r["geo"], r["angles"], nonneg=True)
    assert float(x.min()) < 0 and float(clamped.min()) == 0.0
    # the clamp is the only difference, up to the summation order of the transpose's atomics: the filter returns the same bits every
    # call, and each run of the transpose is within 2e-5 max A^T|y| of the exact A^T of them
    twice = 2 * 2e-5 * float(r["AT"](np.abs(r["y"])).max())
    assert float((clamped - x.clamp(min=0)).abs().max()) <= twice
    grouped = fdk(b, r["geo"], r["angles"], views_per_call=5)
    assert float((grouped - x).abs().max()) <= twice
    soft = fdk(b, r["geo"], r["angles"], filter="shepp-logan")
    want = F.fdk_rehearsal(N, "cone", "shepp-logan")
    bound = 2e-5 * float(want["AT"](np.abs(want["y"])).max()) + want["AT"](F.filter_bound(want["b"], *want["weights"]))
    assert np.all(np.abs(soft.cpu().numpy().astype(np.float64) - want["x"]) <= bound)
    with pytest.raises(ValueError, match="filter"):
        fdk(b, r["geo"], r["angles"], filter="hann")
    data = F.fdk_geometry(N, "parallel")
    data["tilt_angle"] = 30
    with pytest.raises(ValueError, match="tilted"):
        fdk(b, ConeGeometry(data), r["angles"])
    with pytest.raises(ValueError, match="one view per angle"):
        fdk(b[:-1], r["geo"], r["angles"])
    with pytest.raises(RuntimeError, match="no CPU path"):
        fdk(b.cpu(), r["geo"], r["angles"])
