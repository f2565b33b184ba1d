"""The tilted-axis (laminographic) kernels and wiring on the GPU (include/naf_hip.h A5) against the float64
restatements of tests/_lamino_oracle.py: `center.slices_tilted` at every tile, candidate-group, tilt and detector edge,
`reconstruct.lamino_fbp` against its float64 rehearsal, `reconstruct.find_center_tilted` end to end on a phantom with a planted
offset, and the `lamino-fbp` warm start."""
import numpy as np
import pytest
import torch

import _backproject_oracle as B
import _filter_oracle as F
import _lamino_oracle as L

pytestmark = pytest.mark.gpu
_REF = {}


def reference(case):
    if case[0] not in _REF:
        _REF[case[0]] = L.case_reference(case)
    return _REF[case[0]]


def run_slices(case, **kw):
    from neuralvolumetricreconstructionformedicalimages_amd import center
    geo, angles, cand, tilts, z, q = L.case_inputs(case)
    return center.slices_tilted(torch.tensor(q, device="cuda"), geo, angles, cand, tilts, z, **kw)


@pytest.mark.parametrize("case", L.CASES, ids=[c[0] for c in L.CASES])
def test_slices_match_the_float64_oracle_and_repeat(case):
    """Tolerance: four times the float32 restatement's own largest error against float64 over these cases, relative to max |f|
    (L.F32_ERROR, measured on the CPU): the kernel may order the per-view arithmetic differently from numpy, nothing else."""
    want = reference(case)
    first = run_slices(case)
    got = first.cpu().numpy().astype(np.float64)
    assert got.shape == want.shape
    err = float(np.abs(got - want).max() / np.abs(want).max())
    print(f"{case[0]}: relative error {err:.3e} (bound {4 * L.F32_ERROR:.3e})")
    assert err <= 4 * L.F32_ERROR
    out = torch.full_like(first, float("nan"))
    again = run_slices(case, out=out)
    assert again is out and torch.equal(first.view(torch.int32), again.view(torch.int32))


def test_default_tilt_is_the_scans_own():
    from neuralvolumetricreconstructionformedicalimages_amd import center
    case = next(c for c in L.CASES if c[0] == "n17-K1")
    geo, angles, cand, tilts, z, q = L.case_inputs(case)
    qd = torch.tensor(q, device="cuda")
    assert tilts.tolist() == [float(geo.tilt_angle)]
    assert torch.equal(center.slices_tilted(qd, geo, angles, cand, None, z), center.slices_tilted(qd, geo, angles, cand, tilts, z))


@pytest.fixture(scope="module")
def small():
    """8 views of 20 rows x 24 columns over a full turn at tilt 30 degrees into 16^3: exact line integrals of the flat phantom, and
    `lamino_fbp_operators` over the float64 convolution and the float64 scatter."""
    from neuralvolumetricreconstructionformedicalimages_amd import phantom
    from neuralvolumetricreconstructionformedicalimages_amd.geometry import ConeGeometry
    from neuralvolumetricreconstructionformedicalimages_amd.reconstruct import lamino_fbp_operators
    data = L.lamino_geometry(16)
    data["nDetector"], data["dDetector"] = [24, 20], [307.2 / 24, 307.2 / 20]
    geo = ConeGeometry(data)
    angles = L.full_turn(8)
    rays = np.asarray(B.case_rays(geo, angles), dtype=np.float32)
    b = phantom.line_integrals(torch.tensor(rays), L.flat_table()).numpy().reshape(8, 20, 24)
    kept = {}

    def rows(p, taps, pre, post, view_scale):
        kept["weights"] = (taps, pre, post, view_scale)
        kept["y"] = F.filter_rows(p, taps, pre, post, view_scale)
        return kept["y"]

    def AT(y):
        return B.backproject_rays(np.asarray(y).reshape(-1), geo.dVoxel, rays, (16, 16, 16), geo.accuracy)

    x = lamino_fbp_operators(AT, rows, b.astype(np.float64), geo, angles)
    return {"geo": geo, "angles": angles, "b": b, "x": x, "y": kept["y"], "weights": kept["weights"], "AT": AT}


def test_lamino_fbp_matches_the_rehearsal(small):
    """The bound of tests/test_hip_fdk.py: 2e-5 max A^T|y| for the transpose on signed data, plus A^T of the row filter's bound."""
    from neuralvolumetricreconstructionformedicalimages_amd.reconstruct import lamino_fbp
    r = small
    b = torch.tensor(r["b"], device="cuda")
    before = b.clone()
    with pytest.warns(UserWarning, match=r"window keeps 124\.1 mm .* the volume reaches 220\.8 mm"):     # the cube's corners, not the phantom
        x = lamino_fbp(b, r["geo"], r["angles"])
    assert x.dtype == torch.float32 and tuple(x.shape) == (16, 16, 16) and x.device == b.device and torch.equal(b, before)
    bound = 2e-5 * float(r["AT"](np.abs(r["y"])).max()) + r["AT"](F.filter_bound(r["b"], *r["weights"]))
    err = np.abs(x.cpu().numpy().astype(np.float64) - r["x"])
    print(f"max |x - float64| {err.max():.3e} of max |x| {np.abs(r['x']).max():.3f}; bound {bound.min():.3e} .. {bound.max():.3e}, "
          f"worst ratio {(err / bound).max():.4f}")
    assert np.all(err <= bound)
    # the atomic-free transpose accepts the tilted beam: the same volume within the same bound, and the same bits twice
    d1, d2 = (lamino_fbp(b, r["geo"], r["angles"], deterministic=True) for _ in range(2))
    assert torch.equal(d1.view(torch.int32), d2.view(torch.int32))
    assert np.all(np.abs(d1.cpu().numpy().astype(np.float64) - r["x"]) <= bound)
    clamped = lamino_fbp(b, r["geo"], r["angles"], nonneg=True)
    assert float(x.min()) < 0 and float(clamped.min()) == 0.0
    with pytest.raises(ValueError, match="less than a full turn"):
        lamino_fbp(b, r["geo"], r["angles"] / 2)


@pytest.fixture(scope="module")
def planted():
    b, geo, angles, data = L.planted_scan(32, 64, 1.5)
    return torch.tensor(b, device="cuda"), geo, angles, data


def test_find_center_tilted_recovers_the_planted_offset(planted):
    from neuralvolumetricreconstructionformedicalimages_amd import center, reconstruct as R
    b, geo, angles, _ = planted
    found = R.find_center_tilted(b, geo, angles, max_shift=4, step=0.5, refine=False)
    print(f"found {found['best_px']:+.2f} px; curve / max: {' '.join(f'{v:.3f}' for v in found['scores'] / found['scores'].max())}")
    assert found["metric"] == "sharpness" and not found["edge"]
    assert abs(found["offset_px"] - 1.5) <= 0.5 and found["offset"] == found["offset_px"] * float(geo.dDetector[0])
    # the float64 rehearsal of the same search draws the same curve
    cand = center.candidates(4, 0.5)
    scores = L.search(b.cpu().numpy(), geo, angles, cand, max_shift=4)
    assert np.array_equal(cand, found["candidates"]) and np.allclose(found["scores"], scores, rtol=1e-3)


def test_lamino_fbp_is_better_after_recenter(planted):
    from neuralvolumetricreconstructionformedicalimages_amd import reconstruct as R, utils
    from neuralvolumetricreconstructionformedicalimages_amd.geometry import ConeGeometry
    b, geo, angles, data = planted
    found = R.find_center_tilted(b, geo, angles, max_shift=4, step=0.5)
    truth = torch.tensor(data["image"], device="cuda")
    before = float(utils.get_psnr_3d(R.lamino_fbp(b, geo, angles), truth))
    after = float(utils.get_psnr_3d(R.lamino_fbp(b, ConeGeometry(R.recenter(data, found["offset"])), angles), truth))
    print(f"lamino_fbp psnr_3d {before:.2f} dB before, {after:.2f} dB after recenter ({found['offset_px']:+.2f} px)")
    assert after > before


def test_lamino_fbp_warm_start_fits_a_field():
    from neuralvolumetricreconstructionformedicalimages_amd import pretrain
    from neuralvolumetricreconstructionformedicalimages_amd.encoder import HashEncoder
    from neuralvolumetricreconstructionformedicalimages_amd.network import DensityNetwork
    b, geo, angles, _ = L.planted_scan(16, 16)
    init = pretrain.init_volume_config({"init_volume": "lamino-fbp", "init_steps": 5, "init_points": 1 << 10})
    pretrain.check_init_geometry(init, geo)
    volume = pretrain.init_volume_tensor(init, geo, torch.tensor(b, device="cuda"), angles, "cuda")
    assert tuple(volume.shape) == (16, 16, 16) and float(volume.min()) == 0.0 and float(volume.max()) > 0.0
    torch.manual_seed(0)
    net = DensityNetwork(HashEncoder(3, 4, 2, 16, 12), bound=0.3, num_layers=4, hidden_dim=32, skips=[2], out_dim=1,
                         last_activation="sigmoid").cuda()
    losses = pretrain.fit_volume(net, volume, geo, init["steps"], n_points=init["points"])
    assert losses.shape == (5,) and bool(torch.isfinite(losses).all())
