"""The tilted-axis centre search without a GPU: the sign convention against the ray generator's phantom, the
float64 rehearsal's recoveries, why negativity is not offered, the helpers, and the stand-alone host check of
csrc/center_tilted_device.h."""
import tempfile

import numpy as np
import pytest

import _host_check
import _lamino_oracle as L

N, VIEWS = 32, 64


def test_sign_of_both_detector_axes_is_the_ray_generators():
    """The slice z = 0 at c = 0 of an unshifted tilted scan (made by `_rays_cpu`) is the phantom's central slice, not a mirror image
    or the transpose: a flipped column axis mirrors it, a flipped row axis or ray direction mixes in the wrong heights."""
    from neuralvolumetricreconstructionformedicalimages_amd import center
    from neuralvolumetricreconstructionformedicalimages_amd.reconstruct import lamino_fbp_weights
    import _center_oracle as C
    b, geo, angles, data = L.planted_scan(N, VIEWS)
    g = center.tilted_scalars(geo)
    taps, _, _, scale = lamino_fbp_weights(geo, angles)
    q = C.filter_rows(b, taps, None, None, scale)
    f = L.slices_tilted(q.astype(np.float32), center.trig(angles), center.tilted_candidates([0.0], [g["tilt"]]), [0.0], g)[0, 0]
    truth = np.asarray(data["image"], dtype=np.float64)[:, :, N // 2 - 1:N // 2 + 1].mean(-1)

    def corr(a, c):
        return float(np.corrcoef(a.ravel(), c.ravel())[0, 1])
    straight = corr(f, truth)
    print(f"correlation with the central slice {straight:.3f}; mirrors and transpose "
          f"{[round(corr(f, m), 3) for m in (truth[::-1], truth[:, ::-1], truth.T)]}")
    assert straight > 0.8
    for mirror in (truth[::-1], truth[:, ::-1], truth.T):
        assert straight > corr(f, mirror) + 0.05


@pytest.mark.parametrize("planted", [1.5, -2.5])
def test_planted_centre_is_recovered_by_the_maximum_of_sharpness(planted):
    """tilt 30 degrees, 64 views over a full turn, 32^3, candidates +-4 px in steps of 0.5: within one step is asked; the float64
    rehearsal finds the planted value itself (DESIGN.md section 35 tabulates the curves)."""
    from neuralvolumetricreconstructionformedicalimages_amd import center
    b, geo, angles, _ = L.planted_scan(N, VIEWS, planted)
    cand = center.candidates(4, 0.5)
    scores = L.search(b, geo, angles, cand, max_shift=4)
    best = float(cand[np.argmax(scores)])
    print(f"planted {planted:+.1f}: best {best:+.1f}; curve / max: {' '.join(f'{v:.3f}' for v in scores / scores.max())}")
    assert abs(best - planted) <= 0.5


def test_negativity_is_largest_near_the_true_centre_and_is_refused():
    """Why the rule of CT is not offered: the missing cone makes the focused slice negative beside every edge."""
    import torch
    import _center_oracle as C
    from neuralvolumetricreconstructionformedicalimages_amd import center, reconstruct as R
    b, geo, angles, _ = L.planted_scan(N, VIEWS, 1.5)
    g = center.tilted_scalars(geo)
    cand = center.candidates(4, 0.5)
    radius = center.tilted_mask_radius(geo, 4)
    kept = {}

    def metrics(f):
        kept["m"] = C.metrics(f, g["dx"], g["dy"], radius)
        return kept["m"]

    def slices(q, offsets, tilts):
        table = center.tilted_candidates(np.asarray(offsets) / g["du"], np.full(len(offsets), g["tilt"]))
        return L.slices_tilted(q.astype(np.float32), center.trig(angles), table, [0.0], g)

    R.find_center_tilted_operators(C.filter_rows, slices, metrics, b, geo, angles, cand)
    negativity = kept["m"][0, :, 0]
    assert abs(float(cand[np.argmax(negativity)]) - 1.5) <= 0.5 and abs(float(cand[np.argmin(negativity)]) - 1.5) > 1.0
    with pytest.raises(ValueError, match="negativity is largest at the true value"):
        R.find_center_tilted(torch.zeros(1), geo, angles, metric="negativity")
    with pytest.raises(ValueError, match="metric must be 'sharpness' or None"):
        R.find_center_tilted(torch.zeros(1), geo, angles, metric="entropy")


def test_refusals_and_the_untilted_search_keeps_its_own():
    from neuralvolumetricreconstructionformedicalimages_amd import center, phantom, reconstruct as R
    from neuralvolumetricreconstructionformedicalimages_amd.geometry import ConeGeometry
    b, geo, angles, _ = L.planted_scan(N, VIEWS)
    cand = center.candidates(4, 0.5)

    def search(geo, angles=angles, b=b):
        return R.find_center_tilted_operators(None, None, None, b, geo, angles, cand)
    with pytest.raises(ValueError, match="cone-beam laminography"):
        search(ConeGeometry(dict(L.lamino_geometry(N), mode="cone")))
    with pytest.raises(ValueError, match="tilt_angle is 0"):
        search(ConeGeometry(phantom.scan_geometry(N, "parallel")))
    with pytest.raises(ValueError, match="less than a full turn"):
        search(geo, angles=angles / 2)
    with pytest.raises(ValueError, match="one view per angle"):
        search(geo, b=b[:-1])
    with pytest.raises(ValueError, match="candidates are needed"):
        R.find_center_tilted_operators(None, None, None, b, geo, angles, np.zeros(65))
    with pytest.raises(ValueError, match="must be 'parallel'"):
        center.tilted_scalars(ConeGeometry(dict(L.lamino_geometry(N), mode="cone")))
    with pytest.raises(ValueError, match="an untilted scan is searched by find_center"):
        center.tilted_scalars(ConeGeometry(phantom.scan_geometry(N, "parallel")))
    with pytest.raises(ValueError, match="slice must be square"):
        center.tilted_scalars(ConeGeometry(dict(L.lamino_geometry(N), nVoxel=[N, N + 1, N])))
    # the untilted entry points refuse the tilted scan as before
    with pytest.raises(ValueError, match=r"center: a tilted \(laminographic\) scan is not supported"):
        center.scalars(geo)
    with pytest.raises(ValueError, match="tilted"):
        center.mask_radius(geo, 4)
    with pytest.raises(ValueError, match="tilted"):
        R.find_center_operators(None, None, None, b, geo, angles, cand, "sharpness", None)


def test_mask_radius_keeps_every_candidate_on_the_detector():
    from neuralvolumetricreconstructionformedicalimages_amd import center
    from neuralvolumetricreconstructionformedicalimages_amd.geometry import ConeGeometry
    data = L.lamino_geometry(N)
    data["nDetector"] = [40, 12]                                    # narrower and much lower than the slice's shadow
    data["offDetector"] = [1.0, -2.0]
    geo = ConeGeometry(data)
    g = center.tilted_scalars(geo)
    tilts, z = [26.0, 34.0], [0.0, 4e-3]
    r = center.tilted_mask_radius(geo, 3, tilts, z)
    assert 0 < r < 0.5 * (N - 1) * g["dx"]
    phi = np.linspace(0, 2 * np.pi, 721)
    s, t = r * np.cos(phi), r * np.sin(phi)
    for c in (-3, 3):
        k = (t - g["ou"] - c * g["du"]) / g["du"] - 0.5 + g["W"] / 2
        assert k.min() >= -1e-9 and k.max() <= g["W"] - 1 + 1e-9
    tight = 0.0
    for tilt in tilts:
        for height in (-4e-3, 0.0, 4e-3):
            v = np.sin(np.radians(tilt)) * s - np.cos(np.radians(tilt)) * height
            row = (v - g["ov"]) / g["dv"] - 0.5 + g["H"] / 2
            assert row.min() >= -1e-9 and row.max() <= g["H"] - 1 + 1e-9
            tight = max(tight, float(np.abs(row - (g["H"] - 1) / 2).max()))
    assert tight > (g["H"] - 1) / 2 - 1e-6                            # the rows are what limits it, and it is the largest such radius
    assert center.tilted_mask_radius(geo, 3, [30.0]) > r and center.tilted_mask_radius(geo, 3) == center.tilted_mask_radius(geo, 3, [30.0])
    wide = center.tilted_mask_radius(ConeGeometry(L.lamino_geometry(N)), 4)
    assert wide == 0.5 * (N - 1) * g["dx"]                            # the inscribed circle caps it on the full detector
    with pytest.raises(ValueError, match="no pixel of the slice stays on the detector"):
        center.tilted_mask_radius(geo, 30)
    with pytest.raises(ValueError, match="no pixel of the slice stays on the detector"):
        center.tilted_mask_radius(geo, 3, z=[0.2])
    with pytest.raises(ValueError, match="strictly between 0 and 90"):
        center.tilted_mask_radius(geo, 3, [0.0])


def test_float32_restatement_error_is_the_recorded_one():
    worst = L.measure_f32_error()
    assert 0.5 * L.F32_ERROR < worst <= L.F32_ERROR


def test_leaves_case_exercises_the_zero_branch_and_tilts_are_distinct():
    from neuralvolumetricreconstructionformedicalimages_amd import center
    case = next(c for c in L.CASES if c[0] == "leaves")
    geo, angles, cand, tilts, z, q = L.case_inputs(case)
    g = center.tilted_scalars(geo)
    ones = L.slices_tilted(np.ones_like(q), center.trig(angles), center.tilted_candidates(cand / g["du"], tilts), z, g)
    count = ones / np.cos(np.radians(tilts))[None, :, None, None]     # the number of views that reach a pixel
    assert count.min() < 0.5 * len(angles) and abs(count.max() - len(angles)) < 1e-5          # the table's cosine is float32
    assert len(set(np.round(tilts, 6))) == len(tilts)


def test_planting_a_tilt_error_keeps_the_nominal_scan():
    from neuralvolumetricreconstructionformedicalimages_amd import dataset
    nominal = L.lamino_geometry(16)
    plain = dataset.synthetic_scan(geometry=nominal, n_train=3, n_val=1)
    zero = dataset.plant_tilt_error(nominal, 0.0, n_train=3, n_val=1)
    assert np.array_equal(plain["train"]["projections"], zero["train"]["projections"]) and zero["tilt_angle"] == 30.0
    moved = dataset.plant_tilt_error(nominal, 1.0, n_train=3, n_val=1)
    assert moved["tilt_angle"] == 30.0 and moved["tilt_planted"] == {"error_deg": 1.0, "tilt_angle": 31.0}
    assert not np.array_equal(plain["train"]["projections"], moved["train"]["projections"])
    assert np.array_equal(plain["image"], moved["image"])
    with pytest.raises(ValueError, match="no tilt_angle"):
        dataset.plant_tilt_error(dict(nominal, tilt_angle=0), 1.0, n_train=3, n_val=1)


@_host_check.needs_compiler
def test_host_check_runs_clean():
    drv = _host_check.load("center_tilted")
    with tempfile.TemporaryDirectory() as workdir:
        exe = drv.build(workdir)
        assert drv.check_slices(L, exe, workdir) > 0
