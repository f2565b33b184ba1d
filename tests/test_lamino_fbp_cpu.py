"""Laminographic FBP on the CPU: the float64 rehearsal of `reconstruct.lamino_fbp_operators` on exact line
integrals of the flat phantom at two grid sizes, which decides the constant; the weights against their closed form; the refusals;
and `fdk`'s own refusal of the same scan, unchanged."""
import math

import numpy as np
import pytest

import _lamino_oracle as L


def test_rehearsal_converges_under_refinement():
    """The flat phantom (twelve ellipsoids in a 256 mm cube, z squeezed to 0.3) at tilt 30 degrees, 2 n views over a full turn on a
    detector of 1.5 n pixels a side, reconstructed in float64 at 16^3 and at its 2 x refinement in voxels, detector pixels and
    views.  scale = the least-squares factor of the volume against the phantom with its missing cone zeroed in the FFT, over the
    central block (true value 1):
        16^3: scale 0.83392 (against the plain phantom 0.54009)     32^3: scale 0.91960 (0.58157)
    |scale - 1| falls 0.16608 -> 0.08040, by 2.07; at least 1.5 is asked.  A wrong constant (2, pi / 2, a missing cos(tilt) = 0.866)
    leaves |scale - 1| where it is."""
    coarse, fine = (L.fbp_rehearsal(n) for n in L.REHEARSAL_SIZES)
    print(f"scale {coarse['scale']:.5f} -> {fine['scale']:.5f}; against the plain phantom {coarse['scale_plain']:.5f} -> "
          f"{fine['scale_plain']:.5f}")
    assert coarse["x"].shape == (16, 16, 16) and fine["x"].shape == (32, 32, 32)
    assert abs(fine["scale"] - 1) * 1.5 <= abs(coarse["scale"] - 1)
    assert abs(fine["scale"] - 1) < abs(fine["scale_plain"] - 1)          # the missing cone is what the rest of the deficit is


def tilted(**changes):
    from neuralvolumetricreconstructionformedicalimages_amd.geometry import ConeGeometry
    data = L.lamino_geometry(16)
    data["nDetector"], data["dDetector"], data["offDetector"] = [6, 4], [3.0, 5.0], [1.0, -2.0]
    data.update(changes)
    return ConeGeometry(data)


def test_weights_are_the_closed_form():
    from neuralvolumetricreconstructionformedicalimages_amd.filter import ramp_taps
    from neuralvolumetricreconstructionformedicalimages_amd.reconstruct import lamino_fbp_weights
    angles = L.full_turn(8)
    taps, pre, post, scale = lamino_fbp_weights(tilted(), angles)
    assert pre is None and post is None and taps.dtype == np.float32 and scale.dtype == np.float32 and scale.shape == (8,)
    assert np.array_equal(taps, ramp_taps(6, 0.003))                       # tap spacing du, no magnification
    want = np.float32((np.pi / 8) * math.cos(math.radians(30.0)) * (0.003 * 0.005) / 0.016 ** 3)
    assert np.abs(scale - want).max() <= np.spacing(want)                  # formed in float64, rounded once
    assert np.array_equal(lamino_fbp_weights(tilted(), angles, "shepp-logan")[0], ramp_taps(6, 0.003, "shepp-logan"))
    # unequal steps: w_i = pi gap_i / sum gap, in the order of the angles
    uneven = np.array([0.0, 1.0, 2.5, 4.0, 5.5])                           # steps 1, 1.25, 1.5, 1.5, 1.5: 6.75 rad covered
    w = lamino_fbp_weights(tilted(tilt_angle=61), uneven)[3].astype(np.float64)
    const = math.cos(math.radians(61.0)) * (0.003 * 0.005) / 0.016 ** 3
    assert np.allclose(w, np.pi * np.array([1, 1.25, 1.5, 1.5, 1.5]) / 6.75 * const, rtol=1e-6)


def test_refusals_name_the_case():
    from neuralvolumetricreconstructionformedicalimages_amd.reconstruct import lamino_fbp_operators, lamino_fbp_weights
    full = L.full_turn(8)
    with pytest.raises(ValueError, match="cone-beam laminography is not supported"):
        lamino_fbp_weights(tilted(mode="cone"), full)
    with pytest.raises(ValueError, match="tilt_angle is 0.*use fdk"):
        lamino_fbp_weights(tilted(tilt_angle=0), full)
    for tilt in (90, -30, 120):
        with pytest.raises(ValueError, match="strictly between 0 and 90"):
            lamino_fbp_weights(tilted(tilt_angle=tilt), full)
    with pytest.raises(ValueError, match=r"8 views cover 180\.0 degrees \(largest gap 202\.5 degrees, .*\), less than a full turn"):
        lamino_fbp_weights(tilted(), np.linspace(0, np.pi, 9)[:-1])
    with pytest.raises(ValueError, match="less than a full turn"):
        lamino_fbp_weights(tilted(), np.linspace(0, 1.7 * np.pi, 9)[:-1])
    with pytest.raises(ValueError, match="at least two views"):
        lamino_fbp_weights(tilted(), [0.3])
    with pytest.raises(ValueError, match="at least two views"):
        lamino_fbp_weights(tilted(), [])
    for bad in (np.nan, np.inf):
        with pytest.raises(ValueError, match="must be finite"):
            lamino_fbp_weights(tilted(), [0.0, bad, 3.0])
    with pytest.raises(ValueError, match="filter"):
        lamino_fbp_weights(tilted(), full, "hann")
    with pytest.raises(ValueError, match="one view per angle"):
        lamino_fbp_operators(lambda y: y, lambda *a: a[0], np.zeros((7, 4, 6)), tilted(), full)
    assert lamino_fbp_operators(lambda y: y - 1.0, lambda b, *w: b, np.zeros((8, 4, 6)), tilted(), full, nonneg=True).max() == 0.0


def test_fdk_still_refuses_the_tilted_scan():
    from neuralvolumetricreconstructionformedicalimages_amd import pretrain
    from neuralvolumetricreconstructionformedicalimages_amd.reconstruct import fdk_operators, fdk_weights
    full = L.full_turn(8)
    with pytest.raises(ValueError, match="tilted .laminographic. scan is not supported.*its constant and filter direction are not verified"):
        fdk_weights(tilted(), full)
    with pytest.raises(ValueError, match="tilted"):
        fdk_operators(lambda y: y, lambda *a: a[0], np.zeros((8, 4, 6)), tilted(), full)
    with pytest.raises(ValueError, match="fdk refuses a tilted"):
        pretrain.check_init_geometry(pretrain.init_volume_config({"init_volume": "fdk"}), tilted())
    init = pretrain.init_volume_config({"init_volume": "lamino-fbp", "init_steps": 3})
    assert init == {"source": "lamino-fbp", "steps": 3, "points": pretrain.DEFAULT_POINTS}
    pretrain.check_init_geometry(init, tilted())
    with pytest.raises(ValueError, match="'lamino-fbp' needs a scan that reconstruct.lamino_fbp accepts"):
        pretrain.check_init_geometry(init, tilted(tilt_angle=0))
    with pytest.raises(ValueError, match="'lamino-fbp' needs"):
        pretrain.check_init_geometry(init, tilted(mode="cone"))


def test_window_depth_is_reported():
    """`get_near_far` ignores the tilt: at DSO = 1000 mm the far plane lies 31 mm behind the rotation centre along the rays, at the
    400 mm the tests scan with 124 mm, which holds the flat phantom (at most 0.866 * 109 + 0.5 * 35 = 112 mm deep) but not the
    corners of the 256 mm cube (221 mm)."""
    from neuralvolumetricreconstructionformedicalimages_amd import phantom
    from neuralvolumetricreconstructionformedicalimages_amd.geometry import ConeGeometry
    from neuralvolumetricreconstructionformedicalimages_amd.reconstruct import lamino_window
    kept, reach = lamino_window(ConeGeometry(phantom.scan_geometry(32, "parallel", 30)))
    far = 1.0 + math.hypot(0.128, 0.128) + 0.005
    assert abs(kept - (far - 1.0 / math.cos(math.radians(30)))) < 1e-12 and abs(kept - 0.0313) < 1e-4
    assert abs(reach - (math.cos(math.radians(30)) * math.hypot(0.128, 0.128) + 0.5 * 0.128)) < 1e-12
    kept, same = lamino_window(ConeGeometry(L.lamino_geometry(32)))
    assert same == reach and 0.112 < kept < reach and abs(kept - 0.1241) < 1e-4
