"""The gather transpose's enumeration without a GPU (csrc/backproject_gather_device.h): the float32
restatement in tests/_backproject_gather_oracle.py -- footprint rectangle, k-range, corner membership -- must cover every
(ray, sample, voxel) to which the scatter gives a non-zero float32 weight, and therefore sums to the columns of the forward
oracle's dense matrix.  Also the refusals of the Python surface that need no kernel."""
import functools

import numpy as np
import pytest

import _backproject_gather_oracle as G
import _backproject_oracle as B

NAMES = sorted(G.geometries())


@functools.lru_cache(maxsize=None)
def _case(name):
    from neuralvolumetricreconstructionformedicalimages_amd.geometry import ConeGeometry
    data, angles = G.geometries()[name]
    geo = ConeGeometry(data)
    rays = B.case_rays(geo, angles)
    return geo, angles, rays, G.candidates(geo, angles, rays)


def test_the_geometries_are_what_they_claim():
    assert len(NAMES) == 7
    geo, _, rays, _ = _case("axis-parallel")
    assert np.abs(rays[:, 3:6]).min() < 1e-15 and geo.tilt_angle == 0          # cos(pi / 2) in float32: as parallel as a pose gets
    dims = tuple(int(v) for v in geo.nVoxel)
    for name, share in (("clipped", 1.0), ("off-detector", 0.7)):
        geo, _, rays, _ = _case(name)
        hit = B.ray_lengths(rays, dims, geo.dVoxel, geo.accuracy) > 0
        assert share - 0.4 <= hit.mean() <= share, (name, hit.mean())             # every ray of the small detector hits, half of the shifted one's
    assert any(np.asarray(_case(n)[0].offDetector).any() for n in NAMES)
    assert len(set(np.asarray(_case("anisotropic")[0].dVoxel).tolist())) == 3


@pytest.mark.parametrize("name", NAMES)
def test_candidates_cover_the_scatter(name):
    geo, angles, rays, (ok, k_lo, k_hi) = _case(name)
    dims = tuple(int(v) for v in geo.nVoxel)
    triples = G.scatter_triples(rays, dims, geo.dVoxel, geo.accuracy)
    ray, k, vox = triples.T
    assert len(triples) > 2000 and len(np.unique(vox)) > 50
    covered = ok[ray, vox] & (k >= k_lo[ray, vox]) & (k <= k_hi[ray, vox])
    assert covered.all(), triples[~covered][:10]
    # and it is an enumeration, not the whole scan: the visited pixels and samples per voxel stay small
    pixels, samples = ok.sum(0), np.where(ok, k_hi - k_lo + 1, 0).sum(0)
    print(f"{name}: {len(triples)} non-zero terms; per voxel and view {pixels.mean() / len(angles):.1f} pixels visited of "
          f"{ok.shape[0] // len(angles)}, {samples.mean() / len(angles):.1f} candidate samples, "
          f"{len(triples) / ok.shape[1] / len(angles):.1f} non-zero")
    if name not in ("clipped",):
        assert pixels.mean() < 0.5 * ok.shape[0]


@pytest.mark.parametrize("name", NAMES)
def test_gathered_column_equals_the_dense_matrix(name):
    geo, angles, rays, (ok, k_lo, k_hi) = _case(name)
    dims = tuple(int(v) for v in geo.nVoxel)
    A = B.dense_matrix(dims, geo.dVoxel, rays, geo.accuracy)
    got = G.gathered_matrix(geo, rays, ok, k_lo, k_hi)
    assert A.max() > 0
    assert np.abs(got - A).max() <= 1e-12 * A.max()
    assert (got[A == 0] == 0).all()


def test_k_range_with_a_zero_direction_component():
    """d[k] == 0 exactly, as clip_ray (ray_span) treats it: inside the slab the axis does not constrain t, outside there is no sample."""
    f32 = np.float32
    lo, hi = np.array([-1, -1, -1], dtype=f32), np.array([1, 1, 1], dtype=f32)
    d = np.array([1, 0, 0], dtype=f32)
    inside, outside = np.array([-8, 0.5, 1.0], dtype=f32), np.array([-8, 0.5, 1.0001], dtype=f32)
    ok, k_lo, k_hi = G.k_range(lo, hi, inside, d, f32(0.25), 64)
    assert ok and k_lo <= 27 and k_hi >= 35 and k_hi - k_lo <= 11              # t in [7, 9]: k + 1/2 in [28, 36]
    assert not G.k_range(lo, hi, outside, d, f32(0.25), 64)[0]
    assert not G.k_range(lo, hi, inside, d, f32(0.25), 20)[0]                 # the span ends before the box
    ok, k_lo, k_hi = G.k_range(lo, hi, np.array([-8, 0.5, 0.5], dtype=f32), np.array([1, 0, 1e-30], dtype=f32), f32(0.25), 64)
    assert ok and k_lo <= 27 and k_hi >= 35                                    # a tiny component: huge but finite bounds


def test_python_surface_refuses_without_a_kernel():
    import torch

    from neuralvolumetricreconstructionformedicalimages_amd import projector, sart
    from neuralvolumetricreconstructionformedicalimages_amd.geometry import ConeGeometry
    geo = ConeGeometry(B.case_geometry(*B.CASES[0]))
    for fn in (projector.backproject_scan, sart.backproject_scan):
        with pytest.raises(ValueError, match="method must be one of"):
            fn(torch.zeros(2, 8, 10), geo, B.CASE_ANGLES, method="x")
        with pytest.raises(RuntimeError, match="no CPU path"):
            fn(torch.zeros(2, 8, 10), geo, B.CASE_ANGLES, method="gather")
    assert projector.gather_workspace(3, 8, 10, "cpu", span_table=False) is None
    assert projector.gather_workspace(3, 8, 10, "cpu").numel() == 3 * 80 * projector.GATHER_SPAN_BYTES
    assert projector.gather_workspace(10 ** 6, 512, 512, "meta").numel() == (projector.GATHER_WORKSPACE_CAP // (40 * 512 * 512)) * 40 * 512 * 512
    assert projector.gather_workspace(1, 2048, 2048, "meta").numel() == 40 * 2048 * 2048       # one view always fits
    assert "scatter only" in projector.backproject_rays.__doc__


def test_entry_point_refusals_need_no_gpu():
    """Bad arguments are refused before any HIP call; an empty call is a no-op."""
    import ctypes

    from neuralvolumetricreconstructionformedicalimages_amd import _abi
    lib = _abi.lib()
    one = ctypes.c_void_p(16)
    dims, dv = (ctypes.c_uint32 * 3)(4, 4, 4), (ctypes.c_float * 3)(1e-3, 1e-3, 1e-3)

    def call(values=one, index=None, n_sub=2, n_scan=2, poses=one, w=8, h=8, du=1e-3, dvp=1e-3, dsd=1.5, volume=one, den=None,
             work=None, size=0, d=dims, null_det=False):
        det = None if null_det else ctypes.byref(_abi.Detector(w, h, du, dvp, 0.0, 0.0, dsd, 0.0, 2.0, 0))
        return lib.naf_backproject_scan_gather(values, index, n_sub, n_scan, d and ctypes.byref(d), ctypes.byref(dv), poses, det, 5e-4,
                                               volume, den, work, size, None)

    assert call(n_sub=0, values=None, poses=None, volume=None, d=None, null_det=True) == 0
    for kwargs, text in (({"values": None}, b"null pointer"), ({"volume": None}, b"null pointer"), ({"w": 0}, b"empty detector"),
                         ({"null_det": True}, b"backproject_scan_gather: null pointer"),
                         ({"dsd": 0.0}, b"DSD"), ({"du": 0.0}, b"pitch"), ({"dvp": float("nan")}, b"pitch"),
                         ({"n_sub": 3}, b"n_sub must be <="), ({"den": one}, b"two volumes"),
                         ({"work": ctypes.c_void_p(12), "size": 1 << 20}, b"8-byte aligned"),
                         ({"work": one, "size": 40 * 64 - 1}, b"workspace too small")):
        assert call(**kwargs) == -1, kwargs
        assert text in lib.naf_last_error(), (kwargs, lib.naf_last_error())


def test_the_tools_hand_deterministic_to_the_fdk_start(monkeypatch):
    """`--init fdk` builds x0 with the transpose the solve takes: tools/reconstruct_sirt.py's start_volume, which the ASD-POCS and
    OS-SART tools share, passes `--deterministic` on to `fdk`."""
    import argparse
    import importlib.util
    import os

    import neuralvolumetricreconstructionformedicalimages_amd as pkg
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "reconstruct_sirt.py")
    spec = importlib.util.spec_from_file_location("reconstruct_sirt_under_test", path)
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    seen = []
    monkeypatch.setattr(pkg, "fdk", lambda proj, geo, angles, **kwargs: seen.append(kwargs) or "x0")
    monkeypatch.setattr(pkg, "sirt", lambda proj, geo, angles, **kwargs: (seen.append(kwargs) or kwargs["x0"], []))
    for flag in (True, False):
        args = argparse.Namespace(init="fdk", deterministic=flag, iters=1, relax=1.0, no_nonneg=False)
        assert tool._sirt(args, None, None, None)[0] == "x0"
        assert [k["deterministic"] for k in seen[-2:]] == [flag, flag] and seen[-2]["nonneg"] is True
    assert tool.start_volume(argparse.Namespace(init="zeros", deterministic=True), None, None, None) is None
    for name in ("reconstruct_asd_pocs.py", "reconstruct_os_sart.py"):
        source = open(os.path.join(os.path.dirname(path), name)).read()
        assert "reconstruct_sirt.start_volume(args, proj, geo, angles)" in source and "deterministic=args.deterministic" in source
