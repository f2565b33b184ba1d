#!/usr/bin/env python3
"""Host check of the volume sampler's per-point arithmetic: compiles tools/volume_sample_host_check.cpp (sample_point, sample_cell
and sample_draw of csrc/volume_sample_device.h over heap volumes of exactly n1 n2 n3 floats; the kernels' launch geometry and their
12-byte point accesses are not part of it) for the CPU with AddressSanitizer and UBSan and runs it as a process of its own on random
and adversarial points: every voxel centre, the box's faces and corners, points far outside, +-inf and NaN, on the shapes of the GPU
tests and on 1 x 1 x 1.  It asserts that
  - the sanitizers report nothing,
  - inside the program, against its own float64 evaluation: NaN exactly where a coordinate is NaN, everything else within the bound
    of tests/_volume_sample_oracle.py; and the cells of grids of more than 2^32 voxels have the offsets 64-bit integers give,
  - here, against the numpy oracle: the same bound, voxel centres bit-equal to the voxels where the voxel size is a power of two,
    drawn points bit-equal to the oracle's hash and inside [lo, hi], drawn targets bit-equal to the sample at those points.
The program is never loaded into Python.  No GPU.

    python tools/volume_sample_host_check.py
"""
import functools
import os
import sys
import tempfile

import numpy as np

sys.path.append(os.path.dirname(os.path.abspath(__file__)))          # tools/, for a caller that loads this file by its path
import host_check  # noqa: E402

SHAPES = ((5, 6, 7), (1, 4, 4), (4, 1, 1), (2, 2, 2), (1, 1, 1))

compiler = host_check.compiler                                       # such a caller asks the driver, not host_check
build = functools.partial(host_check.build, "volume_sample")


def _grid_args(volume, dvoxel):
    return [*volume.shape, *[repr(float(np.float32(v))) for v in dvoxel]]


def sample(exe, workdir, volume, dvoxel, points):
    """sample_point at `points` [n, 3] -> (float32 [n], the program's largest error in units of 2^-24 max n max|f|, its NaN count)."""
    (out,), stdout = host_check.run(exe, ["sample", *_grid_args(volume, dvoxel), len(points)], [volume, points],
                                    [(np.float32, len(points))])
    words = stdout.split()
    assert words[0::2] == ["worst", "nan"], words
    return out, float(words[1]), int(words[3])


def draw(exe, workdir, volume, dvoxel, lo, hi, seed, step, n):
    """sample_draw + sample_point for n points -> (points float32 [n, 3], targets float32 [n]); no coordinate may leave [lo, hi]."""
    box = [repr(float(np.float32(v))) for v in (*lo, *hi)]
    (points, targets), stdout = host_check.run(exe, ["draw", *_grid_args(volume, dvoxel), n, int(seed), int(step), *box], [volume],
                                               [(np.float32, 3 * n), (np.float32, n)])
    assert stdout.split() == ["outside", "0"], stdout
    return points.reshape(n, 3), targets


def check_offsets(exe):
    assert host_check.run(exe, ["offsets"])[1].split() == ["offsets", "0"]


def check_shape(O, exe, workdir, dims, dvoxel, exact_centres):
    """One shape: random points in 1.5 times the box, the centres, the faces and corners, non-finite points -> the largest
    |fp32 - float64| / bound."""
    volume = O.make_volume(dims)
    bad, is_nan = O.non_finite_points(dims, dvoxel)
    cen = O.centres(dims, dvoxel)
    pts = np.concatenate([O.random_points(dims, dvoxel), cen, O.faces_and_corners(dims, dvoxel), bad])
    got, worst, nans = sample(exe, workdir, volume, dvoxel, pts)
    want = O.sample(volume, dvoxel, pts)
    assert nans == int(is_nan.sum()) and np.array_equal(np.isnan(got), np.isnan(want))
    assert worst <= O.C_BOUND, (dims, worst)
    ok = ~np.isnan(want)
    ratio = float(np.abs(got[ok].astype(np.float64) - want[ok]).max() / O.bound(volume))
    assert ratio <= 1.0, (dims, ratio)
    at_centres = got[4096:4096 + len(cen)]
    if exact_centres:
        assert np.array_equal(at_centres.view(np.uint32), volume.reshape(-1).view(np.uint32)), dims
    lo, hi = -O.half_extent(dims, dvoxel) * np.float32(0.8), O.half_extent(dims, dvoxel) * np.float32(0.9)
    points, targets = draw(exe, workdir, volume, dvoxel, lo, hi, 0x1234567890abcdef, 7, 2048)
    assert np.array_equal(points.view(np.uint32), O.draw(0x1234567890abcdef, 7, 2048, lo, hi).view(np.uint32)), dims
    again, _, _ = sample(exe, workdir, volume, dvoxel, points)
    assert np.array_equal(again.view(np.uint32), targets.view(np.uint32)), dims
    return ratio


def main():
    import _volume_sample_oracle as O
    with tempfile.TemporaryDirectory() as workdir:
        exe = build(workdir)
        check_offsets(exe)
        worst = 0.0
        for dims in SHAPES:
            for dvoxel, exact in ((O.DVOXEL_EXACT, True), (O.DVOXEL_PLAIN, False)):
                ratio = check_shape(O, exe, workdir, dims, dvoxel, exact)
                worst = max(worst, ratio)
                print(f"{dims} at voxel size {dvoxel}: largest |fp32 - float64| / bound {ratio:.3f}", flush=True)
        print(f"no sanitizer report; 64-bit offsets right; largest |. - float64| / bound over everything: {worst:.3f}")


if __name__ == "__main__":
    main()
