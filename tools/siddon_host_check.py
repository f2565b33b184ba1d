#!/usr/bin/env python3
"""Host check of the Siddon pair's two walks: compiles tools/siddon_host_check.cpp (siddon_forward and siddon_transpose of
csrc/siddon_device.h over heap volumes of exactly n1 n2 n3 floats; the device deposits, the kernels' ray generation and their
tiling are not part of it) for the CPU with AddressSanitizer and UBSan and runs it as a process of its own on the GPU tests' ray
sets, the NaN / Inf rays and the hot-voxel volumes (tests/_siddon_oracle.py, tests/_siddon_transpose_oracle.py) with mixed-sign,
zero, NaN and Inf values.  It asserts that
  - the sanitizers report nothing,
  - inside the program, bit for bit against its ungrouped restatement of the walk: the kind, acc and row of the forward walk, with
    and without the row sum, and the steps each deposit of the transpose walk is called with (none for a deposit that declines),
  - the forward results are within the float64 oracle's per-ray bound, NaN where the definition says NaN and 0 on an empty span,
  - the numbers of sent terms are the oracle's, and the value deposit's volume, num and den stay inside the per-voxel bound
    against float64.
The program is never loaded into Python.  No GPU.

    python tools/siddon_host_check.py
"""
import functools
import os
import sys
import tempfile

import numpy as np

sys.path.append(os.path.dirname(os.path.abspath(__file__)))          # tools/, for a caller that loads this file by its path
import host_check  # noqa: E402

compiler = host_check.compiler                                       # such a caller asks the driver, not host_check
build = functools.partial(host_check.build, "siddon")


def walk(exe, workdir, volume, dvoxel, rays, y=None, start=None):
    """Both walks over `rays` [n, 8]: the forward on `volume`, the value deposit of `y` (default zeros) into `start` (default zeros),
    the pair deposit into zeroed num and den -> dict of acc [n], value, num, den (flat volumes) and the counts of terms sent to
    each.  A sanitizer report or a mismatch inside the program is an error."""
    y = np.zeros(len(rays)) if y is None else y
    start = np.zeros(volume.shape) if start is None else start
    arrays, stdout = host_check.run(exe, [*volume.shape, *[repr(float(np.float32(v))) for v in dvoxel], len(rays)],
                                    [volume, start, rays, y], [(np.float32, len(rays))] + [(np.float32, volume.size)] * 3)
    words = stdout.split()
    assert words[0::2] == ["value", "num", "den", "mismatches"] and int(words[7]) == 0, stdout
    out = dict(zip(("acc", "value", "num", "den"), arrays))
    out.update(n_value=int(words[1]), n_num=int(words[3]), n_den=int(words[5]))
    return out


def value_vectors(T, n):
    """The three value vectors: mixed signs, every seventh 0, and NaN / 0 / Inf."""
    plain = T.values(n)
    planted = plain.copy()
    planted[::7] = 0.0
    special = plain.copy()
    special[0::4], special[1::4], special[2::4] = np.nan, 0.0, np.inf
    return (("mixed signs", plain), ("every seventh 0", planted), ("NaN / 0 / Inf", special))


def check_forward(S, exe, workdir, volume, dvoxel, rays):
    """Largest |acc - float64| / bound over the rays, NaN and 0 exactly where the definition has them."""
    want, bound = S.project_rays(volume, dvoxel, rays)
    got = walk(exe, workdir, volume, dvoxel, rays)["acc"]
    assert np.array_equal(np.isnan(got), np.isnan(want)), (got, want)
    return float(S.use(got, want, bound).max())


def check_set(S, T, exe, workdir, name, dims, dvoxel, volume, rays):
    """One ray set of the transpose oracle through both walks with the three value vectors -> the largest ratio to a bound."""
    t = T.walk_triples(dims, dvoxel, rays)
    v0, zero = T.start_volume(dims), np.zeros(dims)
    want_acc, bound_acc = S.project_rays(volume, dvoxel, rays)
    want_den, bound_den, m_den = T.want_and_bound(t, np.ones(len(rays)), zero)
    worst = 0.0
    for label, y in value_vectors(T, len(rays)):
        want_value, bound_value, m = T.want_and_bound(t, y, v0)
        want_num, bound_num, _ = T.want_and_bound(t, y, zero)
        got = walk(exe, workdir, volume, dvoxel, rays, y, v0)
        assert np.array_equal(np.isnan(got["acc"]), np.isnan(want_acc)), name
        ratio = max(float(S.use(got["acc"], want_acc, bound_acc).max()), float(T.use(got["value"], want_value, bound_value).max()),
                    float(T.use(got["num"], want_num, bound_num).max()), float(T.use(got["den"], want_den, bound_den).max()))
        worst = max(worst, ratio)
        print(f"{name}, y {label}: {len(rays)} rays, {got['n_value']} terms to the volume and {got['n_num']} to num, {got['n_den']} to "
              f"den, every walk its restatement's; largest |. - float64| / bound {ratio:.3f}", flush=True)
        assert got["n_value"] == got["n_num"] == int(m.sum()) and got["n_den"] == int(m_den.sum()), (name, got, int(m.sum()))
        assert ratio <= 1.0, name
    return worst


def main():
    import _siddon_oracle as S
    import _siddon_transpose_oracle as T
    with tempfile.TemporaryDirectory() as workdir:
        exe = build(workdir)
        worst = 0.0
        for name, (dims, dvoxel, volume, rays) in T.ray_sets().items():     # _siddon_oracle.ray_sets() and the non-finite rays
            worst = max(worst, check_set(S, T, exe, workdir, name, dims, dvoxel, volume, rays))
        dims, dvoxel, volume, rays = S.ray_sets()["c random"]
        for ijk in S.hot_voxels(dims):
            ratio = check_forward(S, exe, workdir, S.hot_volume(dims, ijk), dvoxel, rays)
            worst = max(worst, ratio)
            assert ratio <= 1.0, ijk
        bad = S.non_finite_rays(rays)
        want, _ = S.project_rays(volume, dvoxel, bad)
        got = walk(exe, workdir, volume, dvoxel, bad)["acc"]
        assert np.array_equal(np.isnan(got), np.isnan(want)) and np.all(got[~np.isnan(want)] == 0), (got, want)
        print(f"no sanitizer report, no mismatch; largest |. - float64| / bound over everything: {worst:.3f}")


if __name__ == "__main__":
    main()
