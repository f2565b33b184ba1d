#!/usr/bin/env python3
"""Host check of the Siddon traversal: compiles tools/siddon_host_check.cpp (the per-ray walk of csrc/siddon_device.h over a heap
volume of exactly n1 n2 n3 floats; the kernels' own ray generation and tiling in csrc/siddon.hip are not part of it) for the CPU
with AddressSanitizer and UBSan, walks the GPU tests' ray sets, NaN / Inf rays and hot-voxel volumes (tests/_siddon_oracle.py) and
asserts every result within the float64 oracle's per-ray bound.  The program is never loaded into Python.  No GPU.

    python tools/siddon_host_check.py
"""
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))


def build(workdir):
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    if cxx is None:
        raise RuntimeError("no host C++ compiler found")
    exe = os.path.join(workdir, "siddon_host_check")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-Wall", os.path.join(REPO, "tools", "siddon_host_check.cpp"), "-o", exe])
    return exe


def walk(exe, workdir, volume, dvoxel, rays):
    """The program's float32 result for `rays` [n, 8]; any sanitizer report is an error."""
    vol_path, ray_path, out_path = (os.path.join(workdir, name) for name in ("volume.f32", "rays.f32", "out.f32"))
    np.ascontiguousarray(volume, dtype=np.float32).tofile(vol_path)
    np.ascontiguousarray(rays, dtype=np.float32).tofile(ray_path)
    done = subprocess.run([exe, *[str(n) for n in volume.shape], *[repr(float(np.float32(v))) for v in dvoxel], str(len(rays)),
                           vol_path, ray_path, out_path], capture_output=True, text=True)
    if done.returncode != 0 or done.stderr.strip():
        raise RuntimeError(f"exit {done.returncode}; sanitizer output:\n{done.stderr}")
    return np.fromfile(out_path, dtype=np.float32, count=len(rays))


def main():
    import _siddon_oracle as S
    with tempfile.TemporaryDirectory() as workdir:
        exe = build(workdir)
        worst = 0.0
        for name, (dims, dvoxel, volume, rays) in S.ray_sets().items():
            want, bound = S.project_rays(volume, dvoxel, rays)
            ratio = S.use(walk(exe, workdir, volume, dvoxel, rays), want, bound).max()
            worst = max(worst, ratio)
            print(f"{name}: {len(rays)} rays, largest |. - float64| / bound {ratio:.3f}", flush=True)
            assert ratio <= 1.0, name
        dims, dvoxel, volume, rays = S.ray_sets()["c random"]
        for ijk in S.hot_voxels(dims):
            hot = S.hot_volume(dims, ijk)
            want, bound = S.project_rays(hot, dvoxel, rays)
            ratio = S.use(walk(exe, workdir, hot, dvoxel, rays), want, bound).max()
            worst = max(worst, ratio)
            assert ratio <= 1.0, ijk
        bad = S.non_finite_rays(rays)
        want, bound = S.project_rays(volume, dvoxel, bad)
        got = walk(exe, workdir, volume, dvoxel, bad)
        assert np.array_equal(np.isnan(got), np.isnan(want)) and np.all(got[~np.isnan(want)] == 0), (got, want)
        print(f"no sanitizer report; largest |. - float64| / bound over everything: {worst:.3f}")


if __name__ == "__main__":
    main()
