#!/usr/bin/env python3
"""Host check of the OS-SART subset step's two walks on the Siddon pair: compiles tools/siddon_sart_host_check.cpp
(siddon_line_integral_and_row and siddon_scatter_pair of csrc/siddon_device.h over heap volumes of exactly n1 n2 n3 floats; the
kernels' own ray generation and tiling in csrc/siddon_sart.hip are not part of it) for the CPU with AddressSanitizer and UBSan,
walks the GPU tests' ray sets and the NaN / Inf rays (tests/_siddon_transpose_oracle.py) with mixed-sign, zero, NaN and Inf values,
and asserts that
  - the sanitizers report nothing,
  - acc and row are siddon_line_integral's on the volume and on ones, bit for bit (checked inside the program),
  - the (offset, term) pairs sent to num are siddon_scatter's, bit for bit and in order, with and without a den (inside the program),
  - the (offset, len) pairs sent to den are the forward walk's steps of positive length, whatever y is (inside the program),
  - the numbers of sent terms are the oracle's, and num and den stay inside the per-voxel bound against float64.
The program is never loaded into Python.  No GPU.

    python tools/siddon_sart_host_check.py
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
    exe = os.path.join(workdir, "siddon_sart_host_check")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-Wall", os.path.join(REPO, "tools", "siddon_sart_host_check.cpp"), "-o", exe])
    return exe


def walk(exe, workdir, volume, dvoxel, rays, y):
    """-> (num, den, terms sent to num, terms sent to den); a sanitizer report or a mismatch inside the program is an error."""
    paths = [os.path.join(workdir, name) for name in ("volume.f32", "rays.f32", "values.f32", "num_out.f32", "den_out.f32")]
    for path, a in zip(paths, (volume, rays, y)):
        np.ascontiguousarray(a, dtype=np.float32).tofile(path)
    done = subprocess.run([exe, *[str(n) for n in volume.shape], *[repr(float(np.float32(v))) for v in dvoxel], str(len(rays)), *paths],
                          capture_output=True, text=True)
    if done.returncode != 0 or done.stderr.strip():
        raise RuntimeError(f"exit {done.returncode}: {done.stdout}\nsanitizer output:\n{done.stderr}")
    words = done.stdout.split()
    assert words[0] == "num" and words[2] == "den" and words[4] == "mismatches" and int(words[5]) == 0, done.stdout
    num, den = (np.fromfile(p, dtype=np.float32, count=volume.size) for p in paths[3:])
    return num, den, int(words[1]), int(words[3])


def main():
    import _siddon_transpose_oracle as T
    with tempfile.TemporaryDirectory() as workdir:
        exe = build(workdir)
        worst = 0.0
        for name, (dims, dvoxel, vol, rays) in T.ray_sets().items():
            t = T.walk_triples(dims, dvoxel, rays)
            zero = np.zeros(dims)
            plain = T.values(len(rays))
            planted = plain.copy()
            planted[::7] = 0.0
            special = plain.copy()
            special[0::4], special[1::4], special[2::4] = np.nan, 0.0, np.inf
            want_den, bound_den, m_den = T.want_and_bound(t, np.ones(len(rays)), zero)
            for label, y in (("mixed signs", plain), ("every seventh 0", planted), ("NaN / 0 / Inf", special)):
                want, bound, m = T.want_and_bound(t, y, zero)
                num, den, n_num, n_den = walk(exe, workdir, vol, dvoxel, rays, y)
                ratio = max(float(T.use(num, want, bound).max()), float(T.use(den, want_den, bound_den).max()))
                worst = max(worst, ratio)
                print(f"{name}, y {label}: {len(rays)} rays, {n_num} terms to num (siddon_scatter's), {n_den} to den (the forward "
                      f"walk's lengths), acc and row siddon_line_integral's; largest |. - float64| / bound {ratio:.3f}", flush=True)
                assert n_num == int(m.sum()) and n_den == int(m_den.sum()), (name, n_num, int(m.sum()), n_den, int(m_den.sum()))
                assert ratio <= 1.0, name
        print(f"no sanitizer report; largest |. - float64| / bound over everything: {worst:.3f}")


if __name__ == "__main__":
    main()
