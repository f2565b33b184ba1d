#!/usr/bin/env python3
"""Host check of the Siddon transpose: compiles tools/siddon_transpose_host_check.cpp (siddon_scatter of csrc/siddon_device.h over
a heap volume of exactly n1 n2 n3 floats; the kernels' own ray generation and tiling in csrc/siddon_backproject.hip are not part of
it) for the CPU with AddressSanitizer and UBSan, scatters the GPU tests' ray sets and the NaN / Inf rays
(tests/_siddon_transpose_oracle.py) with mixed-sign, zero, NaN and Inf values, and asserts that
  - the sanitizers report nothing,
  - every sent (offset, term) is the forward walk's (offset, len) times y, bit for bit and in order (checked inside the program),
  - the number of sent terms is the oracle's, and the volume stays inside the per-voxel bound against float64.
The program is never loaded into Python.  No GPU.

    python tools/siddon_transpose_host_check.py
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
    exe = os.path.join(workdir, "siddon_transpose_host_check")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-Wall", os.path.join(REPO, "tools", "siddon_transpose_host_check.cpp"),
                           "-o", exe])
    return exe


def scatter(exe, workdir, v0, dvoxel, rays, y):
    """-> (volume after the scatter, number of sent terms); a sanitizer report or a term that is not the forward walk's is an error."""
    paths = [os.path.join(workdir, name) for name in ("volume_in.f32", "rays.f32", "values.f32", "volume_out.f32")]
    for path, a in zip(paths, (v0, rays, y)):
        np.ascontiguousarray(a, dtype=np.float32).tofile(path)
    done = subprocess.run([exe, *[str(n) for n in v0.shape], *[repr(float(np.float32(v))) for v in dvoxel], str(len(rays)), *paths],
                          capture_output=True, text=True)
    if done.returncode != 0 or done.stderr.strip():
        raise RuntimeError(f"exit {done.returncode}: {done.stdout}\nsanitizer output:\n{done.stderr}")
    words = done.stdout.split()
    assert words[0] == "sent" and words[2] == "mismatches" and int(words[3]) == 0, done.stdout
    return np.fromfile(paths[3], dtype=np.float32, count=v0.size), int(words[1])


def main():
    import _siddon_transpose_oracle as T
    with tempfile.TemporaryDirectory() as workdir:
        exe = build(workdir)
        worst = 0.0
        for name, (dims, dvoxel, _, rays) in T.ray_sets().items():
            t = T.walk_triples(dims, dvoxel, rays)
            v0 = T.start_volume(dims)
            plain = T.values(len(rays))
            special = plain.copy()
            special[0::4], special[1::4], special[2::4] = np.nan, 0.0, np.inf
            for label, y in (("mixed signs", plain), ("NaN / 0 / Inf", special)):
                want, bound, m = T.want_and_bound(t, y, v0)
                got, sent = scatter(exe, workdir, v0, dvoxel, rays, y)
                ratio = T.use(got, want, bound).max()
                worst = max(worst, ratio)
                print(f"{name}, y {label}: {len(rays)} rays, {sent} terms sent, each the forward walk's (offset, len) * y; "
                      f"largest |. - float64| / bound {ratio:.3f}", flush=True)
                assert sent == int(m.sum()), (name, sent, int(m.sum()))
                assert ratio <= 1.0, name
        print(f"no sanitizer report; largest |. - float64| / bound over everything: {worst:.3f}")


if __name__ == "__main__":
    main()
