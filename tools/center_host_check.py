#!/usr/bin/env python3
"""Host check of the centre-of-rotation search: compiles tools/center_host_check.cpp (center_coord, center_term, center_sample,
center_accumulate, center_in_mask, center_negativity and center_step of csrc/center_device.h over heap blocks of exactly the
elements they may touch; the kernel's LDS staging and launch geometry are not part of it) for the CPU with AddressSanitizer and
UBSan and -ffp-contract=off, and runs it as a process of its own.  Its output is compared with tests/_center_oracle.py:
  - the slices of the GPU tests' cases: `==` on the bits of the float32 restatement, and within its recorded error of float64,
  - both scores of fixed slices at radii from 0 to beyond the slice: 1e-12 relative to the float64 sums.
The program is never loaded into Python.  No GPU.

    python tools/center_host_check.py
"""
import functools
import os
import sys
import tempfile

import numpy as np

sys.path.append(os.path.dirname(os.path.abspath(__file__)))          # tools/, for a caller that loads this file by its path
import host_check  # noqa: E402

compiler = host_check.compiler                                       # a caller asks the driver, not host_check
build = functools.partial(host_check.build, "center")


def float_bits(x):
    return int(np.float32(x).view(np.uint32))


def check_slices(O, exe, workdir, names=None):
    from neuralvolumetricreconstructionformedicalimages_amd import center
    total = 0
    for case in O.CASES:
        if names is not None and case[0] not in names:
            continue
        geo, angles, cand, q = O.case_inputs(case)
        g = center.scalars(geo)
        S, N, W = q.shape
        K, n = len(cand), g["n"]
        args = ["slices", S, N, W, K, n, g["parallel"], *[float_bits(g[k]) for k in ("DSO", "DSD", "du", "ou", "dx", "dy", "ox", "oy")]]
        (got,), _ = host_check.run(exe, args, [q, center.trig(angles), cand], [(np.float32, S * K * n * n)])
        got = got.reshape(S, K, n, n)
        want32, want64 = O.case_reference(case, np.float32), O.case_reference(case)
        if not np.array_equal(got.view(np.uint32), want32.view(np.uint32)):
            raise RuntimeError(f"{case[0]}: the slices differ from the float32 restatement")
        err = float(np.abs(got.astype(np.float64) - want64).max() / np.abs(want64).max())
        if err > O.F32_ERROR:
            raise RuntimeError(f"{case[0]}: relative error {err:.3e} against float64, above {O.F32_ERROR:.3e}")
        total += got.size
    return total


def check_metrics(O, exe, workdir, seed=0):
    rng = np.random.default_rng(seed)
    total = 0
    for n in (1, 16, 33):
        f = rng.standard_normal((4, n, n)).astype(np.float32)
        f[0], f[1] = np.abs(f[0]), -np.abs(f[1])
        f[2] = 0.0
        f[2, n // 2, n // 2] = -3.0
        dx, dy = np.float32(1e-3), np.float32(1.25e-3)
        for radius_px in (0.0, 1.0, 7.3, 100.0):
            r = np.float32(radius_px * 1e-3)
            (got,), _ = host_check.run(exe, ["metrics", 4, n, float_bits(dx), float_bits(dy), float_bits(r)], [f], [(np.float64, 8)])
            want = O.metrics(f[None], dx, dy, r)[0].reshape(-1)
            if not np.all(np.abs(got - want) <= 1e-12 * np.abs(want)):
                raise RuntimeError(f"metrics differ at n = {n}, r = {radius_px} px: {got} against {want}")
            total += f.size
    return total


def main():
    import _center_oracle as O
    with tempfile.TemporaryDirectory() as workdir:
        exe = build(workdir)
        print(f"slices: {check_slices(O, exe, workdir)} pixels equal the float32 restatement bit for bit", flush=True)
        print(f"metrics: {check_metrics(O, exe, workdir)} pixels scored as the oracle scores them", flush=True)
    print("no sanitizer report")


if __name__ == "__main__":
    main()
