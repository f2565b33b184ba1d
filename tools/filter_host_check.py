#!/usr/bin/env python3
"""Host check of the row filter's device code: compiles tools/filter_host_check.cpp (the per-output arithmetic of
csrc/filter_device.h, fed by a plain loop over every row; the kernel's own LDS staging, padded tap slots and sliding register window
in csrc/filter.hip are not part of it) for the CPU with AddressSanitizer and UBSan, runs it over the shapes of the GPU tests, with and
without the three factors, and prints its largest error as a share of the bound (W + 3) 2^-24 |view_scale post| sum |taps pre in|
that tests/test_hip_filter.py asserts, next to the float64 convolution of tests/_filter_oracle.py.  Then the same with the weight per
view and column of naf_filter_rows_views, `col`, against tests/_short_scan_oracle.py and the bound (W + 4) 2^-24 ... of
tests/test_hip_short_scan.py; a `col` of ones must return the bits of the run without it.  The program is a stand-alone executable;
nothing of it is loaded into Python.  No GPU.

    python tools/filter_host_check.py
"""
import tempfile

import numpy as np

import host_check


def run(exe, x, taps, pre, post, scale, col=None):
    (out,), _ = host_check.run(exe, x.shape, [x, taps, pre, post, scale, col], [(np.float32, x.size)])
    return out.reshape(x.shape)


def main():
    import _filter_oracle as F
    worst = 0.0
    with tempfile.TemporaryDirectory() as workdir:
        exe = host_check.build("filter", workdir)
        for shape in F.SHAPES:
            x, taps, pre, post, scale = F.filter_inputs(shape)
            for name, w in (("plain", (None, None, None)), ("weighted", (pre, post, scale))):
                got = run(exe, x, taps, *w).astype(np.float64)
                want, bound = F.filter_rows(x, taps, *w), F.filter_bound(x, taps, *w)
                err = np.abs(got - want)
                ratio = float((err / np.maximum(bound, np.finfo(np.float64).tiny)).max())
                print(f"{shape} {name:8s}: max |out - float64| {err.max():.3e}  worst ratio to the bound {ratio:.4f}")
                assert np.all(err <= bound), (shape, name)
                worst = max(worst, ratio)
            for k0 in sorted({0, shape[2] // 2, shape[2] - 1}):
                imp = np.zeros(shape, dtype=np.float32)
                imp[..., k0] = 1.0
                got = run(exe, imp, taps, None, None, None)
                assert got[0, 0].tobytes() == taps[np.abs(np.arange(shape[2]) - k0)].tobytes(), (shape, k0)
        print(f"largest error over all cases: {worst:.4f} of the bound; an impulse returns the taps bit for bit; no sanitizer report")
        import _short_scan_oracle as S
        worst = 0.0
        for shape in S.SHAPES:
            x, taps, pre, post, scale, col = S.filter_inputs(shape)
            for name, w in (("col", (None, None, None, col)), ("all", (pre, post, scale, col))):
                got = run(exe, x, taps, *w).astype(np.float64)
                want, bound = S.filter_rows(x, taps, *w), S.filter_bound(x, taps, *w)
                err = np.abs(got - want)
                ratio = float((err / np.maximum(bound, np.finfo(np.float64).tiny)).max())
                print(f"{shape} {name:8s}: max |out - float64| {err.max():.3e}  worst ratio to the bound {ratio:.4f}")
                assert np.all(err <= bound), (shape, name)
                worst = max(worst, ratio)
            ones = run(exe, x, taps, pre, post, scale, np.ones_like(col))
            assert ones.tobytes() == run(exe, x, taps, pre, post, scale).tobytes(), shape
        print(f"with col, largest error over all cases: {worst:.4f} of the bound; a col of ones changes no bit; no sanitizer report")


if __name__ == "__main__":
    main()
