#!/usr/bin/env python3
"""Host check of the alignment arithmetic: compiles tools/align_host_check.cpp (align_term, align_peak, align_axis and align_sample of
csrc/align_device.h over heap views of exactly H W floats; the kernels' LDS staging, tiles and launch geometry are not part of it) for
the CPU with AddressSanitizer and UBSan and runs it as a process of its own on extents down to 1 x 1, R = 0 and the largest R, NaN and
+-inf shifts and pixels.  It asserts that
  - the sanitizers report nothing,
  - the scores are within (terms + 1) 2^-53 of the numpy oracle's, and not finite exactly where the oracle's are not,
  - the peaks and flags are the oracle's (the shifts to the bit, rounded to float32),
  - the resampled views are within the bound of tests/_align_oracle.py of its float64 resampler, NaN exactly where it is, and return
    the source's bits at whole-number shifts.
The program is never loaded into Python.  No GPU.

    python tools/align_host_check.py
"""
import functools
import os
import sys
import tempfile

import numpy as np

sys.path.append(os.path.dirname(os.path.abspath(__file__)))          # tools/, for a caller that loads this file by its path
import host_check  # noqa: E402

# (H, W, Rv, Ru): the GPU tests' shapes, one pixel, one row, one column, no search on an axis, the largest window
SCORE_CASES = ((20, 24, 2, 3), (1, 1, 0, 0), (1, 9, 0, 4), (7, 1, 3, 0), (5, 6, 0, 2), (5, 6, 2, 0), (33, 35, 16, 16), (40, 70, 16, 1))
SHIFT_SHAPES = ((1, 1), (1, 5), (6, 1), (2, 2), (9, 11))
INF, NAN = float("inf"), float("nan")
SHIFTS = ((0.0, 0.0), (1.0, -2.0), (0.5, 0.25), (-0.3, 2.7), (-2.0 ** -30, 2.0 ** -30), (100.0, -100.0), (INF, 0.3), (0.3, -INF),
          (NAN, 0.0), (0.0, NAN), (3e38, -3e38), (-12.0, 13.0))


compiler = host_check.compiler                                       # such a caller asks the driver, not host_check
build = functools.partial(host_check.build, "align")


def scores(exe, workdir, b, p, Rv, Ru, w=None):
    shape = (len(b), 2 * Rv + 1, 2 * Ru + 1)
    (out,), _ = host_check.run(exe, ["scores", *b.shape, Rv, Ru], [b, p, w], [(np.float64, int(np.prod(shape)))])
    return out.reshape(shape)


def peak(exe, workdir, S):
    N, nv, nu = S.shape
    (shifts, flags), _ = host_check.run(exe, ["peak", N, nv // 2, nu // 2], [(S, np.float64)], [(np.float32, 2 * N), (np.int32, N)])
    return shifts.reshape(N, 2), flags


def shift(exe, workdir, views, shifts):
    (out,), _ = host_check.run(exe, ["shift", *views.shape], [views, shifts], [(np.float32, views.size)])
    return out.reshape(views.shape)


def check_scores(O, exe, workdir, H, W, Rv, Ru, seed=0):
    """Random views, with and without weights; then a NaN and an Inf pixel -> the largest relative error / bound."""
    rng = np.random.default_rng(seed)
    b, p = (rng.standard_normal((3, H, W)).astype(np.float32) for _ in range(2))
    w = rng.uniform(0.5, 1.0, (3, H, W)).astype(np.float32)
    w[:, ::3, ::2] = 0.0
    worst = 0.0
    for weights in (None, w):
        got, want = scores(exe, workdir, b, p, Rv, Ru, weights), O.scores(b, p, Rv, Ru, weights)
        bound = (O.terms(H, W, Rv, Ru) + 1) * O.U53 * want
        assert np.all(np.abs(got - want) <= bound), (H, W, Rv, Ru)
        worst = max(worst, float(np.max(np.abs(got - want) / np.maximum(bound, 1e-300))))
    bad = b.copy()
    bad[1, H // 2, W // 2], bad[2, 0, 0] = np.nan, np.inf
    got, want = scores(exe, workdir, bad, p, Rv, Ru), O.scores(bad, p, Rv, Ru)
    assert np.array_equal(np.isfinite(got), np.isfinite(want)) and np.isfinite(got[0]).all()
    s_got, f_got = peak(exe, workdir, got)
    s_want, f_want = O.peak(want)
    assert np.array_equal(f_got, f_want) and f_got[1] == O.FLAG_NON_FINITE and np.array_equal(s_got[1], [0, 0])
    assert np.array_equal(s_got[0].view(np.uint32), s_want[0].astype(np.float32).view(np.uint32))
    return worst


def check_shift(O, exe, workdir, H, W, seed=0):
    rng = np.random.default_rng(seed)
    shifts = np.array(SHIFTS, dtype=np.float32)
    views = rng.standard_normal((len(shifts), H, W)).astype(np.float32)
    views[5, 0, 0] = np.inf                          # a pixel that is not finite stays where the taps reach it
    got, want = shift(exe, workdir, views, shifts), O.shift_views(views, shifts)
    assert np.array_equal(np.isnan(got), np.isnan(want)), (H, W)
    ok = np.isfinite(want)
    assert np.array_equal(got[~ok & ~np.isnan(want)], want[~ok & ~np.isnan(want)].astype(np.float32))
    scale = float(np.abs(views[np.isfinite(views)]).max())
    ratio = float(np.abs(got[ok].astype(np.float64) - want[ok]).max() / (O.C_RESAMPLE * O.U24 * scale))
    assert ratio <= 1.0, (H, W, ratio)
    for n in (0, 1, 5, 11):                          # whole-number shifts: the source's bits at the clamped pixel
        rows = np.clip(np.arange(H) + int(shifts[n, 1]), 0, H - 1)
        cols = np.clip(np.arange(W) + int(shifts[n, 0]), 0, W - 1)
        assert np.array_equal(got[n].view(np.uint32), views[n][rows][:, cols].view(np.uint32)), (H, W, n)
    return ratio


def main():
    import _align_oracle as O
    with tempfile.TemporaryDirectory() as workdir:
        exe = build(workdir)
        for case in SCORE_CASES:
            print(f"scores {case}: largest error / bound {check_scores(O, exe, workdir, *case):.3f}", flush=True)
        for shape in SHIFT_SHAPES:
            print(f"shift {shape}: largest |fp32 - float64| / bound {check_shift(O, exe, workdir, *shape):.3f}", flush=True)
    print("no sanitizer report")


if __name__ == "__main__":
    main()
