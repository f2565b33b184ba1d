#!/usr/bin/env python3
"""Host check of raw-frame conditioning's per-pixel arithmetic: compiles tools/frames_host_check.cpp (frames_transmission,
frames_window_min, frames_select, frames_decide and frames_tail of csrc/frames_device.h over heap blocks of exactly the elements they
may touch; the kernel's LDS staging and launch geometry are not part of it) for the CPU with AddressSanitizer and UBSan and
-ffp-contract=off, and runs it as a process of its own.  The program compares against files the numpy oracle of
tests/_frames_oracle.py wrote:
  - the window word (the key of the transmission, or the bad mark) of float32 and uint16 frames, with NaN, Inf, -0.0, den = 0,
    den < 0 and marked pixels among them: `==` on the bits,
  - the repaired transmission and both counts for every window size on shapes from 3 x 3 up, with dif = 0 and dif > 0: `==`,
  - the tail: `==` without the logarithm; with it within one unit in the last place of -log in float64, the bound of the host's
    logf (the device's is measured by the GPU tests), and no result below zero, nor a -0, under the clamp.
The program is never loaded into Python.  No GPU.

    python tools/frames_host_check.py
"""
import functools
import os
import sys
import tempfile

import numpy as np

sys.path.append(os.path.dirname(os.path.abspath(__file__)))          # tools/, for a caller that loads this file by its path
import host_check  # noqa: E402

# (N, H, W), size
CASES = (((1, 3, 3), 3), ((3, 7, 7), 7), ((2, 5, 37), 3), ((2, 5, 37), 5), ((2, 37, 5), 3), ((2, 37, 5), 5), ((2, 9, 12), 7))
DIFS = (0.0, 0.25)
HOST_LOG_ULP = 1.0                                                   # the host libm's logf is within one ulp

compiler = host_check.compiler                                       # a caller asks the driver, not host_check
build = functools.partial(host_check.build, "frames")


def float_bits(x):
    return int(np.float32(x).view(np.uint32))


def check_words(O, exe, workdir, seed=0):
    total = 0
    for k, u16 in enumerate((False, True)):
        shape = (3, 13, 21)
        raw, dark, flat = O.frames(shape, seed=seed + k, dtype=np.uint16) if u16 else O.special(shape, seed=seed + k)
        marked = (np.random.default_rng(seed + 7).random(shape[1:]) < 0.1).astype(np.uint8)
        t, isbad = O.transmission(raw, dark, flat, marked)
        want = np.where(isbad, O.BAD_KEY, O.key(O.bits(t)))
        full = lambda a: np.broadcast_to(a, shape)                   # noqa: E731  one dark, flat and mark per sample
        host_check.run(exe, ["words", raw.size, int(u16)], [(raw, raw.dtype), full(dark), full(flat), (full(marked), np.uint8),
                                                            (want, np.uint32)])
        total += raw.size
    return total


def check_decide(O, exe, workdir, seed=0):
    total = 0
    for k, (shape, size) in enumerate(CASES):
        for kind in (O.frames, O.special):
            raw, dark, flat = kind(shape, seed=seed + k)
            t, isbad = O.transmission(raw, dark, flat)
            words = np.where(isbad, O.BAD_KEY, O.key(O.bits(t)))
            for dif in DIFS:
                want, counts, _ = O.repaired(raw, dark, flat, None, size, dif)
                host_check.run(exe, ["decide", size, *shape, float_bits(dif)], [(words, np.uint32), (O.bits(want), np.uint32),
                                                                               (counts, np.uint32)])
                total += raw.size
    return total


def check_tail(O, exe, workdir, seed=0):
    rng = np.random.default_rng(seed)
    t_min = np.float32(1e-5)
    t = np.concatenate([rng.random(4096) * 1.2, 1 + (rng.random(1024) - 0.5) * 1e-3, np.exp(rng.uniform(-14, 10, 2048)),
                        [0.0, -0.0, -3.0, 1.0, t_min, np.nextafter(t_min, 0), np.nextafter(t_min, 1), 3e38]]).astype(np.float32)
    (same,), _ = host_check.run(exe, ["tail", t.size, float_bits(t_min), 0], [t], [(np.float32, t.size)])
    if not O.equal_bits(same, t):
        raise RuntimeError("frames_tail without the logarithm changed its argument")
    worst = 0.0
    for flags in (O.LOG, O.LOG | O.CLAMP_NONNEG):
        (got,), _ = host_check.run(exe, ["tail", t.size, float_bits(t_min), flags], [t], [(np.float32, t.size)])
        want = -np.log(np.maximum(t, t_min).astype(np.float64))
        if flags & O.CLAMP_NONNEG:
            want = np.maximum(want, 0.0)
            if np.signbit(got).any():
                raise RuntimeError("frames_tail returned a negative value or a -0 under the clamp")
        worst = max(worst, float(O.ulp_error(got, want).max()))
    if worst > HOST_LOG_ULP:
        raise RuntimeError(f"frames_tail is {worst:.3f} ulp from -log in float64, above the host logf's {HOST_LOG_ULP}")
    return t.size, worst


def main():
    import _frames_oracle as O
    with tempfile.TemporaryDirectory() as workdir:
        exe = build(workdir)
        print(f"words: {check_words(O, exe, workdir)} window words equal", flush=True)
        print(f"decide: {check_decide(O, exe, workdir)} repaired transmissions and their counts equal", flush=True)
        n, worst = check_tail(O, exe, workdir)
        print(f"tail: {n} values, the logarithm within {worst:.3f} ulp", flush=True)
    print("no sanitizer report")


if __name__ == "__main__":
    main()
