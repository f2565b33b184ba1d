#!/usr/bin/env python3
"""Host check of sinogram in-painting: compiles tools/inpaint_host_check.cpp (inpaint_last_word, inpaint_next_word, inpaint_left,
inpaint_right and inpaint_pixel of csrc/inpaint_device.h over heap blocks of exactly the elements they may touch; the kernel's
ballots, LDS and launch geometry are not part of it) for the CPU with AddressSanitizer and UBSan and -ffp-contract=off, and runs it
as a process of its own.  The program compares against files the numpy oracle of tests/_inpaint_oracle.py wrote:
  - the in-painted rows and both counts, with and without a prior, for every mask of the GPU tests at every width of theirs, and
    with a NaN and an Inf at a valid neighbour: `==` on the bits,
  - the left and right neighbour of every column of single rows up to the widest the library takes (16384 columns), among them
    spans that cross many words, a row with one valid pixel and a row with none: `==`.
The program is never loaded into Python.  No GPU.

    python tools/inpaint_host_check.py
"""
import functools
import os
import sys
import tempfile

import numpy as np

sys.path.append(os.path.dirname(os.path.abspath(__file__)))          # tools/, for a caller that loads this file by its path
import host_check  # noqa: E402

SHAPE = (2, 3)                                                       # N, H of every case
NONE = 0xffffffff
SEARCH_WIDTHS = (1, 64, 65, 300, 4097, 16384)

compiler = host_check.compiler                                       # a caller asks the driver, not host_check
build = functools.partial(host_check.build, "inpaint")


def float_bits(x):
    return int(np.float32(x).view(np.uint32))


def check_rows(O, exe, workdir, widths=None, seed=0):
    total = 0
    for W in widths or O.WIDTHS:
        shape = (*SHAPE, W)
        p, prior = O.make_inputs(shape, seed=seed + W)
        if W >= 3:
            p[0, 0, 0], p[1, 1, W - 1], p[0, 2, W // 2] = np.nan, np.inf, -np.inf
        for kind in O.MASKS:
            mask = O.make_mask(kind, shape, seed=seed)
            for pri, eps in ((None, 0.0), (prior, O.EPS)):
                want, counts = O.inpaint(p, mask, pri, eps if pri is not None else None)
                host_check.run(exe, ["rows", *shape, float_bits(eps)], [p, (mask, np.uint8), pri, (O.bits(want), np.uint32),
                                                                        (counts, np.uint32)])
                total += p.size
    return total


def strict_neighbours(mask):
    """L and R of every column of one row, masked or not: the nearest valid column strictly below and strictly above."""
    valid = np.flatnonzero(np.asarray(mask) == 0)
    u = np.arange(len(mask))
    below, above = np.searchsorted(valid, u, "left"), np.searchsorted(valid, u, "right")
    padded = np.concatenate([valid, [NONE]]).astype(np.int64)
    left = np.where(below > 0, padded[np.maximum(below - 1, 0)], NONE)
    right = padded[np.minimum(above, len(valid))]
    return left.astype(np.uint32), right.astype(np.uint32)


def check_search(O, exe, workdir, widths=SEARCH_WIDTHS, seed=0):
    total = 0
    for W in widths:
        rng = np.random.default_rng(seed + W)
        rows = [np.zeros(W, np.uint8), np.ones(W, np.uint8), (rng.random(W) < 0.3).astype(np.uint8), (rng.random(W) < 0.98).astype(np.uint8)]
        for keep in (0, W // 2, W - 1):                              # one valid pixel
            rows.append(np.ones(W, np.uint8))
            rows[-1][keep] = 0
        spans = np.zeros(W, np.uint8)                                # long spans between single valid pixels
        spans[1:W - 1] = 1
        spans[::max(W // 5, 1)] = 0
        rows.append(spans)
        for mask in rows:
            left, right = strict_neighbours(mask)
            host_check.run(exe, ["search", W], [(mask, np.uint8), (left, np.uint32), (right, np.uint32)])
            total += W
    return total


def main():
    import _inpaint_oracle as O
    with tempfile.TemporaryDirectory() as workdir:
        exe = build(workdir)
        print(f"rows: {check_rows(O, exe, workdir)} in-painted values and their counts equal", flush=True)
        print(f"search: {check_search(O, exe, workdir)} left and right neighbours equal", flush=True)
    print("no sanitizer report")


if __name__ == "__main__":
    main()
