#!/usr/bin/env python3
"""Host check of the stripe filter's integer arithmetic: compiles tools/stripe_host_check.cpp (stripe_key / stripe_unkey,
stripe_reflect, the bitonic network's partner and direction arithmetic and stripe_select of csrc/stripe_device.h over heap blocks of
exactly the elements they may touch; the kernels' LDS staging and launch geometry are not part of it) for the CPU with
AddressSanitizer and UBSan and runs it as a process of its own.  The program compares against files the numpy oracle of
tests/_stripe_oracle.py wrote, and the check is `==` on the bits:
  - the key and its round trip over +-0, denormals, +-Inf, NaNs of both signs and random patterns,
  - the reflected index for every W in [3, 70], every legal h and every index a window reaches,
  - the network as a CPU sort for every N in [1, 130] and for 4096, on columns with ties and special values,
  - the selection for every odd size to 63, on random windows, windows of few distinct keys and constant ones.
The program is never loaded into Python.  No GPU.

    python tools/stripe_host_check.py
"""
import functools
import os
import sys
import tempfile

import numpy as np

sys.path.append(os.path.dirname(os.path.abspath(__file__)))          # tools/, for a caller that loads this file by its path
import host_check  # noqa: E402

SORT_COUNTS = tuple(range(1, 131)) + (4096,)
SIZES = tuple(range(3, 64, 2))
WINDOWS = 96                                                         # per size

compiler = host_check.compiler                                       # a caller asks the driver, not host_check
build = functools.partial(host_check.build, "stripe")


def check_key(O, exe, workdir, seed=0):
    rng = np.random.default_rng(seed)
    b = np.concatenate([O.EDGE_BITS, rng.integers(0, 1 << 32, 4096, dtype=np.uint64).astype(np.uint32)])
    host_check.run(exe, ["key", b.size], [(b, np.uint32), (O.key(b), np.uint32)])
    return b.size


def check_reflect(O, exe, workdir):
    want = []
    for W in range(3, 71):
        for h in range(1, O.largest_size(W) // 2 + 1):
            want.append(np.pad(np.arange(W, dtype=np.uint32), h, mode="symmetric"))      # scipy's `reflect`
    want = np.concatenate(want)
    host_check.run(exe, ["reflect", want.size], [(want, np.uint32)])
    return want.size


def check_sort(O, exe, workdir, seed=0):
    """Columns of the "special" kind, which tie often: the oracle's stable argsort of (key << 32 | view) per column."""
    columns, sorted_bits, perms = [], [], []
    for k, N in enumerate(SORT_COUNTS):
        column = O.data("special", (N, 1, 1), seed=seed + k)
        if N > 4:
            column[N // 2:] = column[:N - N // 2]                    # every value twice: the view index decides
        perm, s = O.sort_views(column)
        columns.append(O.bits(column).ravel()), sorted_bits.append(s.ravel()), perms.append(perm.ravel())
    total = sum(SORT_COUNTS)
    host_check.run(exe, ["sort", total, *SORT_COUNTS], [(np.concatenate(columns), np.uint32), (np.concatenate(sorted_bits), np.uint32),
                                                        (np.concatenate(perms), np.uint16)])
    return total


def check_select(O, exe, workdir, seed=0):
    rng = np.random.default_rng(seed)
    for size in SIZES:
        keys = rng.integers(0, 1 << 32, (WINDOWS, size), dtype=np.uint64).astype(np.uint32)
        keys[32:64] = rng.integers(0, 3, (32, size)).astype(np.uint32) * np.uint32(0x7fffffff)      # few distinct keys
        keys[64:72] = keys[64:72, :1]                                                                # constant windows
        want = np.sort(keys, axis=1)[:, size // 2]
        host_check.run(exe, ["select", WINDOWS, size], [(keys, np.uint32), (want, np.uint32)])
    return len(SIZES) * WINDOWS


def main():
    import _stripe_oracle as O
    with tempfile.TemporaryDirectory() as workdir:
        exe = build(workdir)
        print(f"key: {check_key(O, exe, workdir)} patterns equal", flush=True)
        print(f"reflect: {check_reflect(O, exe, workdir)} indices equal", flush=True)
        print(f"sort: {check_sort(O, exe, workdir)} ranks of {len(SORT_COUNTS)} columns equal", flush=True)
        print(f"select: {check_select(O, exe, workdir)} windows equal", flush=True)
    print("no sanitizer report")


if __name__ == "__main__":
    main()
