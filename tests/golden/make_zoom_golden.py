"""tests/golden/make_zoom_golden.py -- regenerates tests/golden/zoom_scipy.npz (needs scipy; the file was made with 1.15.3).

For each shape pair of tests/_zoom_oracle.py: the seeded float32 input in [0.5, 1.5] and what
scipy.ndimage.zoom(input, out / in, order=3, prefilter=False) returns for it (float32).  These are scipy's outputs; the tests
compare the float64 restatement and the HIP kernel against them.

Usage:  python tests/golden/make_zoom_golden.py
"""
import os
import sys

import numpy as np
import scipy
from scipy import ndimage

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import _zoom_oracle as O  # noqa: E402


def main():
    arrays = {"scipy_version": np.array(scipy.__version__)}
    for n, (a, b) in enumerate(O.GOLDEN_PAIRS):
        x = O.inputs(a, seed=100 + n)
        y = ndimage.zoom(x, [q / p for p, q in zip(a, b)], order=3, prefilter=False)
        assert y.shape == b and y.dtype == np.float32, (a, b, y.shape, y.dtype)
        arrays[f"in_{n}"], arrays[f"out_{n}"] = x, y
    path = os.path.join(HERE, "zoom_scipy.npz")
    np.savez_compressed(path, **arrays)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
