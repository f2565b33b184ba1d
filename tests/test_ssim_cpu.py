"""3-D SSIM without a GPU: the float64 restatement (tests/_ssim_oracle.py) against a brute-force window sum, scipy's
uniform_filter formulation and scikit-image where they import, its axis-permutation invariance, and the C ABI's argument
checks of naf_ssim_3d."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

import _ssim_oracle as O


def _pair(shape, seed):
    rng = np.random.default_rng(seed)
    x = rng.random(shape).astype(np.float32)
    y = (x + 0.2 * rng.standard_normal(shape)).astype(np.float32)
    return x, y


def test_oracle_matches_a_brute_force_window_sum():
    x, y = _pair((7, 8, 9), 0)
    a, b = x.astype(np.float64), y.astype(np.float64)
    s = []
    for i, j, k in itertools.product(range(1), range(2), range(3)):
        wa, wb = a[i:i + 7, j:j + 7, k:k + 7], b[i:i + 7, j:j + 7, k:k + 7]
        terms = [float(np.sum(t)) / 343 for t in (wa, wb, wa * wa, wb * wb, wa * wb)]
        s.append(O.ssim_terms(*terms))
    want = float(np.mean(s))
    assert O.ssim_map(x, y).shape == (1, 2, 3)
    assert abs(O.ssim_3d(x, y) - want) <= 1e-15, (O.ssim_3d(x, y), want)


def test_oracle_matches_the_uniform_filter_formulation():
    """The formulation scikit-image uses: scipy.ndimage.uniform_filter means, cropped by 3 on every side."""
    ndimage = pytest.importorskip("scipy.ndimage")
    for shape, seed in (((7, 7, 7), 1), ((9, 40, 33), 2), ((24, 20, 16), 3)):
        x, y = _pair(shape, seed)
        a, b = x.astype(np.float64), y.astype(np.float64)
        u = [ndimage.uniform_filter(t, size=7) for t in (a, b, a * a, b * b, a * b)]
        S = O.ssim_terms(*u)[3:-3, 3:-3, 3:-3]
        assert abs(O.ssim_3d(x, y) - float(S.mean())) <= 1e-14


def test_oracle_matches_scikit_image():
    metrics = pytest.importorskip("skimage.metrics")
    for shape, seed in (((7, 7, 7), 4), ((9, 40, 33), 5)):
        x, y = _pair(shape, seed)
        want = metrics.structural_similarity(x.astype(np.float64), y.astype(np.float64), data_range=2)
        assert abs(O.ssim_3d(x, y) - float(want)) <= 1e-14


def test_oracle_is_invariant_under_axis_permutations():
    x, y = _pair((9, 12, 10), 6)
    base = O.ssim_3d(x, y)
    assert 0.0 < base < 1.0
    for perm in itertools.permutations(range(3)):
        px, py = np.ascontiguousarray(x.transpose(perm)), np.ascontiguousarray(y.transpose(perm))
        assert abs(O.ssim_3d(px, py) - base) <= 1e-15, perm
    assert O.ssim_3d(x, x) == 1.0
    with pytest.raises(ValueError, match="win_size exceeds image extent"):
        O.ssim_3d(x[:6], y[:6])


def test_ssim_abi_rejects_bad_arguments_without_a_gpu():
    """Null pointers, extents below the window and a short workspace are refused before any HIP call."""
    from neuralvolumetricreconstructionformedicalimages_amd import _abi
    lib = _abi.lib()
    one = ctypes.c_void_p(256)
    need = lib.naf_ssim_3d_workspace_bytes(64, 64, 64)
    assert need >= 8 and need % 256 == 0
    assert lib.naf_ssim_3d_workspace_bytes(6, 64, 64) == 0 and lib.naf_ssim_3d_workspace_bytes(64, 64, 6) == 0
    assert lib.naf_ssim_3d_workspace_bytes(1024, 1024, 1024) >= 8 * 1024
    for args in ((None, one, one, one), (one, None, one, one), (one, one, None, one), (one, one, one, None)):
        x, y, out, ws = args
        assert lib.naf_ssim_3d(x, y, 64, 64, 64, out, ws, need, None) == -1
        assert b"null pointer" in lib.naf_last_error()
    for dims in ((6, 64, 64), (64, 6, 64), (64, 64, 6), (0, 0, 0)):
        assert lib.naf_ssim_3d(one, one, *dims, one, one, need, None) == -1
        assert b"win_size exceeds image extent" in lib.naf_last_error()
    assert lib.naf_ssim_3d(one, one, 64, 64, 64, one, one, need - 8, None) == -1
    assert b"workspace too small" in lib.naf_last_error()
    with pytest.raises(RuntimeError, match="ssim_3d"):
        _abi.check(lib.naf_ssim_3d(one, one, 64, 64, 64, one, one, 0, None), "ssim_3d")


def test_ssim_3d_refuses_cpu_tensors():
    from neuralvolumetricreconstructionformedicalimages_amd.metrics import ssim_3d
    with pytest.raises(RuntimeError, match="no CPU path"):
        ssim_3d(torch.zeros(8, 8, 8), torch.zeros(8, 8, 8))
