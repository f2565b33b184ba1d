"""The float64 references of tests/_hash_backward_oracle.py and their bounds, validated on the CPU before a kernel meets them.

oracle/hash_ref.c's backward is an fp32 implementation with a sequential sum: it has to stay inside the same per-element bounds the
HIP kernels are held to (its worst element used 0.29 of the table bound when these references were written).  A reference that were
wrong -- a missing corner, a wrong row, a wrong weight -- would put the C oracle far outside them."""
import numpy as np
import pytest

import _hash_backward_oracle as O
from oracle import c_oracle, hashgrid_ref

DC = [(D, C) for D in (2, 3) for C in (1, 2, 4, 8)]


def _offsets(kind, D):
    return O.matrix_offsets(D) if kind == "matrix" else O.odd_offsets(D)


@pytest.mark.parametrize("D", [2, 3])
@pytest.mark.parametrize("kind", ["matrix", "odd"])
def test_corners_equal_the_c_oracle(kind, D):
    """Rows and weights of hashgrid_ref.corners against oracle/hash_ref.c, point by point, also where a level's size is no power of two."""
    offs = _offsets(kind, D)
    x = O.matrix_points(D, 3)[:64]
    for lvl in range(O.MATRIX_L):
        rows, w = hashgrid_ref.corners(x, lvl, offs, O.MATRIX_H)
        T = int(offs[lvl + 1] - offs[lvl])
        for b in range(x.shape[0]):
            idx, wc = c_oracle.corners(x[b], lvl, O.MATRIX_H, T)
            assert np.array_equal(rows[b] - int(offs[lvl]), idx.astype(np.int64))
            assert np.array_equal(w[b], wc)


@pytest.mark.parametrize("kind,D,C", [("matrix", D, C) for D, C in DC] + [("odd", 2, 2), ("odd", 3, 2)])
def test_c_oracle_backward_is_inside_both_bounds(kind, D, C):
    offs = _offsets(kind, D)
    L, H = O.MATRIX_L, O.MATRIX_H
    x = O.matrix_points(D, 10 * D + C)
    g = O.matrix_grad(C, 100 + 10 * D + C)
    rng = np.random.default_rng(7)
    emb = rng.uniform(-1, 1, (int(offs[-1]), C)).astype(np.float32)
    _, jac = c_oracle.hash_encode_forward(x, emb, offs, H, calc_grad_inputs=True)
    ge, gi = c_oracle.hash_encode_backward(g, x, emb, offs, H, dy_dx=jac)

    s, a, n = O.table_gradient(g, x, offs, H, C)
    assert n.sum() == C * L * x.shape[0] * 2 ** D                             # every corner of every point and level lands somewhere
    assert (n[int(offs[1]):] > 0).any() and (n == 0).any()
    used = np.abs(ge - s) / np.maximum(O.table_bound(a, n), 1e-300)
    print(f"table: worst element uses {used.max():.3f} of the bound")
    assert np.all(np.abs(ge - s) <= O.table_bound(a, n))
    assert np.all(ge[n == 0] == 0.0)

    si, ai = O.input_gradient(g.reshape(-1, L, C), jac, np.zeros_like(gi))
    print(f"inputs: worst element uses {(np.abs(gi - si) / O.input_bound(0.0, ai, L, C)).max():.3f} of the bound")
    assert np.all(np.abs(gi - si) <= O.input_bound(0.0, ai, L, C))


def test_the_bounds_notice_a_wrong_sum():
    """What the bounds are for: one dropped corner, or one contribution of a little-visited row off by a part in 1e4, lies outside."""
    D, C = 3, 8
    offs = O.matrix_offsets(D)
    x, g = O.matrix_points(D, 1), O.matrix_grad(C, 2)
    s, a, n = O.table_gradient(g, x, offs, O.MATRIX_H, C)
    rows, w = hashgrid_ref.corners(x, 5, offs, O.MATRIX_H)
    k = int(np.argmax(w[5]))                                                   # the heaviest corner of point 5 on the finest level
    r = int(rows[5, k])
    dropped = s.copy()
    dropped[r] -= float(w[5, k]) * g[5].reshape(O.MATRIX_L, C)[5]
    assert np.any(np.abs(dropped.astype(np.float32) - s) > O.table_bound(a, n))
    off = s.copy()
    off[r] += 1e-4 * float(w[5, k]) * g[5].reshape(O.MATRIX_L, C)[5]
    assert np.any(np.abs(off.astype(np.float32) - s) > O.table_bound(a, n))
    assert np.all(np.abs(s.astype(np.float32) - s) <= O.table_bound(a, n))


def test_sixteen_bit_gradients_are_upcast_not_rounded_again():
    import torch
    D, C = 2, 4
    offs = O.matrix_offsets(D)
    x = O.matrix_points(D, 4)
    g16 = torch.from_numpy(O.matrix_grad(C, 5)).to(torch.bfloat16)
    s, a, n = O.table_gradient(g16.float().numpy(), x, offs, O.MATRIX_H, C)
    s2, _, _ = O.table_gradient(g16.double().numpy(), x, offs, O.MATRIX_H, C)
    assert np.array_equal(s, s2)
    ge, _ = c_oracle.hash_encode_backward(g16.float().numpy(), x, np.zeros((int(offs[-1]), C), np.float32), offs, O.MATRIX_H)
    assert np.all(np.abs(ge - s) <= O.table_bound(a, n))
