"""Float64 references of the hash-grid encoder's backward, with derived error bounds (not a test module).

Built on oracle/hashgrid_ref.corners (rows and fp32 weights of any D, level and level size; bit-identical to oracle/hash_ref.c in
the forward).  A kernel under test forms fp32 products `w * g` and adds them in fp32 in an order that is not fixed (atomics); the
references below form the same products exactly (an fp32 weight times a gradient of at most 24 significant bits is exact in
float64) and sum them in float64, and return the magnitudes that bound what ANY fp32 summation order can lose.

Bounds (u = 2^-24, the unit roundoff of fp32):
  * n fp32 additions in any order lose at most n*u*sum|t_i| (to first order), the rounding of each product t_i = fl(w*g) another
    u*|t_i|: (n + 1) * u * a with a = sum|w*g|.  Doubled for the second-order terms and for slack that does not depend on the
    kernel: (n + 1) * 2^-23 * a.
  * the input gradient is one sequential chain of L*C products added to what the caller left in grad_inputs:
    (L*C + 1) * 2^-23 * (|start| + sum|g*j|).
"""
import numpy as np

from oracle import hashgrid_ref

U23 = 2.0 ** -23


def table_gradient(grad_BLC, x01, offsets, H, C):
    """grad_BLC [B, L*C] (or [B, L, C]): the gradient values exactly as stored (a 16-bit gradient upcast, never re-rounded).
    -> (s, a, n), float64 [rows, C] each: s = sum w*g, a = sum |w*g|, n = number of contributions to the row."""
    offsets = np.asarray(offsets)
    L = len(offsets) - 1
    x01 = np.ascontiguousarray(x01, dtype=np.float32)
    B = x01.shape[0]
    g = np.asarray(grad_BLC, dtype=np.float64).reshape(B, L, C)
    rows_total = int(offsets[-1])
    s = np.zeros((rows_total, C), dtype=np.float64)
    a = np.zeros((rows_total, C), dtype=np.float64)
    n = np.zeros(rows_total, dtype=np.float64)
    for lvl in range(L):
        rows, w = hashgrid_ref.corners(x01, lvl, offsets, H)                   # [B, 2^D] int64 / float32
        t = w.astype(np.float64)[:, :, None] * g[:, lvl, None, :]              # [B, 2^D, C], exact products
        flat = rows.reshape(-1)
        t = t.reshape(-1, C)
        for c in range(C):                                                     # bincount: a sequential float64 sum per row
            s[:, c] += np.bincount(flat, weights=t[:, c], minlength=rows_total)
            a[:, c] += np.bincount(flat, weights=np.abs(t[:, c]), minlength=rows_total)
        n += np.bincount(flat, minlength=rows_total)
    return s, a, np.repeat(n[:, None], C, axis=1)


def table_bound(a, n):
    """|got - s| <= (n + 1) * 2^-23 * a, per element."""
    return (n + 1.0) * U23 * a


def input_gradient(grad, dy_dx, start):
    """grad [B, L, C], dy_dx [B, L, D, C], start [B, D]: the stored values.  -> (start + sum_{l,c} g*j, sum |g*j|), float64 [B, D]."""
    g = np.asarray(grad, dtype=np.float64)
    j = np.asarray(dy_dx, dtype=np.float64)
    t = g[:, :, None, :] * j                                                   # [B, L, D, C]
    return np.asarray(start, dtype=np.float64) + t.sum(axis=(1, 3)), np.abs(t).sum(axis=(1, 3))


def input_bound(start, a, L, C):
    """|got - s| <= (L*C + 1) * 2^-23 * (|start| + sum|g*j|), per element."""
    return (L * C + 1.0) * U23 * (np.abs(np.asarray(start, dtype=np.float64)) + a)


# ---- the shapes the GPU matrix and the CPU validation of these references share --------------------------------------------------
MATRIX_L, MATRIX_H, MATRIX_LOG2T, MATRIX_B = 6, 4, 9, 777


def matrix_offsets(D):
    """D = 3: level 0 dense, levels 1-5 hashed at 512 rows; D = 2: levels 0-2 dense, 3-5 hashed."""
    return hashgrid_ref.level_offsets(MATRIX_L, MATRIX_H, MATRIX_LOG2T, D)


def odd_offsets(D):
    """Level sizes that are no powers of two: hashed levels there take the `index % size` regime (a real modulo)."""
    sizes = [5 ** D, 500, 777, 1000, 512, 333]
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)


def matrix_points(D, seed):
    """B = 777 uniform points in [0, 1) with an all-0, an all-1 and a mixed face point."""
    rng = np.random.default_rng(seed)
    x = rng.random((MATRIX_B, D), dtype=np.float32)
    x[0], x[1], x[2] = 0.0, 1.0, [0.0, 1.0, 0.5][:D]
    return x


def matrix_grad(C, seed):
    """Standard normal [B, L*C] float32 (the caller rounds it to the storage type under test)."""
    return np.random.default_rng(seed).standard_normal((MATRIX_B, MATRIX_L * C)).astype(np.float32)
