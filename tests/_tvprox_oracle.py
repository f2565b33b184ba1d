"""Numpy restatement of the TV proximal map (include/naf_hip.h, V3) -- not a test module.  Written from
the definitions, in float64, plus one float32 form of a step that follows the stated operation order.

    D_a f[v]   = f[v] - f[v - e_a] if v_a > 0, else 0
    TV(f)      = sum_v sqrt(sum_a (D_a f[v])^2)                                         (exact: no eps)
    (D^T p)[v] = sum_a ([v_a > 0] p_a[v] - [v_a < n_a - 1] p_a[v + e_a])
    P_C(t)     = t, or max(t, 0) with `nonneg`
    step:  u = P_C(b - lam D^T r);  q_a = r_a + D_a u / (12 lam);  p = q / max(1, |q|);  r_next = p + c (p - p_old)
    prox:  p_0 = r_1 = start, t_1 = 1;  t_{k+1} = (1 + sqrt(1 + 4 t_k^2)) / 2, c_k = (t_k - 1) / t_{k+1};  x = P_C(b - lam D^T p)

The planes p_a[v] at v_a = 0 are masked on every read and come back 0."""
import math

import numpy as np

# the step tests' shapes: every degenerate axis, an extent below one wave, one past 256 on the contiguous axis, and odd extents
# that leave ragged 8 x 32 tiles and a ragged last chunk of axis 0
STEP_SHAPES = [(1, 1, 1), (7, 1, 1), (1, 9, 1), (1, 1, 70), (5, 6, 7), (3, 5, 300), (33, 17, 65)]
STEP_LAMBDAS = [0.05, 2.0]
STEP_MOMENTUM = 0.6180339887498949          # c_2 of the sequence; any value in [0, 1) does


def _hi_lo(a):
    hi = tuple(slice(1, None) if k == a else slice(None) for k in range(3))
    lo = tuple(slice(None, -1) if k == a else slice(None) for k in range(3))
    return hi, lo


def differences(f, dtype=np.float64):
    """[D_0 f, D_1 f, D_2 f] as one [3, n1, n2, n3] array."""
    f = np.asarray(f, dtype=dtype)
    d = np.zeros((3,) + f.shape, dtype=dtype)
    for a in range(3):
        hi, lo = _hi_lo(a)
        d[a][hi] = f[hi] - f[lo]
    return d


def masked(p, dtype=np.float64):
    """A copy of the dual variable with the inert planes (p_a[v] at v_a = 0) set to 0: the mask of every read."""
    p = np.array(p, dtype=dtype)
    p[0][0, :, :] = 0
    p[1][:, 0, :] = 0
    p[2][:, :, 0] = 0
    return p


def adjoint_terms(p, dtype=np.float64):
    """The three terms [v_a > 0] p_a[v] - [v_a < n_a - 1] p_a[v + e_a], one per axis."""
    p = masked(p, dtype)
    t = np.array(p)
    for a in range(3):
        hi, lo = _hi_lo(a)
        t[a][lo] -= p[a][hi]
    return t


def adjoint(p):
    t = adjoint_terms(p)
    return t[0] + t[1] + t[2]


def project(t, nonneg):
    return np.where(t < 0, 0, t) if nonneg else t


def primal(b, p, lam, nonneg=False):
    return project(np.asarray(b, dtype=np.float64) - lam * adjoint(p), nonneg)


def step(b, r, p_old, lam, momentum, nonneg=False):
    """One iteration in float64 -> (p, r_next)."""
    u = primal(b, r, lam, nonneg)
    q = masked(r) + differences(u) / (12.0 * lam)
    p = q / np.maximum(1.0, np.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2]))
    return p, p + momentum * (p - masked(p_old))


def primal_f32(b, p, lam, nonneg=False):
    """`primal` in float32, one rounding per operation: the three terms of D^T added in axis order."""
    f = np.float32
    t = adjoint_terms(p, f)
    dt = (t[0] + t[1]) + t[2]
    return project(np.asarray(b, dtype=f) - f(lam) * dt, nonneg).astype(f)


def step_f32(b, r, p_old, lam, momentum, nonneg=False):
    """`step` in float32, one rounding per operation in the stated order: 1 / (12 lam) formed once, q_a = r_a + that * D_a u,
    squares added in axis order, true division."""
    f = np.float32
    lam, momentum = f(lam), f(momentum)
    u = primal_f32(b, r, lam, nonneg)
    inv = f(1) / (f(12) * lam)
    q = masked(r, f) + inv * differences(u, f)              # 0 where v_a = 0: both terms are
    s = q[0] * q[0]
    s = s + q[1] * q[1]
    s = s + q[2] * q[2]
    n = np.sqrt(s)
    p = q / np.where(n > 1, n, f(1))
    r_next = p + momentum * (p - masked(p_old, f))
    assert p.dtype == f and r_next.dtype == f
    return p, r_next


def momenta(n_iter):
    """c_1 .. c_n of the sequence t_1 = 1, in float64."""
    t, out = 1.0, []
    for _ in range(n_iter):
        t_next = (1.0 + math.sqrt(1.0 + 4.0 * t * t)) / 2.0
        out.append((t - 1.0) / t_next)
        t = t_next
    return out


def prox(b, lam, n_iter=50, nonneg=False, dual=None, callback=None):
    """prox_{lam TV + C}(b) in float64 -> (x, p).  `callback(k, p)` sees every iterate."""
    b = np.asarray(b, dtype=np.float64)
    p = np.zeros((3,) + b.shape) if dual is None else masked(dual)
    if lam > 0:
        r = p
        for k, c in enumerate(momenta(n_iter)):
            p, r = step(b, r, p, lam, c, nonneg)
            if callback is not None:
                callback(k, p)
    return primal(b, p, lam, nonneg), p


def tv_exact(f):
    d = differences(f)
    return float(np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]).sum())


def primal_value(x, b, lam):
    """P(x) = 1/2 ||x - b||^2 + lam TV(x)."""
    x, b = np.asarray(x, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return 0.5 * float(((x - b) ** 2).sum()) + lam * tv_exact(x)


def dual_value(p, b, lam):
    """Dual(p) = 1/2 ||b||^2 - 1/2 ||b - lam D^T p||^2, the unconstrained prox's dual at a feasible p (|p[v]| <= 1)."""
    b = np.asarray(b, dtype=np.float64)
    return 0.5 * float((b * b).sum()) - 0.5 * float(((b - lam * adjoint(p)) ** 2).sum())


def gap(b, p, lam):
    """(P - Dual) / max(|P|, |Dual|) at x = b - lam D^T p."""
    P, Dl = primal_value(primal(b, p, lam), b, lam), dual_value(p, b, lam)
    return (P - Dl) / max(abs(P), abs(Dl)), P, Dl


def step_inputs(shape, seed=0):
    """(b, r, p_old) float32: b uniform in [-0.5, 1.5) so that `nonneg` bites, r and p_old uniform in [-1, 1) per component
    (inside and outside the unit ball), with NaN-free garbage of size 1e3 in the inert planes."""
    rng = np.random.default_rng(1000 * seed + sum(shape) + 7 * shape[0])
    b = (2.0 * rng.random(shape) - 0.5).astype(np.float32)
    r = (2.0 * rng.random((3,) + shape) - 1.0).astype(np.float32)
    p_old = (2.0 * rng.random((3,) + shape) - 1.0).astype(np.float32)
    for t in (r, p_old):
        t[0][0, :, :] = 1e3
        t[1][:, 0, :] = -1e3
        t[2][:, :, 0] = 1e3
    return b, r, p_old


def blocky(shape, seed=0, sigma=0.05):
    """A piecewise-constant volume (three nested boxes) plus sigma N(0, 1), float32."""
    rng = np.random.default_rng(seed)
    x = np.zeros(shape, dtype=np.float64)
    n = shape
    x[n[0] // 6:n[0] - n[0] // 6, n[1] // 6:n[1] - n[1] // 6, n[2] // 6:n[2] - n[2] // 6] = 0.5
    x[n[0] // 3:n[0] // 2, n[1] // 3:n[1] - n[1] // 3, n[2] // 4:n[2] // 2] = 1.0
    x[n[0] // 2:n[0] - n[0] // 4, n[1] // 4:n[1] // 2, n[2] // 2:n[2] - n[2] // 4] = 0.2
    return (x + sigma * rng.standard_normal(shape)).astype(np.float32)


# the duality-gap cases: (name, volume, lam, iterations).  The float64 oracle alone brings every one below GAP_BOUND within its
# count (tests/test_tvprox_cpu.py::test_duality_gap checks that); the GPU twin runs the same cases.
GAP_BOUND = 1e-3


def gap_cases():
    rng = np.random.default_rng(3)
    random = rng.random((12, 13, 14)).astype(np.float32)
    block = blocky((16, 15, 18))
    return [("random", random, 0.002, 10), ("random", random, 0.02, 30), ("random", random, 0.2, 200),
            ("blocky", block, 0.002, 10), ("blocky", block, 0.02, 30), ("blocky", block, 0.2, 200)]


def dense_case(rows=240, dims=(4, 5, 6), seed=0, dtype=np.float64):
    """A small dense random non-negative system for `fista_tv_operators`: (M, A, AT, b, x_true).  A third of M's entries are 0."""
    rng = np.random.default_rng(seed)
    n = int(np.prod(dims))
    M = (rng.random((rows, n)) * (rng.random((rows, n)) > 1 / 3)).astype(dtype)
    x_true = np.zeros(dims)
    x_true[1:3, 1:4, 2:5] = 1.0
    x_true[2:, 3:, :2] = 0.4
    b = (M.astype(np.float64) @ x_true.reshape(-1) + 0.05 * rng.standard_normal(rows)).astype(dtype)
    MT = np.ascontiguousarray(M.T)

    def A(x):
        return M @ x.reshape(-1)

    def AT(y):
        return (MT @ y).reshape(dims)

    return M, A, AT, b, x_true


def objective(A, R, b, x, lam):
    """F(x) = 1/2 ||A x - b||^2_R + lam TV(x) in float64."""
    res = np.asarray(A(x), dtype=np.float64) - np.asarray(b, dtype=np.float64)
    return 0.5 * float((np.asarray(R, dtype=np.float64) * res * res).sum()) + lam * tv_exact(x)
