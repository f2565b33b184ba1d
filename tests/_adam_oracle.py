"""torch.optim.Adam (no weight decay, no amsgrad) for ONE step in float64, with the magnitudes its error bounds need (not a test module).

The fp32 arrays and the fp32 values of the hyper-parameters are the exact inputs: everything is widened to float64 first and no
intermediate is rounded to fp32, the bias corrections are formed in double (as torch and make_adam_args do).

Bounds for an fp32 implementation, u = 2^-24 (counted on adam_math.h, each count doubled):
  m:  1 - beta1 in fp32, the gradient scale, the subtraction, the product, the addition          -> |m - m64| <= 8 u A_m
  v:  1 - beta2 in fp32, the scale, three products, the addition                                 -> |v - v64| <= 8 u A_v
  p:  the final subtraction rounds once relative to p; every other rounding (m's, half of v's under the square root, the square
      root, the host-rounded bias terms, the division(s), the product) is relative to the update -> |p - p64| <= u |p64| + K u U
      K = 16 for correctly rounded sqrt and divisions, 32 for the hardware sqrt and reciprocal (1 ulp = 2 u each, plus the
      host-rounded reciprocal of the bias term).
with A_m = |m0| + (1 - beta1) |gs - m0|, A_v = beta2 v0 + (1 - beta2) gs^2, U = step_size A_m / denom, gs = g * grad_scale.
"""
import numpy as np

U24 = 2.0 ** -24


def step(p, m, v, g, lr, beta1, beta2, eps, step, grad_scale=1.0):
    """-> dict(p, m, v, A_m, A_v, U) of float64 arrays."""
    p, m, v, g = (np.asarray(t, dtype=np.float64) for t in (p, m, v, g))
    lr, beta1, beta2, eps, grad_scale = (float(np.float32(t)) for t in (lr, beta1, beta2, eps, grad_scale))
    gs = g * grad_scale
    m1 = m + (gs - m) * (1.0 - beta1)
    v1 = v * beta2 + (1.0 - beta2) * gs * gs
    bias1 = 1.0 - beta1 ** step
    bias2_sqrt = np.sqrt(1.0 - beta2 ** step)
    step_size = lr / bias1
    denom = np.sqrt(v1) / bias2_sqrt + eps
    p1 = p - step_size * (m1 / denom)
    A_m = np.abs(m) + (1.0 - beta1) * np.abs(gs - m)
    A_v = beta2 * v + (1.0 - beta2) * gs * gs
    return {"p": p1, "m": m1, "v": v1, "A_m": A_m, "A_v": A_v, "U": step_size * A_m / denom}


def bounds(ref, K):
    """-> (bound_p, bound_m, bound_v) for an fp32 implementation; K = 16 (exact form) or 32 (hardware sqrt and reciprocal)."""
    return U24 * np.abs(ref["p"]) + K * U24 * ref["U"], 8 * U24 * ref["A_m"], 8 * U24 * ref["A_v"]


def states(n, seed):
    """(p, m, v, g) float32 [n] that the GPU test and the CPU validation share: a random state with v >= 0 in the first half, a state
    three steps into a real trajectory in the second; gradient magnitudes spread over 1e-12 .. 1e12 with exact zeros; every 7th
    element has m = v = g = 0."""
    rng = np.random.default_rng(seed)
    p = rng.standard_normal(n).astype(np.float32)
    m = (rng.standard_normal(n) * 0.1).astype(np.float32)
    v = (rng.standard_normal(n) ** 2 * 0.01).astype(np.float32)
    half = n // 2
    if n - half > 0:                                                            # a real trajectory: three default steps from zero moments
        q, mm, vv = p[half:].astype(np.float64), np.zeros(n - half), np.zeros(n - half)
        for t in range(1, 4):
            r = step(q, mm, vv, rng.standard_normal(n - half).astype(np.float32), 1e-3, 0.9, 0.999, 1e-8, t)
            q, mm, vv = r["p"], r["m"], r["v"]
        p[half:], m[half:], v[half:] = q, mm, vv
    g = (rng.standard_normal(n) * 10.0 ** rng.uniform(-12, 12, n)).astype(np.float32)
    g[rng.random(n) < 0.1] = 0.0
    dead = np.arange(n) % 7 == 3
    m[dead], v[dead], g[dead] = 0.0, 0.0, 0.0
    return p, m, v, g


HYPER = {"default": (1e-3, 0.9, 0.999, 1e-8), "other": (3e-2, 0.5, 0.9, 1e-3)}
GRAD_SCALES = (1.0, 1.0 / 128, 0.37)
STEPS = (1, 2, 1000, 75000)
