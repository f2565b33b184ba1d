"""tests/_adam_oracle.py validated on the CPU: the float64 step is torch.optim.Adam on float64 tensors, and an fp32 restatement of
adam_math.h, rounding by rounding in numpy, stays inside the bounds the HIP kernel is held to."""
import numpy as np
import pytest
import torch

import _adam_oracle as O

f32 = np.float32
CASES = [(h, gs, st) for h in O.HYPER for gs in O.GRAD_SCALES for st in O.STEPS]


@pytest.mark.parametrize("hyper,grad_scale,step", CASES)
def test_step_is_torch_adam_in_float64(hyper, grad_scale, step):
    lr, b1, b2, eps = (float(f32(t)) for t in O.HYPER[hyper])
    p0, m0, v0, g = O.states(1023, step)
    ref = O.step(p0, m0, v0, g, lr, b1, b2, eps, step, grad_scale)
    p = torch.from_numpy(p0).double().requires_grad_(True)
    opt = torch.optim.Adam([p], lr=lr, betas=(b1, b2), eps=eps)
    m, v = torch.from_numpy(m0).double(), torch.from_numpy(v0).double()
    opt.state[p] = {"step": torch.tensor(float(step - 1)), "exp_avg": m, "exp_avg_sq": v}
    p.grad = torch.from_numpy(g).double() * float(f32(grad_scale))
    opt.step()
    assert float(opt.state[p]["step"]) == step
    # relative to the magnitude each result is formed from (a moment that cancels to nothing has no relative accuracy of its own)
    assert np.all(np.abs(p.detach().numpy() - ref["p"]) <= 1e-13 * np.abs(ref["p"]))
    assert np.all(np.abs(m.numpy() - ref["m"]) <= 1e-13 * ref["A_m"])
    assert np.all(np.abs(v.numpy() - ref["v"]) <= 1e-13 * ref["A_v"])
    dead = (m0 == 0) & (v0 == 0) & (g == 0)
    assert dead.any() and np.array_equal(ref["p"][dead], p0[dead].astype(np.float64)) and not ref["m"][dead].any()


def _fma(a, b, c):
    """fp32 fma through float64 (the product of two fp32 is exact there)."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(f32)


def _adam_fp32(p, m, v, g, lr, b1, b2, eps, step, grad_scale, fast):
    """adam_one of adam_math.h with make_adam_args of adam.hip, every operation rounded to fp32 (sqrt and reciprocal correctly
    rounded: no worse than the hardware's 1 ulp)."""
    lr, b1, b2, eps, gs = f32(lr), f32(b1), f32(b2), f32(eps), f32(grad_scale)
    bias1 = f32(1.0 - float(b1) ** step)
    bias2_sqrt = f32(np.sqrt(1.0 - float(b2) ** step))
    one = f32(1.0)
    g = g * gs
    if fast:
        step_size, inv = lr / bias1, one / bias2_sqrt
        m = _fma(g - m, np.full_like(m, one - b1), m)
        v = _fma((one - b2) * g, g, v * b2)
        denom = _fma(np.sqrt(v), np.full_like(v, inv), np.full_like(v, eps))
        p = _fma(-step_size * m, one / denom, p)
    else:
        m = m + (g - m) * (one - b1)
        v = v * b2 + (one - b2) * g * g
        denom = np.sqrt(v) / bias2_sqrt + eps
        p = p - (lr / bias1) * (m / denom)
    assert p.dtype == m.dtype == v.dtype == f32
    return p, m, v


@pytest.mark.parametrize("fast", [False, True])
@pytest.mark.parametrize("hyper,grad_scale,step", CASES)
def test_an_fp32_restatement_of_the_kernel_is_inside_the_bounds(hyper, grad_scale, step, fast):
    lr, b1, b2, eps = O.HYPER[hyper]
    p0, m0, v0, g = O.states(10007, 100 + step)
    ref = O.step(p0, m0, v0, g, lr, b1, b2, eps, step, grad_scale)
    p, m, v = _adam_fp32(p0, m0, v0, g, lr, b1, b2, eps, step, grad_scale, fast)
    bp, bm, bv = O.bounds(ref, 32 if fast else 16)
    with np.errstate(invalid="ignore", divide="ignore"):
        used = [np.nanmax(np.abs(x - ref[k]) / b) for x, k, b in ((p, "p", bp), (m, "m", bm), (v, "v", bv))]
    print(f"fractions of the bounds used: p {used[0]:.3f}, m {used[1]:.3f}, v {used[2]:.3f}")
    assert np.all(np.abs(p - ref["p"]) <= bp)
    assert np.all(np.abs(m - ref["m"]) <= bm)
    assert np.all(np.abs(v - ref["v"]) <= bv)


def test_the_bounds_notice_a_wrong_update():
    """grad_scale ignored, or the second moment decayed with beta1: far outside."""
    lr, b1, b2, eps = O.HYPER["default"]
    p0, m0, v0, g = O.states(1023, 5)
    ref = O.step(p0, m0, v0, g, lr, b1, b2, eps, 2, 0.37)
    _, bm, bv = O.bounds(ref, 16)
    _, m, _ = _adam_fp32(p0, m0, v0, g, lr, b1, b2, eps, 2, 1.0, False)
    assert np.mean(np.abs(m - ref["m"]) > bm) > 0.5
    _, _, v = _adam_fp32(p0, m0, v0, g, lr, b1, b1, eps, 2, 0.37, False)
    assert np.mean(np.abs(v - ref["v"]) > bv) > 0.5
