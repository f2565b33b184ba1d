"""naf_adam_step pinned to torch's Adam in float64 (tests/_adam_oracle.py), one step from a given state at a time.

Single steps accumulate no error, so every bound is the derived one of _adam_oracle.bounds (validated on the CPU against an fp32
restatement of adam_math.h in test_adam_oracle_cpu.py): both moments as well as the parameter, the exact form (no shadow) and the
form with hardware sqrt and reciprocal that every 16-bit shadow table uses, non-default hyper-parameters, gradient scales, late
steps, zero_grad on and off, the ragged head of fewer than four elements at any alignment, and guards behind every buffer."""
import numpy as np
import pytest
import torch

import _adam_oracle as O

pytestmark = pytest.mark.gpu

LP = {"none": None, "fp16": torch.float16, "bf16": torch.bfloat16}
GUARD, GUARD_VALUE = 8, -3.5
INVALID_ARGUMENT = -1


def _abi():
    from neuralvolumetricreconstructionformedicalimages_amd import _abi as A
    return A


class _Buf:
    """A device buffer of n elements `offset` elements into its allocation, with GUARD elements behind it."""

    def __init__(self, host, offset, dtype=torch.float32):
        n = host.numel()
        self.all = torch.full((offset + n + GUARD,), GUARD_VALUE, device="cuda", dtype=dtype)
        self.t = self.all[offset:offset + n]
        self.t.copy_(host)
        self.offset, self.n = offset, n

    def guards_intact(self):
        a = self.all.cpu()
        return bool((a[:self.offset] == GUARD_VALUE).all()) and bool((a[self.offset + self.n:] == GUARD_VALUE).all())


def _run(A, state, lp, hyper, step, grad_scale, zero_grad, offset_bytes=0):
    """One naf_adam_step on copies of `state` -> (rc, p, m, v, g, shadow) as host tensors, after checking the guards."""
    lr, b1, b2, eps = hyper
    p0, m0, v0, g0 = (torch.from_numpy(t) for t in state)
    n = p0.numel()
    bufs = [_Buf(t, offset_bytes // 4) for t in (p0, m0, v0, g0)]
    shadow = _Buf(torch.zeros(n, dtype=lp), offset_bytes // 2, lp) if lp is not None else None
    rc = A.lib().naf_adam_step(*(A.ptr(b.t) for b in bufs), A.ptr(shadow.t) if shadow else None, A.dtype_code(lp) if lp else 0, n,
                               lr, b1, b2, eps, step, grad_scale, int(zero_grad), A.stream_ptr())
    torch.cuda.synchronize()
    for name, b in zip(("param", "exp_avg", "exp_avg_sq", "grad", "shadow"), bufs + ([shadow] if shadow else [])):
        assert b.guards_intact(), f"{name}: written outside its {n} elements"
    return (rc, *(b.t.cpu() for b in bufs), shadow.t.cpu() if shadow else None)


def _check(A, state, lp_name, hyper, step, grad_scale, zero_grad=True, offset_bytes=0):
    lp = LP[lp_name]
    rc, p, m, v, g, shadow = _run(A, state, lp, hyper, step, grad_scale, zero_grad, offset_bytes)
    A.check(rc, "naf_adam_step")
    p0, m0, v0, g0 = state
    ref = O.step(p0, m0, v0, g0, *hyper, step, grad_scale)
    bp, bm, bv = O.bounds(ref, 16 if lp is None else 32)
    what = f"n={p0.size} {lp_name} lr={hyper[0]} step={step} scale={grad_scale:.4g}"
    for name, got, b in (("m", m, bm), ("v", v, bv), ("p", p, bp)):
        err = np.abs(got.double().numpy() - ref[name])
        with np.errstate(invalid="ignore", divide="ignore"):
            print(f"{what}: {name} uses {np.nanmax(np.where(b > 0, err / b, 0.0)):.3f} of its bound")
        assert np.all(err <= b), f"{what}: {name}: {int((err > b).sum())} of {err.size} elements outside the bound"
    dead = (m0 == 0) & (v0 == 0) & (g0 == 0)
    assert np.array_equal(p.numpy()[dead].view(np.uint32), p0[dead].view(np.uint32))          # no update, no NaN from 0 / eps
    assert not m.numpy()[dead].any() and not v.numpy()[dead].any()
    if zero_grad:
        assert np.array_equal(g.numpy().view(np.uint32), np.zeros(g0.size, np.uint32))         # exact (positive) zeros
    else:
        assert np.array_equal(g.numpy().view(np.uint32), g0.view(np.uint32))
    if lp is not None:
        assert torch.equal(shadow.view(torch.int16), p.to(lp).view(torch.int16)), f"{what}: shadow != round(p)"


@pytest.mark.parametrize("step", O.STEPS)
@pytest.mark.parametrize("grad_scale", O.GRAD_SCALES, ids=["1", "1/128", "0.37"])
@pytest.mark.parametrize("hyper", list(O.HYPER))
@pytest.mark.parametrize("lp", list(LP))
def test_single_step_against_float64(lp, hyper, grad_scale, step):
    """n = 10007: several blocks, a scalar tail of three elements."""
    _check(_abi(), O.states(10007, step), lp, O.HYPER[hyper], step, grad_scale, zero_grad=(step != 2))


@pytest.mark.parametrize("n", [4, 5, 1023])
@pytest.mark.parametrize("lp", list(LP))
def test_sizes_around_the_vector_width(lp, n):
    A = _abi()
    _check(A, O.states(n, n), lp, O.HYPER["default"], 3, 0.37)
    _check(A, O.states(n, n + 1), lp, O.HYPER["other"], 1000, 1.0, zero_grad=False)


@pytest.mark.parametrize("n", [1, 2, 3])
@pytest.mark.parametrize("lp", list(LP))
def test_ragged_head_at_any_alignment(lp, n):
    """Fewer than four elements take the scalar tail of the kernel: every pointer 4 bytes into its allocation."""
    A = _abi()
    p, m, v, g = O.states(8, 20 + n)
    for first in (0, 3):                                       # element 3 has m = v = g = 0
        state = tuple(t[first:first + n].copy() for t in (p, m, v, g))
        _check(A, state, lp, O.HYPER["default"], 2, 1.0 / 128, offset_bytes=4)
        _check(A, state, lp, O.HYPER["other"], 75000, 1.0, zero_grad=False, offset_bytes=4)


@pytest.mark.parametrize("lp", list(LP))
def test_misaligned_vector_body_is_refused_and_writes_nothing(lp):
    A = _abi()
    state = O.states(5, 9)
    rc, p, m, v, g, shadow = _run(A, state, LP[lp], O.HYPER["default"], 1, 1.0, True, offset_bytes=4)
    assert rc == INVALID_ARGUMENT and b"16-byte aligned" in A.lib().naf_last_error()
    for got, before in zip((p, m, v, g), state):
        assert np.array_equal(got.numpy().view(np.uint32), before.view(np.uint32))
    if shadow is not None:
        assert not shadow.view(torch.int16).any()
