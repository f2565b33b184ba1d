"""3-D total variation on the device: its value and gradient (`naf_tv_gradient`), normalised steepest descent on it
(`naf_tv_descent`), the regulariser step of the ASD-POCS baseline (`reconstruct.asd_pocs`), and its proximal map (`naf_tv_prox_step`,
`naf_tv_prox_primal`), the regulariser step of the FISTA-TV baseline (`reconstruct.fista_tv`), through libnaf_hip.so.

The definition is written down in include/naf_hip.h (V2) and DESIGN.md section 14: backward differences, m = sqrt(eps + |D f|^2),
TV = sum m, g = the exact gradient of that sum.  A descent step reads the volume twice and writes it once; the gradient is never
stored, and the whole run of steps is queued without returning to the host.  The proximal map is that of the exact isotropic TV
(no eps), include/naf_hip.h (V3) and DESIGN.md section 18: one launch per dual iteration of the fast gradient projection, the
momentum sequence formed on the host.  There is no CPU path, like the rest of the hot path.
"""
from __future__ import annotations

import math

import torch

from . import _abi

DEFAULT_EPS = 1e-8          # TIGRE's


def _check_eps(eps, who):
    eps = float(eps)
    if not (eps > 0.0) or not math.isfinite(eps):
        raise ValueError(f"{who}: eps must be > 0 and finite, got {eps}")
    return eps


def _buffers(x, lib):
    n1, n2, n3 = (int(v) for v in x.shape)
    ws = torch.empty(lib.naf_tv_workspace_bytes(n1, n2, n3), dtype=torch.uint8, device=x.device)
    stats = torch.empty(2, dtype=torch.float64, device=x.device)
    return (n1, n2, n3), ws, stats


def _overlap(a, b):
    """Whether the bytes of two contiguous tensors overlap, wholly or in part (a slice of a larger buffer next to another)."""
    a0, b0 = a.data_ptr(), b.data_ptr()
    return a0 < b0 + b.numel() * b.element_size() and b0 < a0 + a.numel() * a.element_size()


def tv_value_and_gradient(x, eps=DEFAULT_EPS, out=None):
    """TV(x) and its gradient for a CUDA float32 volume [n1, n2, n3] -> (float, float32 tensor of x's shape; `out` if given, which
    must not overlap x)."""
    value, _, out = _gradient_with_stats(x, eps, out)
    return value, out


def _gradient_with_stats(x, eps=DEFAULT_EPS, out=None):
    """`naf_tv_gradient` with both of its fp64 sums -> (TV, sum g^2, g)."""
    _abi.check_volume(x, "tv_value_and_gradient", "x")
    eps = _check_eps(eps, "tv_value_and_gradient")
    if min(x.shape) < 1:
        raise ValueError(f"tv_value_and_gradient: every extent of x must be at least 1, got shape {tuple(x.shape)}")
    if out is None:
        out = torch.empty_like(x)
    else:
        _abi.check_volume(out, "tv_value_and_gradient", "out")
        if out.shape != x.shape or out.device != x.device:
            raise ValueError(f"tv_value_and_gradient: out must be {tuple(x.shape)} on {x.device}, got {tuple(out.shape)} on {out.device}")
        if _overlap(out, x):
            raise ValueError("tv_value_and_gradient: out must not be x or overlap it")
    lib = _abi.lib()
    with torch.cuda.device(x.device):
        dims, ws, stats = _buffers(x, lib)
        _abi.check(lib.naf_tv_gradient(_abi.ptr(x), *dims, eps, _abi.ptr(out), _abi.ptr(stats), _abi.ptr(ws), ws.numel(),
                                       _abi.stream_ptr()), "tv_gradient")
        value, g2 = (float(v) for v in stats.tolist())
        return value, g2, out


def tv_descent(x, step, n_steps=20, eps=DEFAULT_EPS, scratch=None):
    """`n_steps` times x <- x - step * g(x) / ||g(x)||_2, in place on the CUDA float32 volume `x`.  `step` is a Python number (a
    kernel argument, not a device read), `scratch` an optional float32 volume of x's shape to alternate with (its contents are
    lost; it must not overlap x).  Returns (TV, ||g||_2) of the volume before the last step; (nan, nan) for n_steps == 0, which touches nothing."""
    _abi.check_volume(x, "tv_descent", "x")
    if isinstance(step, torch.Tensor) or not isinstance(step, (int, float)) or isinstance(step, bool):
        raise TypeError(f"tv_descent: step must be a Python float, got {type(step).__name__}")
    step = float(step)
    if not math.isfinite(step) or step < 0.0:
        raise ValueError(f"tv_descent: step must be >= 0 and finite, got {step}")
    n_steps = int(n_steps)
    if n_steps < 0:
        raise ValueError(f"tv_descent: n_steps must be >= 0, got {n_steps}")
    eps = _check_eps(eps, "tv_descent")
    if min(x.shape) < 1:
        raise ValueError(f"tv_descent: every extent of x must be at least 1, got shape {tuple(x.shape)}")
    if scratch is not None:
        _abi.check_volume(scratch, "tv_descent", "scratch")
        if scratch.shape != x.shape or scratch.device != x.device:
            raise ValueError(f"tv_descent: scratch must be {tuple(x.shape)} on {x.device}, got {tuple(scratch.shape)} on {scratch.device}")
        if _overlap(scratch, x):
            raise ValueError("tv_descent: scratch must not be x or overlap it")
    if n_steps == 0:
        return math.nan, math.nan
    lib = _abi.lib()
    with torch.cuda.device(x.device):
        if scratch is None:
            scratch = torch.empty_like(x)
        dims, ws, stats = _buffers(x, lib)
        _abi.check(lib.naf_tv_descent(_abi.ptr(x), _abi.ptr(scratch), *dims, step, n_steps, eps, _abi.ptr(stats), _abi.ptr(ws),
                                      ws.numel(), _abi.stream_ptr()), "tv_descent")
        tv, g2 = (float(v) for v in stats.tolist())
        return tv, math.sqrt(g2) if g2 >= 0 else math.nan


def prox_momenta(n_iter):
    """The momentum c_k = (t_k - 1) / t_{k+1} of each of `n_iter` dual iterations, t_1 = 1, t_{k+1} = (1 + sqrt(1 + 4 t_k^2)) / 2,
    in float64 (the kernel argument is rounded to fp32 once)."""
    t, out = 1.0, []
    for _ in range(int(n_iter)):
        t_next = (1.0 + math.sqrt(1.0 + 4.0 * t * t)) / 2.0
        out.append((t - 1.0) / t_next)
        t = t_next
    return out


def tv_prox(b, lam, n_iter=50, nonneg=False, dual=None, return_dual=False):
    """prox_{lam TV + C}(b) = argmin_x 1/2 ||x - b||^2 + lam TV(x) (over x >= 0 with `nonneg`) of a CUDA float32 volume
    [n1, n2, n3], TV the exact isotropic total variation -> a new tensor of b's shape; (x, dual) with `return_dual`.  `n_iter`
    iterations of the fast gradient projection on the dual variable [3, n1, n2, n3], from zeros or from `dual` (a warm start: the
    dual a previous call returned).  With `return_dual` a given `dual` is advanced in place and is the tensor returned; without,
    it is copied and left as it is.  `n_iter` step launches and one primal launch are queued, nothing is
    read back; `lam == 0` or `n_iter == 0` launches the primal only."""
    who = "tv_prox"
    _abi.check_volume(b, who, "b")
    if isinstance(lam, torch.Tensor) or not isinstance(lam, (int, float)) or isinstance(lam, bool):
        raise TypeError(f"{who}: lam must be a Python float, got {type(lam).__name__}")
    lam = float(lam)
    if not math.isfinite(lam) or lam < 0.0:
        raise ValueError(f"{who}: lam must be >= 0 and finite, got {lam}")
    n_iter = int(n_iter)
    if n_iter < 0:
        raise ValueError(f"{who}: n_iter must be >= 0, got {n_iter}")
    if min(b.shape) < 1:
        raise ValueError(f"{who}: every extent of b must be at least 1, got shape {tuple(b.shape)}")
    if dual is not None:
        if not isinstance(dual, torch.Tensor) or not dual.is_cuda:
            raise RuntimeError(f"{who}: dual must be a CUDA/HIP tensor (no CPU path)")
        if dual.dtype != torch.float32:
            raise TypeError(f"{who}: dual must be float32, got {dual.dtype}")
        if tuple(dual.shape) != (3, *b.shape) or dual.device != b.device:
            raise ValueError(f"{who}: dual must be {(3, *b.shape)} on {b.device}, got {tuple(dual.shape)} on {dual.device}")
        if not dual.is_contiguous():
            raise ValueError(f"{who}: dual must be contiguous")
        if _overlap(dual, b):
            raise ValueError(f"{who}: dual must not overlap b")
    lib = _abi.lib()
    dims = tuple(int(v) for v in b.shape)
    flag = int(bool(nonneg))
    with torch.cuda.device(b.device):
        p = torch.zeros((3, *dims), dtype=torch.float32, device=b.device) if dual is None else (dual if return_dual else dual.clone())
        if lam > 0.0 and n_iter > 0:
            # r_1 = p_0; the extrapolated point alternates between two buffers, because a step reads it at neighbours
            r, r_next = p.clone(), (torch.empty_like(p) if n_iter > 1 else None)
            for k, c in enumerate(prox_momenta(n_iter)):
                last = k == n_iter - 1
                _abi.check(lib.naf_tv_prox_step(_abi.ptr(b), _abi.ptr(r), _abi.ptr(p), None if last else _abi.ptr(r_next), *dims, lam,
                                                c, flag, _abi.stream_ptr()), "tv_prox_step")
                r, r_next = r_next, r
        x = torch.empty_like(b)
        _abi.check(lib.naf_tv_prox_primal(_abi.ptr(b), _abi.ptr(p), _abi.ptr(x), *dims, lam, flag, _abi.stream_ptr()), "tv_prox_primal")
    return (x, p) if return_dual else x
