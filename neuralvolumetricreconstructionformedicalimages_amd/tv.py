"""3-D total variation on the device: its value and gradient (`naf_tv_gradient`) and normalised steepest descent on it
(`naf_tv_descent`), the regulariser step of the ASD-POCS baseline (`reconstruct.asd_pocs`), through libnaf_hip.so.

The definition is written down in include/naf_hip.h (V2) and DESIGN.md section 14: backward differences, m = sqrt(eps + |D f|^2),
TV = sum m, g = the exact gradient of that sum.  A descent step reads the volume twice and writes it once; the gradient is never
stored, and the whole run of steps is queued without returning to the host.  There is no CPU path, like the rest of the hot path.
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
