"""The vector half of a CGLS iteration through libnaf_hip.so (`naf_cgls_wdot`, `naf_cgls_residual_step`,
`naf_cgls_direction_step`; include/naf_hip.h K1).

    wdot            scalars[slot] = sum w a^2 (fp64, fixed order, no atomics)
    residual_step   history[k] = sum w r^2;  r -= alpha q;  y = w r          alpha = gamma / delta
    direction_step  x += alpha p;  p = s + beta p                             beta = gamma' / gamma

The scalars stay on the device in a `Workspace`; `reconstruct.cgls` is the solver on top, with `projector.project_scan` and
`sart.backproject_scan` as A and A^T.  (The module is not called `cgls` because the package exports the solver under that name.)  There is no CPU fallback, like the rest of the hot path.
"""
from __future__ import annotations

import torch

from . import _abi

# Layout of `Workspace.scalars` (float64), as include/naf_hip.h K1 fixes it
SLOT_GAMMA = (0, 1)         # gamma of iteration k is in SLOT_GAMMA[k & 1], gamma' in SLOT_GAMMA[(k + 1) & 1]
SLOT_DELTA = 2
SLOT_STOPPED = 3            # 0 while running, k + 1 once iteration k was a breakdown
HISTORY = 8                 # scalars[HISTORY + k] = sum w r^2 of the residual iteration k was given


class Workspace:
    """Device memory of one solve: the fp64 scalars, the history of `n_iter_max` iterations and the per-workgroup partial sums for
    arrays of up to `n_max` elements.  `scalars` is a float64 view of its head with the layout above, which a test may write
    (gamma, delta, the stop mark) and a solver reads back once at the end; a fresh workspace is all zeros (`reset`)."""

    def __init__(self, n_max, n_iter_max, device):
        self.n_max, self.n_iter_max = int(n_max), int(n_iter_max)
        if self.n_max < 0 or self.n_iter_max < 0:
            raise ValueError(f"cgls_kernels.Workspace: n_max and n_iter_max must be >= 0, got {n_max} and {n_iter_max}")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("cgls_kernels.Workspace: device must be a CUDA/HIP device (no CPU path)")
        with torch.cuda.device(self.device):
            self.device = torch.device("cuda", torch.cuda.current_device())
            nbytes = _abi.lib().naf_cgls_workspace_bytes(self.n_max, self.n_iter_max)
            self.buffer = torch.zeros(nbytes // 8, dtype=torch.float64, device=self.device)
        self.scalars = self.buffer[:HISTORY + self.n_iter_max]

    def reset(self):
        self.buffer.zero_()

    @property
    def nbytes(self):
        return self.buffer.numel() * 8

    def history(self):
        """sum w r^2 per iteration, float64 [n_iter_max] (a view)."""
        return self.scalars[HISTORY:]

    def stopped_at(self):
        """The iteration that met a breakdown, or None; a device read."""
        mark = int(self.scalars[SLOT_STOPPED].item())
        return mark - 1 if mark > 0 else None


def _check_array(t, who, name, like=None):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"{who}: {name} must be a CUDA/HIP tensor (no CPU path)")
    if t.dtype != torch.float32:
        raise TypeError(f"{who}: {name} must be float32, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{who}: {name} must be contiguous")
    if like is not None and (t.shape != like.shape or t.device != like.device):
        raise ValueError(f"{who}: {name} must have the shape {tuple(like.shape)} and device of the other arrays, got "
                         f"{tuple(t.shape)} on {t.device}")


def _overlap(a, b):
    a0, b0 = a.data_ptr(), b.data_ptr()
    return a0 < b0 + b.numel() * b.element_size() and b0 < a0 + a.numel() * a.element_size()


def _check_workspace(ws, first, who, k=None):
    if not isinstance(ws, Workspace):
        raise TypeError(f"{who}: ws must be a cgls_kernels.Workspace, got {type(ws).__name__}")
    if ws.device != first.device:
        raise ValueError(f"{who}: the workspace is on {ws.device}, the arrays on {first.device}")
    if first.numel() > ws.n_max:
        raise ValueError(f"{who}: the workspace was made for up to {ws.n_max} elements, got {first.numel()}")
    if k is not None:
        if isinstance(k, bool) or not isinstance(k, int):
            raise TypeError(f"{who}: k must be an int, got {type(k).__name__}")
        if not (0 <= k < ws.n_iter_max):
            raise ValueError(f"{who}: k must be in [0, {ws.n_iter_max}) for this workspace, got {k}")


def wdot(a, w, slot, ws):
    """ws.scalars[slot] = sum w a^2 in fp64 (`w=None`: sum a^2) for float32 arrays of one shape; `slot` is one of SLOT_GAMMA or
    SLOT_DELTA.  Nothing is read back.  An empty array is a no-op: the slot keeps its value."""
    who = "cgls_kernels.wdot"
    _check_array(a, who, "a")
    if w is not None:
        _check_array(w, who, "w", a)
    _check_workspace(ws, a, who)
    if isinstance(slot, bool) or not isinstance(slot, int) or slot not in (*SLOT_GAMMA, SLOT_DELTA):
        raise ValueError(f"{who}: slot must be SLOT_GAMMA[0], SLOT_GAMMA[1] or SLOT_DELTA, got {slot!r}")
    with torch.cuda.device(a.device):
        _abi.check(_abi.lib().naf_cgls_wdot(_abi.ptr(a), _abi.ptr(w), a.numel(), slot, ws.n_iter_max, _abi.ptr(ws.buffer), ws.nbytes,
                                            _abi.stream_ptr()), "cgls_wdot")


def residual_step(r, q, w, y, k, ws):
    """Iteration k's projection-space pass, in place: ws.history()[k] = sum w r^2, then r -= alpha q and y = w r (`w=None`: y = r),
    alpha = gamma / delta from the workspace; a breakdown (gamma or delta not > 0) or an earlier stop leaves r as it is and sets
    the stop mark -> y."""
    who = "cgls_kernels.residual_step"
    _check_array(r, who, "r")
    _check_array(q, who, "q", r)
    _check_array(y, who, "y", r)
    if w is not None:
        _check_array(w, who, "w", r)
    _check_workspace(ws, r, who, k)
    if _overlap(y, q) or _overlap(y, r) or _overlap(r, q) or (w is not None and (_overlap(w, y) or _overlap(w, r))):
        raise ValueError(f"{who}: y must not be q or r, and r, q, w and y must not overlap")
    with torch.cuda.device(r.device):
        _abi.check(_abi.lib().naf_cgls_residual_step(_abi.ptr(r), _abi.ptr(q), _abi.ptr(w), _abi.ptr(y), r.numel(), k, ws.n_iter_max,
                                                     _abi.ptr(ws.buffer), ws.nbytes, _abi.stream_ptr()), "cgls_residual_step")
    return y


def direction_step(x, p, s, k, ws):
    """Iteration k's volume-space pass, in place: x += alpha p, p = s + beta p, beta = gamma' / gamma with gamma' in the other
    gamma slot; a stopped iteration leaves x and p as they are -> x."""
    who = "cgls_kernels.direction_step"
    _check_array(x, who, "x")
    _check_array(p, who, "p", x)
    _check_array(s, who, "s", x)
    _check_workspace(ws, x, who, k)
    if _overlap(x, p) or _overlap(x, s) or _overlap(p, s):
        raise ValueError(f"{who}: x, p and s must not overlap")
    with torch.cuda.device(x.device):
        _abi.check(_abi.lib().naf_cgls_direction_step(_abi.ptr(x), _abi.ptr(p), _abi.ptr(s), x.numel(), k, ws.n_iter_max,
                                                      _abi.ptr(ws.buffer), ws.nbytes, _abi.stream_ptr()), "cgls_direction_step")
    return x
