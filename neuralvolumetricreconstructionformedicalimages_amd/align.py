"""Reprojection alignment of projections through libnaf_hip.so (`naf_align_shift_scores`, `naf_align_peak`,
`naf_align_shift_views`; include/naf_hip.h A1).

Views are float32 [N, H, W] on the GPU, u along the last axis and v along the rows.  A view's shift is (du, dv) in pixels, stored as
`shifts[N, 2] = (du, dv)`, and the measured view b is the ideal view p translated by +shift: b[n](r, c) ~ p[n](r - dv, c - du).

    shift_scores      S[n, j, i] = sum w (b[n, r + j - Rv, c + i - Ru] - p[n, r, c])^2 over the fixed interior window, fp64
    estimate_shifts   the sub-pixel argmin of every view's table -> (shifts, flags)
    shift_views       out[n](r, c) = views[n](r + dv_n, c + du_n), cubic convolution, clamp-to-edge: undoes a view's shift

Everything stays on the device and nothing is read back; `reconstruct.align_projections` is the loop on top.  `max_shift` is an int
(both axes) or the pair (Ru, Rv).  There is no CPU fallback, like the rest of the hot path.
"""
from __future__ import annotations

import torch

from . import _abi

MAX_SHIFT = 16                      # NAF_ALIGN_MAX_SHIFT
FLAG_BORDER, FLAG_NON_FINITE = 1, 2


def window(max_shift, H, W, who="align"):
    """`max_shift` -> (Rv, Ru) for views of H x W: 0 <= R <= 16 and 2 R < extent on each axis, else ValueError."""
    if isinstance(max_shift, (tuple, list)):
        if len(max_shift) != 2:
            raise ValueError(f"{who}: max_shift must be an int or (Ru, Rv), got {max_shift!r}")
        Ru, Rv = max_shift
    else:
        Ru = Rv = max_shift
    for R in (Ru, Rv):
        if isinstance(R, bool) or not isinstance(R, int):
            raise ValueError(f"{who}: max_shift must be an int or a pair of ints, got {max_shift!r}")
    if not (0 <= Ru <= MAX_SHIFT and 0 <= Rv <= MAX_SHIFT):
        raise ValueError(f"{who}: max_shift must be in [0, {MAX_SHIFT}] on each axis, got (Ru, Rv) = ({Ru}, {Rv})")
    if 2 * Rv >= H or 2 * Ru >= W:
        raise ValueError(f"{who}: the search window needs 2 R < extent on each axis, got (Ru, Rv) = ({Ru}, {Rv}) for views of "
                         f"{H} x {W}")
    return Rv, Ru


def _check_views(t, who, name, like=None):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise ValueError(f"{who}: {name} must be a CUDA/HIP tensor (no CPU path)")
    if t.dtype != torch.float32 or t.dim() != 3 or 0 in t.shape[1:]:
        raise ValueError(f"{who}: {name} must be float32 [N, H, W], got {t.dtype} {tuple(t.shape)}")
    if not t.is_contiguous():
        raise ValueError(f"{who}: {name} must be contiguous")
    if like is not None and (t.shape != like.shape or t.device != like.device):
        raise ValueError(f"{who}: {name} must have the shape {tuple(like.shape)} and device of the other views, got "
                         f"{tuple(t.shape)} on {t.device}")


def _check_array(t, dtype, shape, like, who, name):
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.device != like.device:
        raise ValueError(f"{who}: {name} must be a CUDA/HIP tensor on the device of the views")
    if t.dtype != dtype or tuple(t.shape) != tuple(shape) or not t.is_contiguous():
        raise ValueError(f"{who}: {name} must be contiguous {dtype} {tuple(shape)}, got {t.dtype} {tuple(t.shape)}")


def scores_workspace(N, H, W, max_shift, device):
    """The scratch of `shift_scores` for up to N views of H x W searched over `max_shift`: a float64 device tensor of the per-tile
    partial sums.  A larger one serves as well and changes no bit."""
    Rv, Ru = window(max_shift, int(H), int(W), "align.scores_workspace")
    if int(N) < 0:
        raise ValueError(f"align.scores_workspace: N must be >= 0, got {N}")
    device = torch.device(device)
    if device.type != "cuda":
        raise ValueError("align.scores_workspace: device must be a CUDA/HIP device (no CPU path)")
    nbytes = _abi.lib().naf_align_scores_workspace_bytes(int(N), int(H), int(W), Rv, Ru)
    if int(N) > 0 and nbytes == 0:
        raise ValueError(f"align.scores_workspace: {N} views of {H} x {W} are too many tiles for one call")
    return torch.empty(max(nbytes // 8, 1), dtype=torch.float64, device=device)


def shift_scores(measured, reprojected, max_shift, weights=None, workspace=None, out=None):
    """Scores of every integer translation in the window of `max_shift` of `measured` [N, H, W] against `reprojected` -> float64
    [N, 2 Rv + 1, 2 Ru + 1]; entry [n, j, i] is the translation dv = j - Rv, du = i - Ru.  `weights` (float32 [N, H, W], None for all
    ones) weighs the squared differences by the pixel of `reprojected` they belong to.  `workspace` is `scores_workspace(...)` for at
    least these shapes (default: made here)."""
    who = "align.shift_scores"
    _check_views(measured, who, "measured")
    _check_views(reprojected, who, "reprojected", measured)
    if weights is not None:
        _check_views(weights, who, "weights", measured)
    N, H, W = measured.shape
    Rv, Ru = window(max_shift, H, W, who)
    shape = (N, 2 * Rv + 1, 2 * Ru + 1)
    lib = _abi.lib()
    need = lib.naf_align_scores_workspace_bytes(N, H, W, Rv, Ru)
    if N > 0 and need == 0:
        raise ValueError(f"{who}: {N} views of {H} x {W} are too many tiles for one call")
    if workspace is None:
        workspace = torch.empty(max(need // 8, 1), dtype=torch.float64, device=measured.device)
    else:
        if (not isinstance(workspace, torch.Tensor) or workspace.device != measured.device or workspace.dtype != torch.float64
                or not workspace.is_contiguous()):
            raise ValueError(f"{who}: workspace must be a contiguous float64 tensor on the views' device (align.scores_workspace)")
        if workspace.numel() * 8 < need:
            raise ValueError(f"{who}: workspace too small ({workspace.numel() * 8} bytes, need {need})")
    if out is None:
        out = torch.empty(shape, dtype=torch.float64, device=measured.device)
    else:
        _check_array(out, torch.float64, shape, measured, who, "out")
    with torch.cuda.device(measured.device):
        _abi.check(lib.naf_align_shift_scores(_abi.ptr(measured), _abi.ptr(reprojected), _abi.ptr(weights), N, H, W, Rv, Ru,
                                              _abi.ptr(workspace), workspace.numel() * 8, _abi.ptr(out), _abi.stream_ptr()),
                   "align_shift_scores")
    return out


def peak(scores, shifts=None, flags=None):
    """The sub-pixel minimum of every table of `scores` (float64 [N, 2 Rv + 1, 2 Ru + 1]) -> (shifts float32 [N, 2] = (du, dv),
    flags int32 [N]).  FLAG_BORDER: the minimum lies on the border of the window on a searched axis (the shift is the integer one);
    FLAG_NON_FINITE: a score of the view is not finite (the shift is (0, 0))."""
    who = "align.peak"
    if not isinstance(scores, torch.Tensor) or not scores.is_cuda:
        raise ValueError(f"{who}: scores must be a CUDA/HIP tensor (no CPU path)")
    if scores.dtype != torch.float64 or scores.dim() != 3 or not scores.is_contiguous():
        raise ValueError(f"{who}: scores must be contiguous float64 [N, 2 Rv + 1, 2 Ru + 1], got {scores.dtype} {tuple(scores.shape)}")
    N, nv, nu = scores.shape
    if nv % 2 == 0 or nu % 2 == 0 or nv > 2 * MAX_SHIFT + 1 or nu > 2 * MAX_SHIFT + 1:
        raise ValueError(f"{who}: a score table has odd extents of at most {2 * MAX_SHIFT + 1}, got {nv} x {nu}")
    if shifts is None:
        shifts = torch.empty(N, 2, dtype=torch.float32, device=scores.device)
    else:
        _check_array(shifts, torch.float32, (N, 2), scores, who, "shifts")
    if flags is None:
        flags = torch.empty(N, dtype=torch.int32, device=scores.device)
    else:
        _check_array(flags, torch.int32, (N,), scores, who, "flags")
    with torch.cuda.device(scores.device):
        _abi.check(_abi.lib().naf_align_peak(_abi.ptr(scores), N, nv // 2, nu // 2, _abi.ptr(shifts), _abi.ptr(flags),
                                             _abi.stream_ptr()), "align_peak")
    return shifts, flags


def estimate_shifts(measured, reprojected, max_shift, weights=None, workspace=None):
    """`peak(shift_scores(...))` -> (shifts float32 [N, 2] = (du, dv), flags int32 [N]): the translation of every view of `measured`
    against `reprojected`, to a fraction of a pixel where the score's minimum is inside the window."""
    return peak(shift_scores(measured, reprojected, max_shift, weights, workspace))


def shift_views(views, shifts, out=None):
    """out[n](r, c) = views[n](r + dv_n, c + du_n) for `shifts` [N, 2] = (du, dv): the views with their shifts undone, by cubic
    convolution with clamp-to-edge.  A whole-number shift copies pixels; a NaN shift makes that view NaN.  `out` must not be `views`."""
    who = "align.shift_views"
    _check_views(views, who, "views")
    N, H, W = views.shape
    _check_array(shifts, torch.float32, (N, 2), views, who, "shifts")
    if out is None:
        out = torch.empty_like(views)
    else:
        _check_views(out, who, "out", views)
        a0, b0, nbytes = out.data_ptr(), views.data_ptr(), views.numel() * 4
        if a0 < b0 + nbytes and b0 < a0 + nbytes:
            raise ValueError(f"{who}: out must not overlap views")
    with torch.cuda.device(views.device):
        _abi.check(_abi.lib().naf_align_shift_views(_abi.ptr(views), _abi.ptr(shifts), N, H, W, _abi.ptr(out), _abi.stream_ptr()),
                   "align_shift_views")
    return out
