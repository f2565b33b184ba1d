"""Sinogram stripe removal by sorting through libnaf_hip.so (`naf_stripe_remove_sorting`; include/naf_hip.h A2):
algorithm 3 of Vo, Atwood and Drakopoulos, Opt. Express 26 (2018), which tomopy ships as `remove_stripe_based_sorting`.

Projections are float32 [N, H, W] on the GPU: N views, H detector rows, W detector columns.  A detector pixel with a wrong gain leaves
a constant stripe along the views of its sinogram column and a ring in the volume.  Per detector row the filter sorts every sinogram
column along the views, median-filters the sorted sinogram across columns (window `size`, reflected at the edges) and puts every
value back at the view it came from.  It does no arithmetic: every output is one of the input's floats, bit for bit, and equal
inputs give equal bits.  There is no CPU fallback, like the rest of the hot path.
"""
from __future__ import annotations

import torch

from . import _abi

MAX_SIZE = 63                       # NAF_STRIPE_MAX_SIZE
MAX_VIEWS = 4096                    # NAF_STRIPE_MAX_VIEWS
MAX_EXTENT = 1 << 24


def default_size(W):
    """The window for a detector of W columns: the smallest odd integer >= max(5, 0.02 W), capped at 63 (W = 512 -> 11)."""
    W = int(W)
    if W < 1:
        raise ValueError(f"stripe.default_size: W must be >= 1, got {W}")
    size = max(5, -(-2 * W // 100))                     # ceil(0.02 W) in integers
    return min(size | 1, MAX_SIZE)


def check_size(size, W, who="stripe"):
    """`size` as an int: odd, 3 <= size <= 63 and size <= W, else ValueError."""
    if isinstance(size, bool) or not isinstance(size, int):
        raise ValueError(f"{who}: size must be an int, got {size!r}")
    if size < 3 or size > MAX_SIZE or size % 2 == 0:
        raise ValueError(f"{who}: size must be odd and in [3, {MAX_SIZE}], got {size}")
    if size > W:
        raise ValueError(f"{who}: size {size} is above the {W} detector columns")
    return size


def _check_kind(t, who, name):
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{who}: {name} must be a tensor, got {type(t).__name__}")
    if t.dtype != torch.float32 or t.dim() != 3:
        raise ValueError(f"{who}: {name} must be float32 [N, H, W], got {t.dtype} {tuple(t.shape)}")


def _check_views(t, who, name):
    _check_kind(t, who, name)
    if not t.is_cuda:
        raise ValueError(f"{who}: {name} must be a CUDA/HIP tensor (no CPU path)")
    if not t.is_contiguous():
        raise ValueError(f"{who}: {name} must be contiguous")


def workspace_bytes(N, H, W, rows=None):
    """The bytes `remove_stripes` needs to filter `rows` detector rows at a time (default: all H)."""
    rows = int(H) if rows is None else int(rows)
    nbytes = _abi.lib().naf_stripe_workspace_bytes(int(N), int(H), int(W), rows)
    if nbytes == 0:
        raise ValueError(f"stripe.workspace_bytes: illegal shape N, H, W = {N}, {H}, {W} with rows = {rows} (1 <= N <= {MAX_VIEWS}, "
                         f"1 <= H, W <= 2^24, 1 <= rows <= H)")
    return nbytes


def remove_stripes(projections, size=5, out=None, workspace_bytes=None):
    """`projections` (float32 [N, H, W] on the GPU) with the stripes of window `size` removed -> `out` (default: a new tensor; it may
    be `projections` itself).  `size` is odd, 3 <= size <= 63 and size <= W; `default_size(W)` is a starting point.  At most 4096
    views.  `workspace_bytes` bounds the scratch the call allocates: detector rows are filtered in groups that fit it, at least one
    row (N W 6 bytes, rounded up) at a time; the default holds all rows.  Any grouping returns the same bits."""
    who = "stripe.remove_stripes"
    _check_kind(projections, who, "projections")                 # the shape and the size first: they are refused without a GPU too
    N, H, W = projections.shape
    size = check_size(size, W, who)
    _check_views(projections, who, "projections")
    if N > MAX_VIEWS:
        raise ValueError(f"{who}: at most {MAX_VIEWS} views, got {N}")
    if H > MAX_EXTENT or W > MAX_EXTENT:
        raise ValueError(f"{who}: H and W are at most 2^24, got {H} x {W}")
    if out is None:
        out = torch.empty_like(projections)
    else:
        _check_views(out, who, "out")
        if out.shape != projections.shape or out.device != projections.device:
            raise ValueError(f"{who}: out must have the shape {tuple(projections.shape)} and device of projections, got "
                             f"{tuple(out.shape)} on {out.device}")
        if out.data_ptr() != projections.data_ptr():
            a0, b0, nbytes = out.data_ptr(), projections.data_ptr(), projections.numel() * 4
            if a0 < b0 + nbytes and b0 < a0 + nbytes:
                raise ValueError(f"{who}: out must be projections itself or not overlap it")
    if projections.numel() == 0:
        return out
    lib = _abi.lib()
    one_row, full = lib.naf_stripe_workspace_bytes(N, H, W, 1), lib.naf_stripe_workspace_bytes(N, H, W, H)
    if workspace_bytes is None:
        workspace_bytes = full
    elif isinstance(workspace_bytes, bool) or not isinstance(workspace_bytes, int) or workspace_bytes < one_row:
        raise ValueError(f"{who}: workspace_bytes must be an int of at least one detector row ({one_row} bytes), got {workspace_bytes!r}")
    nbytes = min(workspace_bytes, full)
    workspace = torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=projections.device)
    with torch.cuda.device(projections.device):
        _abi.check(lib.naf_stripe_remove_sorting(_abi.ptr(projections), N, H, W, size, _abi.ptr(workspace), nbytes, _abi.ptr(out),
                                                 _abi.stream_ptr()), "stripe_remove_sorting")
    return out
