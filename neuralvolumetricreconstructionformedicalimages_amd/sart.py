"""The subset step of OS-SART through libnaf_hip.so (`naf_sart_residual_scan`, `naf_sart_backproject_scan`, `naf_sart_update`;
include/naf_hip.h P4).

    residual_scan     y = (b - A x) / len and r = b - A x for a list of views of a scan, read in place from the whole scan
    backproject_scan  num += A_s^T y and, where asked, den += A_s^T 1 for the same list
    update            x += relax * num / den, clamped at 0; num = 0; den = 0 where asked

A and A^T are `projector.project_scan` and `projector.backproject_scan` restricted to the list; `reconstruct.os_sart` is the solver
on top.  `residual_scan` and `backproject_scan` take `kind`: "siddon" runs the same step on the ray-voxel intersection pair
(`naf_sart_residual_scan_siddon`, `naf_sart_backproject_scan_siddon`; P8), where `len` is the ray's row sum
A 1 taken in the same walk as A x; `update` serves both kinds.  There is no CPU fallback, like the rest of the hot path.
"""
from __future__ import annotations

import torch

from . import _abi, projector
from .projector import Scan, ViewList                       # where they live; `sart.Scan` and `sart.ViewList` are the same objects


def _views(views, scan):
    """-> (ViewList or None, number of launch views)."""
    if views is None:
        return None, scan.N
    if not isinstance(views, ViewList):
        views = ViewList(views, scan.N, scan.device)
    elif views.n_views != scan.N:
        raise ValueError(f"sart: the view list was checked for {views.n_views} views, the scan has {scan.N}")
    return views, len(views)


def residual_scan(volume, projections, geo, angles, views=None, y=None, r=None, want_r=True, scan=None, kind="interpolated"):
    """Weighted residual of the views `views` (indices into the scan; None: all, in order) of the scan `projections` [N, H, W] for
    the volume `volume` -> (y, r), float32 [len(views), H, W]: r = b - A x and y = r / len (0 on a ray that misses the volume).
    `y` and `r` may be given to be written into; `want_r=False` skips r and returns None for it.  `scan` is a `Scan` of the same
    `geo` and `angles` to reuse across calls.  `kind="siddon"` takes A of the ray-voxel intersection projector (P6) and for `len`
    the ray's row sum (A 1)_r, the bits `project_scan(ones, kind="siddon")` returns (P8)."""
    who = "sart.residual_scan"
    projector.check_kind(kind, who)
    _abi.check_volume(volume, who)
    projector.check_geometry(volume, geo)
    scan = projector.scan_for(geo, angles, volume.device, scan, "sart")
    _abi.check_stack(projections, (scan.N, scan.H, scan.W), volume, who, "projections")
    views, m = _views(views, scan)
    shape = (m, scan.H, scan.W)
    if y is None:
        y = torch.empty(shape, device=volume.device, dtype=torch.float32)
    else:
        _abi.check_stack(y, shape, volume, who, "y")
    if not want_r:
        r = None
    elif r is None:
        r = torch.empty(shape, device=volume.device, dtype=torch.float32)
    else:
        _abi.check_stack(r, shape, volume, who, "r")
    if m:
        scan.residual(volume, views, m, projections, y, r, kind)
    return y, r


def backproject_scan(y, geo, angles, views=None, num=None, den=None, scan=None, method="scatter", workspace=None,
                     kind="interpolated"):
    """Transpose over the same view list: adds A_s^T y into `num` (None: a zeroed volume) and, if `den` is given, A_s^T 1 into
    `den`, both float32 volumes on the voxel grid of `geo` that are accumulated into -> num.  `method="gather"` takes the
    atomic-free gather form (naf_hip.h P5; the same bits on every call) instead of the scatter; `workspace` is then a span table
    from `projector.gather_workspace` to reuse across calls (None: one is made; False: none, the spans are recomputed).
    `kind="siddon"` is the transpose of the ray-voxel intersection projector (P7) with the paired column sums (P8); it sums with
    atomics only, so with `method="gather"` it raises ValueError."""
    who = "sart.backproject_scan"
    projector.check_kind_and_method(kind, method, who)
    if not isinstance(y, torch.Tensor) or not y.is_cuda:
        raise RuntimeError(f"{who}: y must be a CUDA/HIP tensor (no CPU path)")
    scan = projector.scan_for(geo, angles, y.device, scan, "sart")
    views, m = _views(views, scan)
    _abi.check_stack(y, (m, scan.H, scan.W), None, who, "y")
    num = projector.check_out(num, scan.dims, y, who)
    projector.check_geometry(num, geo)
    if den is not None:
        _abi.check_volume(den, who, "den")
        if tuple(den.shape) != scan.dims or den.device != y.device:
            raise ValueError(f"{who}: den must be a contiguous float32 {scan.dims} tensor on the input's device")
        if den.data_ptr() == num.data_ptr():
            raise ValueError(f"{who}: num and den must be two volumes")
    if m and method == "gather":
        if workspace is None:
            workspace = projector.gather_workspace(m, scan.H, scan.W, y.device)
        elif workspace is False:
            workspace = None
        elif (not isinstance(workspace, torch.Tensor) or workspace.dtype != torch.uint8 or workspace.dim() != 1
              or not workspace.is_contiguous() or workspace.device != y.device):
            raise ValueError(f"{who}: workspace must be a contiguous uint8 [bytes] tensor on the input's device "
                             "(projector.gather_workspace), None or False")
        scan.gather(y, views, m, num, den, workspace)
    elif m:
        scan.backproject_views(y, views, m, num, den, kind)
    return num


def update(x, num, den, relax=1.0, nonneg=True, den_is_reciprocal=False, zero_den=False):
    """The element-wise tail of a subset step, in place on three float32 tensors of one shape:
    x += relax * (c * num) with c = 1 / den where den > 0 and 0 elsewhere (c = den itself if `den_is_reciprocal`), x = max(x, 0) if
    `nonneg`, num = 0, and den = 0 if `zero_den` -> x."""
    who = "sart.update"
    for name, t in (("x", x), ("num", num), ("den", den)):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise RuntimeError(f"{who}: {name} must be a CUDA/HIP tensor (no CPU path)")
        if t.dtype != torch.float32:
            raise TypeError(f"{who}: {name} must be float32, got {t.dtype}")
        if not t.is_contiguous():
            raise ValueError(f"{who}: {name} must be contiguous")
        if t.shape != x.shape or t.device != x.device:
            raise ValueError(f"{who}: {name} must have x's shape {tuple(x.shape)} and device, got {tuple(t.shape)} on {t.device}")
    if den_is_reciprocal and zero_den:
        raise ValueError(f"{who}: a reciprocal den is only read, zero_den cannot be set with it")
    _abi.check(_abi.lib().naf_sart_update(_abi.ptr(x), _abi.ptr(num), _abi.ptr(den), x.numel(), float(relax), int(bool(nonneg)),
                                          int(bool(den_is_reciprocal)), int(bool(zero_den)), _abi.stream_ptr()), "sart_update")
    return x
