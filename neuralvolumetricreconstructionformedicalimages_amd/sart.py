"""The subset step of OS-SART through libnaf_hip.so (`naf_sart_residual_scan`, `naf_sart_backproject_scan`, `naf_sart_update`;
include/naf_hip.h P4).

    residual_scan     y = (b - A x) / len and r = b - A x for a list of views of a scan, read in place from the whole scan
    backproject_scan  num += A_s^T y and, where asked, den += A_s^T 1 for the same list
    update            x += relax * num / den, clamped at 0; num = 0; den = 0 where asked

A and A^T are `projector.project_scan` and `projector.backproject_scan` restricted to the list; `reconstruct.os_sart` is the solver
on top.  There is no CPU fallback, like the rest of the hot path.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _abi, projector
from .geometry import RayGenerator


class Scan:
    """What every call on one scan shares, made once: the poses of all views on the device and the geometry arguments."""

    def __init__(self, geo, angles, device):
        self.geo = geo
        self.angles = np.asarray(angles, dtype=np.float64).reshape(-1)
        self.raygen = RayGenerator(geo, self.angles, device)
        self.device = self.raygen.poses.device              # with its index, as tensors report it
        self.N, self.H, self.W = len(self.angles), self.raygen.H, self.raygen.W
        self.dims = tuple(int(v) for v in geo.nVoxel)
        self._cdims = (ctypes.c_uint32 * 3)(*self.dims)
        self._dvoxel = projector._dvoxel(geo.dVoxel)
        self._step = projector.sample_step(geo.dVoxel, geo.accuracy)

    def detector_args(self):
        g = self.geo
        return (self.W, self.H, float(g.dDetector[0]), float(g.dDetector[1]), float(g.offDetector[0]), float(g.offDetector[1]),
                float(g.DSD), float(self.raygen.near), float(self.raygen.far), int(g.mode == "parallel"), self._step)


class ViewList:
    """A list of views of an N-view scan, checked on the host (every index in [0, N)) and held on the device as well."""

    def __init__(self, views, n_views, device):
        idx = np.asarray(views).reshape(-1)
        if idx.size and not np.issubdtype(idx.dtype, np.integer):
            raise ValueError(f"sart: view indices must be integers, got {idx.dtype}")
        idx = idx.astype(np.int64)
        if idx.size and (idx.min() < 0 or idx.max() >= n_views):
            raise ValueError(f"sart: view index out of range for a scan of {n_views} views: {idx.tolist()}")
        self.host, self.n_views = idx, int(n_views)
        self.device = torch.tensor(idx.astype(np.int32), device=device) if idx.size else None      # the same bits as u32

    def __len__(self):
        return int(self.host.size)


def _scan(geo, angles, device, scan):
    if scan is None:
        return Scan(geo, angles, device)
    if scan.geo is not geo or scan.device != device:
        raise ValueError("sart: `scan` was made for another geometry or device")
    return scan


def _views(views, scan):
    """-> (ViewList or None, number of launch views)."""
    if views is None:
        return None, scan.N
    if not isinstance(views, ViewList):
        views = ViewList(views, scan.N, scan.device)
    elif views.n_views != scan.N:
        raise ValueError(f"sart: the view list was checked for {views.n_views} views, the scan has {scan.N}")
    return views, len(views)


def _check_stack(t, shape, like, who, name):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"{who}: {name} must be a CUDA/HIP tensor (no CPU path)")
    if t.dtype != torch.float32 or tuple(t.shape) != tuple(shape):
        raise ValueError(f"{who}: {name} must be float32 {tuple(shape)}, got {t.dtype} {tuple(t.shape)}")
    if not t.is_contiguous():
        raise ValueError(f"{who}: {name} must be contiguous")
    if like is not None and t.device != like.device:
        raise ValueError(f"{who}: {name} must be on the device of the other arguments")


def _index_ptr(views):
    return None if views is None else _abi.ptr(views.device)


def residual_scan(volume, projections, geo, angles, views=None, y=None, r=None, want_r=True, scan=None):
    """Weighted residual of the views `views` (indices into the scan; None: all, in order) of the scan `projections` [N, H, W] for
    the volume `volume` -> (y, r), float32 [len(views), H, W]: r = b - A x and y = r / len (0 on a ray that misses the volume).
    `y` and `r` may be given to be written into; `want_r=False` skips r and returns None for it.  `scan` is a `Scan` of the same
    `geo` and `angles` to reuse across calls."""
    who = "sart.residual_scan"
    _abi.check_volume(volume, who)
    projector.check_geometry(volume, geo)
    scan = _scan(geo, angles, volume.device, scan)
    _check_stack(projections, (scan.N, scan.H, scan.W), volume, who, "projections")
    views, m = _views(views, scan)
    shape = (m, scan.H, scan.W)
    if y is None:
        y = torch.empty(shape, device=volume.device, dtype=torch.float32)
    else:
        _check_stack(y, shape, volume, who, "y")
    if not want_r:
        r = None
    elif r is None:
        r = torch.empty(shape, device=volume.device, dtype=torch.float32)
    else:
        _check_stack(r, shape, volume, who, "r")
    if m:
        _abi.check(_abi.lib().naf_sart_residual_scan(
            _abi.ptr(volume), ctypes.byref(scan._cdims), ctypes.byref(scan._dvoxel), _abi.ptr(scan.raygen.poses), m,
            *scan.detector_args(), _index_ptr(views), scan.N, _abi.ptr(projections), _abi.ptr(y), _abi.ptr(r), _abi.stream_ptr()),
            "sart_residual_scan")
    return y, r


def backproject_scan(y, geo, angles, views=None, num=None, den=None, scan=None, method="scatter", workspace=None):
    """Transpose over the same view list: adds A_s^T y into `num` (None: a zeroed volume) and, if `den` is given, A_s^T 1 into
    `den`, both float32 volumes on the voxel grid of `geo` that are accumulated into -> num.  `method="gather"` takes the
    atomic-free gather form (naf_hip.h P5; the same bits on every call) instead of the scatter; `workspace` is then a span table
    from `projector.gather_workspace` to reuse across calls (None: one is made; False: none, the spans are recomputed)."""
    who = "sart.backproject_scan"
    projector.check_method(method, who)
    if not isinstance(y, torch.Tensor) or not y.is_cuda:
        raise RuntimeError(f"{who}: y must be a CUDA/HIP tensor (no CPU path)")
    scan = _scan(geo, angles, y.device, scan)
    views, m = _views(views, scan)
    _check_stack(y, (m, scan.H, scan.W), None, who, "y")
    num = projector._check_out(num, scan.dims, y, who)
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
        _abi.check(_abi.lib().naf_backproject_scan_gather(
            _abi.ptr(y), _index_ptr(views), m, scan.N, ctypes.byref(scan._cdims), ctypes.byref(scan._dvoxel),
            _abi.ptr(scan.raygen.poses), *scan.detector_args(), _abi.ptr(num), _abi.ptr(den), _abi.ptr(workspace),
            0 if workspace is None else workspace.numel(), _abi.stream_ptr()), "backproject_scan_gather")
    elif m:
        _abi.check(_abi.lib().naf_sart_backproject_scan(
            _abi.ptr(y), _index_ptr(views), m, scan.N, ctypes.byref(scan._cdims), ctypes.byref(scan._dvoxel),
            _abi.ptr(scan.raygen.poses), *scan.detector_args(), _abi.ptr(num), _abi.ptr(den), _abi.stream_ptr()),
            "sart_backproject_scan")
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
