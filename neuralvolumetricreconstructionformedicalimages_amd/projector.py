"""Forward projector and its transpose: line integrals of a voxel volume through libnaf_hip.so (`naf_project_rays`,
`naf_project_scan`, `naf_backproject_rays`, `naf_backproject_scan` and their `_siddon` counterparts).

This is what TIGRE's `tigre.Ax` does for the reference's dataGenerator/generateData.py:178,189: it turns a CT volume into the
projections of a scan.  The projection is defined in include/naf_hip.h (P1) and DESIGN.md section 10: trilinear interpolation,
clamp-to-edge inside the box and zero outside, midpoint rule with `n = max(1, ceil(len / (accuracy * min(dVoxel))))` samples
over the part of the ray inside the box.  Pixel (p, row, col) of `project_scan` integrates the very ray `RayGenerator` makes for
that pixel, so projections and training rays agree by construction (no TIGRE axis flips).  Bit-parity with TIGRE is not pinned.

`kind="siddon"` selects the other discretisation (P6): the volume constant inside each voxel and exact chord
lengths, the ray-voxel intersection projector TIGRE's `Ax` takes by default.  It has no sample step, so `accuracy` plays no part.
`backproject_rays` and `backproject_scan` take the same `kind`: with "siddon" they add the exact transpose of that projector (P7,
DESIGN.md section 21), one fp32 atomic per voxel a ray crosses, so A and A^T of either kind are a matched pair.  The Siddon transpose
has the scatter form only.  The default everywhere is `kind="interpolated"`; `reconstruct.sirt`, `asd_pocs`, `cgls`, `os_sart` and
`fista_tv` take `kind` as well (the last two on the fused subset kernels of P8); FDK stays on the
interpolated pair.

There is no CPU fallback, like the rest of the hot path.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _abi
from .geometry import RayGenerator

# pixels per launch of naf_project_scan: keeps one launch of a 720 x 1024^2 scan to a bounded grid
MAX_PIXELS_PER_CALL = 1 << 26
# the gather transpose's span table (naf_hip.h P5): 40 bytes per ray, and at most this much of it, so that it stays in the caches
GATHER_SPAN_BYTES = 40
GATHER_WORKSPACE_CAP = 32 << 20
METHODS = ("scatter", "gather")
KINDS = ("interpolated", "siddon")


def _check_volume(volume):
    _abi.check_volume(volume, "projector")


def sample_step(dvoxel, accuracy=0.5):
    """Target sample spacing in metres: accuracy * min(dVoxel) (TIGRE's geo.accuracy is in voxels per sample)."""
    step = float(accuracy) * float(np.min(np.asarray(dvoxel, dtype=np.float64)))
    if not step > 0:
        raise ValueError(f"projector: accuracy * min(dVoxel) must be > 0, got {step}")
    return step


def _dvoxel(dvoxel):
    d = np.asarray(dvoxel, dtype=np.float64).reshape(-1)
    if d.size != 3 or not np.all(d > 0):
        raise ValueError(f"projector: dVoxel must be three positive sizes, got {dvoxel}")
    return (ctypes.c_float * 3)(*[float(v) for v in d])


def check_kind(kind, who):
    if kind not in KINDS:
        raise ValueError(f"{who}: kind must be one of {KINDS}, got {kind!r}")
    return kind


class Scan:
    """What every call on one scan shares, made once: the poses of all views on the device and the geometry arguments, with one
    method per scan entry point of the library that owns its argument list."""

    def __init__(self, geo, angles, device):
        self.geo = geo
        self.angles = np.asarray(angles, dtype=np.float64).reshape(-1)
        self.raygen = RayGenerator(geo, self.angles, device)
        self.device = self.raygen.poses.device              # with its index, as tensors report it
        self.N, self.H, self.W = len(self.angles), self.raygen.H, self.raygen.W
        self.dims = tuple(int(v) for v in geo.nVoxel)
        self._cdims = (ctypes.c_uint32 * 3)(*self.dims)
        self._dvoxel = _dvoxel(geo.dVoxel)
        self._step = sample_step(geo.dVoxel, geo.accuracy)

    def _grid_and_poses(self, first=0):
        return ctypes.byref(self._cdims), ctypes.byref(self._dvoxel), _abi.ptr(self.raygen.poses[first:])

    def _detector(self, kind="interpolated"):
        """The detector and, for the interpolated entry points, the sample step; the Siddon ones have none."""
        det = ctypes.byref(self.raygen.detector)
        return (det,) if kind == "siddon" else (det, self._step)

    @staticmethod
    def _entry(name, kind):
        """The scan entry point `naf_<name>` of that `kind`, and its name for the error message."""
        what = name + "_siddon" if kind == "siddon" else name
        return getattr(_abi.lib(), "naf_" + what), what

    def project(self, volume, out, first, count, kind):
        """out[first:first + count] = A volume for those views."""
        fn, what = self._entry("project_scan", kind)
        _abi.check(fn(_abi.ptr(volume), *self._grid_and_poses(first), count, *self._detector(kind), _abi.ptr(out[first:first + count]),
                      _abi.stream_ptr()), what)

    def backproject(self, projections, out, first, count, kind="interpolated"):
        """out += A^T projections over the views [first, first + count), by the scatter of that `kind`."""
        fn, what = self._entry("backproject_scan", kind)
        _abi.check(fn(_abi.ptr(projections[first:first + count]), *self._grid_and_poses(first), count, *self._detector(kind),
                      _abi.ptr(out), _abi.stream_ptr()), what)

    def residual(self, volume, views, m, projections, y, r, kind="interpolated"):
        """y, r of the `m` views `views` (None: the first m) by the fused forward walk of that `kind`."""
        fn, what = self._entry("sart_residual_scan", kind)
        _abi.check(fn(_abi.ptr(volume), *self._grid_and_poses(), m, *self._detector(kind), _index_ptr(views), self.N,
                      _abi.ptr(projections), _abi.ptr(y), _abi.ptr(r), _abi.stream_ptr()), what)

    def backproject_views(self, y, views, m, num, den, kind="interpolated"):
        """num += A_s^T y and, where `den` is given, den += A_s^T 1 over the same views, by the paired scatter of that `kind`."""
        fn, what = self._entry("sart_backproject_scan", kind)
        _abi.check(fn(_abi.ptr(y), _index_ptr(views), m, self.N, *self._grid_and_poses(), *self._detector(kind), _abi.ptr(num),
                      _abi.ptr(den), _abi.stream_ptr()), what)

    def gather(self, values, views, m, num, den, workspace, first=0, n_scan_views=None):
        """The gather transpose of `m` launch views: a view list into the whole scan, or without one the views from `first` on."""
        _abi.check(_abi.lib().naf_backproject_scan_gather(
            _abi.ptr(values), _index_ptr(views), m, self.N if n_scan_views is None else n_scan_views, *self._grid_and_poses(first),
            *self._detector(), _abi.ptr(num), _abi.ptr(den), _abi.ptr(workspace), 0 if workspace is None else workspace.numel(),
            _abi.stream_ptr()), "backproject_scan_gather")


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


def _index_ptr(views):
    return None if views is None else _abi.ptr(views.device)


def scan_for(geo, angles, device, scan, who):
    """`scan` if given (it must be of this `geo` and `device`), else a new Scan."""
    if scan is None:
        return Scan(geo, angles, device)
    if scan.geo is not geo or scan.device != device:
        raise ValueError(f"{who}: `scan` was made for another geometry or device")
    return scan


def project_rays(volume, dvoxel, rays, accuracy=0.5, out=None, kind="interpolated"):
    """Line integrals of `volume` [n1, n2, n3] (voxel size `dvoxel` in metres) along `rays` [n, 8] -> float32 [n].
    `kind="siddon"` integrates exact chord lengths through piecewise-constant voxels (P6); `accuracy` is ignored then."""
    check_kind(kind, "project_rays")
    _check_volume(volume)
    n = _abi.check_rays(rays, volume, "project_rays", "volume's")
    if not rays.is_contiguous():
        raise ValueError("project_rays: rays must be contiguous")
    if out is None:
        out = torch.empty(n, device=volume.device, dtype=torch.float32)
    elif out.shape != (n,) or out.dtype != torch.float32 or out.device != volume.device or not out.is_contiguous():
        raise ValueError("project_rays: out must be a contiguous float32 [n] tensor on the volume's device")
    n1, n2, n3 = volume.shape
    if kind == "siddon":
        _abi.check(_abi.lib().naf_project_rays_siddon(_abi.ptr(volume), n1, n2, n3, ctypes.byref(_dvoxel(dvoxel)), _abi.ptr(rays), n,
                                                      _abi.ptr(out), _abi.stream_ptr()), "project_rays_siddon")
        return out
    _abi.check(_abi.lib().naf_project_rays(_abi.ptr(volume), n1, n2, n3, ctypes.byref(_dvoxel(dvoxel)), _abi.ptr(rays), n,
                                           sample_step(dvoxel, accuracy), _abi.ptr(out), _abi.stream_ptr()), "project_rays")
    return out


def check_geometry(volume, geo):
    """`volume` must sit on the voxel grid of `geo` (get_voxels): same dims, no origin offset."""
    if np.any(np.asarray(geo.offOrigin, dtype=np.float64) != 0):
        raise ValueError(f"projector: offOrigin must be zero (the voxel grid of get_voxels is centred), got {geo.offOrigin}")
    want = tuple(int(v) for v in geo.nVoxel)
    if tuple(volume.shape) != want:
        raise ValueError(f"projector: volume shape {tuple(volume.shape)} does not match nVoxel {want}")


def project_scan(volume, geo, angles, views_per_call=None, kind="interpolated", scan=None):
    """Projections of `volume` for the scan geometry `geo` (ConeGeometry) at `angles` (radians) -> float32 [N, H, W] on the
    volume's device.  Views go to the kernel in groups of `views_per_call` (default: as many as fit MAX_PIXELS_PER_CALL).
    `kind="siddon"` integrates exact chord lengths through piecewise-constant voxels (P6); `geo.accuracy` is ignored then.
    `scan` is a `Scan` of the same `geo` and `angles` to reuse across calls."""
    check_kind(kind, "project_scan")
    _check_volume(volume)
    check_geometry(volume, geo)
    scan = scan_for(geo, angles, volume.device, scan, "projector")
    N, H, W = scan.N, scan.H, scan.W
    out = torch.empty(N, H, W, device=volume.device, dtype=torch.float32)
    per_call = views_per_call or max(1, MAX_PIXELS_PER_CALL // (H * W))
    for first in range(0, N, per_call):
        scan.project(volume, out, first, min(per_call, N - first), kind)
    return out


def check_out(out, shape, like, who):
    """`out=None` allocates zeros; a given `out` is accumulated into."""
    if out is None:
        return torch.zeros(shape, device=like.device, dtype=torch.float32)
    _abi.check_volume(out, who, "out")
    if tuple(out.shape) != tuple(shape) or out.device != like.device:
        raise ValueError(f"{who}: out must be a contiguous float32 {tuple(shape)} tensor on the input's device")
    return out


def backproject_rays(values, dvoxel, rays, dims, accuracy=0.5, out=None, kind="interpolated"):
    """Transpose of `project_rays`: adds `values` [n] along `rays` [n, 8] into a volume of `dims` = (n1, n2, n3) voxels of size
    `dvoxel` -> float32 [n1, n2, n3].  Sums are fp32 atomics: equal to A^T values up to summation order (naf_hip.h, P2).
    Arbitrary rays lie on no pixel lattice, so this entry point keeps the scatter only: the atomic-free gather form
    (`backproject_scan(..., method="gather")`) exists for scans.  `kind="siddon"` is the transpose of `project_rays(kind="siddon")`
    (P7): values times exact chord lengths, one atomic per voxel crossed; `accuracy` is ignored then."""
    check_kind(kind, "backproject_rays")
    if not isinstance(values, torch.Tensor) or not values.is_cuda:
        raise RuntimeError("backproject_rays: values must be a CUDA/HIP tensor (no CPU path)")
    n = _abi.check_rays(rays, values, "backproject_rays", "values'")
    if values.dtype != torch.float32 or tuple(values.shape) != (n,):
        raise ValueError(f"backproject_rays: values must be float32 [{n}], got {values.dtype} {tuple(values.shape)}")
    if not rays.is_contiguous() or not values.is_contiguous():
        raise ValueError("backproject_rays: values and rays must be contiguous")
    dims = tuple(int(v) for v in dims)
    if len(dims) != 3 or min(dims) < 1:
        raise ValueError(f"backproject_rays: dims must be three positive extents, got {dims}")
    out = check_out(out, dims, values, "backproject_rays")
    if kind == "siddon":
        _abi.check(_abi.lib().naf_backproject_rays_siddon(_abi.ptr(values), _abi.ptr(rays), n, dims[0], dims[1], dims[2],
                                                          ctypes.byref(_dvoxel(dvoxel)), _abi.ptr(out), _abi.stream_ptr()),
                   "backproject_rays_siddon")
        return out
    _abi.check(_abi.lib().naf_backproject_rays(_abi.ptr(values), _abi.ptr(rays), n, dims[0], dims[1], dims[2],
                                               ctypes.byref(_dvoxel(dvoxel)), sample_step(dvoxel, accuracy), _abi.ptr(out),
                                               _abi.stream_ptr()), "backproject_rays")
    return out


def check_method(method, who):
    if method not in METHODS:
        raise ValueError(f"{who}: method must be one of {METHODS}, got {method!r}")
    return method


def gather_workspace(n_views, H, W, device, span_table=True):
    """Span table of the gather transpose for calls of up to `n_views` views of H x W pixels -> uint8 tensor, or None without a
    table.  At least one view, at most GATHER_WORKSPACE_CAP bytes beyond that: the entry point walks the views in groups that fit."""
    if not span_table:
        return None
    per_view = GATHER_SPAN_BYTES * H * W
    views = max(1, min(int(n_views), GATHER_WORKSPACE_CAP // per_view))
    return torch.empty(views * per_view, device=device, dtype=torch.uint8)


def check_kind_and_method(kind, method, who):
    """The Siddon transpose exists as a scatter only: there is no atomic-free (gather) form of it."""
    check_kind(kind, who)
    check_method(method, who)
    if kind == "siddon" and method == "gather":
        raise ValueError(f"{who}: kind='siddon' has no method='gather': the Siddon transpose sums with atomics only, and the "
                         "atomic-free gather exists for the interpolated pair")


def backproject_scan(projections, geo, angles, views_per_call=None, out=None, method="scatter", span_table=True, scan=None,
                     kind="interpolated"):
    """Transpose of `project_scan`: adds `projections` [N, H, W] of the scan geometry `geo` at `angles` into a volume on the voxel
    grid of `geo` -> float32 nVoxel.  Views go to the kernel in groups of `views_per_call` like `project_scan`'s.
    `method="scatter"` (the default) is the ray scatter on fp32 atomics, equal to A^T y up to summation order; `method="gather"`
    is the same operator evaluated per voxel in a fixed order with no atomics (naf_hip.h P5): two calls return the same bits,
    whatever `views_per_call` and `span_table` (whether the rays' spans are tabulated by a pre-pass or recomputed) are.  `scan` is a `Scan` of the same `geo` and `angles` to reuse across calls.
    `kind="siddon"` is the transpose of `project_scan(kind="siddon")` (P7), a scatter on fp32 atomics; it has no gather form, so
    with `method="gather"` it raises ValueError."""
    check_kind_and_method(kind, method, "backproject_scan")
    angles = np.asarray(angles, dtype=np.float64).reshape(-1)
    N, H, W = len(angles), int(geo.nDetector[1]), int(geo.nDetector[0])
    _abi.check_stack(projections, (N, H, W), None, "backproject_scan", "projections")
    out = check_out(out, tuple(int(v) for v in geo.nVoxel), projections, "backproject_scan")
    check_geometry(out, geo)
    if N == 0:
        return out
    scan = scan_for(geo, angles, projections.device, scan, "projector")
    per_call = views_per_call or max(1, MAX_PIXELS_PER_CALL // (H * W))
    work = gather_workspace(min(per_call, N), H, W, projections.device, span_table) if method == "gather" else None
    for first in range(0, N, per_call):
        count = min(per_call, N - first)
        if method == "gather":
            scan.gather(projections[first:first + count], None, count, out, None, work, first, count)
        else:
            scan.backproject(projections, out, first, count, kind)
    return out
