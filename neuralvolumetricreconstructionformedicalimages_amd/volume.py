"""Volume preparation on the device: `resize_volume`, the cubic B-spline resize of the reference's `loadImage`
(dataGenerator/generateData.py:111-150: scipy.ndimage.zoom(order=3, prefilter=False)), through libnaf_hip.so
(`naf_resize_volume`), and `prepare_volume`, `loadImage` itself: HU -> attenuation, resize to nVoxel, normalise to [0, 1].

The definition is written down in include/naf_hip.h (V1) and DESIGN.md section 12: output j of an axis sits at
x = j (a - 1) / (b - 1), the taps floor(x) - 1 .. floor(x) + 2 carry the cubic B-spline weights, taps outside the volume are
mirrored about the edge samples, and nothing is prefiltered (an axis that keeps its extent is still smoothed).  There is no CPU
path, like the rest of the hot path.

`sample_points` and `draw_sample` read a volume back at world points (`naf_volume_sample_points`, `naf_volume_draw_sample`;
include/naf_hip.h V4): trilinear between the voxel centres of `get_voxels`, clamp-to-edge, with P1's cell
convention.  `draw_sample` draws its points from a counter-based hash of (seed, step, index, axis) and samples them in the same
pass: it is what `pretrain.fit_volume` runs every step.  The float64 restatement is tests/_volume_sample_oracle.py.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _abi

MU_WATER, MU_AIR = 0.206, 0.0004


def attenuation_affine(rescale_slope, rescale_intercept):
    """(scale, shift) of mu = scale * data + shift: HU = slope * data + intercept, mu = mu_water + (mu_water - mu_air) / 1000 * HU
    (generateData.py:77-103)."""
    k = (MU_WATER - MU_AIR) / 1000
    return k * float(rescale_slope), MU_WATER + k * float(rescale_intercept)


def resize_volume(volume, shape, scale=1.0, shift=0.0, return_minmax=False):
    """Resize a CUDA float32 volume [n1, n2, n3] to `shape` (cubic B-spline, no prefilter) -> a new CUDA float32 volume.

    Input values pass through `scale * v + shift` as they are read.  With `return_minmax` the result is
    (volume, minimum, maximum) of the output, two floats (both NaN if a NaN reaches any output)."""
    _abi.check_volume(volume, "resize_volume")
    shape = tuple(int(v) for v in shape)
    if len(shape) != 3:
        raise ValueError(f"resize_volume: shape must be (n1, n2, n3), got {shape}")
    if min(shape) < 1 or min(volume.shape) < 1:
        raise ValueError(f"resize_volume: every extent must be at least 1, got {tuple(volume.shape)} -> {shape}")
    in_dims = (ctypes.c_uint32 * 3)(*(int(v) for v in volume.shape))
    out_dims = (ctypes.c_uint32 * 3)(*shape)
    lib = _abi.lib()
    with torch.cuda.device(volume.device):
        ws = torch.empty(lib.naf_resize_volume_workspace_bytes(in_dims, out_dims), dtype=torch.uint8, device=volume.device)
        out = torch.empty(shape, dtype=torch.float32, device=volume.device)
        minmax = torch.empty(2, dtype=torch.float32, device=volume.device) if return_minmax else None
        _abi.check(lib.naf_resize_volume(_abi.ptr(volume), in_dims, float(scale), float(shift), _abi.ptr(out), out_dims,
                                         _abi.ptr(minmax), _abi.ptr(ws), ws.numel(), _abi.stream_ptr()), "resize_volume")
        if not return_minmax:
            return out
        lo, hi = minmax.tolist()
        return out, lo, hi


def prepare_volume(image, n_voxel, convert, rescale_slope, rescale_intercept, normalize=True, device="cuda"):
    """loadImage of generateData.py:106-150 on the device: HU -> attenuation, resize to n_voxel, normalise to [0, 1].

    `image` is a numpy array or a torch tensor [n1, n2, n3]; the result is a CUDA float32 volume of shape n_voxel.  The volume is
    resized only if some extent differs (the conversion then rides on the resize as its fused affine); the minimum and maximum
    are those after the resize, and the reference's condition `normalize and min != 0 and max != 1` is kept as written.  With
    nothing to do the volume comes back unchanged."""
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError("prepare_volume: device must be a CUDA/HIP device (no CPU path)")
    if isinstance(image, torch.Tensor):
        vol = image.to(device=dev, dtype=torch.float32).contiguous()
    else:
        vol = torch.from_numpy(np.ascontiguousarray(np.asarray(image).astype(np.float32))).to(dev)
    if vol.dim() != 3:
        raise ValueError(f"prepare_volume: image must be [n1, n2, n3], got shape {tuple(vol.shape)}")
    n_voxel = tuple(int(v) for v in (n_voxel if n_voxel is not None else (256, 256, 256)))
    shared = isinstance(image, torch.Tensor) and vol.data_ptr() == image.data_ptr()      # in-place steps need a copy then
    if tuple(vol.shape) != n_voxel:
        scale, shift = attenuation_affine(rescale_slope, rescale_intercept) if convert else (1.0, 0.0)
        vol, lo, hi = resize_volume(vol, n_voxel, scale, shift, return_minmax=True)
        shared = False
    else:
        if convert:
            # the host function's four rounded fp32 steps: a volume that needs no resize gets the bits it gets there
            vol, shared = (vol.clone() if shared else vol), False
            vol.mul_(float(rescale_slope)).add_(float(rescale_intercept)).mul_((MU_WATER - MU_AIR) / 1000).add_(MU_WATER)
        lo, hi = float(vol.min()), float(vol.max())
    if normalize and lo != 0 and hi != 1:
        vol = vol.clone() if shared else vol
        # a device tensor as the divisor: torch multiplies by the reciprocal of a host scalar, which is not the quotient's rounding
        lo_t = torch.tensor(lo, dtype=torch.float32, device=dev)
        vol.sub_(lo_t).div_(torch.tensor(hi, dtype=torch.float32, device=dev) - lo_t)
    return vol


def _voxel_size(dvoxel, who):
    d = [float(v) for v in np.asarray(dvoxel, dtype=np.float64).reshape(-1)]
    if len(d) != 3 or not all(np.isfinite(v) and v > 0 for v in d):
        raise ValueError(f"{who}: dvoxel must be three finite voxel sizes > 0, got {dvoxel}")
    return (ctypes.c_float * 3)(*d)


def _check_sampled_volume(vol, who):
    if not isinstance(vol, torch.Tensor) or not vol.is_cuda:
        raise RuntimeError(f"{who}: volume must be a CUDA/HIP tensor (no CPU path)")
    if vol.dtype != torch.float32:                       # a ValueError like filter_rows' (check_volume's is a TypeError)
        raise ValueError(f"{who}: volume must be float32, got {vol.dtype}")
    _abi.check_volume(vol, who)
    if min(vol.shape) < 1:
        raise ValueError(f"{who}: every extent must be at least 1, got {tuple(vol.shape)}")


def sample_points(vol, dvoxel, points):
    """`naf_volume_sample_points`: the CUDA float32 volume [n1, n2, n3] with voxel size `dvoxel` (three lengths, metres) sampled
    trilinearly at the CUDA float32 world points [n, 3] -> float32 [n].  Clamp-to-edge outside the hull of the voxel centres; a NaN
    coordinate gives NaN for that point alone."""
    who = "sample_points"
    _check_sampled_volume(vol, who)
    if not isinstance(points, torch.Tensor) or not points.is_cuda or points.device != vol.device:
        raise RuntimeError(f"{who}: points must be a CUDA/HIP tensor on the volume's device (no CPU path)")
    if points.dtype != torch.float32 or points.dim() != 2 or points.shape[1] != 3 or not points.is_contiguous():
        raise ValueError(f"{who}: points must be a contiguous float32 [n, 3] tensor, got {points.dtype} {tuple(points.shape)}")
    d = _voxel_size(dvoxel, who)
    n = int(points.shape[0])
    out = torch.empty(n, dtype=torch.float32, device=vol.device)
    if n == 0:
        return out
    n1, n2, n3 = (int(v) for v in vol.shape)
    with torch.cuda.device(vol.device):
        _abi.check(_abi.lib().naf_volume_sample_points(_abi.ptr(vol), n1, n2, n3, d, _abi.ptr(points), n, _abi.ptr(out),
                                                       _abi.stream_ptr()), who)
    return out


def draw_sample(vol, dvoxel, lo, hi, seed, step, n, points_out=None, targets_out=None):
    """`naf_volume_draw_sample`: `n` points uniform in the box [lo, hi] (three floats each) from the counter-based hash of
    (seed, step, index, axis), and the volume's trilinear value at each, in one launch -> (points [n, 3], targets [n]), float32 on
    the volume's device.  No state and no torch generator: equal arguments give equal bits.  `points_out` / `targets_out` are
    written in place when given."""
    who = "draw_sample"
    _check_sampled_volume(vol, who)
    d = _voxel_size(dvoxel, who)
    box = []
    for name, v in (("lo", lo), ("hi", hi)):
        v = [float(np.float32(x)) for x in np.asarray(v, dtype=np.float64).reshape(-1)]
        if len(v) != 3 or not all(np.isfinite(x) for x in v):
            raise ValueError(f"{who}: {name} must be three finite floats, got {v}")
        box.append(v)
    if any(a > b for a, b in zip(*box)):
        raise ValueError(f"{who}: the box must have lo <= hi on every axis, got {box[0]} .. {box[1]}")
    n, seed, step = int(n), int(seed), int(step)
    if not 0 <= n < 2 ** 32 or not 0 <= step < 2 ** 32 or not 0 <= seed < 2 ** 64:
        raise ValueError(f"{who}: n and step must fit 32 bits and seed 64 bits, got n {n}, step {step}, seed {seed}")
    if points_out is None:
        points_out = torch.empty((n, 3), dtype=torch.float32, device=vol.device)
    else:
        _abi.check_stack(points_out, (n, 3), vol, who, "points_out")
    if targets_out is None:
        targets_out = torch.empty(n, dtype=torch.float32, device=vol.device)
    else:
        _abi.check_stack(targets_out, (n,), vol, who, "targets_out")
    if n == 0:
        return points_out, targets_out
    dims = (ctypes.c_uint32 * 3)(*(int(v) for v in vol.shape))
    with torch.cuda.device(vol.device):
        _abi.check(_abi.lib().naf_volume_draw_sample(_abi.ptr(vol), dims, d, (ctypes.c_float * 3)(*box[0]), (ctypes.c_float * 3)(*box[1]),
                                                     seed, step, n, _abi.ptr(points_out), _abi.ptr(targets_out), _abi.stream_ptr()), who)
    return points_out, targets_out
