"""Volume preparation on the device: `resize_volume`, the cubic B-spline resize of the reference's `loadImage`
(dataGenerator/generateData.py:111-150: scipy.ndimage.zoom(order=3, prefilter=False)), through libnaf_hip.so
(`naf_resize_volume`), and `prepare_volume`, `loadImage` itself: HU -> attenuation, resize to nVoxel, normalise to [0, 1].

The definition is written down in include/naf_hip.h (V1) and DESIGN.md section 12: output j of an axis sits at
x = j (a - 1) / (b - 1), the taps floor(x) - 1 .. floor(x) + 2 carry the cubic B-spline weights, taps outside the volume are
mirrored about the edge samples, and nothing is prefiltered (an axis that keeps its extent is still smoothed).  There is no CPU
path, like the rest of the hot path.
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
