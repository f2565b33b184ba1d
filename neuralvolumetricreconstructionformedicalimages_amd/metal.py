"""Metal artefact reduction by sinogram in-painting through libnaf_hip.so (`naf_inpaint_rows`; include/naf_hip.h A4, DESIGN.md section
32): linear-interpolation MAR (Kalender et al., Radiology 164, 1987) and its normalised form NMAR (Meyer et al., Med. Phys. 37, 2010).

A filling or an implant saturates the detector along its trace, and every reconstruction of such rays draws dark streaks between the
metal parts.  The remedy replaces the trace: in every detector row of every view the masked pixels take the value interpolated
between their nearest valid neighbours along the row (`inpaint_rows`).  With a `prior` (the forward projection of a volume in which
soft tissue is flat and bone is kept, `prior_volume`) the interpolation runs on the sinogram divided by the prior's and the result
is multiplied back, which keeps the edges the prior knows about.  The trace is the forward projection of the metal voxels
(`metal_trace`), the metal voxels those of a first reconstruction above a threshold; `reconstruct.reduce_metal` strings the steps
together.  Projections are float32 [N, H, W] on the GPU.  Every output of `inpaint_rows` is the float32 numpy restatement's, bit
for bit.  There is no CPU fallback, like the rest of the hot path.
"""
from __future__ import annotations

import math

import torch

from . import _abi

MAX_W = 16384                       # NAF_INPAINT_MAX_W
MAX_ROWS = 1 << 24
MAX_ALL_ROWS = (1 << 31) - 1


def _check_kind(t, who, name, dtypes, shape):
    """`t` is a tensor of one of `dtypes` and of `shape` (an int: that many dimensions)."""
    kinds = " or ".join(str(d).replace("torch.", "") for d in dtypes)
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{who}: {name} must be a tensor, got {type(t).__name__}")
    if isinstance(shape, int):
        if t.dtype not in dtypes or t.dim() != shape:
            raise ValueError(f"{who}: {name} must be {kinds} [N, H, W], got {t.dtype} {tuple(t.shape)}")
    elif t.dtype not in dtypes or tuple(t.shape) != tuple(shape):
        raise ValueError(f"{who}: {name} must be {kinds} {tuple(shape)}, got {t.dtype} {tuple(t.shape)}")


def _check_device(t, like, who, name):
    if not t.is_cuda:
        raise ValueError(f"{who}: {name} must be a CUDA/HIP tensor (no CPU path)")
    if not t.is_contiguous():
        raise ValueError(f"{who}: {name} must be contiguous")
    if like is not None and t.device != like.device:
        raise ValueError(f"{who}: {name} must be on the device of projections")


def _overlaps(a, b):
    a0, b0 = a.data_ptr(), b.data_ptr()
    return a0 < b0 + b.numel() * b.element_size() and b0 < a0 + a.numel() * a.element_size()


def inpaint_rows(projections, mask, prior=None, eps=None, out=None, counts=False):
    """`projections` (float32 [N, H, W] on the GPU) with the pixels that `mask` marks replaced -> `out` (float32 [N, H, W]; default: a
    new tensor; it may be `projections` itself, and must not overlap anything else).

    mask    uint8 or bool [N, H, W]: non-zero marks a pixel of the trace.  Such a pixel takes q[L] + w (q[R] - q[L]), w = (u - L) /
            (R - L), with L and R the nearest columns of its row that are not masked; with only one of them, that one's value; in a
            row with none it stays as it is.  Every other pixel keeps its bits.
    prior   float32 [N, H, W] or None.  None: q = projections (LI-MAR).  Otherwise q = projections / max(prior, eps) and the
            interpolated value is multiplied by max(prior, eps) of its own pixel (NMAR).
    eps     with a prior only, and then required: finite, > 0
    counts  True: returns (out, counts) with counts [N, 2] as int64: per view the pixels replaced and the masked pixels left"""
    who = "metal.inpaint_rows"
    _check_kind(projections, who, "projections", (torch.float32,), 3)     # shapes, dtypes and numbers first: refused without a GPU too
    N, H, W = projections.shape
    _check_kind(mask, who, "mask", (torch.uint8, torch.bool), (N, H, W))
    if prior is not None:
        _check_kind(prior, who, "prior", (torch.float32,), (N, H, W))
    if out is not None:
        _check_kind(out, who, "out", (torch.float32,), (N, H, W))
    if prior is None:
        if eps is not None:
            raise ValueError(f"{who}: eps is given without a prior")
        eps = 0.0
    else:
        if isinstance(eps, bool) or not isinstance(eps, (int, float)):
            raise ValueError(f"{who}: eps must be a number with a prior, got {eps!r}")
        eps = float(eps)
        if not math.isfinite(eps) or eps <= 0.0:
            raise ValueError(f"{who}: eps must be finite and above zero, got {eps}")
    if N * H * W > 0:
        if W > MAX_W:
            raise ValueError(f"{who}: at most {MAX_W} detector columns, got {W}")
        if H > MAX_ROWS or N * H > MAX_ALL_ROWS:
            raise ValueError(f"{who}: at most 2^24 detector rows and 2^31 - 1 over all views, got {N} x {H}")
    _check_device(projections, None, who, "projections")
    for name, t in (("mask", mask), ("prior", prior), ("out", out)):
        if t is not None:
            _check_device(t, projections, who, name)
    if out is None:
        out = torch.empty_like(projections)
    elif out.numel():
        if out.data_ptr() != projections.data_ptr() and _overlaps(out, projections):
            raise ValueError(f"{who}: out must be projections itself or not overlap it")
        for name, t in (("mask", mask), ("prior", prior)):
            if t is not None and _overlaps(out, t):
                raise ValueError(f"{who}: out must not overlap {name}")
    tally = torch.zeros((N, 2), dtype=torch.int32, device=projections.device) if counts else None
    if projections.numel() > 0:
        with torch.cuda.device(projections.device):
            _abi.check(_abi.lib().naf_inpaint_rows(_abi.ptr(projections), _abi.ptr(mask.view(torch.uint8)), _abi.ptr(prior), eps, N, H, W,
                                                   _abi.ptr(out), _abi.ptr(tally), _abi.stream_ptr()), "inpaint_rows")
    return (out, tally.to(torch.int64) & 0xffffffff) if counts else out


def dilate(trace, grow):
    """A uint8 / bool mask [N, H, W] grown by `grow` pixels along both detector axes (a (2 grow + 1)^2 maximum) -> uint8."""
    grow = int(grow)
    if grow < 0:
        raise ValueError(f"metal: grow must be >= 0, got {grow}")
    trace = trace.to(torch.uint8)
    if grow == 0 or trace.numel() == 0:
        return trace
    grown = torch.nn.functional.max_pool2d(trace[:, None].float(), 2 * grow + 1, stride=1, padding=grow)
    return (grown[:, 0] > 0).to(torch.uint8)


def metal_trace(metal, geo, angles, min_length=0.0, grow=0, kind="interpolated", views_per_call=None):
    """The trace of the voxels `metal` (bool or any number type, [n1, n2, n3] on the GPU: non-zero is metal) on the detector of `geo`
    at `angles`: the pixels whose ray runs more than `min_length` (metres) through metal, grown by `grow` pixels -> uint8 [N, H, W]."""
    from .projector import project_scan
    if not isinstance(metal, torch.Tensor) or metal.dim() != 3:
        raise ValueError("metal.metal_trace: metal must be a tensor [n1, n2, n3]")
    length = project_scan((metal != 0).float().contiguous(), geo, angles, views_per_call=views_per_call, kind=kind)
    return dilate(length > float(min_length), grow)


def prior_volume(x, metal, air, bone):
    """The prior of NMAR from a reconstruction `x` and its metal voxels `metal` (arrays of one kind and shape: torch tensors or numpy
    arrays): voxels below `air` become 0; voxels in [air, bone) and every metal voxel become the mean of the voxels in [air, bone) that
    are not metal (0 if there are none); the others, bone, are kept."""
    air, bone = float(air), float(bone)
    if not air < bone:
        raise ValueError(f"metal.prior_volume: air must be below bone, got {air} and {bone}")
    if tuple(x.shape) != tuple(metal.shape):
        raise ValueError(f"metal.prior_volume: x and metal must have one shape, got {tuple(x.shape)} and {tuple(metal.shape)}")
    metal = metal != 0
    tissue = (x >= air) & (x < bone)
    body = tissue & ~metal
    level = float(x[body].mean()) if bool(body.any()) else 0.0
    out = x.clone() if isinstance(x, torch.Tensor) else x.copy()
    out[x < air] = 0.0
    out[tissue | metal] = level
    return out


def insert_metal(x, metal, value):
    """A copy of the volume `x` with the voxels `metal` set to `value`: the metal put back into a reconstruction of corrected views."""
    if tuple(x.shape) != tuple(metal.shape):
        raise ValueError(f"metal.insert_metal: x and metal must have one shape, got {tuple(x.shape)} and {tuple(metal.shape)}")
    out = x.clone() if isinstance(x, torch.Tensor) else x.copy()
    out[metal != 0] = float(value)
    return out
