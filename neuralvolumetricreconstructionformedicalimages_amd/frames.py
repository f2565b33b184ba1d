"""Raw-frame conditioning through libnaf_hip.so (`naf_frames_condition`; include/naf_hip.h A3): what lies
between the frames a detector delivers and the line integrals every other entry point starts from, in one kernel launch:

  1. the flat-field: t = (raw - dark) / (flat - dark), the transmission;
  2. the repair of zingers (single pixels hit by a stray photon) and of dead pixels: a pixel whose t exceeds the median of its
     size x size neighbourhood in the same view by more than `dif`, or which is bad (marked in `bad`, flat <= dark, t not finite),
     takes the lower median of the neighbourhood's pixels that are not bad;
  3. the negative logarithm, p = -ln(max(t, t_min)).

Steps 1 and 2 are tomopy's `normalize` and `remove_outlier` (bright outliers only, scipy's "reflect" at the edges) and step 3 its
`minus_log`; dead pixels are what neither covers.  The repair is made on the transmission, before the logarithm: a dead pixel's 0 / 0
has no logarithm to repair afterwards, and `dif` is then a difference of transmissions whatever the thickness of the sample.  Frames
are [N, H, W] on the GPU, float32 or uint16.  Without the logarithm every output is a quotient or one of the window's floats, bit
for bit what the float32 numpy restatement gives.  There is no CPU fallback, like the rest of the hot path.
"""
from __future__ import annotations

import math

import torch

from . import _abi
from .dataset import NOISE_I0

SIZES = (3, 5, 7)                   # up to NAF_FRAMES_MAX_SIZE
MAX_EXTENT = 1 << 24
RAW_F32, RAW_U16 = 0, 1             # NAF_FRAMES_RAW_*
LOG, CLAMP_NONNEG = 1, 2            # NAF_FRAMES_*
DEFAULT_T_MIN = 1.0 / NOISE_I0      # one photon of dataset.add_noise's i0: the clamp its counts take before their logarithm


def check_size(size, H, W, who="frames"):
    """`size` as an int: 3, 5 or 7 and at most H and W, else ValueError."""
    if isinstance(size, bool) or not isinstance(size, int):
        raise ValueError(f"{who}: size must be an int, got {size!r}")
    if size not in SIZES:
        raise ValueError(f"{who}: size must be 3, 5 or 7, got {size}")
    if size > H:
        raise ValueError(f"{who}: size {size} is above the {H} detector rows")
    if size > W:
        raise ValueError(f"{who}: size {size} is above the {W} detector columns")
    return size


def _check_number(x, who, name, positive):
    if isinstance(x, bool) or not isinstance(x, (int, float)):
        raise ValueError(f"{who}: {name} must be a number, got {x!r}")
    x = float(x)
    if not math.isfinite(x) or (x <= 0.0 if positive else x < 0.0):
        raise ValueError(f"{who}: {name} must be finite and {'above zero' if positive else 'not negative'}, got {x}")
    return x


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
        raise ValueError(f"{who}: {name} must be on the device of raw")


def _overlaps(a, b):
    a0, b0 = a.data_ptr(), b.data_ptr()
    return a0 < b0 + b.numel() * b.element_size() and b0 < a0 + a.numel() * a.element_size()


def condition(raw, flat, dark, *, dif, bad=None, size=3, t_min=DEFAULT_T_MIN, log=True, clamp=False, out=None, counts=False):
    """`raw` (float32 or uint16 [N, H, W] on the GPU) flat-fielded with `flat` and `dark` (float32 [H, W]), repaired and, with `log`,
    turned into line integrals -> `out` (float32 [N, H, W]; default: a new tensor).  `out` must not overlap an input: a pixel's
    window is read from `raw` while other pixels are stored.

    bad     uint8 or bool [H, W]: non-zero marks a known defective pixel; flat <= dark and a transmission that is not finite
            mark one without it
    size    the window, 3, 5 or 7, at most H and W
    dif     a pixel that is not bad is replaced iff its transmission is more than `dif` above the window's median: finite, >= 0.
            It has no default: it is the noise of the transmission that sets it, and only the caller knows the detector's.
    t_min   the floor of the transmission under the logarithm: finite, > 0; the default is 1 / dataset.NOISE_I0
    clamp   only with `log`: no line integral below zero
    counts  True: returns (out, counts) with counts uint32 [N, 2] as int64: per view the pixels replaced as outliers and as bad"""
    who = "frames.condition"
    _check_kind(raw, who, "raw", (torch.float32, torch.uint16), 3)        # shapes, dtypes and numbers first: refused without a GPU too
    N, H, W = raw.shape
    _check_kind(flat, who, "flat", (torch.float32,), (H, W))
    _check_kind(dark, who, "dark", (torch.float32,), (H, W))
    if bad is not None:
        _check_kind(bad, who, "bad", (torch.uint8, torch.bool), (H, W))
    if out is not None:
        _check_kind(out, who, "out", (torch.float32,), (N, H, W))
    if N * H * W > 0:
        size = check_size(size, H, W, who)
        if H > MAX_EXTENT or W > MAX_EXTENT:
            raise ValueError(f"{who}: H and W are at most 2^24, got {H} x {W}")
    dif = _check_number(dif, who, "dif", positive=False)
    t_min = _check_number(t_min, who, "t_min", positive=True)
    if clamp and not log:
        raise ValueError(f"{who}: clamp needs log")
    _check_device(raw, None, who, "raw")
    for name, t in (("flat", flat), ("dark", dark), ("bad", bad), ("out", out)):
        if t is not None:
            _check_device(t, raw, who, name)
    if out is None:
        out = torch.empty((N, H, W), dtype=torch.float32, device=raw.device)
    else:
        for name, t in (("raw", raw), ("flat", flat), ("dark", dark), ("bad", bad)):
            if t is not None and t.numel() and _overlaps(out, t):
                raise ValueError(f"{who}: out must not overlap {name}")
    tally = torch.zeros((N, 2), dtype=torch.int32, device=raw.device) if counts else None
    if raw.numel() > 0:
        mask = None if bad is None else bad.view(torch.uint8)
        flags = (LOG if log else 0) | (CLAMP_NONNEG if clamp else 0)
        with torch.cuda.device(raw.device):
            _abi.check(_abi.lib().naf_frames_condition(_abi.ptr(raw), RAW_F32 if raw.dtype == torch.float32 else RAW_U16, _abi.ptr(dark),
                                                       _abi.ptr(flat), _abi.ptr(mask), N, H, W, size, dif, t_min, flags, _abi.ptr(out),
                                                       _abi.ptr(tally), _abi.stream_ptr()), "frames_condition")
    return (out, tally.to(torch.int64) & 0xffffffff) if counts else out
