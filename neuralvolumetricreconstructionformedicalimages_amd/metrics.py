"""Volume metrics on the device: `ssim_3d`, the reference's 3-D SSIM (src/utils/util.py:87-139 with scikit-image 0.19.3's
defaults, called by train.py:220-288), through libnaf_hip.so (`naf_ssim_3d`).

The definition is written down in include/naf_hip.h (M1) and DESIGN.md section 11: a 7 x 7 x 7 uniform window, sample
covariance, data_range 2, the fp64 mean of S over the interior windows.  The kernel reads both fp32 volumes where they are and
keeps no full-size intermediate.  There is no CPU path, like the rest of the hot path.
"""
from __future__ import annotations

import torch

from . import _abi

WIN_SIZE = 7


def ssim_3d(pred, gt):
    """3-D SSIM of two CUDA float32 volumes [n1, n2, n3] of the same shape -> float (NaN if a NaN reaches a window)."""
    _abi.check_volume(pred, "ssim_3d", "pred")
    _abi.check_volume(gt, "ssim_3d", "gt")
    if pred.shape != gt.shape:
        raise ValueError(f"ssim_3d: pred and gt must have the same shape, got {tuple(pred.shape)} and {tuple(gt.shape)}")
    if pred.device != gt.device:
        raise RuntimeError(f"ssim_3d: pred and gt must be on the same device, got {pred.device} and {gt.device}")
    if min(pred.shape) < WIN_SIZE:
        raise ValueError(f"win_size exceeds image extent: every extent of the volume must be at least {WIN_SIZE}, "
                         f"got shape {tuple(pred.shape)}")
    n1, n2, n3 = (int(v) for v in pred.shape)
    lib = _abi.lib()
    with torch.cuda.device(pred.device):
        ws = torch.empty(lib.naf_ssim_3d_workspace_bytes(n1, n2, n3), dtype=torch.uint8, device=pred.device)
        out = torch.empty(1, dtype=torch.float64, device=pred.device)
        _abi.check(lib.naf_ssim_3d(_abi.ptr(pred), _abi.ptr(gt), n1, n2, n3, _abi.ptr(out), _abi.ptr(ws), ws.numel(),
                                   _abi.stream_ptr()), "ssim_3d")
        return float(out.item())
