"""Detector-row filter on the device (`naf_filter_rows`, include/naf_hip.h P3) and the host-side pieces of the FDK baseline that
feed it: the ramp filter's taps, the angular weights of the views and the cosine weights of the detector.  DESIGN.md section 15.

`filter_rows` convolves every row of a stack of projections [N, H, W] with one symmetric tap array,

    out[i, r, n] = view_scale[i] * post[r, n] * sum_k taps[|n - k|] * (pre[r, k] * in[i, r, k]),

a dense fp32 sum per output (W^2 FMAs per row, no FFT); with a weight per view and column, `col[i, k]`, multiplied onto the input
after `pre` (`naf_filter_rows_views`: Parker's short-scan weights, `parker_weights`).  There is no CPU path, like the rest of the hot path; the float64
restatement the tests compare with is tests/_filter_oracle.py.
"""
from __future__ import annotations

import math

import numpy as np

FILTERS = ("ram-lak", "shepp-logan")
MAX_WIDTH = 16384           # NAF_FILTER_MAX_WIDTH: the row and its taps are staged in LDS


def ramp_taps(W, tau, kind="ram-lak"):
    """The W taps t[m] = tau * h(m tau) of the band-limited ramp filter sampled at spacing `tau` (Kak and Slaney, ch. 3), computed
    in float64 and returned as float32 [W]:
        ram-lak      t[0] = 1 / (4 tau), t[m] = -1 / (pi^2 m^2 tau) for odd m, 0 for even m != 0
        shepp-logan  t[m] = -2 / (pi^2 tau (4 m^2 - 1))"""
    W, tau = int(W), float(tau)
    if W < 1:
        raise ValueError(f"ramp_taps: W must be at least 1, got {W}")
    if not (tau > 0.0) or not math.isfinite(tau):
        raise ValueError(f"ramp_taps: tau must be > 0 and finite, got {tau}")
    m = np.arange(W, dtype=np.float64)
    if kind == "ram-lak":
        t = np.zeros(W, dtype=np.float64)
        t[0] = 1.0 / (4.0 * tau)
        t[1::2] = -1.0 / (np.pi ** 2 * m[1::2] ** 2 * tau)
    elif kind == "shepp-logan":
        t = -2.0 / (np.pi ** 2 * tau * (4.0 * m * m - 1.0))
    else:
        raise ValueError(f"ramp_taps: filter must be one of {FILTERS}, got {kind!r}")
    return t.astype(np.float32)


def view_gaps(angles):
    """The angular step each view stands for, float64 [N] in the order of `angles`: half the sum of the two gaps to the view's
    neighbours among the sorted angles, the single gap for the first and the last.  One view alone gets 1."""
    a = np.asarray(angles, dtype=np.float64).reshape(-1)
    if a.size == 0 or not np.all(np.isfinite(a)):
        raise ValueError("view_weights: angles must be a non-empty list of finite values")
    if a.size == 1:
        return np.ones(1)
    order = np.argsort(a, kind="stable")
    gap = np.diff(a[order])
    step = np.empty(a.size)
    step[0], step[-1] = gap[0], gap[-1]
    step[1:-1] = 0.5 * (gap[:-1] + gap[1:])
    if not step.sum() > 0:
        raise ValueError("view_weights: all angles are equal")
    out = np.empty(a.size)
    out[order] = step
    return out


def view_weights(angles):
    """w_i = pi * gap_i / sum_j gap_j (float64 [N], `view_gaps`): equally spaced views get pi / N each whatever range they cover,
    which is what TIGRE's FDK does."""
    gap = view_gaps(angles)
    return np.pi * gap / gap.sum()


def covered_range(angles):
    """sum of `view_gaps`, radians: N equally spaced views of step g cover N g."""
    a = np.asarray(angles, dtype=np.float64).reshape(-1)
    return float(view_gaps(a).sum()) if a.size > 1 else 0.0


def cosine_weights(geo):
    """cos(gamma) = DSD / sqrt(DSD^2 + u^2 + v^2) at the centre of every detector pixel, float64 [H, W]; u runs along the last axis
    (pitch dDetector[0]), v along the rows, both with the detector's offset, as `RayGenerator` places the pixels."""
    W, H = int(geo.nDetector[0]), int(geo.nDetector[1])
    u = (np.arange(W, dtype=np.float64) + 0.5 - W / 2) * float(geo.dDetector[0]) + float(geo.offDetector[0])
    v = (np.arange(H, dtype=np.float64) + 0.5 - H / 2) * float(geo.dDetector[1]) + float(geo.offDetector[1])
    D = float(geo.DSD)
    return D / np.sqrt(D * D + u[None, :] ** 2 + v[:, None] ** 2)


FAN_SIGN = -1.0             # s of `fan_angles`: the sign for which rays (beta, gamma) and (beta + pi + 2 gamma, -gamma) are one line


def fan_angles(geo):
    """The fan angle of every detector column, float64 [W]: gamma_k = s * atan(u_k / DSD), u_k as in `cosine_weights`.  s = -1:
    `angle2pose` puts the detector's column axis at Rz(angle) e_y and the central ray at -Rz(angle) e_x, so a ray through column
    coordinate u > 0 is turned clockwise from the central ray, and the ray of the opposite sense through the same line leaves the
    source at angle + pi - 2 atan(u / DSD) through column coordinate -u (tests/test_short_scan_cpu.py holds the ray generator to
    that).  A parallel beam has no fan: zeros."""
    W = int(geo.nDetector[0])
    if geo.mode == "parallel":
        return np.zeros(W)
    u = (np.arange(W, dtype=np.float64) + 0.5 - W / 2) * float(geo.dDetector[0]) + float(geo.offDetector[0])
    return FAN_SIGN * np.arctan(u / float(geo.DSD))


def parker_weight(beta_prime, gamma, theta):
    """Parker's short-scan weight as a continuous function: the weight of the ray at fan angle `gamma` of the view at
    `beta_prime` in [0, theta] of a scan that covers `theta` radians, delta = (theta - pi) / 2 (float64, broadcast):
        sin^2(pi/4 * beta' / (delta - gamma))                       where beta' < 2 delta - 2 gamma
        sin^2(pi/4 * (pi + 2 delta - beta') / (delta + gamma))      where beta' > pi - 2 gamma
        1                                                           otherwise
    in that order.  The ray's partner (beta' + pi + 2 gamma, -gamma) is the same line; where both lie in [0, theta] their
    weights sum to 1, and a ray whose partner lies outside keeps 1.  Either region may be empty (theta < pi + 2 |gamma|)."""
    b, g = np.broadcast_arrays(np.asarray(beta_prime, dtype=np.float64), np.asarray(gamma, dtype=np.float64))
    delta = 0.5 * (float(theta) - np.pi)
    head, tail = b < 2.0 * (delta - g), b > np.pi - 2.0 * g
    lo = np.where(head, delta - g, 1.0)                       # a region that is empty never divides
    hi = np.where(tail, delta + g, 1.0)
    rise = np.sin(0.25 * np.pi * b / lo) ** 2
    fall = np.sin(0.25 * np.pi * (np.pi + 2.0 * delta - b) / hi) ** 2
    return np.where(head, rise, np.where(tail, fall, 1.0))


def parker_weights(geo, angles):
    """Parker's weights of a short scan of `geo` at `angles`, float64 [N, W]: `parker_weight(beta'_i, fan_angles(geo)[k], theta)`
    with theta = `covered_range(angles)` and beta'_i = a_i - min(a) + g / 2, g the `view_gaps` entry of the smallest angle, which
    puts every view at the centre of the interval it stands for on [0, theta].  ValueError for fewer than two views, for
    non-finite angles, for a range below pi less half a view step (a limited-angle scan: no weights make it complete) and for one
    above 2 pi less half a view step (a full scan measures every ray twice and needs none)."""
    a = np.asarray(angles, dtype=np.float64).reshape(-1)
    if a.size < 2:
        raise ValueError(f"parker_weights: a short scan needs at least two views, got {a.size}")
    if not np.all(np.isfinite(a)):
        raise ValueError("parker_weights: angles must be finite")
    gaps = view_gaps(a)
    theta = float(gaps.sum())
    half_step = 0.5 * theta / a.size
    if theta < np.pi - half_step:
        raise ValueError(f"parker_weights: the views cover {math.degrees(theta):.2f} degrees, less than 180: a limited-angle scan")
    if theta > 2.0 * np.pi - half_step:
        raise ValueError(f"parker_weights: the views cover {math.degrees(theta):.2f} degrees, a full scan, which needs no "
                         "short-scan weights")
    first = int(np.argmin(a))
    beta = a - a[first] + 0.5 * gaps[first]
    return parker_weight(beta[:, None], fan_angles(geo)[None, :], theta)


def _check_weight(t, shape, like, name):
    import torch
    if t is None:
        return
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.device != like.device:
        raise RuntimeError(f"filter_rows: {name} must be a CUDA/HIP tensor on the projections' device (no CPU path)")
    if t.dtype != torch.float32 or tuple(t.shape) != tuple(shape) or not t.is_contiguous():
        raise ValueError(f"filter_rows: {name} must be a contiguous float32 {tuple(shape)} tensor, got {t.dtype} {tuple(t.shape)}")


def filter_rows(projections, taps, pre=None, post=None, view_scale=None, col=None, out=None):
    """`naf_filter_rows` on CUDA float32 `projections` [N, H, W]: `taps` [W], `pre` / `post` [H, W] or None, `view_scale` [N] or
    None, all float32 on the same device -> float32 [N, H, W].  With `col` [N, W], a weight per view and detector column that
    multiplies the input after `pre`, the call is `naf_filter_rows_views`.  `out` may be `projections` itself (filtering in place)
    or a tensor that does not overlap it; the default allocates."""
    import torch

    from . import _abi
    from .tv import _overlap
    _abi.check_volume(projections, "filter_rows", "projections")
    N, H, W = (int(v) for v in projections.shape)
    if W < 1 or W > MAX_WIDTH:
        raise ValueError(f"filter_rows: the row width must be in 1 .. {MAX_WIDTH}, got {W}")
    if taps is None:
        raise ValueError("filter_rows: taps must be given")
    _check_weight(taps, (W,), projections, "taps")
    _check_weight(pre, (H, W), projections, "pre")
    _check_weight(post, (H, W), projections, "post")
    _check_weight(view_scale, (N,), projections, "view_scale")
    _check_weight(col, (N, W), projections, "col")
    if out is None:
        out = torch.empty_like(projections)
    else:
        _abi.check_volume(out, "filter_rows", "out")
        if tuple(out.shape) != (N, H, W) or out.device != projections.device:
            raise ValueError(f"filter_rows: out must be a contiguous float32 {(N, H, W)} tensor on the input's device")
        if out.data_ptr() != projections.data_ptr() and _overlap(out, projections):
            raise ValueError("filter_rows: out must be the projections themselves or not overlap them")
    if N * H == 0:
        return out
    with torch.cuda.device(projections.device):
        if col is not None:
            _abi.check(_abi.lib().naf_filter_rows_views(_abi.ptr(projections), N, H, W, _abi.ptr(taps), _abi.ptr(pre), _abi.ptr(post),
                                                        _abi.ptr(view_scale), _abi.ptr(col), _abi.ptr(out), _abi.stream_ptr()),
                       "filter_rows_views")
            return out
        _abi.check(_abi.lib().naf_filter_rows(_abi.ptr(projections), N, H, W, _abi.ptr(taps), _abi.ptr(pre), _abi.ptr(post),
                                              _abi.ptr(view_scale), _abi.ptr(out), _abi.stream_ptr()), "filter_rows")
    return out
