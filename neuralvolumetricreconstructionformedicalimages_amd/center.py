"""Centre-of-rotation search through libnaf_hip.so (`naf_center_slices`, `naf_center_metrics`; include/naf_hip.h A5, DESIGN.md
section 34): the estimator of tomopy's `find_center` (Donath et al., J. Opt. Soc. Am. A 23, 2006).

Every entry point takes `offDetector[0]` of a scan as exact; on a real scanner the projected rotation axis is known to a few pixels,
and an error of one pixel draws tuning-fork streaks and doubled edges in every reconstruction.  The remedy is a number: reconstruct
one slice for each of K candidate offsets of the detector's column axis (`slices`, one launch for all K from rows that were filtered
once on the nominal geometry), score each slice (`metrics`) and add the best candidate to `offDetector[0]`
(`reconstruct.find_center`, `reconstruct.recenter`).  Filtered rows are float32 [S, N, W] on the GPU, slices float32 [S, K, n, n],
`f[s, k, ix, iy]` on the x and y voxel centres of the volume.  There is no CPU fallback, like the rest of the hot path; the float64
restatement the tests compare with is tests/_center_oracle.py.

A tilted-axis (laminographic) parallel-beam scan has two such numbers, the projected rotation axis and the tilt, and a pixel's
detector row moves with the view: `tilted_scalars`, `tilted_mask_radius` and `slices_tilted` (`naf_center_slices_tilted`, DESIGN.md
section 35) are the same search on whole filtered views [N, H, W], a candidate being an (offset, tilt) pair and a slice a height z;
`metrics` scores both kinds.  Their restatement is tests/_lamino_oracle.py.
"""
from __future__ import annotations

import math

import numpy as np

MAX_W = 16384                       # NAF_CENTER_MAX_W
MAX_K = 64                          # NAF_CENTER_MAX_K
MAX_SIZE = 4096                     # NAF_CENTER_MAX_SIZE
GROUP = 8                           # NAF_CENTER_GROUP: candidates one workgroup takes
METRICS = ("negativity", "sharpness")


def scalars(geo):
    """What `naf_center_slices` takes of a geometry, as a dict of Python numbers: parallel, DSO, DSD, du, ou, W, n, dx, dy, ox, oy.
    ValueError for a tilted scan, an unknown mode and a slice that is not square."""
    if geo.mode not in ("cone", "parallel"):
        raise ValueError(f"center: mode must be 'cone' or 'parallel', got {geo.mode!r}")
    if float(geo.tilt_angle) != 0.0:
        raise ValueError(f"center: a tilted (laminographic) scan is not supported, got tilt_angle {geo.tilt_angle}")
    n1, n2 = int(geo.nVoxel[0]), int(geo.nVoxel[1])
    if n1 != n2:
        raise ValueError(f"center: the slice must be square, got nVoxel {n1} x {n2}")
    return {"parallel": int(geo.mode == "parallel"), "DSO": float(geo.DSO), "DSD": float(geo.DSD), "du": float(geo.dDetector[0]),
            "ou": float(geo.offDetector[0]), "W": int(geo.nDetector[0]), "n": n1, "dx": float(geo.dVoxel[0]), "dy": float(geo.dVoxel[1]),
            "ox": float(geo.offOrigin[0]), "oy": float(geo.offOrigin[1])}


def trig(angles):
    """(cos a_i, sin a_i), formed in float64 and rounded once -> float32 numpy [N, 2]."""
    a = np.asarray(angles, dtype=np.float64).reshape(-1)
    return np.stack([np.cos(a), np.sin(a)], -1).astype(np.float32)


def candidates(max_shift, step):
    """The symmetric grid of candidate offsets in pixels, 0 included: step * (-m .. m) with m = floor(max_shift / step), float64.
    ValueError for more than 64 values, and for a max_shift or step that is not finite and above zero."""
    max_shift, step = float(max_shift), float(step)
    if not (math.isfinite(max_shift) and math.isfinite(step)) or not step > 0.0 or not max_shift > 0.0:
        raise ValueError(f"center.candidates: max_shift and step must be finite and above zero, got {max_shift} and {step}")
    m = int(math.floor(max_shift / step + 1e-9))
    if 2 * m + 1 > MAX_K:
        raise ValueError(f"center.candidates: at most {MAX_K} candidates, got {2 * m + 1} for max_shift {max_shift} and step {step}")
    return step * np.arange(-m, m + 1, dtype=np.float64)


def midplane_rows(geo):
    """(r0, r1, w): the row at v = 0 is (1 - w) row r0 + w row r1 under `offDetector[1]`.  ValueError if v = 0 is off the detector,
    that is outside the span of the rows' centres."""
    H, dv, ov = int(geo.nDetector[1]), float(geo.dDetector[1]), float(geo.offDetector[1])
    at = H / 2 - 0.5 - ov / dv                                       # v_r = (r + 0.5 - H / 2) dv + ov
    if not -1e-9 <= at <= H - 1 + 1e-9:
        raise ValueError(f"center.midplane: v = 0 is off the detector (row coordinate {at:.3f} of {H} rows)")
    at = min(max(at, 0.0), float(H - 1))
    r0 = min(int(math.floor(at)), max(H - 2, 0))
    return r0, min(r0 + 1, H - 1), at - r0


def midplane(filtered, geo):
    """The row at v = 0 of filtered projections [N, H, W] (a torch tensor or a numpy array) -> [1, N, W]: the linear blend of the two
    rows that bracket v = 0 under `offDetector[1]`."""
    if len(filtered.shape) != 3 or int(filtered.shape[1]) != int(geo.nDetector[1]):
        raise ValueError(f"center.midplane: filtered must be [N, {int(geo.nDetector[1])}, W], got {tuple(filtered.shape)}")
    r0, r1, w = midplane_rows(geo)
    return ((1.0 - w) * filtered[:, r0] + w * filtered[:, r1])[None]


def mask_radius(geo, max_shift):
    """The largest radius (metres) about the slice's origin at which every pixel projects between the centres of the first and the
    last detector column in every view for every candidate within +-`max_shift` pixels, capped by the circle inscribed in the
    pixel centres of the slice.  ValueError if nothing is left."""
    g = scalars(geo)
    reach = (g["W"] / 2 - 0.5) * g["du"] - abs(g["ou"]) - abs(float(max_shift)) * g["du"]
    if g["parallel"]:
        rho = reach
    else:
        rho = g["DSO"] * reach / math.sqrt(g["DSD"] ** 2 + reach ** 2) if reach > 0 else reach
    r = min(rho - math.hypot(g["ox"], g["oy"]), 0.5 * (g["n"] - 1) * min(g["dx"], g["dy"]))
    if not r > 0.0:
        raise ValueError(f"center.mask_radius: no pixel of the slice stays on the detector for shifts of +-{max_shift} pixels")
    return r


def _check(t, shape, like, who, name, dtype=None):
    import torch
    dtype = dtype or torch.float32
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{who}: {name} must be a tensor, got {type(t).__name__}")
    if t.dtype != dtype or (shape is not None and tuple(t.shape) != tuple(shape)):
        raise ValueError(f"{who}: {name} must be {str(dtype).replace('torch.', '')} {tuple(shape) if shape is not None else ''}, got "
                         f"{t.dtype} {tuple(t.shape)}")
    if not t.is_cuda:
        raise RuntimeError(f"{who}: {name} must be a CUDA/HIP tensor (no CPU path)")
    if not t.is_contiguous():
        raise ValueError(f"{who}: {name} must be contiguous")
    if like is not None and t.device != like.device:
        raise ValueError(f"{who}: {name} must be on the device of the other arguments")


def slices(q, geo, angles, candidates, out=None):
    """`naf_center_slices`: the slice z = 0 .. of filtered rows `q` (float32 [S, N, W] on the GPU, one slice per leading index)
    back-projected for every candidate offset -> float32 [S, K, n, n].  `candidates` are offsets in METRES added to
    `geo.offDetector[0]` (a sequence of at most 64); `angles` one per view."""
    import torch

    from . import _abi
    who = "center.slices"
    g = scalars(geo)
    cand = np.asarray(candidates, dtype=np.float64).reshape(-1)
    if not 1 <= cand.size <= MAX_K or not np.all(np.isfinite(cand)):
        raise ValueError(f"{who}: 1 .. {MAX_K} finite candidates are needed, got {cand.size}")
    tr = trig(angles)
    if not isinstance(q, torch.Tensor) or q.dim() != 3:
        raise ValueError(f"{who}: q must be a float32 tensor [S, N, W]")
    S, N, W = (int(v) for v in q.shape)
    if N != tr.shape[0] or N < 1 or W != g["W"]:
        raise ValueError(f"{who}: q must be [S, {tr.shape[0]}, {g['W']}] with one view per angle, got {tuple(q.shape)}")
    if W > MAX_W or g["n"] > MAX_SIZE:
        raise ValueError(f"{who}: at most {MAX_W} detector columns and {MAX_SIZE} pixels along a side, got {W} and {g['n']}")
    _check(q, (S, N, W), None, who, "q")
    K, n = cand.size, g["n"]
    if out is None:
        out = torch.empty((S, K, n, n), dtype=torch.float32, device=q.device)
    else:
        _check(out, (S, K, n, n), q, who, "out")
    if S * n == 0:
        return out
    trig_d = torch.tensor(tr, device=q.device)
    cand_d = torch.tensor(cand.astype(np.float32), device=q.device)
    with torch.cuda.device(q.device):
        _abi.check(_abi.lib().naf_center_slices(_abi.ptr(q), _abi.ptr(trig_d), _abi.ptr(cand_d), S, N, W, K, n, g["parallel"], g["DSO"],
                                                g["DSD"], g["du"], g["ou"], g["dx"], g["dy"], g["ox"], g["oy"], _abi.ptr(out),
                                                _abi.stream_ptr()), "center_slices")
    return out


def tilted_scalars(geo):
    """What `naf_center_slices_tilted` takes of a tilted-axis (laminographic) geometry, as a dict of Python numbers: tilt (degrees),
    du, dv, ou, ov, W, H, n, dx, dy, ox, oy.  ValueError unless the beam is parallel, the tilt strictly between 0 and 90 degrees and
    the slice square.  `scalars` keeps refusing such a scan: the untilted kernel has no row axis."""
    if geo.mode != "parallel":
        raise ValueError(f"center (tilted): mode must be 'parallel', got {geo.mode!r}: cone-beam laminography is not supported")
    tilt = float(geo.tilt_angle)
    if not 0.0 < tilt < 90.0:
        raise ValueError(f"center (tilted): tilt_angle must lie strictly between 0 and 90 degrees, got {geo.tilt_angle}; an untilted scan "
                         "is searched by find_center")
    n1, n2 = int(geo.nVoxel[0]), int(geo.nVoxel[1])
    if n1 != n2:
        raise ValueError(f"center (tilted): the slice must be square, got nVoxel {n1} x {n2}")
    return {"tilt": tilt, "du": float(geo.dDetector[0]), "dv": float(geo.dDetector[1]), "ou": float(geo.offDetector[0]),
            "ov": float(geo.offDetector[1]), "W": int(geo.nDetector[0]), "H": int(geo.nDetector[1]), "n": n1,
            "dx": float(geo.dVoxel[0]), "dy": float(geo.dVoxel[1]), "ox": float(geo.offOrigin[0]), "oy": float(geo.offOrigin[1])}


def _tilts(g, tilts, K, who):
    """One tilt in degrees per candidate, float64 [K]: the scan's own where `tilts` is None."""
    if tilts is None:
        return np.full(K, g["tilt"], dtype=np.float64)
    t = np.asarray(tilts, dtype=np.float64).reshape(-1)
    if t.size != K or not np.all(np.isfinite(t)) or not np.all((t > 0.0) & (t < 90.0)):
        raise ValueError(f"{who}: tilts must be {K} finite values strictly between 0 and 90 degrees, one per candidate")
    return t


def tilted_candidates(candidates, tilts):
    """The candidate table of `naf_center_slices_tilted`: (c_k / du in pixels, sin tau_k, cos tau_k), formed in float64 and rounded
    once -> float32 numpy [K, 3].  `candidates` in pixels, `tilts` in degrees."""
    c = np.asarray(candidates, dtype=np.float64).reshape(-1)
    t = np.radians(np.asarray(tilts, dtype=np.float64).reshape(-1))
    return np.stack([c, np.sin(t), np.cos(t)], -1).astype(np.float32)


def tilted_mask_radius(geo, max_shift, tilts=None, z=(0.0,)):
    """The largest radius (metres) about the slice's origin at which every pixel of every slice height in `z` (metres) projects
    between the centres of the first and the last detector column AND row, in every view, for every candidate within +-`max_shift`
    pixels and every tilt in `tilts` (degrees; None: the scan's own), capped by the circle inscribed in the pixel centres of the
    slice.  ValueError if nothing is left."""
    g = tilted_scalars(geo)
    t = np.radians(_tilts(g, tilts, 1 if tilts is None else np.asarray(tilts).size, "center.tilted_mask_radius"))
    zs = np.abs(np.asarray(z, dtype=np.float64).reshape(-1))
    if zs.size < 1 or not np.all(np.isfinite(zs)):
        raise ValueError("center.tilted_mask_radius: z must be a non-empty list of finite heights")
    reach_u = (g["W"] / 2 - 0.5) * g["du"] - abs(g["ou"]) - abs(float(max_shift)) * g["du"]
    reach_v = (g["H"] / 2 - 0.5) * g["dv"] - abs(g["ov"])
    rho_v = float(np.min((reach_v - np.cos(t) * zs.max()) / np.sin(t)))         # |sin tau s - cos tau z| <= sin tau rho + cos tau |z|
    r = min(min(reach_u, rho_v) - math.hypot(g["ox"], g["oy"]), 0.5 * (g["n"] - 1) * min(g["dx"], g["dy"]))
    if not r > 0.0:
        raise ValueError(f"center.tilted_mask_radius: no pixel of the slice stays on the detector for shifts of +-{max_shift} pixels, "
                         f"the tilts and the heights given")
    return r


def slices_tilted(q, geo, angles, candidates, tilts=None, z=(0.0,), out=None):
    """`naf_center_slices_tilted`: the slices at the heights `z` (metres, S of them) of a tilted-axis parallel-beam scan,
    back-projected from whole filtered views `q` (float32 [N, H, W] on the GPU) for every candidate -> float32 [S, K, n, n].
    `candidates` are offsets in METRES added to `geo.offDetector[0]` (at most 64), `tilts` one tilt in degrees per candidate (None:
    the scan's own for all of them), `angles` one per view.  Each slice carries its candidate's Jacobian cos(tilt); the weights of
    `reconstruct.lamino_fbp_weights` are expected in `q` with the nominal tilt's cosine taken out (`find_center_tilted` does that)."""
    import ctypes

    import torch

    from . import _abi
    who = "center.slices_tilted"
    g = tilted_scalars(geo)
    cand = np.asarray(candidates, dtype=np.float64).reshape(-1)
    if not 1 <= cand.size <= MAX_K or not np.all(np.isfinite(cand)):
        raise ValueError(f"{who}: 1 .. {MAX_K} finite candidates are needed, got {cand.size}")
    table = np.ascontiguousarray(tilted_candidates(cand / g["du"], _tilts(g, tilts, cand.size, who)))
    heights = np.asarray(z, dtype=np.float64).reshape(-1)
    if heights.size < 1 or not np.all(np.isfinite(heights)):
        raise ValueError(f"{who}: z must be a non-empty list of finite heights, got {z!r}")
    tr = trig(angles)
    if not isinstance(q, torch.Tensor) or q.dim() != 3:
        raise ValueError(f"{who}: q must be a float32 tensor [N, H, W]")
    N, H, W = (int(v) for v in q.shape)
    if N != tr.shape[0] or N < 1 or W != g["W"] or H != g["H"]:
        raise ValueError(f"{who}: q must be [{tr.shape[0]}, {g['H']}, {g['W']}] with one view per angle, got {tuple(q.shape)}")
    if W > MAX_W or W < 2 or H < 2 or g["n"] > MAX_SIZE:
        raise ValueError(f"{who}: 2 .. {MAX_W} detector columns, at least 2 rows and at most {MAX_SIZE} pixels along a side, got "
                         f"{W}, {H} and {g['n']}")
    _check(q, (N, H, W), None, who, "q")
    S, K, n = heights.size, cand.size, g["n"]
    if out is None:
        out = torch.empty((S, K, n, n), dtype=torch.float32, device=q.device)
    else:
        _check(out, (S, K, n, n), q, who, "out")
    if n == 0:
        return out
    trig_d = torch.tensor(tr, device=q.device)
    z_d = torch.tensor(heights.astype(np.float32), device=q.device)
    with torch.cuda.device(q.device):
        _abi.check(_abi.lib().naf_center_slices_tilted(_abi.ptr(q), _abi.ptr(trig_d), table.ctypes.data_as(ctypes.c_void_p), _abi.ptr(z_d),
                                                       S, N, H, W, K, n, g["du"], g["dv"], g["ou"], g["ov"], g["dx"], g["dy"], g["ox"],
                                                       g["oy"], _abi.ptr(out), _abi.stream_ptr()), "center_slices_tilted")
    return out


def slice_grid(geo):
    """What `metrics` reads of a geometry, tilted or not: n, dx, dy of the square slice.  ValueError for a slice that is not square."""
    n1, n2 = int(geo.nVoxel[0]), int(geo.nVoxel[1])
    if n1 != n2:
        raise ValueError(f"center: the slice must be square, got nVoxel {n1} x {n2}")
    return {"n": n1, "dx": float(geo.dVoxel[0]), "dy": float(geo.dVoxel[1])}


def metrics_workspace(S, K, n, device):
    """The workspace of `metrics` for slices [S, K, n, n]: a float64 tensor on `device`."""
    import torch

    from . import _abi
    need = int(_abi.lib().naf_center_metrics_workspace_bytes(int(S), int(K), int(n)))
    return torch.empty(max(need // 8, 1), dtype=torch.float64, device=device)


def metrics(f, geo, radius, workspace=None):
    """`naf_center_metrics` on slices `f` (float32 [S, K, n, n] on the GPU) -> float64 [S, K, 2] on the device: per slice and
    candidate the negativity sum -min(f, 0) and the sharpness sum |f[x+1, y] - f[x, y]| + |f[x, y+1] - f[x, y]| over the pixels, and
    the forward differences with both ends, within `radius` (metres) of the slice's centre.  fp64 sums in a fixed order: two calls
    return the same bits.  `workspace` is `metrics_workspace(...)`, allocated if None."""
    import torch

    from . import _abi
    who = "center.metrics"
    g = slice_grid(geo)
    radius = float(radius)
    if not math.isfinite(radius) or radius < 0.0:
        raise ValueError(f"{who}: radius must be finite and not below zero, got {radius}")
    if not isinstance(f, torch.Tensor) or f.dim() != 4 or int(f.shape[2]) != g["n"] or int(f.shape[3]) != g["n"]:
        raise ValueError(f"{who}: f must be a float32 tensor [S, K, {g['n']}, {g['n']}]")
    _check(f, tuple(f.shape), None, who, "f")
    S, K, n = int(f.shape[0]), int(f.shape[1]), g["n"]
    if n > MAX_SIZE:
        raise ValueError(f"{who}: at most {MAX_SIZE} pixels along a side, got {n}")
    out = torch.zeros((S, K, 2), dtype=torch.float64, device=f.device)
    if S * K * n == 0:
        return out
    need = int(_abi.lib().naf_center_metrics_workspace_bytes(S, K, n))
    if workspace is None:
        workspace = metrics_workspace(S, K, n, f.device)
    else:
        _check(workspace, None, f, who, "workspace", torch.float64)
        if workspace.numel() * 8 < need:
            raise ValueError(f"{who}: workspace too small ({workspace.numel() * 8} bytes, need {need})")
    with torch.cuda.device(f.device):
        _abi.check(_abi.lib().naf_center_metrics(_abi.ptr(f), S, K, n, g["dx"], g["dy"], radius, _abi.ptr(out), _abi.ptr(workspace),
                                                 workspace.numel() * 8, _abi.stream_ptr()), "center_metrics")
    return out
