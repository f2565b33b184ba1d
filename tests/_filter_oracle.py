"""Float64 numpy restatement of the detector-row filter (include/naf_hip.h, P3) as a direct convolution, its
fp32 error bound, and the FDK rehearsal: `reconstruct.fdk_operators` run in float64 over this convolution and the float64
back-projector of tests/_backproject_oracle.py, on exact line integrals of one centred ball -- not a test module."""
import numpy as np

import _backproject_oracle as B

U = 2.0 ** -24          # unit roundoff of fp32

# (n_views, H, W) of the kernel tests: the smallest widths with a lane tail (37: five lanes, the last with five outputs), a full
# wave of lanes (64 -> 8 lanes; 65 adds a ninth with one output), a partial wave (300: 38 lanes), a row longer than one workgroup pass
# (4099 > 8 x 256) whose LDS image is well past one 4 KiB page, and widths 1 and 2 where every tap index is 0 or 1
SHAPES = [(1, 1, 1), (2, 3, 2), (3, 5, 37), (2, 4, 64), (2, 3, 65), (1, 2, 300), (1, 1, 4099)]


def _rows(x, taps, absolute):
    """sum_k taps[|n - k|] x[..., k] (of the absolute values if `absolute`) for every row of x [..., W], by np.convolve: a direct
    float64 sum, no FFT."""
    x = np.asarray(x, dtype=np.float64)
    t = np.asarray(taps, dtype=np.float64)
    if absolute:
        x, t = np.abs(x), np.abs(t)
    W = x.shape[-1]
    assert t.shape == (W,)
    kernel = np.concatenate([t[:0:-1], t])                        # taps[|m|], m = -(W - 1) .. W - 1
    flat = x.reshape(-1, W)
    out = np.empty_like(flat)
    for i, row in enumerate(flat):
        out[i] = np.convolve(row, kernel)[W - 1:2 * W - 1]
    return out.reshape(x.shape)


def _factors(shape, pre, post, view_scale):
    N, H, W = shape
    pre = np.ones((H, W)) if pre is None else np.asarray(pre, dtype=np.float64)
    post = np.ones((H, W)) if post is None else np.asarray(post, dtype=np.float64)
    s = np.ones(N) if view_scale is None else np.asarray(view_scale, dtype=np.float64)
    return pre[None], post[None], s[:, None, None]


def filter_rows(x, taps, pre=None, post=None, view_scale=None):
    """out[i, r, n] = view_scale[i] post[r, n] sum_k taps[|n - k|] pre[r, k] x[i, r, k] in float64."""
    x = np.asarray(x, dtype=np.float64)
    pre, post, s = _factors(x.shape, pre, post, view_scale)
    return s * post * _rows(pre * x, taps, False)


def filter_bound(x, taps, pre=None, post=None, view_scale=None):
    """Per-element bound on an fp32 evaluation of `filter_rows`: (W + 3) 2^-24 |view_scale post| sum_k |taps pre x|, the standard
    bound of a length-W fma chain plus the three scalings."""
    x = np.asarray(x, dtype=np.float64)
    pre, post, s = _factors(x.shape, pre, post, view_scale)
    return (x.shape[-1] + 3) * U * np.abs(s * post) * _rows(pre * x, taps, True)


def filter_inputs(shape, seed=0):
    """Seeded float32 inputs of a kernel test: (x, taps, pre, post, view_scale); taps of either sign, weights in [0.5, 1.5)."""
    N, H, W = shape
    rng = np.random.default_rng(seed + 7 * N + 13 * H + W)
    x = rng.standard_normal(shape).astype(np.float32)
    taps = (rng.standard_normal(W) / (1.0 + np.arange(W))).astype(np.float32)
    pre = (0.5 + rng.random((H, W))).astype(np.float32)
    post = (0.5 + rng.random((H, W))).astype(np.float32)
    scale = (0.5 + rng.random(N)).astype(np.float32)
    return x, taps, pre, post, scale


# ---- the FDK rehearsal ----------------------------------------------------------------------------------------------------------
# A centred ball of attenuation 1 and radius 0.35 x the volume's side in a cubic volume of n^3 voxels (side 256 mm), detector
# 1.5 n x 1.5 n pixels (side 460.8 mm: the ball's shadow is 292 mm wide), DSO 1000 mm, DSD 1500 mm.  Cone: 2 n views over a full
# turn; parallel: n views over a half turn (detector side 307.2 mm).  Refining n doubles voxels, detector pixels and views.
SIDE_MM = 256.0
BALL_RADIUS = 0.35 * SIDE_MM / 1000
REHEARSAL_SIZES = (16, 32)
_CACHE = {}


def fdk_geometry(n, mode):
    det = 3 * n // 2
    pitch = (460.8 if mode == "cone" else 307.2) / det
    return {"DSD": 1500.0, "DSO": 1000.0, "nDetector": [det, det], "dDetector": [pitch, pitch], "nVoxel": [n] * 3,
            "dVoxel": [SIDE_MM / n] * 3, "offOrigin": [0, 0, 0], "offDetector": [0, 0], "accuracy": 0.5, "mode": mode, "filter": None}


def fdk_angles(n, mode):
    return np.linspace(0, 2 * np.pi, 2 * n + 1)[:-1] if mode == "cone" else np.linspace(0, np.pi, n + 1)[:-1]


def ball_table():
    return {"c": np.zeros((1, 3)), "a": np.full((1, 3), BALL_RADIUS), "R": np.eye(3)[None], "rho": np.ones(1)}


def ball_interior(geo, shrink_voxels=2.0):
    """Mask of the voxels whose centre lies in the ball shrunk by `shrink_voxels` voxels."""
    from neuralvolumetricreconstructionformedicalimages_amd.geometry import get_voxels
    r = BALL_RADIUS - shrink_voxels * float(np.max(geo.dVoxel))
    return np.linalg.norm(get_voxels(geo), axis=-1) <= r


def fdk_case(n, mode):
    """(geo, angles, rays float32 [N H W, 8], b float32 [N, H, W] exact line integrals of the ball, truth float32 [n, n, n])."""
    import torch
    from neuralvolumetricreconstructionformedicalimages_amd import phantom
    from neuralvolumetricreconstructionformedicalimages_amd.geometry import ConeGeometry
    geo = ConeGeometry(fdk_geometry(n, mode))
    angles = fdk_angles(n, mode)
    rays = np.asarray(B.case_rays(geo, angles), dtype=np.float32)
    W, H = int(geo.nDetector[0]), int(geo.nDetector[1])
    b = phantom.line_integrals(torch.tensor(rays), ball_table()).numpy().reshape(len(angles), H, W)
    truth = phantom.volume(geo, ball_table()).numpy()
    return geo, angles, rays, b, truth


def fdk_rehearsal(n, mode, filter="ram-lak"):
    """`fdk_operators` in float64 over `filter_rows` above and `_backproject_oracle.backproject_rays` -> dict with the case, the
    filtered projections `y`, the volume `x`, rho = mean of x over the shrunk ball / 1 and psnr_3d against the voxelised ball.
    Computed once per (n, mode, filter)."""
    key = (n, mode, filter)
    if key not in _CACHE:
        from neuralvolumetricreconstructionformedicalimages_amd.reconstruct import fdk_operators
        from neuralvolumetricreconstructionformedicalimages_amd.utils import get_psnr_3d
        geo, angles, rays, b, truth = fdk_case(n, mode)
        dims = tuple(int(v) for v in geo.nVoxel)
        kept = {}

        def rows(p, taps, pre, post, view_scale):
            kept["weights"] = (taps, pre, post, view_scale)
            kept["y"] = filter_rows(p, taps, pre, post, view_scale)
            return kept["y"]

        def AT(y):
            return B.backproject_rays(np.asarray(y).reshape(-1), geo.dVoxel, rays, dims, geo.accuracy)

        x = fdk_operators(AT, rows, b.astype(np.float64), geo, angles, filter=filter)
        for v in (x, b, truth, kept["y"]):
            v.setflags(write=False)
        _CACHE[key] = {"geo": geo, "angles": angles, "rays": rays, "b": b, "truth": truth, "x": x, "y": kept["y"], "AT": AT,
                       "weights": kept["weights"], "rho": float(x[ball_interior(geo)].mean()),
                       "psnr": float(get_psnr_3d(x, truth))}
    return _CACHE[key]
