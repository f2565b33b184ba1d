"""numpy restatement of the centre-of-rotation search (include/naf_hip.h A5): `slices` is
`naf_center_slices` in float64, or in float32 with every operation rounded as csrc/center_device.h rounds it; `metrics` is
`naf_center_metrics` in float64; `find_center` runs `reconstruct.find_center_operators` over them and the float64 row filter of
tests/_filter_oracle.py.  The inputs are the float32 values the kernel is given."""
import numpy as np

import _filter_oracle as F

GROUP = 8                                                           # NAF_CENTER_GROUP
LDS_FLOATS = 8192                                                   # kCenterLdsFloats: a view chunk splits where N W exceeds it


def coord(n, d, o, dtype):
    i = np.arange(n).astype(dtype)
    return (i - dtype(0.5) * dtype(n - 1)) * dtype(d) + dtype(o)


def slices(q, trig, cand, g, dtype=np.float64):
    """q [S, N, W], trig [N, 2], cand [K] (metres), g = center.scalars(geo) -> f [S, K, n, n] in `dtype`."""
    T = dtype
    q = np.asarray(q, dtype=np.float32).astype(T)
    trig, cand = np.asarray(trig, dtype=np.float32).astype(T), np.asarray(cand, dtype=np.float32).astype(T)
    S, N, W = q.shape
    n, K = int(g["n"]), cand.size
    x = coord(n, np.float32(g["dx"]), np.float32(g["ox"]), T)[:, None]
    y = coord(n, np.float32(g["dy"]), np.float32(g["oy"]), T)[None, :]
    DSO, DSD, ou, du = (T(np.float32(g[k])) for k in ("DSO", "DSD", "ou", "du"))
    inv_du = T(1) / du
    half = T(0.5) * T(W) - T(0.5)
    shift = cand / du
    f = np.zeros((S, K, n, n), dtype=T)
    for i in range(N):
        ca, sa = trig[i]
        t = y * ca - x * sa
        if g["parallel"]:
            ustar, weight = t, np.ones_like(t)
        else:
            s = x * ca + y * sa
            U = DSO - s
            ustar = DSD * t / U
            m = DSO / U
            weight = m * m
        base = (ustar - ou) * inv_du + half
        for k in range(K):
            col = base - shift[k]
            fl = np.floor(col)
            ok = (fl >= 0) & (fl <= W - 2)
            j = np.where(ok, fl, 0).astype(np.int64)
            j = np.minimum(j, max(W - 2, 0))
            w = col - fl
            for s_ in range(S):
                row = q[s_, i]
                lo = row[j]
                hi = row[np.minimum(j + 1, W - 1)]
                v = np.where(ok, lo + w * (hi - lo), T(0))
                f[s_, k] = f[s_, k] + weight * v
    return f


def mask(n, dx, dy, r):
    mid = 0.5 * (n - 1)
    X = (np.arange(n, dtype=np.float64) - mid) * float(np.float32(dx))
    Y = (np.arange(n, dtype=np.float64) - mid) * float(np.float32(dy))
    return X[:, None] * X[:, None] + Y[None, :] * Y[None, :] <= float(np.float32(r)) * float(np.float32(r))


def metrics(f, dx, dy, r):
    """f [S, K, n, n] (any float type; taken as given) -> float64 [S, K, 2]."""
    f = np.asarray(f).astype(np.float64)
    n = f.shape[-1]
    m = mask(n, dx, dy, r)
    neg = -(np.minimum(f, 0.0) * m).sum((-1, -2)) if n else np.zeros(f.shape[:2])
    gx = np.abs(f[..., 1:, :] - f[..., :-1, :]) * (m[1:, :] & m[:-1, :])
    gy = np.abs(f[..., :, 1:] - f[..., :, :-1]) * (m[:, 1:] & m[:, :-1])
    return np.stack([neg, gx.sum((-1, -2)) + gy.sum((-1, -2))], -1)


def filter_rows(b, taps, pre, post, view_scale, col=None):
    """The float64 row filter on the float32 weights `fdk_weights` returns; `col` multiplies the input after `pre`."""
    b = np.asarray(b, dtype=np.float64)
    if col is not None:
        b = b * np.asarray(col, dtype=np.float64)[:, None, :]
    return F.filter_rows(b, taps, pre, post, view_scale)


def find_center(b, geo, angles, max_shift, step, metric=None, rows=None, short_scan=None, dtype=np.float64, force=False):
    """`reconstruct.find_center` over the restatements above -> (candidates px, scores, metric).  `force` searches a case the
    product refuses (a cone scan under a full turn), for the rehearsal."""
    from neuralvolumetricreconstructionformedicalimages_amd import center, reconstruct as R
    cand = center.candidates(max_shift, step)
    metric = R.center_metric(angles) if metric is None else metric
    g = center.scalars(geo)
    radius = center.mask_radius(geo, max_shift)
    tr = center.trig(angles)

    def run():
        return R.find_center_operators(filter_rows, lambda q, c: slices(q.astype(np.float32), tr, c, g, dtype),
                                       lambda f: metrics(f, g["dx"], g["dy"], radius), np.asarray(b), geo, angles, cand, metric, rows,
                                       short_scan=short_scan)
    if not force:
        return cand, run(), metric
    keep = dict(R.CENTER_CONE_SHORT_SCAN)
    try:
        R.CENTER_CONE_SHORT_SCAN.update({None: True, "parker": True})
        return cand, run(), metric
    finally:
        R.CENTER_CONE_SHORT_SCAN.update(keep)


def planted_scan(n, mode, planted_px, n_views, total=np.pi):
    """A phantom scan whose projections were taken with offDetector[0] = planted_px pixels while the returned geometry states 0
    -> (projections float32 [N, H, W], nominal geometry, angles, the scan dict)."""
    from neuralvolumetricreconstructionformedicalimages_amd import dataset, phantom
    from neuralvolumetricreconstructionformedicalimages_amd.geometry import ConeGeometry
    angles = np.linspace(0.0, total, n_views + 1)[:-1]
    data = dataset.plant_center_offset(phantom.scan_geometry(n, mode), planted_px, n_val=1, train_angles=angles)
    return np.asarray(data["train"]["projections"], dtype=np.float32), ConeGeometry(data), angles, data


# The slice cases of tests/test_hip_center.py and tools/center_host_check.py: (name, n, W, N, K, S, mode, ou in pixels, origin in
# pixels, half-width of the candidates in pixels).  A detector a little wider than the slice's shadow, so that candidates of a
# third of its width push part of every row's reach off either end.
def _cases():
    out = []
    for n in (15, 16, 17, 33):
        out.append((f"n{n}", n, 64, 3, 1, 1, "cone", 0.0, (0.0, 0.0), 2.0))
    for W in (63, 64, 65, 130):
        out.append((f"W{W}", 17, W, 3, GROUP, 1, "parallel", 0.0, (0.0, 0.0), 3.0))
    for N in (1, 3, 50):
        out.append((f"N{N}", 16, 65, N, 3, 1, "cone", 0.0, (0.0, 0.0), 2.0))
    for K in (1, GROUP, GROUP + 1):
        out.append((f"K{K}", 17, 63, 3, K, 3, "parallel" if K == GROUP else "cone", 0.0, (0.0, 0.0), 4.0))
    out.append(("offsets-cone", 33, 130, 5, GROUP + 1, 3, "cone", 2.75, (1.5, -2.25), 3.0))
    out.append(("offsets-parallel", 33, 130, 5, GROUP + 1, 1, "parallel", -1.25, (-0.5, 3.0), 3.0))
    out.append(("leaves-cone", 17, 64, 7, 2 * GROUP + 1, 1, "cone", 0.0, (0.0, 0.0), 24.0))
    out.append(("leaves-parallel", 17, 65, 7, 2 * GROUP + 1, 1, "parallel", 0.0, (0.0, 0.0), 24.0))
    out.append(("chunk-split", 17, 200, 50, 3, 1, "cone", 0.5, (0.0, 0.0), 2.0))            # 50 x 200 floats: chunks of 40 and 10 views
    out.append(("one-row-chunks", 16, LDS_FLOATS + 8, 3, 2, 1, "parallel", 0.0, (0.0, 0.0), 2.0))
    return out


CASES = _cases()
# The largest |float32 restatement - float64| / max |float64| over CASES, measured on the CPU; the GPU test
# allows four times it.
F32_ERROR = 2.46e-5


def case_geometry(case):
    """A geometry object with the fields `center.scalars` reads."""
    from types import SimpleNamespace
    _, n, W, N, K, S, mode, ou_px, origin, span = case
    dx = 1e-2                                                       # a slice of up to a third of DSO: a real cone
    du = 1.3 * 1.5 * n * dx / W if mode == "cone" else 1.3 * n * dx / W
    return SimpleNamespace(mode=mode, tilt_angle=0, DSO=1.0, DSD=1.5, nDetector=np.array([W, 4]), dDetector=np.array([du, du]),
                           offDetector=np.array([ou_px * du, 0.0]), nVoxel=np.array([n, n, 4]), dVoxel=np.array([dx, dx, dx]),
                           offOrigin=np.array([origin[0] * dx, origin[1] * dx, 0.0]))


def case_inputs(case):
    """-> (geo, angles float64 [N], candidates in metres float64 [K], q float32 [S, N, W])."""
    name, n, W, N, K, S, mode, ou_px, origin, span = case
    geo = case_geometry(case)
    rng = np.random.default_rng(sum(name.encode()))
    angles = np.sort(rng.uniform(0.0, 2.0 * np.pi, N))
    cand = (np.linspace(-span, span, K) if K > 1 else np.array([0.37 * span])) * float(geo.dDetector[0])
    q = rng.standard_normal((S, N, W)).astype(np.float32)
    if W > 1024:                                                     # a smooth row: at 2^13 columns a float32 column coordinate is
        u = np.arange(W) / 97.0                                      # 2^-10 coarse, and white noise would make that the whole bound
        q = (rng.standard_normal((S, N, 1)) * np.sin(2.0 * np.pi * (u + rng.random((S, N, 1))))).astype(np.float32)
    return geo, angles, cand, q


def case_reference(case, dtype=np.float64):
    from neuralvolumetricreconstructionformedicalimages_amd import center
    geo, angles, cand, q = case_inputs(case)
    return slices(q, center.trig(angles), cand, center.scalars(geo), dtype)


def measure_f32_error():
    worst = 0.0
    for case in CASES:
        f64, f32 = case_reference(case), case_reference(case, np.float32)
        worst = max(worst, float(np.abs(f32.astype(np.float64) - f64).max() / np.abs(f64).max()))
    return worst
