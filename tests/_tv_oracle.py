"""Float64 numpy restatement of the 3-D total variation, its gradient and normalised descent (include/naf_hip.h, V2; DESIGN.md
section 14) -- not a test module.

    D_a f[v] = f[v] - f[v - e_a] if v_a > 0, else 0;   m[v] = sqrt(eps + sum_a (D_a f[v])^2);   TV = sum_v m[v]
    g[v] = (sum_a D_a f[v]) / m[v]  -  sum_a [v_a < n_a - 1] D_a f[v + e_a] / m[v + e_a]

tests/test_tv_cpu.py pins `gradient` to torch autograd of a five-line TV and to central differences of `tv`."""
import numpy as np

SHAPES = [(1, 1, 1), (2, 3, 1), (5, 1, 7), (17, 9, 33)]
# the kernel's further shapes; (19, 21, 70): 3 x 3 workgroup tiles of 8 x 32 and three axis-0 chunks of 7, the last tile / chunk of
# every axis partial
GPU_SHAPES = [(40, 29, 53), (19, 21, 70)]
DESCENT_STEP, DESCENT_STEPS = 0.5, 20               # the descent tests: 20 steps of length 0.5 from the noisy 32^3 phantom
KINDS = ["random", "phantom", "noisy"]
EPS = [1e-8, 1e-4]


def _lower(a):
    """Index tuples (v with v_a > 0, the same voxels shifted by -e_a) of a 3-D array."""
    hi = tuple(slice(1, None) if k == a else slice(None) for k in range(3))
    lo = tuple(slice(None, -1) if k == a else slice(None) for k in range(3))
    return hi, lo


def differences(f):
    """[D_0 f, D_1 f, D_2 f] in float64."""
    f = np.asarray(f, dtype=np.float64)
    if f.ndim != 3 or min(f.shape) < 1:
        raise ValueError(f"tv: a volume [n1, n2, n3] with every extent >= 1 expected, got shape {f.shape}")
    out = []
    for a in range(3):
        d = np.zeros_like(f)
        hi, lo = _lower(a)
        d[hi] = f[hi] - f[lo]
        out.append(d)
    return out


def magnitude(f, eps):
    d = differences(f)
    return np.sqrt(eps + d[0] * d[0] + d[1] * d[1] + d[2] * d[2])


def tv(f, eps=1e-8):
    return float(magnitude(f, eps).sum())


def gradient(f, eps=1e-8):
    """g = dTV/df, float64, of f's shape."""
    d = differences(f)
    m = np.sqrt(eps + d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
    g = (d[0] + d[1] + d[2]) / m
    for a in range(3):
        q = d[a] / m
        hi, lo = _lower(a)
        g[lo] -= q[hi]                                   # voxel v (v_a < n_a - 1) loses D_a f[v + e_a] / m[v + e_a]
    return g


def descent(f, step, n_steps, eps=1e-8):
    """n_steps times f <- f - step * g / ||g||_2 in float64 (a step with ||g|| = 0 leaves f) -> (f, TV and ||g|| before the last
    step; nan for n_steps == 0)."""
    f = np.array(f, dtype=np.float64)
    value = norm = float("nan")
    for _ in range(n_steps):
        g = gradient(f, eps)
        value, norm = tv(f, eps), float(np.sqrt((g * g).sum()))
        if norm > 0:
            f = f - step * g / norm
    return f, value, norm


def constant_neighbourhood(f):
    """True where f is constant over the voxel's 13-point neighbourhood (v, v +- e_a, v + e_a - e_b), positions outside the
    volume ignored: there every difference that enters g[v] is exactly 0."""
    f = np.asarray(f)
    n = f.shape
    same = np.ones(n, dtype=bool)
    offsets = [(0, 0, 0)]
    for a in range(3):
        e = [0, 0, 0]
        e[a] = 1
        offsets += [tuple(e), tuple(-v for v in e)]
        for b in range(3):
            if b != a:
                o = list(e)
                o[b] -= 1
                offsets.append(tuple(o))
    assert len(offsets) == 13
    idx = np.indices(n)
    for o in offsets:
        j = [idx[k] + o[k] for k in range(3)]
        inside = np.ones(n, dtype=bool)
        for k in range(3):
            inside &= (j[k] >= 0) & (j[k] < n[k])
        jc = [np.clip(j[k], 0, n[k] - 1) for k in range(3)]
        same &= ~inside | (f[jc[0], jc[1], jc[2]] == f)
    return same


_PHANTOMS = {}


def phantom(n):
    """`_ssim_oracle.phantom_volume(n)`, computed once per size and handed out read-only."""
    if n not in _PHANTOMS:
        import _ssim_oracle
        v = np.ascontiguousarray(_ssim_oracle.phantom_volume(n), dtype=np.float32)
        v.setflags(write=False)
        _PHANTOMS[n] = v
    return _PHANTOMS[n]


def volume(kind, shape):
    """float32 test input: uniform random in [0, 1), a centred crop of the phantom cube, or that crop plus 0.05 N(0, 1)."""
    rng = np.random.default_rng(sum(shape) + len(kind))
    if kind == "random":
        return rng.random(shape).astype(np.float32)
    n = max(max(shape), 8)
    o = [(n - s) // 2 for s in shape]
    x = np.ascontiguousarray(phantom(n)[o[0]:o[0] + shape[0], o[1]:o[1] + shape[1], o[2]:o[2] + shape[2]])
    if kind == "noisy":
        x = (x + 0.05 * rng.standard_normal(shape)).astype(np.float32)
    return x


def noisy_phantom(n=32, sigma=0.05, seed=0):
    """(clean float32 phantom, float32 phantom + sigma N(0, 1)) at n^3: the descent tests' start."""
    clean = phantom(n)
    rng = np.random.default_rng(seed)
    return clean, (clean + sigma * rng.standard_normal(clean.shape)).astype(np.float32)


# the rehearsal's sparse-view case: 16^3 piecewise-constant phantom, 4 cone views of 24 x 24
POCS_DIMS = (16, 16, 16)
POCS_ANGLES = np.linspace(0, np.pi, 5)[:-1]


def pocs_geometry():
    from test_hip_projector import _geometry
    data = _geometry("cone", 0, POCS_DIMS, (4.0, 4.0, 4.0))
    data["nDetector"] = [24, 24]
    return data


def pocs_phantom():
    x = np.zeros(POCS_DIMS, dtype=np.float32)
    x[3:13, 3:13, 3:13] = 0.5
    x[5:9, 6:12, 4:10] = 1.0
    x[10:12, 4:7, 9:12] = 0.2
    return x


def pocs_case():
    """(A, AT, b, x_true) of the rehearsal case in float64.  A and AT are the dense matrix of the forward oracle and its transpose,
    built in one pass from the oracles' own pieces (`_projector_oracle.segments`, `_backproject_oracle.cell`, the sample positions
    and weights of `backproject_rays`), because 300 iterations through `project_rays` / `backproject_rays` themselves take a
    minute; tests/test_tv_cpu.py checks the matrix against both before it uses it."""
    import _backproject_oracle as B
    import _projector_oracle as P
    from neuralvolumetricreconstructionformedicalimages_amd.geometry import ConeGeometry
    geo = ConeGeometry(pocs_geometry())
    rays = np.asarray(B.case_rays(geo, POCS_ANGLES), dtype=np.float32)
    dims, dvoxel = POCS_DIMS, geo.dVoxel
    step = np.float32(geo.accuracy * float(np.min(np.asarray(dvoxel, dtype=np.float64))))
    t0, t1, length, n = P.segments(rays, dims, dvoxel, step)
    K = int(n.max())
    k = np.arange(K)[None, :]
    mask = k < n[:, None]
    a, b = np.where(n > 0, t0, 0).astype(np.float64), np.where(n > 0, t1, 0).astype(np.float64)
    t = a[:, None] + (k + 0.5) * ((b - a) / np.maximum(n, 1))[:, None]
    p = rays[:, None, 0:3].astype(np.float64) + t[..., None] * rays[:, None, 3:6].astype(np.float64)
    scale = np.where(n > 0, length.astype(np.float64) / np.maximum(n, 1), 0.0)
    idx, w = B.cell(dims, dvoxel, p[mask])
    row = np.broadcast_to(np.arange(len(rays))[:, None], mask.shape)[mask]
    add = np.broadcast_to(scale[:, None], mask.shape)[mask]
    M = np.zeros((len(rays), int(np.prod(dims))))
    for cx in (0, 1):
        for cy in (0, 1):
            for cz in (0, 1):
                ix = np.minimum(idx[0] + cx, dims[0] - 1)
                iy = np.minimum(idx[1] + cy, dims[1] - 1)
                iz = np.minimum(idx[2] + cz, dims[2] - 1)
                wt = (w[0] if cx else 1 - w[0]) * (w[1] if cy else 1 - w[1]) * (w[2] if cz else 1 - w[2])
                np.add.at(M, (row, (ix * dims[1] + iy) * dims[2] + iz), add * wt)
    MT = np.ascontiguousarray(M.T)
    x_true = pocs_phantom().astype(np.float64)

    def A(x):
        return M @ x.reshape(-1)

    def AT(y):
        return (MT @ y).reshape(dims)

    return A, AT, A(x_true), x_true, (geo, rays)


def psnr_3d(x, gt):
    from neuralvolumetricreconstructionformedicalimages_amd.utils import get_psnr_3d
    return float(get_psnr_3d(np.asarray(x), np.asarray(gt)))


# float64 figures of the rehearsal case (asd_pocs_operators / sirt_operators over the two float64 oracles, 300 iterations,
# default parameters), as tests/test_tv_cpu.py::test_asd_pocs_beats_sirt_at_four_views measures and pins them
POCS_ITERS = 300
POCS_PSNR_ASD_POCS = 34.02
POCS_PSNR_SIRT = 30.83
