"""Float64 restatement of the volume sampler (include/naf_hip.h V4, csrc/volume_sample_device.h) on the
float32 inputs, and the exact uint32 restatement of its draw.  numpy only.

`sample` evaluates, in float64, u_a = (p_a + h_a) / d_a - 1/2 with h_a the float32 half extent the library forms, clamps it to
[0, n_a - 1], takes i_a = min(floor(u_a), n_a - 2) and w_a = u_a - i_a, and blends the eight corners; a NaN coordinate gives NaN.

`bound` is the tolerance of the float32 kernel against it, from the count of DESIGN.md section 24 (unit roundoff e = 2^-24):
  u_a     four roundings of relative size e on numbers of magnitude <= n_a (the stored 1 / d_a, the add, the multiply, the
          subtract): |du_a| <= 4 n_a e; w_a = u_a - i_a is exact.  The value is continuous and piecewise linear in u_a with slope
          |c_1 - c_0| <= 2 max|f|, so the three axes move it by at most 3 * 4 n e * 2 max|f| = 24 n e max|f|.
  lerps   each is two fmas, a - w a and then + w b, both of magnitude <= max|f|: <= 2 e max|f|; the three stages pass earlier
          errors on with weights that sum to 1: <= 6 e max|f|.
  total   (24 n + 6) e max|f| <= 30 n e max|f|;  with the factor 2 over it  c = 60:  bound = 60 * 2^-24 * max_a(n_a) * max|f|."""
import numpy as np

C_BOUND = 60.0


def half_extent(dims, dvoxel):
    """h_a = fp32(n_a * d_a / 2) from the float32 voxel size, as voxel_grid of csrc/voxel_grid.h forms it."""
    d = np.asarray(dvoxel, dtype=np.float32).astype(np.float64)
    return (np.asarray(dims, dtype=np.float64) * d / 2.0).astype(np.float32)


def centres(dims, dvoxel):
    """The float32 voxel centres of get_voxels (tigre.py:388-400): linspace(-s, s, n) per axis in float64, cast once -> [n1 n2 n3, 3]."""
    d = np.asarray(dvoxel, dtype=np.float64)
    n = np.asarray(dims, dtype=np.int64)
    s = n * d / 2 - d / 2
    axes = [np.linspace(-s[a], s[a], int(n[a])) for a in range(3)]
    return np.stack(np.meshgrid(*axes, indexing="ij"), -1).reshape(-1, 3).astype(np.float32)


def bound(volume):
    return C_BOUND * 2.0 ** -24 * max(volume.shape) * float(np.abs(volume).max())


def sample(volume, dvoxel, points):
    """volume float32 [n1, n2, n3], dvoxel three float32 sizes, points float32 [n, 3] -> float64 [n]."""
    f = np.asarray(volume, dtype=np.float32).astype(np.float64)
    p = np.asarray(points, dtype=np.float32).astype(np.float64)
    d = np.asarray(dvoxel, dtype=np.float32).astype(np.float64)
    h = half_extent(f.shape, dvoxel).astype(np.float64)
    idx, w = [], []
    with np.errstate(invalid="ignore"):
        for a in range(3):
            n = f.shape[a]
            u = (p[:, a] + h[a]) / d[a] - 0.5
            nan = np.isnan(u)
            u = np.clip(np.where(nan, 0.0, u), 0.0, n - 1.0)
            i = np.minimum(np.floor(u), max(n - 2, 0)).astype(np.int64)
            idx.append((i, np.minimum(i + 1, n - 1)))                     # an axis of one voxel: the upper corner is the lower
            w.append(np.where(nan, np.nan, u - i))
        out = np.zeros(len(p))
        for x in (0, 1):
            for y in (0, 1):
                for z in (0, 1):
                    wx, wy, wz = (w[0] if x else 1 - w[0]), (w[1] if y else 1 - w[1]), (w[2] if z else 1 - w[2])
                    out = out + wx * wy * wz * f[idx[0][x], idx[1][y], idx[2][z]]
    return out


# ---- the draw, exactly ---------------------------------------------------------------------------------------------------------------
def _mix32(h):
    h = h ^ (h >> np.uint32(16))
    h = h * np.uint32(0x7feb352d)
    h = h ^ (h >> np.uint32(15))
    h = h * np.uint32(0x846ca68b)
    return h ^ (h >> np.uint32(16))


def hash_bits(seed, step, n, axis):
    """The 32 bits of (seed, step, i, axis) for i < n, uint32 [n] (wrap-around arithmetic, as in sample_hash)."""
    seed = int(seed)
    i = np.arange(n, dtype=np.uint32)
    with np.errstate(over="ignore"):
        h = _mix32(np.uint32(seed & 0xffffffff) ^ (i * np.uint32(0x9e3779b1)))
        key = np.uint32((seed >> 32) & 0xffffffff) ^ np.uint32((int(step) * 0x85ebca77) & 0xffffffff) ^ np.uint32(0x27d4eb2f)
        h = _mix32(h ^ key)
        return _mix32(h ^ np.uint32(((axis + 1) * 0xc2b2ae3d) & 0xffffffff))


def draw(seed, step, n, lo, hi):
    """The n points of step `step`: float32 [n, 3], every operation a float32 IEEE operation in the kernel's order."""
    lo, hi = np.asarray(lo, dtype=np.float32), np.asarray(hi, dtype=np.float32)
    out = np.empty((n, 3), dtype=np.float32)
    for a in range(3):
        r = (hash_bits(seed, step, n, a) >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)
        e = np.float32(hi[a] - lo[a])
        s = (r * e).astype(np.float32)
        out[:, a] = np.minimum((lo[a] + s).astype(np.float32), hi[a])
    return out


# ---- the test sets, shared by the CPU and the GPU tests --------------------------------------------------------------------------------
SHAPES = ((5, 6, 7), (1, 4, 4), (4, 1, 1), (2, 2, 2))
DVOXEL_EXACT = (2.0 ** -9, 2.0 ** -10, 2.0 ** -8)        # powers of two: every step of u_a is exact at the voxel centres
DVOXEL_PLAIN = (0.001, 0.0013, 0.0007)


def make_volume(dims, seed=0):
    """Mixed-sign values away from 0, float32 [n1, n2, n3]."""
    rng = np.random.RandomState(seed)
    v = rng.uniform(0.25, 1.0, size=dims) * rng.choice([-1.0, 1.0], size=dims)
    return v.astype(np.float32)


def faces_and_corners(dims, dvoxel):
    """The 27 points of the box with every coordinate in {-h_a, 0, +h_a}: its corners, edge and face centres and the middle."""
    h = half_extent(dims, dvoxel)
    pts = [[sx * h[0], sy * h[1], sz * h[2]] for sx in (-1, 0, 1) for sy in (-1, 0, 1) for sz in (-1, 0, 1)]
    return np.asarray(pts, dtype=np.float32)


def random_points(dims, dvoxel, n=4096, seed=1, scale=1.5):
    """n points uniform in `scale` times the box."""
    h = half_extent(dims, dvoxel).astype(np.float64)
    rng = np.random.RandomState(seed)
    return (rng.uniform(-1.0, 1.0, size=(n, 3)) * h * scale).astype(np.float32)


def non_finite_points(dims, dvoxel):
    """Finite points with NaN / +-inf planted on single coordinates -> (points [n, 3], is_nan [n]): a NaN coordinate gives NaN, an
    infinite one the edge value."""
    pts = random_points(dims, dvoxel, n=24, seed=5, scale=0.9)
    pts[0, 0], pts[1, 1], pts[2, 2] = np.nan, np.nan, np.nan
    pts[3] = np.nan
    pts[4, 0], pts[5, 1], pts[6, 2] = np.inf, -np.inf, np.inf
    pts[7] = (-np.inf, np.inf, -np.inf)
    pts[8, 0], pts[8, 1] = np.inf, np.nan
    pts[9] = (3e38, -3e38, 1e30)
    return pts, np.isnan(pts).any(axis=1)
