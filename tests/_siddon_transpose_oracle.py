"""Oracle of the Siddon projector's transpose (include/naf_hip.h P7) -- not a test module.

The float32 walk of csrc/siddon_device.h is restated here (the loop of _siddon_oracle.walk_f32, which returns sums only) so that it
returns every step as a triple (ray, voxel offset, a_rv), a_rv = fl(fl(s_next - s_prev) * |d|) being the matrix entry the forward
walk forms.  From the triples, in float64:

    want_v = v0_v + sum_r y_r a_rv,      m_v = number of sent terms of voxel v (a_rv > 0 and y_r != 0).

Per-voxel bound, u = 2^-24:

    |kernel - want|_v <= 1.001 * (m_v + 1) * u * (|v0_v| + sum_r |y_r| a_rv)

Derivation: every sent term is one fp32 product fl(y_r a_rv), off by at most u |y_r| a_rv; the m_v hardware additions into the
voxel, in whatever order, each round a partial sum that is no larger than the absolute sum S = |v0_v| + sum |y_r| a_rv (1 + O(u)),
so they add at most m_v u S; together (m_v + 1) u S, and the factor 1.001 covers the second-order terms for m_v u < 1e-3."""
import numpy as np

import _siddon_oracle as S
from _siddon_oracle import EMPTY, NOT_FINITE, OK, U, _fma32, half_extent, spans  # noqa: F401

f32, f64 = np.float32, np.float64

DEFECTS = ("zero_length_sent", "drop_last", "no_dn", "neighbour_y", "not_finite_sent")


def ray_sets():
    """_siddon_oracle.ray_sets() and, as one more set, the non-finite rays (every one of them sends nothing)."""
    sets = dict(S.ray_sets())
    dims, dvoxel, vol, rays = sets["c random"]
    sets["h non-finite"] = (dims, dvoxel, vol, S.non_finite_rays(rays))
    return sets


def walk_triples(dims, dvoxel, rays, walk_not_finite=False):
    """The kernel's traversal in float32 numpy, all rays at once -> dict of flat arrays, one entry per step of every walked ray:
    ray (int64), offset (int64 element offset into the C-contiguous volume), ds (float32, s_next - s_prev), a (float32, ds * |d|),
    last (bool: the walk's last step), and per ray `steps` (the trip count, 0 for a ray that is not walked) and `kind`.
    Zero-length steps are kept (a == 0); the kernel does not send them.  `walk_not_finite` walks the rays for which P6 returns NaN
    as well, with the non-finite floats they carry (a defect: the definition walks none of them)."""
    dims = tuple(int(n) for n in dims)
    p0, d, s_end, dn, kind = spans(rays, dims, dvoxel)
    half = half_extent(dims, dvoxel)
    dv = np.asarray(dvoxel, dtype=f32)
    inv = (f32(1) / dv).astype(f32)
    R = len(p0)
    ok = (kind != EMPTY) if walk_not_finite else (kind == OK)
    p0 = np.where(ok[:, None], p0, f32(0))
    s_end = np.where(ok, s_end, f32(0))
    hi = np.asarray(dims, dtype=f32) - f32(1)

    def index(p):
        with np.errstate(all="ignore"):
            u = np.floor((p + half[None, :]) * inv[None, :])
        return np.fmin(np.fmax(u, f32(0)), hi[None, :]).astype(np.int64)

    def crossing(m):
        with np.errstate(all="ignore"):
            q = _fma32(m.astype(f32), dv[None, :], -half[None, :])
            return ((q - p0) / d).astype(f32)

    with np.errstate(all="ignore"):
        i0, i1 = index(p0), index(_fma32(s_end[:, None], d, p0))
    idx = i0.copy()
    dirn = np.sign(i1 - i0)
    rem = np.abs(i1 - i0)
    nxt = crossing(idx + (dirn > 0))
    steps = np.where(ok, rem.sum(1) + 1, 0)
    s_prev = np.zeros(R, dtype=f32)
    out = {"ray": [], "offset": [], "ds": [], "a": [], "last": []}
    for k in range(int(steps.max()) if R else 0):
        live = k < steps
        ax, ay, az = rem[:, 0] > 0, rem[:, 1] > 0, rem[:, 2] > 0
        with np.errstate(invalid="ignore"):
            px = ax & (~ay | (nxt[:, 0] <= nxt[:, 1])) & (~az | (nxt[:, 0] <= nxt[:, 2]))
            py = ~px & ay & (~az | (nxt[:, 1] <= nxt[:, 2]))
        pz = ~px & ~py & az
        pick = np.stack([px, py, pz], 1)
        s = np.where(px, nxt[:, 0], np.where(py, nxt[:, 1], np.where(pz, nxt[:, 2], s_end)))
        s = np.fmin(np.fmax(s, s_prev), s_end).astype(f32)
        with np.errstate(invalid="ignore"):
            ds = (s - s_prev).astype(f32)
            a = (ds * dn).astype(f32)
        offset = (idx[:, 0] * dims[1] + idx[:, 1]) * dims[2] + idx[:, 2]
        where = np.nonzero(live)[0]
        out["ray"].append(where)
        out["offset"].append(offset[where])
        out["ds"].append(ds[where])
        out["a"].append(a[where])
        out["last"].append((k == steps - 1)[where])
        move = pick & live[:, None]
        idx = idx + np.where(move, dirn, 0)
        rem = rem - move
        nxt = np.where(move, crossing(idx + (dirn > 0)), nxt)
        s_prev = np.where(live, s, s_prev)
    empty = {"ray": np.int64, "offset": np.int64, "ds": f32, "a": f32, "last": bool}
    t = {key: (np.concatenate(v) if v else np.zeros(0, dtype=empty[key])) for key, v in out.items()}
    order = np.lexsort((np.arange(len(t["ray"])), t["ray"]))                 # ray order, steps in traversal order within a ray
    t = {key: v[order] for key, v in t.items()}
    t["steps"], t["kind"], t["n_rays"], t["n_voxels"] = steps, kind, R, int(np.prod(dims))
    assert t["offset"].size == 0 or (t["offset"].min() >= 0 and t["offset"].max() < t["n_voxels"])
    return t


def sent(t, y):
    """Mask over the triples of what the definition sends: positive length and y_r != 0 (a NaN y is sent)."""
    return (t["a"] > 0) & (np.asarray(y)[t["ray"]] != 0)


def forward(t, x):
    """sum_v a_rv x_v per ray in float64 -> (value [n_rays], sum |x_v| a_rv [n_rays])."""
    x = np.asarray(x, dtype=f64).reshape(-1)
    keep = t["a"] > 0
    ray, term = t["ray"][keep], t["a"][keep].astype(f64) * x[t["offset"][keep]]
    return np.bincount(ray, weights=term, minlength=t["n_rays"]), np.bincount(ray, weights=np.abs(term), minlength=t["n_rays"])


def transpose(t, y):
    """sum_r y_r a_rv per voxel in float64 (flat [n_voxels]); rays with y_r == 0 and steps of length 0 add nothing."""
    y = np.asarray(y, dtype=f64).reshape(-1)
    keep = sent(t, y)
    return np.bincount(t["offset"][keep], weights=t["a"][keep].astype(f64) * y[t["ray"][keep]], minlength=t["n_voxels"])


def want_and_bound(t, y, v0):
    """-> (want, bound, m), flat float64 / float64 / int64 [n_voxels].  A NaN or Inf y_r makes `want` non-finite at exactly the
    voxels it is sent to; the bound there is NaN."""
    y64, v0 = np.asarray(y, dtype=f64).reshape(-1), np.asarray(v0, dtype=f64).reshape(-1)
    keep = sent(t, y64)
    off, term = t["offset"][keep], t["a"][keep].astype(f64) * y64[t["ray"][keep]]
    with np.errstate(invalid="ignore"):
        want = v0 + np.bincount(off, weights=term, minlength=t["n_voxels"])
        total = np.abs(v0) + np.bincount(off, weights=np.abs(term), minlength=t["n_voxels"])
    m = np.bincount(off, minlength=t["n_voxels"])
    return want, 1.001 * (m + 1) * U * total, m


def use(got, want, bound):
    """|got - want| / bound per voxel; 0 where both are bit-equal as numbers or both NaN, inf where only one is finite."""
    return S.use(np.asarray(got).reshape(-1), want, bound)


def scatter_f32(t, y, v0, order="ray", defect=None, seed=3):
    """The kernel's sums in float32 numpy, one addition at a time in the given `order` of the sent terms ("ray", "reversed" or
    "shuffled") -> flat float32 [n_voxels].  `defect` injects one of DEFECTS ("not_finite_sent" needs triples made with
    walk_not_finite=True)."""
    assert defect is None or defect in DEFECTS
    y = np.asarray(y, dtype=f32).reshape(-1)
    yr = np.roll(y, -1)[t["ray"]] if defect == "neighbour_y" else y[t["ray"]]
    a = t["ds"] if defect == "no_dn" else t["a"]
    with np.errstate(invalid="ignore"):
        keep = yr != 0
        if defect == "zero_length_sent":
            keep &= ~(a < 0)                                                  # every step, whatever its length
        elif defect == "not_finite_sent":
            keep &= (a > 0) | np.isnan(a)
        else:
            keep &= a > 0
        if defect == "drop_last":
            keep &= ~t["last"]
        term = (yr * a).astype(f32)
    where = np.nonzero(keep)[0]
    if order == "reversed":
        where = where[::-1]
    elif order == "shuffled":
        where = np.random.default_rng(seed).permutation(where)
    else:
        assert order == "ray"
    out = np.asarray(v0, dtype=f32).reshape(-1).copy()
    with np.errstate(invalid="ignore", over="ignore"):
        np.add.at(out, t["offset"][where], term[where])                       # unbuffered: one float32 addition per term, in order
    return out


def values(n, seed=21):
    """y with mixed signs, and never 0."""
    y = np.random.default_rng(seed).standard_normal(n).astype(f32)
    return np.where(y == 0, f32(1), y)


def start_volume(dims, seed=22):
    """A non-zero volume to accumulate into."""
    return np.random.default_rng(seed).standard_normal(dims).astype(f32) * f32(1e-3)


def operators(t, shape_b, shape_x):
    """(A, AT) of the triples' matrix as float64 numpy callables, for reconstruct.cgls_operators."""
    def A(x):
        return forward(t, x)[0].reshape(shape_b)

    def AT(y):
        return transpose(t, y).reshape(shape_x)

    return A, AT
