"""Oracle of the OS-SART subset step on the Siddon pair (include/naf_hip.h P8) -- not a test module.

Everything is built from the triples (ray, voxel offset, a_rv) of tests/_siddon_transpose_oracle.walk_triples, the float32 matrix
entries the kernels' walk forms:

    row_f32       the row sum the forward walk keeps beside A x: the float32 sum of a ray's a_rv in traversal order
    pair_f32      the paired scatter in float32 numpy, one addition per sent term: num += fl(y_r a_rv) where y_r != 0 and
                  den += a_rv whatever y_r is, for every step with a_rv > 0; with three defects to inject
    ViewOperators A(x, views) and AT(y, views) of the triples' matrix in float64, restricted to view lists, for
                  reconstruct.os_sart_operators / sirt_operators / fista_tv_operators

The per-voxel bound of both outputs is _siddon_transpose_oracle.want_and_bound's, for den with y = 1 on every ray."""
import functools

import numpy as np

import _sart_oracle as O
import _siddon_oracle as S
import _siddon_transpose_oracle as T

f32, f64 = np.float32, np.float64
psnr_3d = O.T.psnr_3d

PAIR_DEFECTS = ("den_skipped_where_y_is_zero", "den_fed_y_times_len", "zero_length_sent_to_den")

# psnr_3d of the float64 iteration on the phantom case (32^3, 8 cone views of 24 x 24, the triples' matrix, b = A x_true in
# float64, relax 1) after 5 iterations, as tests/test_siddon_sart_cpu.py measures and pins them: (SIRT, OS-SART with 8 subsets of
# one view in subset_order's order, OS-SART with 2 sequential subsets)
PHANTOM_PSNR_5 = (23.008, 23.656, 23.116)


def planted_values(n, seed=21, every=7):
    """_siddon_transpose_oracle.values with every `every`-th value set to exactly 0."""
    y = T.values(n, seed).copy()
    y[::every] = f32(0)
    return y


def row_f32(t):
    """The float32 sum of each ray's a_rv in traversal order -> float32 [n_rays]; 0 for a ray that is not walked (the kernel maps
    an empty span to y = 0 and a non-finite one to NaN before the row sum is looked at)."""
    steps = np.asarray(t["steps"], dtype=np.int64)
    first = np.concatenate([[0], np.cumsum(steps)[:-1]])
    row = np.zeros(t["n_rays"], dtype=f32)
    for k in range(int(steps.max()) if steps.size else 0):
        live = np.nonzero(k < steps)[0]
        row[live] = (row[live] + t["a"][first[live] + k]).astype(f32)
    return row


def pair_f32(t, y, num0, den0, defect=None, order="ray", seed=3):
    """-> (num, den) flat float32 [n_voxels] after the paired scatter of `y` into copies of `num0` and `den0`, one float32 addition
    per sent term in the given order ("ray" or "shuffled")."""
    assert defect is None or defect in PAIR_DEFECTS
    y = np.asarray(y, dtype=f32).reshape(-1)
    yr, a = y[t["ray"]], t["a"]
    with np.errstate(invalid="ignore"):
        positive = a > 0
        to_num = positive & (yr != 0)
        to_den = positive.copy()
        num_term, den_term = (yr * a).astype(f32), a.copy()
        if defect == "den_skipped_where_y_is_zero":
            to_den &= yr != 0
        elif defect == "den_fed_y_times_len":
            den_term = num_term
        elif defect == "zero_length_sent_to_den":
            to_den = ~(a < 0)                                  # every step, whatever its length ...
            den_term = np.where(positive, a, f32(np.nan))      # ... and a step of length 0 carries a poisoned term
    out = []
    for start, keep, term in ((num0, to_num, num_term), (den0, to_den, den_term)):
        where = np.nonzero(keep)[0]
        if order == "shuffled":
            where = np.random.default_rng(seed).permutation(where)
        else:
            assert order == "ray"
        v = np.asarray(start, dtype=f32).reshape(-1).copy()
        with np.errstate(invalid="ignore", over="ignore"):
            np.add.at(v, t["offset"][where], term[where])
        out.append(v)
    return out[0], out[1]


def pair_bounds(t, y, num0, den0):
    """-> ((want, bound, m) of num, (want, bound, m) of den): T.want_and_bound for y and for y = 1 on every ray."""
    return T.want_and_bound(t, y, num0), T.want_and_bound(t, np.ones(t["n_rays"]), den0)


class ViewOperators:
    """A and A^T of the triples' matrix in float64, by view: `per_view` rays per view, the rays in view order."""

    def __init__(self, t, n_views, H, W, dims):
        self.t, self.n_views, self.H, self.W, self.dims = t, n_views, H, W, tuple(dims)
        self.per = H * W
        assert t["n_rays"] == n_views * self.per
        keep = t["a"] > 0
        ray, self.offset, self.a = t["ray"][keep], t["offset"][keep], t["a"][keep].astype(f64)
        self.local = ray % self.per
        self.edge = np.searchsorted(ray, np.arange(n_views + 1) * self.per)        # the triples are sorted by ray

    def _view(self, v):
        return slice(self.edge[v], self.edge[v + 1])

    def A(self, x, views):
        x = np.asarray(x, dtype=f64).reshape(-1)
        out = np.empty((len(views), self.H, self.W))
        for j, v in enumerate(views):
            s = self._view(v)
            out[j] = np.bincount(self.local[s], weights=self.a[s] * x[self.offset[s]], minlength=self.per).reshape(self.H, self.W)
        return out

    def AT(self, y, views):
        y = np.asarray(y, dtype=f64).reshape(len(views), self.per)
        out = np.zeros(int(np.prod(self.dims)))
        for j, v in enumerate(views):
            s = self._view(v)
            out += np.bincount(self.offset[s], weights=self.a[s] * y[j][self.local[s]], minlength=out.size)
        return out.reshape(self.dims)

    def all_views(self):
        views = list(range(self.n_views))
        return (lambda x: self.A(x, views)), (lambda y: self.AT(y, views))


def phantom_operators(rays, dims, dvoxel, n_views=8, det=24):
    """ViewOperators of the phantom case's rays."""
    return ViewOperators(T.walk_triples(dims, dvoxel, rays), n_views, det, det, dims)


@functools.lru_cache(maxsize=None)
def phantom_case():
    """_siddon_oracle.orientation_case (32^3 phantom, 8 cone views of 24 x 24) with the float64 operators of its rays' triples
    and b = A x_true in float64 -> (geo, angles, x_true, ops, b)."""
    _, geo, vol, rays, _, angles = S.orientation_case()
    ops = phantom_operators(rays, vol.shape, geo.dVoxel)
    b = ops.A(vol, list(range(len(angles))))
    b.setflags(write=False)
    vol.setflags(write=False)
    return geo, angles, vol, ops, b
