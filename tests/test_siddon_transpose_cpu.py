"""The oracle of the Siddon transpose (tests/_siddon_transpose_oracle.py; include/naf_hip.h P7) checked against itself: its triples
reproduce the forward restatement, a float32 scatter of them stays inside the per-voxel bound in three summation orders, and five
injected defects each leave the bound.  No GPU."""
import numpy as np
import pytest

import _siddon_oracle as S
import _siddon_transpose_oracle as T


@pytest.fixture(scope="module")
def cases():
    """name -> (dims, dvoxel, volume, rays, triples, y, v0, want, bound), computed once."""
    out = {}
    for name, (dims, dvoxel, vol, rays) in T.ray_sets().items():
        t = T.walk_triples(dims, dvoxel, rays)
        y, v0 = T.values(len(rays)), T.start_volume(dims)
        want, bound, _ = T.want_and_bound(t, y, v0)
        out[name] = (dims, dvoxel, vol, rays, t, y, v0, want, bound)
    return out


def test_triples_reproduce_the_forward_restatement(cases):
    """sum_v a_rv x_v in float64 against walk_f32's fp32 sum in traversal order: they differ by the summation alone, P6's term
    (K + 2) u sum |f| l with K the trip count.  A voxel appears at most once per ray with positive length."""
    worst = {}
    for name, (dims, dvoxel, vol, rays, t, *_) in cases.items():
        value, total = T.forward(t, vol)
        got = S.walk_f32(vol, dvoxel, rays).astype(np.float64)
        ok = t["kind"] == S.OK
        assert np.array_equal(np.isnan(got), t["kind"] == S.NOT_FINITE) and (got[t["kind"] == S.EMPTY] == 0).all(), name
        bound = (t["steps"] + 2) * S.U * total
        assert (np.abs(got[ok] - value[ok]) <= bound[ok]).all(), name
        worst[name] = float((np.abs(got[ok] - value[ok]) / np.where(bound[ok] > 0, bound[ok], 1)).max()) if ok.any() else 0.0
        keep = t["a"] > 0
        pairs = np.stack([t["ray"][keep], t["offset"][keep]], 1)
        assert len(np.unique(pairs, axis=0)) == len(pairs), name
        assert (t["a"] >= 0).all() and (t["steps"][~ok] == 0).all(), name
    print("worst |restatement - sum of triples| / summation term: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


def test_fp32_scatter_stays_within_the_bound_in_three_orders(cases):
    worst = {}
    for name, (dims, _, _, rays, t, y, v0, want, bound) in cases.items():
        for order in ("ray", "reversed", "shuffled"):
            ratio = float(T.use(T.scatter_f32(t, y, v0, order), want, bound).max())
            worst[name] = max(worst.get(name, 0.0), ratio)
    print("worst |fp32 scatter - float64| / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert max(worst.values()) <= 1.0, worst
    # the sets see the volume, and the two that must not leave it as it is
    assert all(int((c[7] != c[6].reshape(-1)).sum()) > 0 for n, c in cases.items() if n not in ("h non-finite",))
    assert np.array_equal(cases["h non-finite"][7], cases["h non-finite"][6].reshape(-1).astype(np.float64))


@pytest.mark.parametrize("defect", T.DEFECTS)
def test_each_injected_defect_leaves_the_bound(cases, defect):
    """The bound is worth only what it rejects: zero-length steps sent with a NaN y, the last segment dropped, |d| omitted from the
    term, y taken from the neighbouring ray, and the rays for which P6 returns NaN sent all the same."""
    broken = []
    for name, (dims, dvoxel, _, rays, t, y, v0, want, bound) in cases.items():
        if defect == "zero_length_sent":
            y = y.copy()
            y[::2] = np.nan
            want, bound, _ = T.want_and_bound(t, y, v0)
            assert T.use(T.scatter_f32(t, y, v0), want, bound).max() <= 1.0, name        # the definition itself passes with this y
        if defect == "not_finite_sent":
            t = T.walk_triples(dims, dvoxel, rays, walk_not_finite=True)
        if T.use(T.scatter_f32(t, y, v0, defect=defect), want, bound).max() > 1.0:
            broken.append(name)
    print(f"{defect}: leaves the bound on {broken}")
    assert broken, defect
    if defect == "zero_length_sent":
        assert "e cube diagonal" in broken
    if defect == "not_finite_sent":
        assert broken == ["h non-finite"]
