"""tests/_scatter_oracle.py validated without a GPU: the coordinate generator's exactness premise, the float64 sums against
oracle/hashgrid_ref.hash_encode_backward, a numpy restatement of the 8-byte-record arithmetic of scatter_v2.h inside its bound on every
case the GPU file runs, and the bound's teeth: four injected faults of the kind a wrong kernel would commit must leave it."""
import numpy as np
import pytest

import _scatter_oracle as O
from oracle import hashgrid_ref

FX_CASES = [n for n, c in O.CASES.items() if c["family"] in ("fx", "fx_gather")]
TEETH_CASES = [n for n, c in O.CASES.items() if c["teeth"]]


@pytest.mark.parametrize("name", list(O.CASES))
def test_positions_are_exact_in_fp32(name):
    """inputs() runs positions(), whose assertions are the premise; here also: the clamp and the axis-parallel rays are present."""
    rays, z, x01, offs, g, prefill = O.inputs(name)
    case = O.CASES[name]
    assert x01.shape == (case["n_rays"] * case["S"], 3) and x01.dtype == np.float32
    assert np.all(np.diff(z, axis=1) >= 0)
    if case["n_rays"] >= 16:
        assert np.any(x01 == np.float32(O.LIM + O.BOUND)) or np.any(x01 == np.float32(O.BOUND - O.LIM)), "no sample takes the clamp"
        assert np.any((rays[:, 3:6] == 0).sum(1) == 2), "no ray parallel to an axis"
    assert int(offs[-1]) == prefill.shape[0] and np.all(prefill != 0)


@pytest.mark.parametrize("name", ["family-fx", "family-f32", "odd-sizes-bf16", "bf16-L8-C4", "levels-5-8-fx"])
def test_sums_agree_with_hashgrid_ref(name):
    case = O.CASES[name]
    _, _, x01, offs, g, _ = O.inputs(name)
    ref = O.reference(name)
    lb, le = case["levels"]
    masked = np.zeros_like(g)
    masked[:, lb:le] = g[:, lb:le]
    want = hashgrid_ref.hash_encode_backward(masked.reshape(len(g), -1), x01, offs, case["H"], int(offs[-1]), case["C"])
    # hash_encode_backward rounds every product w g to fp32 (2^-24 of |w g| each), sums in float64 and rounds the sum to fp32 (2^-24 |s|)
    assert np.all(np.abs(ref["s"] - want.astype(np.float64)) <= 2.0 ** -23 * ref["a"])
    assert float(np.abs(want).max()) > 0.0


@pytest.mark.parametrize("name", FX_CASES)
def test_emulation_stays_inside_the_fx_bound(name):
    _, _, _, _, _, prefill = O.inputs(name)
    ref = O.reference(name)
    got = O.fx_reduce(O.fx_records(name), ref["E"], prefill)
    use, outside = O.worst_use(got, "fx", ref, prefill)
    print(f"{name}: the emulation's worst element uses {use:.3f} of the PairFx bound")
    assert outside == 0
    assert O.CASES[name]["grad"] == "zero" or use > 0.0


def _candidates(name, rec, ref, prefill, level, lo, hi):
    """Records of `level` whose second corner meets the premises of the module's TEETH paragraph, channel 0; the one with the smallest f_x."""
    q, rb = rec["q"][:, 0], rec["row_b"]
    ok = (rec["level"] == level) & (rec["fx"] >= lo) & (rec["fx"] <= hi)
    ok &= (ref["p"][rb, 0] <= 2.0 * q) & (ref["n"][rb, 0] <= 4) & (q >= 2.0 ** (ref["E"] - 8)) & (np.abs(prefill[rb, 0]) <= q / 4)
    ok &= rec["row_a"] != rb
    idx = np.nonzero(ok)[0]
    assert len(idx) > 0, f"{name}: no contribution of level {level} meets the premises"
    return int(idx[np.argmin(rec["fx"][idx])])


def _outside(got, ref, prefill, row, ch=0):
    err = abs(float(got[row, ch]) - (ref["s"][row, ch] + float(prefill[row, ch])))
    return err > O.bound("fx", ref, prefill)[row, ch]


@pytest.mark.parametrize("fault", ["dropped", "swapped", "e-off-by-one", "lane-past-the-batch"])
@pytest.mark.parametrize("name", TEETH_CASES)
def test_the_fx_bound_has_teeth(name, fault):
    case = O.CASES[name]
    _, _, _, offs, _, prefill = O.inputs(name)
    ref = O.reference(name)
    rec = O.fx_records(name)
    assert O.worst_use(O.fx_reduce(rec, ref["E"], prefill), "fx", ref, prefill)[1] == 0
    thr = O.W_X_THRESHOLD
    for level in range(case["levels"][1] - 3, case["levels"][1]):
        bad = {k: v.copy() for k, v in rec.items()}
        if fault == "lane-past-the-batch":
            # a lane behind the last point holds that point's gradient (its clone): not zeroed, every record of the point counts twice
            last = (rec["point"] == rec["point"].max()) & (rec["level"] == level)
            bad = {k: np.concatenate([v, v[last]]) for k, v in rec.items()}
            got = O.fx_reduce(bad, ref["E"], prefill)
            i = np.nonzero(last)[0]
            wx = np.stack([1.0 - rec["fx"][i], rec["fx"][i]], 1)
            rows = np.stack([rec["row_a"][i], rec["row_b"][i]], 1)
            q = rec["q"][i, 0][:, None]
            sure = (wx >= thr) & (ref["p"][rows, 0] <= 2.0 * q) & (ref["n"][rows, 0] <= 4) & (q >= 2.0 ** (ref["E"] - 8)) & (np.abs(prefill[rows, 0]) <= q / 4)
            hit = [_outside(got, ref, prefill, int(r)) for r in rows[sure]]
            print(f"{name} {fault} level {level}: {sum(hit)} of {len(hit)} rows that meet the premises left the bound")
            assert all(hit)
            assert any(_outside(got, ref, prefill, int(r)) for r in rows.ravel()), "a doubled point went unnoticed"
            continue
        i = _candidates(name, rec, ref, prefill, level, thr, 0.25 if fault == "swapped" else 1.0)
        row_b, row_a = int(rec["row_b"][i]), int(rec["row_a"][i])
        if fault == "dropped":                    # the second corner's share never arrives
            bad["keep_b"] = np.ones(len(rec["fq"]))
            bad["keep_b"][i] = 0.0
        elif fault == "swapped":                  # the two x-neighbour corners take each other's weight
            bad["row_a"][i], bad["row_b"][i] = row_b, row_a
        else:                                     # the xor distance one bit too long: the second corner lands in another row of the level
            lo_, T = int(offs[rec["level"][i]]), int(offs[rec["level"][i] + 1] - offs[rec["level"][i]])
            e = bin((row_a - lo_) ^ (row_b - lo_)).count("1")
            bad["row_b"][i] = lo_ + (((row_a - lo_) ^ ((1 << (e + 1)) - 1)) % T)
            assert bad["row_b"][i] != row_b
        got = O.fx_reduce(bad, ref["E"], prefill)
        print(f"{name} {fault} level {level}: w_x = {rec['fx'][i]:.5f} (threshold {thr:.5f}), row {row_b}")
        assert _outside(got, ref, prefill, row_b), "the fault stayed inside the bound"
        if fault == "swapped":
            assert _outside(got, ref, prefill, row_a) or ref["p"][row_a, 0] > 2.0 * rec["q"][i, 0]


def test_the_odd_size_case_holds_a_pair_whose_corners_share_a_row():
    """Behind a true modulo two x-neighbour corners can land in one row (a level of 2^e - 1 rows): the 8-byte records once dropped the
    second corner's share of such a pair.  The GPU case must keep one, and the fault must leave the bound."""
    name = "odd-sizes-fx"
    _, _, _, _, _, prefill = O.inputs(name)
    ref, rec = O.reference(name), O.fx_records(name)
    same = rec["row_a"] == rec["row_b"]
    assert same.any()
    bad = dict(rec, keep_b=np.where(same, 0.0, 1.0))
    use, outside = O.worst_use(O.fx_reduce(bad, ref["E"], prefill), "fx", ref, prefill)
    print(f"{name}: {int(same.sum())} pair(s) in one row; without their second share the worst element uses {use:.1f} of the bound")
    assert outside > 0
