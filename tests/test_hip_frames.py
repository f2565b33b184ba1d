"""Raw-frame conditioning on the GPU (include/naf_hip.h A3): `frames.condition` against the numpy oracle of
tests/_frames_oracle.py.  Without the logarithm the output is a quotient or one of the window's floats, so every comparison is `==` on
int32 views of the floats, and the counts are equal integers.  With it the output is held to -log in float64 within a bound measured
on the device (test_the_logarithm_is_within_the_measured_bound_of_float64)."""
import math

import numpy as np
import pytest
import torch

import _frames_oracle as O

pytestmark = pytest.mark.gpu

# (N, H, W), sizes: each the smallest shape that reaches a distinct path of the 16 x 64 tile
SHAPES = (((1, 3, 3), (3,)),                                   # the window is all reflection
          ((3, 7, 7), (7,)),                                   # size == H == W, three views with their own defects
          ((2, 5, 37), (3, 5)),
          ((2, 37, 5), (3, 5)),                                # three tiles along v, the last of five rows
          ((2, O.TILE_H + 1, O.TILE_W + 1), (3, 7)),           # one more than the tile each way: tiles of one row and of one column
          ((2, O.TILE_H - 1, O.TILE_W - 1), (3, 7)),           # one less: a single cut tile whose halo is all reflection
          ((2, 2 * O.TILE_H + 3, 2 * O.TILE_W + 2), (5,)))     # 3 x 3 tiles: halos cross tile edges on every side
KINDS = ("float32", "uint16", "special")
CASES = [(shape, size, kind) for shape, sizes in SHAPES for size in sizes for kind in KINDS]


def _frames():
    from neuralvolumetricreconstructionformedicalimages_amd import frames
    return frames


def _data(kind, shape, seed):
    if kind == "special":
        return O.special(shape, seed=seed)
    return O.frames(shape, seed=seed, dtype=np.uint16 if kind == "uint16" else np.float32)


def _cuda(*arrays):
    return tuple(None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays)


def _equal(t, a):
    return tuple(t.shape) == a.shape and np.array_equal(t.cpu().numpy().view(np.int32), a.view(np.int32))


def _check(raw, dark, flat, bad, size, dif, what):
    want, want_counts = O.condition(raw, dark, flat, bad, size, dif)
    d = _cuda(raw, flat, dark, bad)
    got, counts = _frames().condition(d[0], d[1], d[2], bad=d[3], size=size, dif=dif, log=False, counts=True)
    assert _equal(got, want), what
    assert np.array_equal(counts.cpu().numpy(), want_counts.astype(np.int64)), what
    return got, counts, d


@pytest.mark.parametrize("shape,size,kind", CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_output_and_counts_equal_the_oracle_bit_for_bit(shape, size, kind):
    raw, dark, flat = _data(kind, shape, seed=11)
    bad = (np.random.default_rng(5).random(shape[1:]) < 0.1).astype(np.uint8)
    for dif, mask in ((0.25, None), (0.0, bad), (0.25, bad)):
        got, counts, d = _check(raw, dark, flat, mask, size, dif, (shape, size, kind, dif))
        again, counts_again = _frames().condition(d[0], d[1], d[2], bad=d[3], size=size, dif=dif, log=False, counts=True)
        assert torch.equal(got.view(torch.int32), again.view(torch.int32)) and torch.equal(counts, counts_again)       # across two calls
        assert np.array_equal(d[0].cpu().numpy().view(np.uint8), np.ascontiguousarray(raw).view(np.uint8))            # the input stays


def test_uint16_and_float32_frames_of_equal_values_give_equal_bits():
    frames = _frames()
    shape = (2, 19, 70)
    raw, dark, flat = O.frames(shape, seed=2, dtype=np.uint16)
    r16, r32, f, d = _cuda(raw, raw.astype(np.float32), flat, dark)
    for size in O.SIZES:
        a, ca = frames.condition(r16, f, d, size=size, dif=0.2, log=False, counts=True)
        b, cb = frames.condition(r32, f, d, size=size, dif=0.2, log=False, counts=True)
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and torch.equal(ca, cb) and int(ca.sum()) > 0


def test_zingers_on_a_corner_on_an_edge_and_two_in_one_window():
    dark, flat = np.zeros((9, 12), dtype=np.float32), np.full((9, 12), 100.0, dtype=np.float32)
    raw = (50 + np.arange(9 * 12, dtype=np.float32).reshape(1, 9, 12) % 7)
    for v, u in ((0, 0), (8, 11), (0, 5), (4, 0), (4, 5), (4, 6)):      # two corners, two edges, two neighbours inside
        raw[0, v, u] = 95.0
    for size in (3, 5):
        got, counts, _ = _check(raw, dark, flat, None, size, 0.2, size)
        assert counts.tolist() == [[6, 0]] and float(got.max()) == float(np.float32(0.56))      # 56 / 100, the largest clean value


def test_a_window_with_no_valid_pixel_and_the_lower_median_of_an_even_count():
    dark = np.zeros((3, 3), dtype=np.float32)
    raw = np.arange(1, 10, dtype=np.float32).reshape(1, 3, 3)
    got, counts, _ = _check(raw, dark, dark, None, 3, 0.0, "flat == dark everywhere")
    assert _equal(got, np.ones((1, 3, 3), dtype=np.float32)) and counts.tolist() == [[0, 9]]
    bad = np.zeros((3, 3), dtype=np.uint8)
    bad[1, 1] = 1
    got, counts, _ = _check(raw, dark, np.ones((3, 3), dtype=np.float32), bad, 3, 100.0, "eight valid neighbours")
    assert float(got[0, 1, 1]) == 4.0 and counts.tolist() == [[0, 1]]          # of 1 2 3 4 6 7 8 9, rank 3


def test_den_zero_den_negative_nan_inf_and_negative_zero():
    dark = np.full((5, 6), 10.0, dtype=np.float32)
    flat = np.full((5, 6), 110.0, dtype=np.float32)
    raw = np.full((1, 5, 6), 60.0, dtype=np.float32)
    flat[0, 0], flat[1, 1] = 10.0, 5.0                                         # den = 0, den < 0
    raw[0, 2, 2], raw[0, 3, 3], raw[0, 4, 4] = np.nan, np.inf, -np.inf
    dark[2, 4], raw[0, 2, 4] = 0.0, -0.0                                       # t = -0 / 110 = -0: valid, and kept with its sign
    got, counts, _ = _check(raw, dark, flat, None, 3, 0.5, "special values")
    assert counts.tolist() == [[0, 5]] and bool(torch.isfinite(got).all())
    assert got.cpu().numpy().view(np.uint32)[0, 2, 4] == 0x80000000


def test_dif_zero_and_a_constant_frame():
    raw = np.full((2, 18, 66), 50.0, dtype=np.float32)
    dark, flat = np.zeros((18, 66), dtype=np.float32), np.full((18, 66), 100.0, dtype=np.float32)
    for size in O.SIZES:
        got, counts, _ = _check(raw, dark, flat, None, size, 0.0, size)        # t - m = 0 is not above 0
        assert int(counts.sum()) == 0 and _equal(got, np.full(raw.shape, 0.5, dtype=np.float32))
    raw, dark, flat = O.frames((2, 18, 66), seed=4, zingers=0.0, dead=0.0)
    for size in O.SIZES:
        _, counts, _ = _check(raw, dark, flat, None, size, 0.0, size)          # every pixel above its window's median goes
        assert int(counts[:, 0].min()) > 0


def test_a_window_never_reads_a_neighbouring_view():
    """Views 0 and 2 hold the same clean frame and view 1 the same frame full of zingers and NaNs: views 0 and 2 come back equal,
    and equal to the frame conditioned alone."""
    frames = _frames()
    one, dark, flat = O.frames((1, 20, 70), seed=6, zingers=0.0, dead=0.0)
    noisy = one.copy()
    pick = np.random.default_rng(8).random(one.shape)
    noisy[pick < 0.2] = 60000.0
    noisy[pick > 0.9] = np.nan
    raw = np.concatenate([one, noisy, one])
    for size in O.SIZES:
        got, counts, d = _check(raw, dark, flat, None, size, 0.1, size)
        alone, counts_alone = frames.condition(d[0][:1].contiguous(), d[1], d[2], size=size, dif=0.1, log=False, counts=True)
        for view in (0, 2):
            assert torch.equal(got[view].view(torch.int32), alone[0].view(torch.int32)) and torch.equal(counts[view], counts_alone[0])
        assert int(counts[1, 0]) > int(counts[0, 0]) and int(counts[1, 1]) > 0 == int(counts[0, 1])


def test_aliasing_is_refused_and_a_side_stream_gives_equal_bits():
    """The rule of include/naf_hip.h: `out` must not overlap an input.  The front end raises, the library returns
    NAF_ERR_INVALID_ARGUMENT before any launch and leaves the frames as they are."""
    from neuralvolumetricreconstructionformedicalimages_amd import _abi
    frames = _frames()
    raw, dark, flat = O.frames((2, 9, 11), seed=9)
    r, f, d = _cuda(raw, flat, dark)
    with pytest.raises(ValueError, match="out must not overlap raw"):
        frames.condition(r, f, d, dif=0.1, out=r)
    both = torch.empty(3, 9, 11, device="cuda")                               # a partial overlap: the second view of raw is the first of out
    both[:2] = r
    with pytest.raises(ValueError, match="out must not overlap raw"):
        frames.condition(both[:2], f, d, dif=0.1, out=both[1:])
    rc = _abi.lib().naf_frames_condition(_abi.ptr(r), 0, _abi.ptr(d), _abi.ptr(f), None, 2, 9, 11, 3, 0.1, 1e-5, 1, _abi.ptr(r), None,
                                         _abi.stream_ptr())
    assert rc == -1 and b"out must not overlap" in _abi.lib().naf_last_error()
    torch.cuda.synchronize()
    assert _equal(r, raw)
    want = frames.condition(r, f, d, dif=0.1, size=3)
    out = torch.full_like(want, float("nan"))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = frames.condition(r, f, d, dif=0.1, size=3, out=out)
    side.synchronize()
    assert got is out and torch.equal(got.view(torch.int32), want.view(torch.int32))
    empty = frames.condition(r[:0], f, d, dif=0.1)
    assert tuple(empty.shape) == (0, 9, 11)


# The worst error of the LOG output over this test's inputs, in float32 units in the last place of -log in float64 of the oracle's
# float32 max(t', t_min), as measured on an MI355X, and the bar: twice that, rounded up to a whole ulp.
MEASURED_LOG_ULP = 1.8332
LOG_BOUND_ULP = math.ceil(2 * MEASURED_LOG_ULP)


def _log_inputs():
    """t = raw exactly (dark = 0, flat = 1, nothing replaced): uniform in (0, 1.2), within 5e-4 of 1, log-uniform from e^-14 to
    e^10, and the edges: +-0, a negative, 1, t_min and its two neighbours, nearly the largest float."""
    rng = np.random.default_rng(0)
    t_min = np.float32(1e-5)
    t = np.concatenate([rng.random(4096) * 1.2, 1 + (rng.random(2048) - 0.5) * 1e-3, np.exp(rng.uniform(-14, 10, 2040)),
                        [0.0, -0.0, -3.0, 1.0, t_min, np.nextafter(t_min, np.float32(0)), np.nextafter(t_min, np.float32(1)), 3e38]])
    return t.astype(np.float32).reshape(2, 64, 64), t_min


def test_the_logarithm_is_within_the_measured_bound_of_float64():
    """Measured on an MI355X: the worst error over these inputs is 1.8332 ulp (t = raw exactly, without the clamp; 1.7889 with it;
    1.8085 and 1.7882 on the two sets of frames), so the bar is ceil(2 x 1.8332) = 4 ulp.  Above 4 ulp the tail would be defective (a
    fast-math logarithm), not loosely held."""
    frames = _frames()
    worst = 0.0
    t, t_min = _log_inputs()
    one, zero = np.ones(t.shape[1:], dtype=np.float32), np.zeros(t.shape[1:], dtype=np.float32)
    cases = [(t, zero, one, None, 3, 3.0e38, float(t_min))]
    for kind, seed in (("float32", 21), ("special", 22)):
        raw, dark, flat = _data(kind, (2, 17, 65), seed)
        cases.append((raw, dark, flat, None, 5, 0.25, 1e-5))
    for raw, dark, flat, bad, size, dif, floor in cases:
        r, f, d = _cuda(raw, flat, dark)
        for clamp in (False, True):
            got = frames.condition(r, f, d, size=size, dif=dif, t_min=floor, log=True, clamp=clamp).cpu().numpy()
            want = O.log_reference(raw, dark, flat, bad, size, dif, floor, clamp)
            err = float(O.ulp_error(got, want).max())
            print(f"log tail: shape {raw.shape} size {size} clamp {clamp}: worst {err:.4f} ulp")
            worst = max(worst, err)
            if clamp:
                assert not np.signbit(got).any()                               # nothing below zero, and no -0
    print(f"log tail: worst {worst:.4f} ulp over all inputs; the bar is {LOG_BOUND_ULP}")
    assert worst <= 4.0, "the tail is defective: this is not a tolerance to widen"
    assert worst <= LOG_BOUND_ULP


def _phantom_frames():
    """A 32^3 phantom, 16 views of 48^2 -> (p, flat, dark, noisy frames without defects)."""
    from neuralvolumetricreconstructionformedicalimages_amd import phantom
    from neuralvolumetricreconstructionformedicalimages_amd.dataset import raw_frames, synthetic_scan
    geometry = phantom.scan_geometry(32)
    geometry["nDetector"], geometry["dDetector"] = [48, 48], [0.8 * 8 * 64 / 48] * 2
    p = np.ascontiguousarray(synthetic_scan(n_train=16, n_val=1, geometry=geometry)["train"]["projections"], dtype=np.float32)
    assert p.shape == (16, 48, 48)
    rng = np.random.default_rng(0)
    dark = (100 + 5 * rng.standard_normal((48, 48))).astype(np.float32)
    flat = (dark + 4000 + 200 * rng.standard_normal((48, 48))).astype(np.float32)
    return p, flat, dark, raw_frames(p, 1e5, flat, dark, 1)


def test_planted_isolated_zingers_are_removed_and_nothing_else_moves():
    from neuralvolumetricreconstructionformedicalimages_amd.dataset import add_zingers
    frames = _frames()
    size, dif, gain = 3, 0.25, 4.0
    p, flat, dark, clean = _phantom_frames()
    planted, hit = add_zingers(clean, 0.01, gain, 2, isolation=size - 1)
    n_hit = hit.sum(axis=(1, 2))
    assert n_hit.min() >= 5
    # the condition on the input: no two planted pixels of a view within one window
    for i, v, u in np.argwhere(hit):
        assert hit[i, max(v - size + 1, 0):v + size, max(u - size + 1, 0):u + size].sum() == 1
    # dif sits above the clean frames' largest t - m, so on clean frames the oracle replaces nothing ...
    _, clean_counts, excess = O.repaired(clean, dark, flat, None, size, dif)
    assert float(excess.max()) < dif and int(clean_counts.sum()) == 0
    # ... and every planted pixel exceeds it, so on the planted frames the oracle replaces exactly those
    _, planted_counts, excess = O.repaired(planted, dark, flat, None, size, dif)
    assert float(excess[hit].min()) > dif
    assert planted_counts[:, 0].tolist() == n_hit.tolist() and int(planted_counts[:, 1].sum()) == 0
    c, z, f, d = _cuda(clean, planted, flat, dark)
    want, want_counts = frames.condition(c, f, d, size=size, dif=dif, counts=True)
    got, counts = frames.condition(z, f, d, size=size, dif=dif, counts=True)
    assert int(want_counts.sum()) == 0
    assert counts[:, 0].cpu().tolist() == n_hit.tolist() and int(counts[:, 1].sum()) == 0
    touched = np.zeros_like(hit)                                               # pixels whose window holds a planted pixel
    for i, v, u in np.argwhere(hit):
        touched[i, max(v - 1, 0):v + 2, max(u - 1, 0):u + 2] = True
    same = torch.from_numpy(~touched).cuda()
    assert torch.equal(got.view(torch.int32)[same], want.view(torch.int32)[same])
