"""Raw-frame conditioning on the CPU: the float32 numpy oracle of tests/_frames_oracle.py against a per-pixel
restatement (float64 quotients rounded once, sorted lists), its properties, the synthetic frames of dataset.py and their round trip,
frames.condition's refusals that need no GPU, and tools/frames_host_check.cpp, which runs csrc/frames_device.h under AddressSanitizer
and UBSan as a process of its own.  No GPU."""
import numpy as np
import pytest

import _frames_oracle as O
from _host_check import load, needs_compiler

D = load("frames")

# (N, H, W), sizes: the shapes of tests/test_hip_frames.py that a plain loop walks in a second or two
CASES = (((1, 3, 3), (3,)), ((3, 7, 7), (7,)), ((2, 5, 37), (3, 5)), ((2, 37, 5), (3, 5)), ((1, 17, 20), (7,)))


@pytest.mark.parametrize("kind", ("frames", "special"))
@pytest.mark.parametrize("shape,sizes", CASES)
def test_oracle_equals_the_per_pixel_restatement(shape, sizes, kind):
    raw, dark, flat = getattr(O, kind)(shape, seed=3)
    bad = (np.random.default_rng(5).random(shape[1:]) < 0.1).astype(np.uint8)
    for size in sizes:
        for dif, mask in ((0.25, None), (0.0, bad)):
            out, counts = O.condition(raw, dark, flat, mask, size, dif)
            want, want_counts = O.condition_loops(raw, dark, flat, mask, size, dif)
            assert O.equal_bits(out, want) and np.array_equal(counts, want_counts), (shape, kind, size, dif)


def test_uint16_and_float32_frames_of_equal_values_give_equal_bits():
    raw, dark, flat = O.frames((2, 9, 11), seed=1, dtype=np.uint16)
    a, ca = O.condition(raw, dark, flat, None, 3, 0.2)
    b, cb = O.condition(raw.astype(np.float32), dark, flat, None, 3, 0.2)
    assert O.equal_bits(a, b) and np.array_equal(ca, cb)


def test_a_window_with_no_valid_pixel_gives_one_and_an_even_count_the_lower_median():
    dark = np.zeros((3, 3), dtype=np.float32)
    flat = np.ones((3, 3), dtype=np.float32)
    raw = np.arange(1, 10, dtype=np.float32).reshape(1, 3, 3)
    out, counts = O.condition(raw, dark, dark, None, 3, 0.0)                 # flat == dark everywhere: every pixel is bad
    assert np.array_equal(out, np.ones((1, 3, 3), dtype=np.float32)) and counts.tolist() == [[0, 9]]
    bad = np.zeros((3, 3), dtype=np.uint8)
    bad[1, 1] = 1
    out, counts = O.condition(raw, dark, flat, bad, 3, 100.0)                # the middle sees 1 2 3 4 6 7 8 9: rank 3 is the 4
    assert out[0, 1, 1] == 4.0 and counts.tolist() == [[0, 1]]
    assert O.equal_bits(np.delete(out.ravel(), 4), np.delete(raw.ravel(), 4))


def test_only_bright_outliers_are_replaced_and_a_constant_frame_comes_back():
    raw = np.full((1, 7, 9), 50.0, dtype=np.float32)
    dark, flat = np.zeros((7, 9), dtype=np.float32), np.full((7, 9), 100.0, dtype=np.float32)
    out, counts = O.condition(raw, dark, flat, None, 5, 0.0)
    assert O.equal_bits(out, np.full((1, 7, 9), 0.5, dtype=np.float32)) and counts.sum() == 0
    raw[0, 0, 0], raw[0, 3, 4] = 90.0, 5.0                                   # a bright corner and a dark pixel
    out, counts = O.condition(raw, dark, flat, None, 5, 0.1)
    assert out[0, 0, 0] == 0.5 and out[0, 3, 4] == np.float32(0.05) and counts.tolist() == [[1, 0]]


def test_the_tail_is_minus_log_with_a_floor_and_a_clamp_that_returns_no_negative_zero():
    # numpy's float32 logarithm is within 4 ulp
    t = np.array([[[2.0, 1.0, 0.5, 0.0, -1.0, 1e-7]]], dtype=np.float32).reshape(1, 1, 6)
    got = O.tail(t, 1e-5, True, False)
    want = -np.log(np.maximum(t.astype(np.float64), np.float64(np.float32(1e-5))))
    assert np.all(O.ulp_error(got, want) <= 4.0) and got[0, 0, 0] < 0 and np.signbit(got[0, 0, 1])      # -log(1) is -0
    clamped = O.tail(t, 1e-5, True, True)
    assert not np.signbit(clamped).any() and clamped[0, 0, 0] == 0 and O.equal_bits(clamped[..., 2:], got[..., 2:])


def _scan(n_views=6):
    from neuralvolumetricreconstructionformedicalimages_amd.dataset import synthetic_scan
    return np.ascontiguousarray(synthetic_scan(n_voxel=16, n_train=n_views, n_val=1)["train"]["projections"], dtype=np.float32)


def _detector(shape, seed=0):
    rng = np.random.default_rng(seed)
    dark = (100 + 5 * rng.standard_normal(shape)).astype(np.float32)
    return (dark + 4000 + 200 * rng.standard_normal(shape)).astype(np.float32), dark


def test_raw_frames_then_the_oracle_return_the_line_integrals():
    """Nothing planted and no noise, so in exact arithmetic the frames invert to p.  In float32, with u = 2^-24 the relative error
    of one rounding: the stored frame is off by u |raw|, which is u (1 + dark / num) of the numerator; num, den and the quotient
    round once each.  With p < 0.08 (t > 0.92), flat - dark >= 3000 and dark <= 130 that is (4 + 130 / 2760) u < 4.05 u relative in
    t, so 4.05 u / 0.92 < 2.7e-7 in p = -log t; numpy's float32 logarithm is within 4 ulp of a result below 0.08, 4 x 7.5e-9 =
    3e-8.  The bound is their sum, 3e-7."""
    from neuralvolumetricreconstructionformedicalimages_amd.dataset import raw_frames
    p = _scan()
    flat, dark = _detector(p.shape[1:])
    assert (flat - dark).min() >= 3000 and dark.max() <= 130 and p.max() < 0.08
    raw = raw_frames(p, 1e5, flat, dark)
    assert raw.dtype == np.float32 and raw.shape == p.shape
    out, counts = O.condition(raw, dark, flat, None, 3, 0.5, t_min=0.5, log=True, clamp=True)
    assert counts.sum() == 0
    err = np.abs(out.astype(np.float64) - p)
    print(f"max |(-log o raw_frames)(p) - p| = {err.max():.3e}")
    assert err.max() <= 3e-7


def test_synthetic_defects_are_reproducible_by_seed_and_keep_their_promises():
    import torch
    from neuralvolumetricreconstructionformedicalimages_amd.dataset import add_dead_pixels, add_zingers, raw_frames
    p = _scan()
    flat, dark = _detector(p.shape[1:])
    noisy = raw_frames(p, 1e5, flat, dark, 3)
    assert O.equal_bits(noisy, raw_frames(p, 1e5, flat, dark, np.random.default_rng(3)))
    assert not O.equal_bits(noisy, raw_frames(p, 1e5, flat, dark, 4))
    raw = raw_frames(p, 1e5, flat, dark)
    for isolation in (0, 1, 4):
        hit_frames, hit = add_zingers(raw, 0.05, 3.0, 7, isolation=isolation)
        again, hit_again = add_zingers(raw, 0.05, 3.0, 7, isolation=isolation)
        assert O.equal_bits(hit_frames, again) and np.array_equal(hit, hit_again) and hit.any()
        assert O.equal_bits(hit_frames[~hit], raw[~hit]) and np.allclose(hit_frames[hit], raw[hit] * 3.0)
        where = np.argwhere(hit)
        for i, v, u in where:                                # no other hit of the view within `isolation` pixels along both axes
            near = where[(where[:, 0] == i) & (np.abs(where[:, 1] - v) <= isolation) & (np.abs(where[:, 2] - u) <= isolation)]
            assert isolation == 0 or len(near) == 1
    dead_flat, dead = add_dead_pixels(flat, dark, 0.1, 11)
    again, dead_again = add_dead_pixels(flat, dark, 0.1, 11)
    assert O.equal_bits(dead_flat, again) and np.array_equal(dead, dead_again) and dead.any() and not dead.all()
    assert O.equal_bits(dead_flat[dead], dark[dead]) and O.equal_bits(dead_flat[~dead], flat[~dead])
    t = add_zingers(torch.from_numpy(raw), 0.05, 3.0, 7)
    assert isinstance(t[0], torch.Tensor) and O.equal_bits(t[0].numpy(), add_zingers(raw, 0.05, 3.0, 7)[0])
    # the frames of a detector with dead pixels: the oracle repairs every dead pixel and counts it once per view
    raw = raw_frames(p, 1e5, dead_flat, dark)
    _, counts = O.condition(raw, dark, dead_flat, None, 3, 0.5)
    assert counts[:, 1].tolist() == [int(dead.sum())] * p.shape[0]
    for bad in ((raw[0], 0.1, 2.0), (raw, -0.1, 2.0), (raw, 0.1, 0.0)):
        with pytest.raises(ValueError):
            add_zingers(*bad, 0)
    with pytest.raises(ValueError):
        add_dead_pixels(flat, dark[:-1], 0.1, 0)
    with pytest.raises(ValueError):
        raw_frames(p, 1e5, flat[:-1], dark)


def test_condition_refuses_bad_shapes_sizes_and_dtypes_without_a_gpu():
    import torch
    from neuralvolumetricreconstructionformedicalimages_amd import frames
    raw, flat, dark = torch.zeros(2, 6, 8), torch.ones(6, 8), torch.zeros(6, 8)
    ok = dict(dif=0.1)
    with pytest.raises(ValueError, match="no CPU path"):
        frames.condition(raw, flat, dark, **ok)
    with pytest.raises(ValueError, match="no CPU path"):
        frames.condition(raw.to(torch.uint16), flat, dark, **ok)
    with pytest.raises(ValueError, match="must be a tensor"):
        frames.condition(raw.numpy(), flat, dark, **ok)
    for bad_raw in (raw.double(), raw[0], raw.to(torch.int16)):
        with pytest.raises(ValueError, match=r"raw must be float32 or uint16 \[N, H, W\]"):
            frames.condition(bad_raw, flat, dark, **ok)
    with pytest.raises(ValueError, match=r"flat must be float32 \(6, 8\)"):
        frames.condition(raw, flat[:5], dark, **ok)
    with pytest.raises(ValueError, match=r"dark must be float32 \(6, 8\)"):
        frames.condition(raw, flat, dark.double(), **ok)
    with pytest.raises(ValueError, match=r"bad must be uint8 or bool \(6, 8\)"):
        frames.condition(raw, flat, dark, bad=torch.zeros(6, 8), **ok)
    with pytest.raises(ValueError, match=r"out must be float32 \(2, 6, 8\)"):
        frames.condition(raw, flat, dark, out=torch.zeros(2, 6, 7), **ok)
    for size in (1, 4, 9, 0, -3):
        with pytest.raises(ValueError, match="size must be 3, 5 or 7"):
            frames.condition(raw, flat, dark, size=size, **ok)
    for size in (2.5, True, "5"):
        with pytest.raises(ValueError, match="must be an int"):
            frames.condition(raw, flat, dark, size=size, **ok)
    with pytest.raises(ValueError, match="above the 6 detector rows"):
        frames.condition(raw, flat, dark, size=7, **ok)
    with pytest.raises(ValueError, match="above the 5 detector columns"):
        frames.condition(torch.zeros(2, 8, 5), torch.ones(8, 5), torch.zeros(8, 5), size=7, **ok)
    for dif in (-0.1, float("nan"), float("inf"), "1", None):
        with pytest.raises(ValueError, match="dif must be"):
            frames.condition(raw, flat, dark, dif=dif)
    for t_min in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="t_min must be"):
            frames.condition(raw, flat, dark, t_min=t_min, **ok)
    with pytest.raises(ValueError, match="clamp needs log"):
        frames.condition(raw, flat, dark, log=False, clamp=True, **ok)
    with pytest.raises(TypeError):
        frames.condition(raw, flat, dark)                                                  # dif has no default
    assert frames.DEFAULT_T_MIN == 1e-5 and frames.SIZES == O.SIZES
    assert frames.check_size(7, 7, 9) == 7


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    workdir = str(tmp_path_factory.mktemp("frames_host_check"))
    return D.build(workdir), workdir


@needs_compiler
def test_host_window_words_equal_the_oracle(program):
    """Exit status 0 and nothing on stderr (`host_check.run` raises otherwise), and the program found no difference."""
    assert D.check_words(O, *program) > 0


@needs_compiler
def test_host_decision_and_counts_equal_the_oracle(program):
    assert D.check_decide(O, *program) > 0


@needs_compiler
def test_host_tail_is_within_the_host_logarithm_of_float64(program):
    n, worst = D.check_tail(O, *program)
    assert n > 0 and worst <= D.HOST_LOG_ULP
