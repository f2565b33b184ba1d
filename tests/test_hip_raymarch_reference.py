"""The stand-alone ray-march operators (csrc/render_ops.hip, and emit_samples of csrc/mlp_tile_io.h through
naf_render_forward_samples) against the float64 restatements of tests/_raymarch_oracle.py, at the smallest shapes that reach each
branch: a second trip of every grid-stride loop, a wave's second ray in fine_depths_kernel, the cdf's 64-interval chunks and
their carry, merged lengths on either side of the sort's power of two, the 64 KiB LDS shape, the `denom < 1e-5` rule, the weight
floor, u on a cdf entry, the lane stride and last distance of the integrals, the range check's ordered min / max and its NaN rule.

Tolerances and where they come from: the oracle module's docstring and tests/test_raymarch_oracle_cpu.py.  Every output buffer is
followed by a guard of NaN that has to stay intact.  Every test prints the worst fraction of its tolerance.

naf_normalize_inputs tested the reduced min / max against the range, and fminf / fmaxf drop a NaN on the way there: read in the
kernel while the nan_* cases of test_normalize_inputs were written (the earlier kernel was not run against them), and changed so
that every value is tested.  Those cases hold the documented rule (flag[0] for a NaN) from now on."""
import functools

import numpy as np
import pytest
import torch

import _mlp16_oracle as M16
import _mlp32_oracle as M32
import _raymarch_oracle as O

pytestmark = pytest.mark.gpu
GUARD = 64
# sigma: the tolerances the MLP oracles hold sigma's line integral to (relative L2; 2e-6 both)
SIGMA_TOL = {"bf16": M16.TOL_ACC, "f32": M32.F32_TOL["acc"]}


def _abi():
    from neuralvolumetricreconstructionformedicalimages_amd import _abi
    return _abi


class Guarded:
    """A device buffer of `shape` with GUARD words of NaN behind it."""

    def __init__(self, *shape, dtype=torch.float32):
        n = int(np.prod(shape))
        self.flat = torch.full((n + GUARD,), float("nan") if dtype.is_floating_point else -559038737, dtype=dtype, device="cuda")
        self.t = self.flat[:n].view(*shape)
        self.dtype = dtype

    def intact(self):
        g = self.flat[-GUARD:]
        return bool(torch.isnan(g).all()) if self.dtype.is_floating_point else bool((g == -559038737).all())

    def numpy(self):
        return self.t.cpu().numpy()


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---- naf_sample_rays ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_pts", [True, False])
@pytest.mark.parametrize("perturb", [0, 1])
@pytest.mark.parametrize("n,S", [(1, 2), (3, 65), (8200, 257)])       # 8 200 x 257 = 2 107 400: one element past two trips of the loop
def test_sample_rays_is_bit_exact(n, S, perturb, with_pts):
    A = _abi()
    rays = O.make_rays(n, 7 + n)
    t_rand = np.random.default_rng(n + S).random((n, S)).astype(np.float32)
    z_ref, p_ref = O.sample(rays, t_rand, S, bool(perturb), 0.3)
    z, pts = Guarded(n, S), Guarded(n, S, 3)
    rd, td = _dev(rays), _dev(t_rand)
    A.check(A.lib().naf_sample_rays(A.ptr(rd), A.ptr(td), A.ptr(z.t), A.ptr(pts.t) if with_pts else None, n, S, perturb, 0.3, 0, 0,
                                    A.stream_ptr()), "sample_rays")
    torch.cuda.synchronize()
    assert z.intact() and pts.intact()
    got = z.numpy()
    assert got[-1, -1] == z_ref[-1, -1]                               # the last ray's last sample: the end of the last trip
    assert np.array_equal(got, z_ref)
    if with_pts:
        assert np.array_equal(pts.numpy()[-1, -1], p_ref[-1, -1]) and np.array_equal(pts.numpy(), p_ref)
    else:
        assert bool(torch.isnan(pts.flat).all())                      # untouched


# ---- naf_integrate_forward / naf_integrate_backward ---------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [5, 32768 + 7])                         # 32 768 waves in the capped grid: the second trip
@pytest.mark.parametrize("S", O.INTEGRATE_S)
def test_integrals_match_the_float64_reference(n, S):
    A = _abi()
    rays, z, sigma, grad = O.integrate_inputs(n, S)
    acc_ref, scale = O.integrate(sigma, z, rays)
    gs_ref = O.integrate_adjoint(grad, z, rays)
    acc, gs = Guarded(n), Guarded(n, S)
    rd, zd, sd, gd = _dev(rays), _dev(z), _dev(sigma), _dev(grad)
    A.check(A.lib().naf_integrate_forward(A.ptr(sd), A.ptr(zd), A.ptr(rd), A.ptr(acc.t), n, S, A.stream_ptr()), "integrate_forward")
    A.check(A.lib().naf_integrate_backward(A.ptr(gd), A.ptr(zd), A.ptr(rd), A.ptr(gs.t), n, S, A.stream_ptr()), "integrate_backward")
    torch.cuda.synchronize()
    assert acc.intact() and gs.intact()
    got, live = acc.numpy().astype(np.float64), scale > 0
    assert (got[~live] == 0).all() and got[n // 2] == 0               # the all-zero ray: an exact 0
    f_acc = O.sum_fraction(got, acc_ref, scale, O.TOL_SUM)
    f_gs = float((np.abs(gs.numpy() - gs_ref) / np.abs(gs_ref)).max()) / O.TOL_GRAD
    print(f"raymarch integrate ({n}, {S}): acc {f_acc:.3f}, grad_sigma {f_gs:.3f} of their tolerances")
    assert f_acc < 1.0 and f_gs < 1.0


# ---- naf_render_forward_samples: emit_samples ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _pair():
    from _naf_helpers import naf_pair
    net, ref = naf_pair(seed=14, oracle=True)
    return net.cuda(), ref


def _net():
    return _pair()[0]


def _sigma_reference(rays, z, prec):
    """sigma of the float64 rehearsal (_mlp16_oracle.forward_points, which _mlp32_oracle takes over unchanged) on the oracle
    encoder's features: rounded to bf16 where they enter an MFMA in bf16 mode, exact (rnd = identity: the f32 layout of
    _mlp32_oracle) in f32 mode."""
    ref = _pair()[1]
    rnd = M32.identity if prec == "f32" else M32.bf16_round
    with torch.no_grad():
        pts = M32.O.R.points_on_rays(torch.from_numpy(rays), torch.from_numpy(z), M32.O.BOUND).reshape(-1, 3)
        x = ref.encoder(pts, M32.O.BOUND).double()
        sig = M32.O.forward_points(rnd(x), M32.O.mlp_params(ref.layers, rnd, torch.float64), rnd)[3]
    return sig.numpy().reshape(z.shape)


@pytest.mark.parametrize("prec", ["f32", "bf16"])
@pytest.mark.parametrize("n", [41, 1])
@pytest.mark.parametrize("S", [2, 15, 16, 17, 33, 64, 65, 100])
def test_running_optical_depth_is_the_scan_of_the_kernels_own_sigma(S, n, prec):
    """tau against the float64 cumulative sum of the kernel's OWN fp32 sigma times dist, per element: the scan and its carry between
    tiles (16 samples in bf16 mode, 32 in f32), the network taken as data.  (S = 1 is refused by the library: below.)"""
    from neuralvolumetricreconstructionformedicalimages_amd import fused
    A = _abi()
    rays = O.make_rays(n, 19)
    t_rand = np.random.default_rng(S).random((n, S)).astype(np.float32)
    z = O.sample(rays, t_rand, S, True, 0.3)[0]
    precision = A.F32 if prec == "f32" else A.BF16
    rd, td = _dev(rays), _dev(t_rand)
    acc, sigma, tau = fused.render_samples(rd, _net(), S, True, t_rand=td, mlp_precision=precision)
    only = fused.render_samples(rd, _net(), S, True, t_rand=td, mlp_precision=precision, want_sigma=False, want_depth=False)[0]
    torch.cuda.synchronize()
    assert torch.equal(only, acc)                                      # the per-sample outputs change no bit of acc
    sg = sigma.cpu().numpy()
    assert np.isfinite(sg).all() and (sg >= 0).all() and (sg <= 1).all()  # a sigmoid
    sg_ref = _sigma_reference(rays, z, prec)
    f_sg = M16.rel_l2(sg, sg_ref) / SIGMA_TOL[prec]
    print(f"raymarch sigma {prec} ({n}, {S}): rel-L2 {f_sg:.3f} of its tolerance, largest |difference| {np.abs(sg - sg_ref).max():.3g}")
    tau_ref, scale = O.running_depth(sg, z, rays)
    f_tau = float((np.abs(tau.cpu().numpy() - tau_ref) / scale).max()) / O.TOL_TAU
    f_acc = float((np.abs(acc.cpu().numpy() - tau_ref[:, -1]) / scale[:, -1]).max()) / O.TOL_SUM
    f_last = float((np.abs(tau[:, -1].cpu().numpy().astype(np.float64) - acc.cpu().numpy()) / scale[:, -1]).max()) / O.TOL_TAU
    print(f"raymarch tau {prec} ({n}, {S}): tau {f_tau:.3f}, acc {f_acc:.3f}, tau[-1] against acc {f_last:.3f} of their tolerances")
    assert f_tau < 1.0 and f_acc < 1.0 and f_last < 1.0 and f_sg < 1.0


def test_one_sample_per_ray_is_refused_by_the_fused_forward():
    from neuralvolumetricreconstructionformedicalimages_amd import fused
    with pytest.raises(RuntimeError, match="n_samples must be >= 2"):
        fused.render_samples(_dev(O.make_rays(3, 1)), _net(), 1, False)


# ---- naf_fine_depths ---------------------------------------------------------------------------------------------------------------------
def _fine(rays, t_rand, sigma, u, NF, det, perturb=1, want_weights=True, seed=0, base=0):
    A = _abi()
    n, S = sigma.shape
    out, w, scratch = Guarded(n, S + NF), Guarded(n, S), Guarded(1, dtype=torch.int32)
    rd, td, sd, ud = _dev(rays), _dev(t_rand), _dev(sigma), _dev(u)
    rc = A.lib().naf_fine_depths(A.ptr(rd), A.ptr(td), A.ptr(sd), A.ptr(ud), A.ptr(out.t), A.ptr(w.t) if want_weights else None, n, S, NF,
                                 perturb, int(det), seed, base, A.ptr(scratch.t), A.stream_ptr())
    A.check(rc, "fine_depths")
    torch.cuda.synchronize()
    assert out.intact() and w.intact() and scratch.intact()
    return out.numpy(), w.numpy() if want_weights else w, scratch.numpy().view(np.float32)[0]


def _hold(name, rays, z, sigma, u, NF, det, got, w, wmax):
    ref = O.resample(sigma, z, u, NF, det)
    n, S = sigma.shape
    assert got.shape == (n, S + NF)
    assert float(wmax) == float(np.float32(ref["wmax"]))              # the scratch word: the call's maximum (differences are exact here or round alike)
    f_w = float(np.abs(w - ref["weights"]).max() / ref["weights"].max()) / O.TOL_WEIGHT
    assert (np.diff(got, axis=-1) >= 0).all()                          # non-decreasing
    assert O.contains_coarse(got, z)                                   # the coarse depths, bit for bit
    m = O.match_rows(ref, got)
    skipped, undecided = O.exclusion(ref)
    print(f"raymarch fine_depths {name} ({n}, {S}, {NF}): weights {f_w:.3f}, depths {m['worst'] / O.TOL_DEPTH:.3f} of their tolerances; "
          f"{m['skipped']} rays skipped, {m['through_alternative']} matched through an alternative, {undecided:.1%} with an undecided sample")
    assert f_w < 1.0 and not m["failed"], m["failed"][:5]
    return m


@pytest.mark.parametrize("case", O.RESAMPLE_CASES, ids=[c[0] for c in O.RESAMPLE_CASES])
def test_fine_depths_match_the_float64_reference(case):
    """What each case reaches: s3 / s4 the smallest legal shapes; p_exact S + NF = 128 = P, p_plus1 129 (P = 256, 127 words of INFINITY);
    one_chunk 64 intervals, a full chunk and no carry; first_carry* 65 intervals, merged 128; p512 merged 257; three_chunks 193
    intervals; lds_64k S = NF = 1 024: 4 waves x (2 048 + 2 048) words = 65 536 bytes of LDS; second_ray 32 775 rays on 32 768
    waves: a wave's LDS reused behind the trailing wave_lds_sync(); second_max_trip 4 100 x 257 = 1 053 700 elements, the second
    trip of fine_weight_max_kernel, the call's maximum in its very last element; det*: evenly spaced u, u = 1.0 included."""
    name, n, S, NF, pattern, det = case
    rays, t_rand, sigma, u = O.resample_inputs(case)
    z = O.sample(rays, t_rand, S, True, 0.3)[0]
    got, w, wmax = _fine(rays, t_rand, sigma, u, NF, det)
    _hold(name, rays, z, sigma, u, NF, det, got, w, wmax)
    if name in ("s3", "first_carry"):
        again, no_w, _ = _fine(rays, t_rand, sigma, u, NF, det, want_weights=False)    # weights_out = NULL is accepted
        assert np.array_equal(again, got) and bool(torch.isnan(no_w.flat).all())


@pytest.mark.parametrize("which", ["equal", "walk"])
def test_fine_depths_hand_built_u(which):
    """u = 0, 0.5 (exactly the middle cdf entry of two equal intervals), the largest float below 1, 0.25, 0.75: no sample of these
    rows is undecided (tests/test_raymarch_oracle_cpu.py), so the rows match directly."""
    rays = O.make_rays(6, 91)
    S = 4 if which == "equal" else 67
    sigma = np.tile(np.array([0.0, 0.25, 0.5, 0.25], np.float32), (6, 1)) if which == "equal" else O.make_sigma("walk", 6, S, 17)
    u = np.tile(np.array([0.0, 0.5, np.nextafter(np.float32(1), np.float32(0)), 0.25, 0.75], np.float32), (6, 1))
    t_rand = np.random.default_rng(4).random((6, S)).astype(np.float32)
    z = O.sample(rays, t_rand, S, True, 0.3)[0]
    got, w, wmax = _fine(rays, t_rand, sigma, u, 5, False)
    m = _hold("hand-built " + which, rays, z, sigma, u, 5, False, got, w, wmax)
    assert m["skipped"] == 0 and m["through_alternative"] == 0


def test_fine_depths_device_jitter_is_reproducible_and_shardable():
    """t_rand = u = NULL: the counter-based generator.  No reference here: the same seed gives the same bits, and rays[k:] with
    ray_index_base = k give rows k: of the full call (the weights' maximum is the full call's in both: it sits in the rows kept)."""
    n, S, NF, k = 50, 67, 61, 13
    rays = O.make_rays(n, 23)
    sigma = O.make_sigma("walk", n, S, 29)
    sigma[-1, -1] = sigma[-1, -2] + np.float32(1.0)
    a, wa, _ = _fine(rays, None, sigma, None, NF, False, seed=7)
    b, wb, _ = _fine(rays, None, sigma, None, NF, False, seed=7)
    c, _, _ = _fine(rays, None, sigma, None, NF, False, seed=8)
    tail, wt, _ = _fine(rays[k:], None, sigma[k:], None, NF, False, seed=7, base=k)
    assert np.array_equal(a, b) and np.array_equal(wa, wb) and not np.array_equal(a, c)
    assert np.array_equal(tail, a[k:]) and np.array_equal(wt, wa[k:])


def test_fine_depths_error_returns():
    """S < 3, NF = 0, S > 1 024 and S + NF > 2 048 are refused before anything is launched.  The `lds > 64 KiB` branch of
    naf_fine_depths cannot be reached under those limits: the largest legal shape, S = NF = 1 024, needs 4 x (2 x 1 024 + 2 048) x 4
    = 65 536 bytes exactly, which the lds_64k case above runs."""
    A = _abi()
    rays, sigma = _dev(O.make_rays(2, 1)), torch.zeros(2, 2048, device="cuda")
    out, scratch = torch.zeros(2, 4096, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    for S, NF in ((2, 4), (8, 0), (1025, 1), (1024, 1025), (1000, 1049)):
        rc = A.lib().naf_fine_depths(A.ptr(rays), None, A.ptr(sigma), None, A.ptr(out), None, 2, S, NF, 0, 1, 0, 0, A.ptr(scratch), A.stream_ptr())
        assert rc != 0, (S, NF)
    torch.cuda.synchronize()
    assert not out.any()


# ---- naf_normalize_inputs ------------------------------------------------------------------------------------------------------------------
def _normalize_cases():
    f = np.float32
    size = f(0.3)
    up, down = np.nextafter(size, f(1)), np.nextafter(size, f(0))
    inside = ((np.random.default_rng(0).random(63) * 2 - 1) * down).astype(f)
    big = ((np.random.default_rng(1).random(2097152 + 5) * 2 - 1) * down).astype(f)
    big_out = big.copy()
    big_out[-1] = up                                                   # out of range in the last element of the second trip only
    big_nan = big.copy()
    big_nan[-1] = np.nan
    return size, {
        "one": np.array([0.125], f), "all_negative": -np.abs(inside) - f(1e-6), "zeros": np.array([-0.0, 0.0, -0.0], f),
        "denormal": np.array([1e-45, -1e-45, 0.1], f), "exactly_size": np.array([-size, size, 0.0], f),
        "one_ulp_above": np.concatenate([inside, [up, 0.0]]).astype(f), "one_ulp_below": np.concatenate([[0.0, -up], inside]).astype(f),
        "inf": np.array([0.0, np.inf], f), "minus_inf": np.array([-np.inf, 0.0], f),
        "nan_last": np.concatenate([inside, [0.1, np.nan]]).astype(f), "nan_first": np.concatenate([[np.nan, 0.1], inside]).astype(f),
        "nan_alone": np.array([np.nan], f),
        "two_trips": big, "two_trips_out_last": big_out, "two_trips_nan_last": big_nan,
    }


_SIZE, _NORM = _normalize_cases()


@pytest.mark.parametrize("name", list(_NORM))
def test_normalize_inputs(name):
    """n = 1, 3, 63, 65 and 2 097 152 + 5 (one wave past the capped grid's first trip).  flag[0], and flag[1] / flag[2] decoded, against
    the oracle; out01 bit for bit; out01 = NULL."""
    A = _abi()
    x = _NORM[name]
    out_ref, flag_ref, mn, mx = O.normalize(x, _SIZE)
    xd = _dev(x)
    init = torch.tensor([0, O.INT32_MAX, O.INT32_MIN], dtype=torch.int32, device="cuda")
    for with_out in (True, False):
        out, flag = Guarded(x.size), Guarded(3, dtype=torch.int32)
        flag.t.copy_(init)
        A.check(A.lib().naf_normalize_inputs(A.ptr(xd), x.size, float(_SIZE), A.ptr(out.t) if with_out else None, A.ptr(flag.t), A.stream_ptr()),
                "normalize_inputs")
        torch.cuda.synchronize()
        assert out.intact() and flag.intact()
        bad, lo, hi = flag.t.tolist()
        assert bool(bad) == flag_ref, (name, bad)
        if mn is None:
            assert (lo, hi) == (O.INT32_MAX, O.INT32_MIN)
        else:
            assert O.unordered_float(lo) == mn and O.unordered_float(hi) == mx, (name, O.unordered_float(lo), O.unordered_float(hi), mn, mx)
        if with_out:
            real = ~np.isnan(x)                                        # bit for bit (+-0 told apart); a NaN's payload aside
            assert np.array_equal(out.numpy()[real].view(np.int32), out_ref[real].view(np.int32))
            assert np.isnan(out.numpy()[np.isnan(x)]).all()
        else:
            assert bool(torch.isnan(out.flat).all())
