"""The row filter with a weight per view and column on the GPU (naf_filter_rows_views, filter.filter_rows(..., col=...)) against
the float64 convolution of tests/_short_scan_oracle.py, and `reconstruct.fdk(..., short_scan="parker")` against its float64
rehearsal (include/naf_hip.h P3).

The kernel's bound is that of tests/test_hip_filter.py with one more rounding, for the multiply by `col`:
(W + 4) 2^-24 |view_scale post| sum_k |taps pre in col| per element.  The volume's bound is that of tests/test_hip_fdk.py."""
import ctypes

import numpy as np
import pytest
import torch

import _filter_oracle as F
import _short_scan_oracle as S

pytestmark = pytest.mark.gpu

N = S.REHEARSAL_SIZES[0]


def _dev(a):
    return None if a is None else torch.tensor(a, device="cuda")


def _run(x, taps, pre=None, post=None, scale=None, col=None, out=None):
    from neuralvolumetricreconstructionformedicalimages_amd.filter import filter_rows
    return filter_rows(x, _dev(taps), _dev(pre), _dev(post), _dev(scale), _dev(col), out=out)


def _entry(name, x, taps, pre, post, scale, *col):
    """The library's entry point `name` called directly, every factor a device tensor or None -> the output tensor."""
    from neuralvolumetricreconstructionformedicalimages_amd import _abi
    n, h, w = x.shape
    out = torch.full_like(x, float("nan"))
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    args = [p(x), n, h, w, p(taps), p(pre), p(post), p(scale), *(p(c) for c in col), p(out), _abi.stream_ptr()]
    assert getattr(_abi.lib(), name)(*args) == 0, _abi.lib().naf_last_error()
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("factors", ["all", "col"])
@pytest.mark.parametrize("shape", S.SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_kernel_matches_the_convolution(shape, factors):
    x, taps, pre, post, scale, col = S.filter_inputs(shape)
    if factors == "col":
        pre = post = scale = None
    want = S.filter_rows(x, taps, pre, post, scale, col)
    bound = S.filter_bound(x, taps, pre, post, scale, col)
    xd = _dev(x)
    got = _run(xd, taps, pre, post, scale, col)
    assert got.shape == xd.shape and got.dtype == torch.float32 and got.data_ptr() != xd.data_ptr()
    assert torch.equal(xd, _dev(x))                                   # the input is left as it is
    err = np.abs(got.cpu().numpy().astype(np.float64) - want)
    ratio = float((err / np.maximum(bound, np.finfo(np.float64).tiny)).max())
    print(f"{shape} {factors}: max |out - float64| {err.max():.3e}, worst ratio to the bound {ratio:.4f}")
    assert np.all(err <= bound)
    assert float(np.abs(want - F.filter_rows(x, taps, pre, post, scale)).max()) > 0      # col changes the result


def test_bits_against_the_plain_entry():
    """`col` NULL and `col` of ones through naf_filter_rows_views are naf_filter_rows, bit for bit (1 * x is x); a `col` that is zero
    for one view zeroes exactly that view (+-0: view_scale * post is finite); in place, into a buffer, and twice: the same bits."""
    shape = (3, 5, 300)
    x, taps, pre, post, scale, col = S.filter_inputs(shape)
    xd, td, pd, qd, sd = (_dev(a) for a in (x, taps, pre, post, scale))
    plain = _entry("naf_filter_rows", xd, td, pd, qd, sd)
    assert bool(torch.isfinite(plain).all()) and float(plain.abs().max()) > 0
    assert torch.equal(_entry("naf_filter_rows_views", xd, td, pd, qd, sd, None), plain)
    assert torch.equal(_entry("naf_filter_rows_views", xd, td, pd, qd, sd, torch.ones(3, 300, device="cuda")), plain)
    assert torch.equal(_entry("naf_filter_rows", xd, td, None, None, None), _entry("naf_filter_rows_views", xd, td, None, None, None, None))
    assert torch.equal(_run(xd, taps, pre, post, scale), plain)
    gate = np.ones((3, 300), dtype=np.float32)
    gate[1] = 0.0
    gated = _run(xd, taps, pre, post, scale, gate)
    assert bool(torch.isfinite(_dev(scale)[:, None, None] * _dev(post)).all())
    assert float(gated[1].abs().max()) == 0.0 and torch.equal(gated[0], plain[0]) and torch.equal(gated[2], plain[2])
    first = _run(xd, taps, pre, post, scale, col)
    assert not torch.equal(first, plain)
    assert torch.equal(_run(xd, taps, pre, post, scale, col), first)
    out = torch.full_like(first, float("nan"))
    assert _run(xd, taps, pre, post, scale, col, out=out) is out and torch.equal(out, first)
    work = xd.clone()
    same = _run(work, taps, pre, post, scale, col, out=work)
    assert same.data_ptr() == work.data_ptr() and torch.equal(work, first)


def test_col_is_checked_like_the_other_weights():
    from neuralvolumetricreconstructionformedicalimages_amd.filter import filter_rows
    x = torch.rand(2, 3, 16, device="cuda")
    taps = torch.rand(16, device="cuda")
    col = torch.rand(2, 16, device="cuda")
    with pytest.raises(RuntimeError, match="no CPU path"):
        filter_rows(x, taps, col=col.cpu())
    with pytest.raises(ValueError, match="col must be"):
        filter_rows(x, taps, col=torch.rand(3, 16, device="cuda"))
    with pytest.raises(ValueError, match="col must be"):
        filter_rows(x, taps, col=col.double())
    with pytest.raises(ValueError, match="col must be"):
        filter_rows(x, taps, col=torch.rand(16, 2, device="cuda").t())
    t8 = torch.ones(8, device="cuda")
    assert tuple(filter_rows(torch.zeros(0, 4, 8, device="cuda"), t8, col=torch.zeros(0, 8, device="cuda")).shape) == (0, 4, 8)


@pytest.mark.parametrize("deterministic", [False, True], ids=["atomic", "deterministic"])
def test_short_scan_volume_matches_the_rehearsal(deterministic):
    from neuralvolumetricreconstructionformedicalimages_amd import fdk
    r = S.short_scan_rehearsal(N, "parker")
    b = torch.tensor(r["b"], device="cuda")
    x = fdk(b, r["geo"], r["angles"], short_scan="parker", deterministic=deterministic)
    assert x.dtype == torch.float32 and tuple(x.shape) == (N, N, N) and x.device == b.device
    got = x.cpu().numpy().astype(np.float64)
    e_filter = S.filter_bound(r["b"], *r["weights"])
    bound = 2e-5 * float(r["AT"](np.abs(r["y"])).max()) + r["AT"](e_filter)
    err = np.abs(got - r["x"])
    interior, background = S.masks(r["geo"])
    print(f"{N}^3 over 220 degrees, deterministic={deterministic}: max |x - float64| {err.max():.3e} of max |x| "
          f"{np.abs(r['x']).max():.3f}; bound {bound.min():.3e} .. {bound.max():.3e}, worst ratio {(err / bound).max():.4f}; "
          f"background mean |x| {np.abs(got[background]).mean():.5f} (float64 {r['background']:.5f})")
    assert np.all(err <= bound)
    if deterministic:
        again = fdk(b, r["geo"], r["angles"], short_scan="parker", deterministic=True)
        assert torch.equal(again, x)
    plain = fdk(b, r["geo"], r["angles"], deterministic=deterministic).cpu().numpy().astype(np.float64)
    want = S.short_scan_rehearsal(N, None)
    assert np.all(np.abs(plain - want["x"]) <= 2e-5 * float(want["AT"](np.abs(want["y"])).max())
                  + want["AT"](F.filter_bound(want["b"], *want["weights"])))
    with pytest.raises(ValueError, match="short_scan"):
        fdk(b, r["geo"], r["angles"], short_scan="hann")
