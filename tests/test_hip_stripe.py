"""Sinogram stripe removal by sorting on the GPU (include/naf_hip.h A2): `stripe.remove_stripes` against the numpy
oracle of tests/_stripe_oracle.py.  The filter does no arithmetic, so every comparison is `==` on int32 views of the floats, which
also counts NaNs."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest
import torch

import _stripe_oracle as O

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (N, H, W, size): each the smallest shape that reaches a distinct path
ALL_KINDS = ((1, 1, 3, 3),            # the minimum
             (2, 3, 5, 5),            # size == W
             (48, 4, 64, 5),          # baseline
             (64, 2, 64, 9),          # an exact power of two, no padding
             (65, 2, 37, 7))          # the first padded rank; W a multiple of no tile
RANDOM_ONLY = ((50, 3, 130, 63),      # the largest window
               (300, 2, 270, 5),      # two runs of the median kernel, the second one short
               (1000, 1, 40, 5),      # 8 columns per workgroup of the sort kernel
               (4096, 1, 16, 3))      # the view cap: 2 columns per workgroup, 64 KiB of LDS
CASES = [(shape, kind) for shape in ALL_KINDS for kind in O.KINDS] + [(shape, "normal") for shape in RANDOM_ONLY]


def _stripe():
    from neuralvolumetricreconstructionformedicalimages_amd import stripe
    return stripe


def _equal(t, a):
    return tuple(t.shape) == a.shape and np.array_equal(t.cpu().numpy().view(np.int32), a.view(np.int32))


@pytest.mark.parametrize("shape,kind", CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else v)
def test_output_equals_the_oracle_bit_for_bit(shape, kind):
    N, H, W, size = shape
    p = O.data(kind, (N, H, W), seed=11)
    want = O.remove_stripes(p, size)
    d = torch.from_numpy(p).cuda()
    got = _stripe().remove_stripes(d, size=size)
    assert _equal(got, want), (shape, kind)
    assert _equal(d, p)                                                    # the input is left as it is
    assert _equal(_stripe().remove_stripes(d, size=size), want)            # across two calls


@pytest.mark.parametrize("kind", ("normal", "special"))
def test_equal_bits_in_place_by_row_groups_and_on_another_stream(kind):
    stripe = _stripe()
    N, H, W, size = 48, 5, 64, 5
    p = O.data(kind, (N, H, W), seed=13)
    want = O.remove_stripes(p, size)
    d = torch.from_numpy(p).cuda()
    one_row = stripe.workspace_bytes(N, H, W, rows=1)
    assert _equal(stripe.remove_stripes(d, size=size, workspace_bytes=one_row), want)            # five groups of one row
    assert _equal(stripe.remove_stripes(d, size=size, workspace_bytes=2 * one_row + 7), want)    # groups of 2, 2 and 1 rows
    assert _equal(stripe.remove_stripes(d, size=size, workspace_bytes=1 << 40), want)            # more than all rows need
    out = torch.full_like(d, 7.0)
    assert stripe.remove_stripes(d, size=size, out=out) is out and _equal(out, want)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        other = stripe.remove_stripes(d, size=size)
    stream.synchronize()
    assert _equal(other, want)
    for workspace in (None, one_row):                                                           # out is projections
        e = d.clone()
        assert stripe.remove_stripes(e, size=size, out=e, workspace_bytes=workspace) is e and _equal(e, want)


def test_empty_scans_are_a_no_op():
    stripe = _stripe()
    for shape in ((0, 4, 8), (3, 0, 8)):
        assert tuple(stripe.remove_stripes(torch.zeros(shape, device="cuda"), size=3).shape) == shape


def test_refusals_leave_out_untouched():
    stripe = _stripe()
    d = torch.from_numpy(O.data("normal", (6, 3, 8), seed=1)).cuda()
    out = torch.full_like(d, 7.0)
    bad = [dict(size=4), dict(size=9), dict(size=1), dict(size=65), dict(size=5.0), dict(workspace_bytes=6 * 8 * 6 - 1),
           dict(workspace_bytes=0), dict(workspace_bytes=1e6)]
    for kwargs in bad:
        with pytest.raises(ValueError):
            stripe.remove_stripes(d, out=out, **{"size": 5, **kwargs})
    for wrong in (torch.full((6, 3, 9), 7.0, device="cuda"), torch.full((6, 3, 8), 7.0), torch.full((6, 3, 8), 7.0, device="cuda",
                                                                                                  dtype=torch.float64)):
        with pytest.raises(ValueError):
            stripe.remove_stripes(d, size=5, out=wrong)
        assert bool((wrong == 7.0).all())
    with pytest.raises(ValueError, match="contiguous"):
        stripe.remove_stripes(d.transpose(1, 2), size=3, out=out)
    with pytest.raises(ValueError, match="contiguous"):
        stripe.remove_stripes(d, size=5, out=torch.full((6, 8, 3), 7.0, device="cuda").transpose(1, 2))
    flat = torch.full((d.numel() + 8,), 7.0, device="cuda")
    with pytest.raises(ValueError, match="overlap"):
        stripe.remove_stripes(flat[:d.numel()].view(6, 3, 8), size=5, out=flat[8:].view(6, 3, 8))
    with pytest.raises(ValueError, match="no CPU path"):
        stripe.remove_stripes(d.cpu(), size=5, out=out)
    with pytest.raises(ValueError, match="at most 4096 views"):
        stripe.remove_stripes(torch.zeros(4097, 1, 3, device="cuda"), size=3)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


def test_tool_filters_a_striped_pickle_and_two_runs_write_the_same_bytes(tmp_path):
    from neuralvolumetricreconstructionformedicalimages_amd.dataset import TIGREDataset
    sys.path.insert(0, os.path.join(REPO, "tools"))
    try:
        import remove_stripes as tool
    finally:
        sys.path.remove(os.path.join(REPO, "tools"))
    scan = str(tmp_path / "striped.pickle")
    made = subprocess.run([sys.executable, os.path.join(REPO, "tools", "make_synthetic_scan.py"), "--out", scan, "--n-voxel", "16",
                           "--n-train", "8", "--n-val", "2", "--device", "cpu", "--stripes", "0.1", "0.05"],
                          capture_output=True, text=True, timeout=300)
    assert made.returncode == 0, made.stderr
    with open(scan, "rb") as handle:
        data = pickle.load(handle)
    assert data["stripes"] == {"fraction": 0.1, "sigma": 0.05, "seed": 0}
    outs = [str(tmp_path / f"out{k}.pickle") for k in range(2)]
    results = [tool.main(["--scan", scan, "--out", path]) for path in outs]
    with open(outs[0], "rb") as a, open(outs[1], "rb") as b:
        first = a.read()
        assert first == b.read()
    filtered = pickle.loads(first)
    W = data["train"]["projections"].shape[2]
    size = _stripe().default_size(W)
    assert results[0]["train"]["size"] == size and "psnr_3d" in results[0]["before"] and "ssim_3d" in results[0]["after"]
    for split in ("train", "val"):
        views = torch.from_numpy(np.ascontiguousarray(data[split]["projections"], dtype=np.float32)).cuda()
        assert _equal(_stripe().remove_stripes(views, size=size), filtered[split]["projections"])
        assert filtered[split]["stripe_size"] == size
        assert np.array_equal(filtered[split]["angles"], data[split]["angles"])
        ds = TIGREDataset(outs[0], n_rays=64, type=split, device="cuda")
        assert _equal(ds.projs, filtered[split]["projections"])
