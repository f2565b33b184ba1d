#!/usr/bin/env python3
"""Volume resize benchmark: volume.resize_volume (naf_resize_volume, cubic B-spline, no prefilter) at the shapes a scan is made
from, against the same definition as three dense tap-matrix products in torch on the GPU and scipy.ndimage.zoom on the host.

    python tools/resize_bench.py                                  # one JSON line per shape and kernel form
    python tools/resize_bench.py --shapes 128,128,128:256,256,256 --cpu

Reported per shape: the kernel time of the library's own choice of form and of each forced form that fits (device events around
`--iters` calls after warm-up, median of `--repeats` windows; the workspace is allocated once, the minimum / maximum pass is
included), the algorithmic bytes 4 x (inputs + outputs) and their rate, the torch baseline (fp32 `tensordot` with dense [b, a] tap
matrices, one per axis), the largest difference of the kernel from the float64 definition on `--probe` seeded output voxels, and
with `--cpu` one run of scipy.ndimage.zoom(order=3, prefilter=False) where scipy imports.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DEFAULT_SHAPES = "128,128,128:256,256,256;512,512,300:256,256,256;256,256,256:512,512,512;512,512,512:1024,1024,1024"


def axis_taps(a, b):
    """The definition for one axis in float64: mirrored tap indices [b, 4] and cubic B-spline weights [b, 4]."""
    r = np.float64(a - 1) / np.float64(b - 1) if b > 1 else np.float64(1.0)
    x = np.arange(b, dtype=np.float64) * r
    f = np.floor(x)
    t = x - f
    w = np.stack([(1 - t) ** 3 / 6, (3 * t ** 3 - 6 * t ** 2 + 4) / 6, (-3 * t ** 3 + 3 * t ** 2 + 3 * t + 1) / 6, t ** 3 / 6], 1)
    idx = f.astype(np.int64)[:, None] - 1 + np.arange(4)[None, :]
    if a == 1:
        idx[:] = 0
    else:
        idx = np.mod(idx, 2 * (a - 1))
        idx = np.where(idx >= a, 2 * (a - 1) - idx, idx)
    return idx, w


def tap_matrix(a, b):
    idx, w = axis_taps(a, b)
    m = np.zeros((b, a), dtype=np.float64)
    np.add.at(m, (np.repeat(np.arange(b), 4), idx.reshape(-1)), w.reshape(-1))
    return m


def torch_resize(x, mats):
    """Three tensordots with the dense per-axis tap matrices (fp32 on the device)."""
    v = torch.tensordot(mats[0], x, dims=([1], [0]))
    v = torch.tensordot(mats[1], v, dims=([1], [1])).permute(1, 0, 2)
    return torch.tensordot(v, mats[2], dims=([2], [1])).contiguous()


def probe_error(xh, out, b, count, seed):
    """max |kernel - float64 definition| on `count` seeded output voxels (each from its 64 taps)."""
    taps = [axis_taps(xh.shape[k], b[k]) for k in range(3)]
    rng = np.random.default_rng(seed)
    pts = np.stack([rng.integers(0, b[k], count) for k in range(3)], 1)
    got = out[tuple(torch.as_tensor(pts[:, k], device=out.device) for k in range(3))].cpu().numpy()
    worst = 0.0
    for p, g in zip(pts, got):
        i, w = zip(*((taps[k][0][p[k]], taps[k][1][p[k]]) for k in range(3)))
        ref = np.einsum("i,j,k,ijk->", w[0], w[1], w[2], xh[np.ix_(i[0], i[1], i[2])].astype(np.float64))
        worst = max(worst, abs(float(g) - float(ref)))
    return worst


def _events(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def run(a, b, warmup, iters, repeats, baseline_iters, probe, cpu):
    from neuralvolumetricreconstructionformedicalimages_amd import _abi
    g = torch.Generator(device="cuda").manual_seed(0)
    x = torch.rand(a, device="cuda", generator=g) * 4000 - 1000                  # HU-like values
    lib = _abi.lib()
    ad, bd = (ctypes.c_uint32 * 3)(*a), (ctypes.c_uint32 * 3)(*b)
    ws = torch.empty(lib.naf_resize_volume_workspace_bytes(ad, bd), dtype=torch.uint8, device="cuda")
    out = torch.empty(b, dtype=torch.float32, device="cuda")
    minmax = torch.empty(2, dtype=torch.float32, device="cuda")

    def kernel():
        return lib.naf_resize_volume(_abi.ptr(x), ad, 1.0, 0.0, _abi.ptr(out), bd, _abi.ptr(minmax), _abi.ptr(ws), ws.numel(),
                                     _abi.stream_ptr())

    algo = 4 * (int(np.prod(a)) + int(np.prod(b)))
    res = {"in": list(a), "out": list(b), "algorithmic_bytes": algo}
    xh = x.cpu().numpy()
    for form in ("auto", "tiled", "direct"):
        os.environ.pop("NAF_RESIZE_FORM", None)
        if form != "auto":
            os.environ["NAF_RESIZE_FORM"] = form
        if kernel() == -2:                                                     # the tiled form does not fit these shapes
            res[f"{form}_ms"] = None
            continue
        for _ in range(warmup):
            _abi.check(kernel(), "resize_volume")
        torch.cuda.synchronize()
        ms = statistics.median(_events(kernel, iters) for _ in range(repeats))
        res[f"{form}_ms"] = round(ms, 4)
        res[f"{form}_algorithmic_GB_per_s"] = round(algo / ms * 1e-6, 1)
        res[f"{form}_max_abs_err"] = probe_error(xh, out, b, probe, seed=1)
    os.environ.pop("NAF_RESIZE_FORM", None)
    res["max_abs_input"] = float(np.abs(xh).max())
    try:
        mats = [torch.as_tensor(tap_matrix(a[k], b[k]), dtype=torch.float32, device="cuda") for k in range(3)]
        ref = torch_resize(x, mats)
        _abi.check(kernel(), "resize_volume")
        res["abs_diff_vs_torch"] = float((ref - out).abs().max())
        del ref
        torch.cuda.synchronize()
        bms = statistics.median(_events(lambda: torch_resize(x, mats), 1) for _ in range(baseline_iters))
        res.update(torch_tensordot_ms=round(bms, 3), speedup_vs_torch=round(bms / res["auto_ms"], 1))
        del mats
    except torch.cuda.OutOfMemoryError:
        res.update(torch_tensordot_ms=None, torch_note="out of device memory")
    torch.cuda.empty_cache()
    if cpu:
        try:
            from scipy import ndimage
            t0 = time.perf_counter()
            ref = ndimage.zoom(xh, [q / p for p, q in zip(a, b)], order=3, prefilter=False)
            res["scipy_s"] = round(time.perf_counter() - t0, 2)
            _abi.check(kernel(), "resize_volume")
            res["abs_diff_vs_scipy"] = float(np.abs(out.cpu().numpy() - ref).max())
        except ImportError:
            res["scipy_s"] = None
    del x, out
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=DEFAULT_SHAPES, help="a1,a2,a3:b1,b2,b3 pairs separated by ';'")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--baseline-iters", type=int, default=3)
    ap.add_argument("--probe", type=int, default=2048, help="output voxels checked against the float64 definition")
    ap.add_argument("--cpu", action="store_true", help="also time scipy.ndimage.zoom on the host (one run per shape)")
    ap.add_argument("--cpu-max-voxels", type=int, default=1 << 27, help="largest output scipy is run on")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("resize_bench.py needs an MI355X: naf_resize_volume has no CPU path")
    for pair in args.shapes.split(";"):
        a, b = (tuple(int(v) for v in side.split(",")) for side in pair.split(":"))
        res = run(a, b, args.warmup, args.iters, args.repeats, args.baseline_iters, args.probe,
                  args.cpu and int(np.prod(b)) <= args.cpu_max_voxels)
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
