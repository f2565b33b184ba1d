#!/usr/bin/env python3
"""3-D SSIM benchmark: metrics.ssim_3d (naf_ssim_3d) at 256^3 (chest), 512^3 and 1024^3 (foot), against the same definition
written in torch fp64 on the GPU (avg_pool3d of the five moments, kernel_size 7, stride 1).

    python tools/ssim_bench.py                      # one JSON line per size
    python tools/ssim_bench.py --sizes 256 --cpu    # + the float64 numpy / scipy restatement on the host

Reported per size: the kernel time (device events around `--iters` calls after warm-up, median of `--repeats` windows), the
whole `ssim_3d` call from the host (workspace allocation and the device-to-host read of the scalar included: what one
evaluation pays), the algorithmic bytes 2 x 4 x n^3 and their rate, the torch fp64 baseline where its ~20 full-size fp64
arrays fit in memory, and the largest difference between the two values.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def torch_ssim(x, y):
    """The definition (include/naf_hip.h, M1) in torch fp64: box means by avg_pool3d, mean of S over the interior windows."""
    import torch.nn.functional as F
    x, y = x.double()[None, None], y.double()[None, None]
    u = [F.avg_pool3d(t, kernel_size=7, stride=1) for t in (x, y, x * x, y * y, x * y)]
    cov_norm, C1, C2 = 343.0 / 342.0, (0.01 * 2) ** 2, (0.03 * 2) ** 2
    ux, uy, uxx, uyy, uxy = u
    vx, vy, vxy = cov_norm * (uxx - ux * ux), cov_norm * (uyy - uy * uy), cov_norm * (uxy - ux * uy)
    S = ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux * ux + uy * uy + C1) * (vx + vy + C2))
    return float(S.mean())


def cpu_ssim(x, y):
    """The float64 numpy / scipy restatement (uniform_filter, the formulation scikit-image uses), as a host evaluation pays it."""
    import numpy as np
    from scipy.ndimage import uniform_filter
    a, b = x.astype(np.float64), y.astype(np.float64)
    u = [uniform_filter(t, size=7) for t in (a, b, a * a, b * b, a * b)]
    cov_norm, C1, C2 = 343.0 / 342.0, (0.01 * 2) ** 2, (0.03 * 2) ** 2
    ux, uy, uxx, uyy, uxy = u
    vx, vy, vxy = cov_norm * (uxx - ux * ux), cov_norm * (uyy - uy * uy), cov_norm * (uxy - ux * uy)
    S = ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux * ux + uy * uy + C1) * (vx + vy + C2))
    return float(S[3:-3, 3:-3, 3:-3].mean())


def _events(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def volumes(n, seed=0):
    """A phantom-like pair: smooth random field x and a noisy copy y (fp32, on the device)."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.rand((n, n, n), device="cuda", generator=g)
    y = x + 0.05 * torch.randn((n, n, n), device="cuda", generator=g)
    return x, y


def run(n, warmup, iters, repeats, baseline_iters, cpu):
    from neuralvolumetricreconstructionformedicalimages_amd import _abi
    from neuralvolumetricreconstructionformedicalimages_amd.metrics import ssim_3d
    x, y = volumes(n)
    lib = _abi.lib()
    ws = torch.empty(lib.naf_ssim_3d_workspace_bytes(n, n, n), dtype=torch.uint8, device="cuda")
    out = torch.empty(1, dtype=torch.float64, device="cuda")

    def kernel():
        _abi.check(lib.naf_ssim_3d(_abi.ptr(x), _abi.ptr(y), n, n, n, _abi.ptr(out), _abi.ptr(ws), ws.numel(), _abi.stream_ptr()))

    for _ in range(warmup):
        kernel()
    torch.cuda.synchronize()
    ms = statistics.median(_events(kernel, iters) for _ in range(repeats))
    value = ssim_3d(x, y)
    calls = []
    for _ in range(max(3, repeats)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ssim_3d(x, y)
        calls.append((time.perf_counter() - t0) * 1e3)
    algo = 2 * 4 * n ** 3
    res = {"n": n, "ssim": value, "kernel_ms": round(ms, 4), "call_ms": round(statistics.median(calls), 4),
           "algorithmic_bytes": algo, "algorithmic_GB_per_s": round(algo / ms * 1e-6, 1),
           "windows_per_s": (n - 6) ** 3 / ms * 1e3}
    try:
        ref = torch_ssim(x, y)
        torch.cuda.synchronize()
        bms = statistics.median(_events(lambda: torch_ssim(x, y), 1) for _ in range(baseline_iters))
        res.update(torch_fp64_ms=round(bms, 3), speedup_vs_torch_fp64=round(bms / ms, 1), abs_diff_vs_torch_fp64=abs(ref - value))
    except torch.cuda.OutOfMemoryError:
        res.update(torch_fp64_ms=None, torch_fp64_note="out of device memory")
    torch.cuda.empty_cache()
    if cpu:
        xh, yh = x.cpu().numpy(), y.cpu().numpy()
        t0 = time.perf_counter()
        ref = cpu_ssim(xh, yh)
        res.update(cpu_fp64_s=round(time.perf_counter() - t0, 2), abs_diff_vs_cpu=abs(ref - value))
    del x, y
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="256,512,1024")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--baseline-iters", type=int, default=2)
    ap.add_argument("--cpu", action="store_true", help="also time the float64 numpy / scipy restatement (256^3 only)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ssim_bench.py needs an MI355X: naf_ssim_3d has no CPU path")
    for n in (int(s) for s in args.sizes.split(",")):
        res = run(n, args.warmup, args.iters, args.repeats, args.baseline_iters, args.cpu and n <= 256)
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
