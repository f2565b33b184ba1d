#!/usr/bin/env python3
"""Times the alignment kernels (include/naf_hip.h A1) with device events: `align.shift_scores`, `align.peak` and
`align.shift_views` on N views of H x W with a window of R pixels, the same score table composed from torch ops (one slice,
subtraction, square and sum per shift), and one whole outer iteration of `reconstruct.align_projections` on a phantom scan of the
same views (SIRT), so that the kernels' share of it is on record.  Each figure is the median over `--windows` windows of `--reps`
back-to-back calls after a warm-up, with the smallest and largest window beside it.  One JSON line per measurement.

    python tools/align_bench.py                       # 50 x 512^2, R = 8
    python tools/align_bench.py --views 24 --size 128 --shift 4 --volume 64 --out profiles/align_bench.jsonl
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, reps, windows, warmup):
    """Median, minimum and maximum milliseconds per call over `windows` windows of `reps` calls, by device events."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(windows):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(reps):
            fn()
        stop.record()
        stop.synchronize()
        out.append(start.elapsed_time(stop) / reps)
    return {"ms": round(float(np.median(out)), 4), "ms_min": round(min(out), 4), "ms_max": round(max(out), 4), "reps": reps,
            "windows": windows}


def torch_scores(b, p, R):
    """The score table from torch ops: 2 R + 1 squared slices per axis, fp64 sums."""
    N, H, W = b.shape
    pi = p[:, R:H - R, R:W - R]
    out = torch.empty(N, 2 * R + 1, 2 * R + 1, dtype=torch.float64, device=b.device)
    for j in range(2 * R + 1):
        for i in range(2 * R + 1):
            d = b[:, j:j + H - 2 * R, i:i + W - 2 * R] - pi
            out[:, j, i] = (d.double() ** 2).sum((1, 2))
    return out


def main(argv=None):
    from neuralvolumetricreconstructionformedicalimages_amd import align, phantom, projector, reconstruct
    from neuralvolumetricreconstructionformedicalimages_amd.geometry import ConeGeometry
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--views", type=int, default=50)
    ap.add_argument("--size", type=int, default=512, help="detector H = W")
    ap.add_argument("--shift", type=int, default=8, help="R on both axes")
    ap.add_argument("--volume", type=int, default=256, help="voxels per axis of the outer iteration's volume")
    ap.add_argument("--iters", type=int, default=20, help="SIRT iterations of the outer iteration")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="append the JSON lines here")
    args = ap.parse_args(argv)
    N, H, R = args.views, args.size, args.shift
    data = phantom.scan_geometry(args.volume)
    data["nDetector"], data["dDetector"] = [H, H], [0.8 * 512.0 / H] * 2
    geo = ConeGeometry(data)
    angles = np.linspace(0, np.pi, N, endpoint=False)
    volume = phantom.volume(geo, phantom.ellipsoid_table(seed=0, extent=float(geo.sVoxel[0]) / 2), device="cuda")
    p = projector.project_scan(volume, geo, angles)
    gen = torch.Generator(device="cuda").manual_seed(0)
    shifts = (torch.rand(N, 2, device="cuda", generator=gen) - 0.5) * 5.0
    b = align.shift_views(p, -shifts)
    ws = align.scores_workspace(N, H, H, R, "cuda")
    scores = align.shift_scores(b, p, R, workspace=ws)
    rel = float(((scores - torch_scores(b, p, R)).abs() / scores).max())
    head = {"views": N, "detector": [H, H], "R": R, "device": torch.cuda.get_device_name(0)}
    lines = [
        {"what": "shift_scores", **timed(lambda: align.shift_scores(b, p, R, workspace=ws, out=scores), args.reps, args.windows, args.warmup),
         "workspace_mib": round(ws.numel() * 8 / 2 ** 20, 1), "largest_relative_difference_to_torch": rel},
        {"what": "peak", **timed(lambda: align.peak(scores), args.reps, args.windows, args.warmup)},
        {"what": "shift_views", **timed(lambda: align.shift_views(b, shifts), args.reps, args.windows, args.warmup)},
        {"what": "torch_scores", **timed(lambda: torch_scores(b, p, R), 1, args.windows, 1)},
        {"what": "project_scan", "volume": args.volume, **timed(lambda: projector.project_scan(volume, geo, angles), 2, args.windows, 1)},
        {"what": "outer_iteration", "solver": "sirt", "iters": args.iters, "volume": args.volume,
         **timed(lambda: reconstruct.align_projections(b, geo, angles, n_outer=1, max_shift=R, n_iter=args.iters), 1, args.windows, 1)},
    ]
    for line in lines:
        text = json.dumps({**line, **head})
        print(text, flush=True)
        if args.out:
            with open(args.out, "a") as handle:
                handle.write(text + "\n")


if __name__ == "__main__":
    main()
