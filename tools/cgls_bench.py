#!/usr/bin/env python3
"""CGLS benchmark at the chest shape (50 views of 512 x 512, a 256^3 volume): the vector launches of one iteration through
naf_cgls_wdot / naf_cgls_residual_step / naf_cgls_direction_step next to the same iteration written in torch ops with `.item()`
scalars, on the same device in the same process, and one whole iteration including the projector pair, so that the share of the
vector part is on record.  The projector pair is the expensive part and these kernels do not change it.

    python tools/cgls_bench.py
    python tools/cgls_bench.py --views 50 --detector 512 --volume 256 --iters 20

Reported: device-event time per iteration (median of `--windows` windows of `--iters` iterations after warm-up) of the vector part
alone for both forms, the bytes it must move (projection space: wdot reads q and w, the residual step reads r, q, w and writes r,
y; volume space: wdot reads s, the direction step reads x, p, s and writes x, p) and the GB/s that makes, and the time of a whole
iteration with A and A^T.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _time(fn, warmup, iters, windows):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / iters)
    return statistics.median(out), min(out), max(out)


def _geometry(views, det, vol):
    from neuralvolumetricreconstructionformedicalimages_amd.geometry import ConeGeometry
    data = {"DSD": 1500.0, "DSO": 1000.0, "nDetector": [det, det], "dDetector": [460.8 / det] * 2, "nVoxel": [vol] * 3,
            "dVoxel": [256.0 / vol] * 3, "offOrigin": [0, 0, 0], "offDetector": [0, 0], "accuracy": 0.5, "mode": "cone",
            "filter": None}
    return ConeGeometry(data), np.linspace(0, np.pi, views + 1)[:-1]


def run(views, det, vol, warmup, iters, windows, whole_iters):
    from neuralvolumetricreconstructionformedicalimages_amd import cgls, cgls_kernels as K, projector
    gen = torch.Generator(device="cuda").manual_seed(0)
    proj_shape, vol_shape = (views, det, det), (vol, vol, vol)

    def rand(shape):
        return torch.rand(shape, device="cuda", generator=gen)

    # delta ~ 4e6 and gamma = 1 give alpha ~ 3e-7, and s ~ 1e-20 gives beta ~ 1e-33: every array stays finite over thousands of
    # repetitions, while the kernels do the same loads, fmas and stores as in a solve
    r, q, w, y = rand(proj_shape), rand(proj_shape), 0.5 + 0.5 * rand(proj_shape), torch.empty(proj_shape, device="cuda")
    x, p, s = rand(vol_shape), rand(vol_shape), 1e-20 * rand(vol_shape)
    n_proj, n_vol = r.numel(), x.numel()
    ws = K.Workspace(max(n_proj, n_vol), 2, "cuda")
    ws.scalars[K.SLOT_GAMMA[0]] = 1.0

    def hip_vector():
        K.wdot(q, w, K.SLOT_DELTA, ws)
        K.residual_step(r, q, w, y, 0, ws)
        K.wdot(s, None, K.SLOT_GAMMA[1], ws)
        K.direction_step(x, p, s, 0, ws)

    def torch_vector():
        # the composition a solver without the kernels runs: fp64 sums, two host read-backs, alpha and beta as Python floats
        gamma = 1.0
        delta = float((w.double() * q.double() * q.double()).sum().item())
        norm2 = (w.double() * r.double() * r.double()).sum()             # the history entry, left on the device
        alpha = gamma / delta
        r.add_(q, alpha=-alpha)
        torch.mul(w, r, out=y)
        beta = float((s.double() * s.double()).sum().item()) / gamma
        x.add_(p, alpha=alpha)
        p.mul_(beta).add_(s)
        return norm2

    t_hip = _time(hip_vector, warmup, iters, windows)
    assert ws.stopped_at() is None
    t_ops = _time(torch_vector, warmup, iters, windows)
    assert bool(torch.isfinite(x).all()) and bool(torch.isfinite(r).all())
    del r, q, y, s, p

    # a whole iteration, projector pair included: the difference of two solves of different length through reconstruct.cgls
    geo, angles = _geometry(views, det, vol)
    b = projector.project_scan(x, geo, angles)

    def solve(n_iter):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        cgls(b, geo, angles, n_iter=n_iter, weights=w)
        stop.record()
        stop.synchronize()
        return start.elapsed_time(stop)

    solve(1)
    per = sorted((solve(2 + whole_iters) - solve(2)) / whole_iters for _ in range(3))
    t_whole = (per[1], per[0], per[2])
    bytes_vector = 4 * (n_proj * (2 + 5) + n_vol * (1 + 5))
    return {"views": views, "detector": [det, det], "volume": [vol] * 3,
            "hip_vector_ms_per_iteration": round(t_hip[0], 4), "hip_vector_ms_min_max": [round(t_hip[1], 4), round(t_hip[2], 4)],
            "torch_vector_ms_per_iteration": round(t_ops[0], 4), "torch_vector_ms_min_max": [round(t_ops[1], 4), round(t_ops[2], 4)],
            "speedup_vector_part": round(t_ops[0] / t_hip[0], 2), "vector_bytes_per_iteration": bytes_vector,
            "hip_vector_GB_per_s": round(bytes_vector / t_hip[0] * 1e-6, 1),
            "whole_iteration_ms": round(t_whole[0], 2), "whole_iteration_ms_min_max": [round(t_whole[1], 2), round(t_whole[2], 2)],
            "vector_share_of_iteration": round(t_hip[0] / t_whole[0], 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=50)
    ap.add_argument("--detector", type=int, default=512)
    ap.add_argument("--volume", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--whole-iters", type=int, default=3)
    args = ap.parse_args()
    print(json.dumps(run(args.views, args.detector, args.volume, args.warmup, args.iters, args.windows, args.whole_iters)), flush=True)


if __name__ == "__main__":
    main()
