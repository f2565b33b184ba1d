#!/usr/bin/env python3
"""Forward projector benchmark: naf_project_scan at the chest shape (50 x 512^2 pixels through a 256^3 volume, accuracy 0.5)
and at a 1024^3 volume with a 1024^2 detector, against the same projection written with torch.nn.functional.grid_sample.

    python tools/project_bench.py                      # both shapes, one JSON line each
    python tools/project_bench.py --shape chest --lib lib/ab/rows.so     # an A/B variant of libnaf_hip.so
    python tools/project_bench.py --siddon             # the Siddon scan kernel next to the interpolated one, same run

Reported: device-event time after warm-up, rays/s, samples/s (the exact count of the step-count formula, computed on the
host in float32 like the kernel) and ALGORITHMIC gather bytes/s (8 corners x 4 B per sample: the caches serve most of them,
so this can exceed the HBM peak).  The grid_sample baseline (3-D, align_corners=True, padding_mode="border", points in
chunks) runs on the first `--baseline-views` views; its speed-up is the ratio of the two samples/s rates on those views.
"""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def segments(rays, dims, dvoxel, step):
    """float32 (t0, t1, len, n) of the projector's definition for rays [n, 8] (torch, any device); n = 0 for a miss."""
    o, d = rays[:, 0:3], rays[:, 3:6]
    t0, t1 = rays[:, 6].clone(), rays[:, 7].clone()
    half = [float(np.float32(float(n) * float(np.float32(dv)) / 2.0)) for n, dv in zip(dims, dvoxel)]
    for k in range(3):
        ok, dk = o[:, k], d[:, k]
        flat = dk == 0
        ta, tb = (-half[k] - ok) / dk, (half[k] - ok) / dk
        lo, hi = torch.minimum(ta, tb), torch.maximum(ta, tb)
        t0 = torch.where(~flat & (lo > t0), lo, t0)
        t1 = torch.where(~flat & (hi < t1), hi, t1)
        t1 = torch.where(flat & ((ok < -half[k]) | (ok > half[k])), torch.full_like(t1, -math.inf), t1)
    hit = t1 > t0
    dn = torch.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    length = torch.where(hit, (t1 - t0) * dn, torch.zeros_like(t0))
    n = torch.where(hit, torch.clamp(torch.ceil(length / np.float32(step)), min=1.0), torch.zeros_like(t0))
    return t0, t1, length, n.long()


def grid_sample_projection(volume, dvoxel, rays, accuracy=0.5, max_points=1 << 24):
    """The projection a user would write in PyTorch: sample points of every ray through F.grid_sample (trilinear,
    align_corners=True, border padding = clamp-to-edge), masked sum in chunks of rays -> float32 [n]."""
    import torch.nn.functional as F
    from neuralvolumetricreconstructionformedicalimages_amd.projector import sample_step
    dims = volume.shape
    t0, t1, length, n = segments(rays, dims, dvoxel, sample_step(dvoxel, accuracy))
    out = torch.zeros(rays.shape[0], device=rays.device)
    inp = volume[None, None]                                     # [1, 1, D=n1, H=n2, W=n3]
    d = torch.tensor([float(v) for v in dvoxel], device=rays.device)
    half = torch.tensor([float(a) for a in dims], device=rays.device) * d / 2
    order = torch.argsort(n, descending=True)                   # rays of similar length share a chunk: less padding
    n_host = n[order].cpu().numpy()
    n_hit = int((n_host > 0).sum())                              # rays that miss the box stay 0
    i = 0
    while i < n_hit:
        K = int(n_host[i])
        R = max(1, min(max_points // K, n_hit - i))
        idx = order[i:i + R]
        nk = n[idx].float()
        k = torch.arange(K, device=rays.device, dtype=torch.float32)[None, :]
        seg = (t1[idx] - t0[idx]) / nk
        o, dr = rays[idx, 0:3].double(), rays[idx, 3:6].double()
        p0 = (o + t0[idx].double()[:, None] * dr).float()       # entry point in float64: the origin is ~1 m away
        p = p0[:, None, :] + ((k + 0.5) * seg[:, None])[..., None] * rays[idx, None, 3:6]
        u = (p + half) / d - 0.5                                # continuous voxel index per axis
        g = u / (torch.tensor([float(a) for a in dims], device=rays.device) - 1).clamp(min=1) * 2 - 1
        grid = g.flip(-1).reshape(1, R, K, 1, 3)               # grid_sample's (x, y, z) index (W, H, D) = our axes (2, 1, 0)
        f = F.grid_sample(inp, grid, mode="bilinear", padding_mode="border", align_corners=True).reshape(R, K)
        f = torch.where(k < nk[:, None], f, torch.zeros_like(f))
        out[idx] = f.sum(1) * (length[idx] / nk)
        i += R
    return out


def _time(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


SHAPES = {
    # name: (n_voxel, detector pixels, views, detector pitch mm, voxel mm)
    "chest": (256, 512, 50, 0.8, 1.0),
    "big": (1024, 1024, 4, 0.4, 0.25),
}


def siddon_steps(rays, dims, dvoxel):
    """Voxel steps of the Siddon walk (naf_hip.h P6) over rays [n, 8]: per hit ray the plane crossings between the voxels of the
    two ends of its clipped segment, plus one.  Counted on the device in float64 (the count the kernel takes, up to rounding)."""
    t0, t1, _, n = segments(rays, dims, dvoxel, 1.0)
    hit = n > 0
    steps = hit.long()
    for a in range(3):
        half = float(dims[a]) * float(dvoxel[a]) / 2
        ends = [((rays[:, a].double() + t.double() * rays[:, 3 + a].double() + half) / float(dvoxel[a])).floor().clamp(0, dims[a] - 1)
                for t in (t0, t1)]
        steps = steps + torch.where(hit, (ends[1] - ends[0]).abs().long(), torch.zeros_like(steps))
    return int(steps.sum())


def run_siddon(shape, warmup, iters, windows):
    """The Siddon and the interpolated scan kernels at one shape, timed in alternating windows of `iters` calls each."""
    from neuralvolumetricreconstructionformedicalimages_amd import phantom, projector
    from neuralvolumetricreconstructionformedicalimages_amd.geometry import ConeGeometry, RayGenerator
    nv, det, views, pitch, vox = SHAPES[shape]
    data = phantom.scan_geometry(256)
    data.update(nVoxel=[nv] * 3, dVoxel=[vox] * 3, nDetector=[det, det], dDetector=[pitch, pitch])
    geo = ConeGeometry(data)
    table = phantom.ellipsoid_table(seed=0, extent=float(geo.sVoxel[0]) / 2)
    volume = phantom.volume(geo, table, device="cuda", slab=max(1, (1 << 22) // (nv * nv)))
    angles = np.linspace(0, np.pi, views + 1)[:-1]
    calls = {kind: (lambda kind=kind: projector.project_scan(volume, geo, angles, kind=kind)) for kind in projector.KINDS}
    times = {kind: [] for kind in calls}
    for kind, fn in calls.items():
        _time(fn, warmup, 1)
    for _ in range(windows):
        for kind, fn in calls.items():
            times[kind].append(_time(fn, 0, iters))
    raygen = RayGenerator(geo, angles, "cuda")
    step = projector.sample_step(geo.dVoxel, geo.accuracy)
    samples = steps = 0
    for i in range(views):
        r = raygen.rays_for_projection(i)
        samples += int(segments(r, volume.shape, geo.dVoxel, step)[3].sum())
        steps += siddon_steps(r, volume.shape, geo.dVoxel)
    a, b = calls["siddon"](), calls["interpolated"]()
    res = {"shape": shape, "volume": [nv] * 3, "detector": [det, det], "views": views, "windows": windows, "calls_per_window": iters}
    for kind, work, bytes_per in (("siddon", steps, 4), ("interpolated", samples, 32)):
        t = sorted(times[kind])
        ms = t[len(t) // 2]
        res[kind] = {"median_ms": round(ms, 4), "min_ms": round(t[0], 4), "max_ms": round(t[-1], 4),
                     "steps" if kind == "siddon" else "samples": work, "per_s": work / ms * 1e3,
                     "algorithmic_gather_GB_per_s": work * bytes_per / ms * 1e-6}
    res["siddon_over_interpolated_time"] = round(res["siddon"]["median_ms"] / res["interpolated"]["median_ms"], 3)
    res["rel_l2_siddon_vs_interpolated"] = float((a - b).norm() / b.norm())
    return res


def run(shape, warmup, iters, baseline_views, baseline_iters):
    from neuralvolumetricreconstructionformedicalimages_amd import phantom, projector
    from neuralvolumetricreconstructionformedicalimages_amd.geometry import ConeGeometry, RayGenerator
    nv, det, views, pitch, vox = SHAPES[shape]
    data = phantom.scan_geometry(256)
    data.update(nVoxel=[nv] * 3, dVoxel=[vox] * 3, nDetector=[det, det], dDetector=[pitch, pitch])
    geo = ConeGeometry(data)
    table = phantom.ellipsoid_table(seed=0, extent=float(geo.sVoxel[0]) / 2)
    volume = phantom.volume(geo, table, device="cuda", slab=max(1, (1 << 22) // (nv * nv)))
    angles = np.linspace(0, np.pi, views + 1)[:-1]
    proj = projector.project_scan(volume, geo, angles)
    ms = _time(lambda: projector.project_scan(volume, geo, angles), warmup, iters)
    raygen = RayGenerator(geo, angles, "cuda")
    step = projector.sample_step(geo.dVoxel, geo.accuracy)
    samples = 0
    for i in range(views):
        samples += int(segments(raygen.rays_for_projection(i), volume.shape, geo.dVoxel, step)[3].sum())
    rays = views * det * det
    res = {"shape": shape, "volume": [nv] * 3, "detector": [det, det], "views": views, "accuracy": geo.accuracy,
           "kernel_ms": round(ms, 4), "rays_per_s": rays / ms * 1e3, "samples": samples, "samples_per_s": samples / ms * 1e3,
           "algorithmic_gather_GB_per_s": samples * 32 / ms * 1e-6}
    if baseline_views > 0:
        bv = min(baseline_views, views)
        r = torch.cat([raygen.rays_for_projection(i) for i in range(bv)])
        ref = grid_sample_projection(volume, geo.dVoxel, r, geo.accuracy)
        ours = proj[:bv].reshape(-1)
        bms = _time(lambda: grid_sample_projection(volume, geo.dVoxel, r, geo.accuracy), 1, baseline_iters)
        kms = _time(lambda: projector.project_scan(volume, geo, angles[:bv]), warmup, iters)
        res.update(baseline_views=bv, grid_sample_ms=round(bms, 3), kernel_ms_same_views=round(kms, 4),
                   speedup_vs_grid_sample=round(bms / kms, 1),
                   max_rel_diff_vs_grid_sample=float((ours - ref).abs().max() / ref.abs().max()))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=["chest", "big", "all"], default="all")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--baseline-views", type=int, default=2)
    ap.add_argument("--baseline-iters", type=int, default=2)
    ap.add_argument("--lib", default=None, help="load this libnaf_hip.so instead of the in-tree build (layout A/B)")
    ap.add_argument("--siddon", action="store_true", help="time the Siddon scan kernel next to the interpolated one")
    ap.add_argument("--windows", type=int, default=5, help="timed windows per kernel with --siddon (median and min-max)")
    args = ap.parse_args()
    if args.lib:
        from neuralvolumetricreconstructionformedicalimages_amd import build
        build.LIB_PATH = os.path.abspath(args.lib)
    for shape in (["chest", "big"] if args.shape == "all" else [args.shape]):
        if args.siddon:
            res = run_siddon(shape, args.warmup, args.iters, args.windows)
        else:
            res = run(shape, args.warmup, args.iters, args.baseline_views, args.baseline_iters)
        if args.lib:
            res["lib"] = os.path.basename(args.lib)
        print(json.dumps(res), flush=True)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
