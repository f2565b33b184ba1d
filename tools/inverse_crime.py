#!/usr/bin/env python3
"""How much do the baselines gain from reconstructing with the operator that made the data (the "inverse crime")?

The analytic phantom at 64^3 and 50 views gives three training sets for one voxel volume: its projections by the interpolated
projector (the operator the baselines reconstruct with), by the Siddon projector (another discretisation)
and the phantom's analytic line integrals.  `reconstruct.sirt` (50 iterations), `reconstruct.cgls` (15 iterations) and `reconstruct.os_sart`
(20 iterations, one view per subset) run on each, once on the interpolated pair and once on the Siddon pair (kind="siddon": that
projector and its exact transpose, DESIGN.md sections 21 and 22); printed are psnr_3d and ssim_3d against the voxel volume.  A measurement, not a test.

    python tools/inverse_crime.py [--n 64] [--views 50]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--views", type=int, default=50)
    ap.add_argument("--sirt-iters", type=int, default=50)
    ap.add_argument("--cgls-iters", type=int, default=15)
    ap.add_argument("--sart-iters", type=int, default=20)
    args = ap.parse_args()
    from neuralvolumetricreconstructionformedicalimages_amd import metrics, phantom, projector, reconstruct
    from neuralvolumetricreconstructionformedicalimages_amd.geometry import ConeGeometry, RayGenerator
    from neuralvolumetricreconstructionformedicalimages_amd.utils import get_psnr_3d
    geo = ConeGeometry(phantom.scan_geometry(args.n))
    table = phantom.ellipsoid_table(seed=0, extent=float(geo.sVoxel[0]) / 2)
    volume = phantom.volume(geo, table, device="cuda")
    angles = np.linspace(0, np.pi, args.views + 1)[:-1]
    gen = RayGenerator(geo, angles, "cuda")
    H, W = gen.H, gen.W
    sets = {"interpolated": projector.project_scan(volume, geo, angles),
            "siddon": projector.project_scan(volume, geo, angles, kind="siddon"),
            "analytic": torch.stack([phantom.line_integrals(gen.rays_for_projection(i), table).reshape(H, W)
                                     for i in range(len(angles))]).contiguous()}
    print(f"| data | pair | solver | psnr_3d | ssim_3d |\n|---|---|---|---|---|")
    for kind in projector.KINDS:
        for name, projections in sets.items():
            for solver, run in (("sirt", lambda b: reconstruct.sirt(b, geo, angles, n_iter=args.sirt_iters, kind=kind)),
                                ("cgls", lambda b: reconstruct.cgls(b, geo, angles, n_iter=args.cgls_iters, kind=kind)),
                                ("os_sart", lambda b: reconstruct.os_sart(b, geo, angles, n_iter=args.sart_iters, kind=kind))):
                x = run(projections)
                x = x[0] if isinstance(x, tuple) else x
                row = {"data": name, "pair": kind, "solver": solver, "psnr_3d": float(get_psnr_3d(x, volume)),
                       "ssim_3d": float(metrics.ssim_3d(x, volume))}
                print(f"| {name} | {kind} | {solver} | {row['psnr_3d']:.2f} | {row['ssim_3d']:.4f} |", flush=True)
                print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
