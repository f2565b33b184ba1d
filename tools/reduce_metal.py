#!/usr/bin/env python3
"""Reduces the metal artefacts of a scan in the pickle schema train.py reads (reconstruct.reduce_metal, DESIGN.md section 32: a first
FDK reconstruction, the voxels above a threshold taken as metal, their trace on the detector in-painted along the rows) and writes
the same schema with the corrected views in place.  `train` and, when present, `val` are corrected separately, `val` with the metal
voxels found on `train`; the trace, the threshold, the method and the counts are stored beside the views as `metal_trace` (uint8),
`metal_threshold`, `metal_method` and `metal_counts`.  train.py trains on the output with no change to the trainer.

    python tools/reduce_metal.py --scan data/jaw_metal.pickle --out data/jaw_mar.pickle --threshold 2.0
    python tools/reduce_metal.py --scan in.pickle --out out.pickle --threshold 2.0 --method nmar --air 0.05 --bone 0.4

`--threshold` has no default: it is a property of the scan's units.  `--method nmar` interpolates the sinogram normalised by the
projection of a prior (air below `--air`, one tissue level up to `--bone`, bone kept) and needs both.  `--grow` widens the trace by
that many detector pixels (default 1).  Prints one JSON line; when the pickle carries a ground-truth volume (`image`), it has
psnr_3d / ssim_3d of an FDK volume of the training views before and after, both with the ground truth's metal voxels (`image` above
the threshold, grown by one voxel) set to zero in the volume and in the truth, so that the score measures the streaks and not the
metal.
"""
import argparse
import json
import os
import pickle
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None):
    from neuralvolumetricreconstructionformedicalimages_amd import fdk, metal, metrics, reduce_metal
    from neuralvolumetricreconstructionformedicalimages_amd.geometry import ConeGeometry
    from neuralvolumetricreconstructionformedicalimages_amd.utils import get_psnr_3d
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scan", required=True)
    ap.add_argument("--out", required=True)
    ap.add_argument("--threshold", type=float, required=True, help="voxels of the first reconstruction above it are metal")
    ap.add_argument("--method", choices=["li", "nmar"], default="li")
    ap.add_argument("--air", type=float, default=None)
    ap.add_argument("--bone", type=float, default=None)
    ap.add_argument("--grow", type=int, default=1, help="widen the trace by this many detector pixels")
    ap.add_argument("--projector", choices=["interpolated", "siddon"], default="interpolated")
    ap.add_argument("--device", default="cuda")
    args = ap.parse_args(argv)
    if args.method == "nmar" and (args.air is None or args.bone is None):
        ap.error("--method nmar needs --air and --bone")
    with open(args.scan, "rb") as handle:
        data = pickle.load(handle)
    geo = ConeGeometry(data)
    image = data.get("image")
    train_angles = np.asarray(data["train"]["angles"], dtype=np.float64)

    def score(proj):
        x = fdk(proj, geo, train_angles)
        truth = torch.tensor(np.asarray(image, dtype=np.float32), device=x.device)
        hole = torch.nn.functional.max_pool3d((truth > args.threshold).float()[None, None], 3, stride=1, padding=1)[0, 0] > 0
        x, truth = metal.insert_metal(x, hole, 0.0), metal.insert_metal(truth, hole, 0.0)
        return {"psnr_3d": float(get_psnr_3d(x.cpu().numpy(), truth.cpu().numpy())), "ssim_3d": float(metrics.ssim_3d(x, truth))}

    out = dict(data)
    res = {"scan": os.path.basename(args.scan), "method": args.method, "threshold": args.threshold}
    seconds, initial = 0.0, None
    for split in ("train", "val"):
        if split not in data or data[split] is None or len(data[split]["projections"]) == 0:
            continue
        proj = torch.tensor(np.ascontiguousarray(data[split]["projections"], dtype=np.float32), device=args.device)
        angles = np.asarray(data[split]["angles"], dtype=np.float64)
        torch.cuda.synchronize()
        start = time.perf_counter()
        corrected, info = reduce_metal(proj, geo, angles, args.threshold, method=args.method, air=args.air, bone=args.bone, grow=args.grow,
                                       initial=initial, kind=args.projector)
        torch.cuda.synchronize()
        seconds += time.perf_counter() - start
        initial = info["initial"]                              # the validation views take the metal found on the training views
        counts = info["counts"].cpu().numpy()
        out[split] = dict(data[split], projections=corrected.cpu().numpy(), metal_trace=info["trace"].cpu().numpy(),
                          metal_threshold=args.threshold, metal_method=args.method, metal_counts=counts)
        res[split] = {"views": int(proj.shape[0]), "metal_voxels": int(info["metal"].sum()), "replaced": int(counts[:, 0].sum()),
                      "left": int(counts[:, 1].sum()), "trace": float(info["trace"].float().mean())}
        if split == "train" and image is not None:
            res["before"], res["after"] = score(proj), score(corrected)
    res["seconds"] = round(seconds, 4)
    with open(args.out, "wb") as handle:
        pickle.dump(out, handle, pickle.HIGHEST_PROTOCOL)
    print(json.dumps(res), flush=True)
    return res


if __name__ == "__main__":
    main()
