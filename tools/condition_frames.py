#!/usr/bin/env python3
"""Turns the raw detector frames of a scan pickle into the line integrals train.py and the reconstruction tools read
(frames.condition, DESIGN.md section 29: flat-field, zinger and dead-pixel median, -log) and writes the same schema with
`projections` filled in for `train` and, when present, `val`.  It reads `<split>["frames"]` (float32 or uint16 [N, H, W]) and the
top-level `flat`, `dark` and optional `bad_pixels` ([H, W]), as tools/make_synthetic_scan.py --raw-frames writes them; the parameters
are stored as `frames_params` and the per-view counts of replaced outliers and bad pixels as `<split>["frames_counts"]` ([N, 2]).

    python tools/condition_frames.py --scan data/chest_50_raw.pickle --out data/chest_50.pickle --dif 0.1
    python tools/condition_frames.py --scan in.pickle --out out.pickle --size 5 --dif 0.05 --t-min 1e-4

`--size` is 3, 5 or 7 (default 3).  `--dif` is how far above its window's median a transmission must lie to be replaced; it has no
default, because the noise of the detector sets it.  `--t-min` floors the transmission under the logarithm (default: 1 /
dataset.NOISE_I0).  Prints one JSON line.  When the pickle carries a ground-truth volume (`image`) and the scan is one reconstruct.fdk
accepts, the line has psnr_3d / ssim_3d of an FDK volume of the training views conditioned three ways: `unrepaired` (dif at the largest
float, so no outlier is replaced; pixels that are bad by flat <= dark still are, they have no transmission), `repaired`, and
`defect_free` (the frames and flat stored before the defects were planted, `train["frames_clean"]` and `flat_clean`, when present).
"""
import argparse
import json
import os
import pickle
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

LARGEST = float(np.finfo(np.float32).max)


def _frames_tensor(a, device):
    a = np.ascontiguousarray(a)
    if a.dtype != np.uint16:
        a = a.astype(np.float32)
    return torch.from_numpy(a).to(device)


def main(argv=None):
    from neuralvolumetricreconstructionformedicalimages_amd import fdk, frames, metrics
    from neuralvolumetricreconstructionformedicalimages_amd.geometry import ConeGeometry
    from neuralvolumetricreconstructionformedicalimages_amd.utils import get_psnr_3d
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scan", required=True)
    ap.add_argument("--out", required=True)
    ap.add_argument("--size", type=int, default=3, help="the median window: 3, 5 or 7")
    ap.add_argument("--dif", type=float, required=True, help="replace a transmission more than this above its window's median")
    ap.add_argument("--t-min", type=float, default=frames.DEFAULT_T_MIN, help="the floor of the transmission under the logarithm")
    ap.add_argument("--device", default="cuda")
    args = ap.parse_args(argv)
    with open(args.scan, "rb") as handle:
        data = pickle.load(handle)
    for name in ("flat", "dark"):
        if data.get(name) is None:
            raise SystemExit(f"{args.scan}: no `{name}` frame (tools/make_synthetic_scan.py --raw-frames writes one)")
    as_frame = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(args.device)      # noqa: E731
    flat, dark = as_frame(data["flat"]), as_frame(data["dark"])
    bad = data.get("bad_pixels")
    if bad is not None:
        bad = torch.from_numpy(np.ascontiguousarray(np.asarray(bad) != 0)).to(args.device)
    image = data.get("image")

    def score(proj):
        try:
            x = fdk(proj, ConeGeometry(data), np.asarray(data["train"]["angles"], dtype=np.float64))
        except ValueError as refusal:                   # not a scan FDK reconstructs (a tilted axis, a short arc it refuses)
            return {"fdk": str(refusal)}
        truth = np.asarray(image, dtype=np.float32)
        return {"psnr_3d": float(get_psnr_3d(x.cpu().numpy(), truth)),
                "ssim_3d": float(metrics.ssim_3d(x, torch.tensor(truth, device=x.device)))}

    out = dict(data)
    out["frames_params"] = {"size": args.size, "dif": args.dif, "t_min": args.t_min}
    res = {"scan": os.path.basename(args.scan), **out["frames_params"]}
    for split in ("train", "val"):
        if split not in data or data[split] is None or data[split].get("frames") is None or len(data[split]["frames"]) == 0:
            continue
        raw = _frames_tensor(data[split]["frames"], args.device)
        proj, counts = frames.condition(raw, flat, dark, bad=bad, size=args.size, dif=args.dif, t_min=args.t_min, counts=True)
        counts = counts.cpu().numpy()
        out[split] = dict(data[split], projections=proj.cpu().numpy(), frames_counts=counts)
        res[split] = {"views": int(raw.shape[0]), "outliers": int(counts[:, 0].sum()), "bad": int(counts[:, 1].sum())}
        if split == "train" and image is not None:
            res["unrepaired"] = score(frames.condition(raw, flat, dark, size=3, dif=LARGEST, t_min=args.t_min))
            res["repaired"] = score(proj)
            if data[split].get("frames_clean") is not None:
                clean_flat = as_frame(data["flat_clean"]) if data.get("flat_clean") is not None else flat
                clean = frames.condition(_frames_tensor(data[split]["frames_clean"], args.device), clean_flat, dark, size=args.size,
                                         dif=args.dif, t_min=args.t_min)
                res["defect_free"] = score(clean)
    with open(args.out, "wb") as handle:
        pickle.dump(out, handle, pickle.HIGHEST_PROTOCOL)
    print(json.dumps(res), flush=True)
    return res


if __name__ == "__main__":
    main()
