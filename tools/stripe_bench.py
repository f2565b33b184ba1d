#!/usr/bin/env python3
"""Times sinogram stripe removal (include/naf_hip.h A2) at 50 x 512^2 and 720 x 512 x 512: the whole call of
`stripe.remove_stripes` with device events, its two kernels through the library's per-kernel events (naf_profile_enable), and the
same operation composed from torch ops in the same process (`torch.sort` along the views, `unfold` of the reflect-padded sorted
sinogram, `median` of the windows, `scatter_` back to the views).  Each event figure is the median over `--windows` windows of
`--reps` back-to-back calls after a warm-up, with the smallest and largest window beside it.  One JSON line per measurement.

The traffic floor: per element the sort kernel reads 4 bytes of p and writes 4 of s and 2 of perm, and the median kernel reads 4 of
s and 2 of perm and writes 4 of out: 20 bytes, plus the halo, 2 h floats re-read per run of min(256, W) columns.  `floor_ms` is that
byte count at `--tbps` (default 8.0, the HBM3E peak of the MI355X) and `ratio_to_floor` the measured time over it.  No time here is a
pass condition.

    python tools/stripe_bench.py
    python tools/stripe_bench.py --shapes 50x512x512 --size 11 --out profiles/stripe_bench.jsonl
"""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

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


def torch_remove_stripes(p, size):
    """The same operation from torch ops.  Its sort compares floats, so its bits differ from the kernels' where -0 or NaNs occur."""
    h = size // 2
    s, perm = torch.sort(p, dim=0, stable=True)
    padded = torch.cat([s[..., :h].flip(-1), s, s[..., -h:].flip(-1)], dim=-1)
    m = padded.unfold(-1, size, 1).median(dim=-1).values
    return torch.empty_like(p).scatter_(0, perm, m)


def traffic_bytes(N, H, W, size):
    run = min(256, W)
    return N * H * W * (20.0 + 4.0 * (size - 1) / run)


def main(argv=None):
    from neuralvolumetricreconstructionformedicalimages_amd import _abi, stripe
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", default="50x512x512,720x512x512", help="comma-separated NxHxW")
    ap.add_argument("--size", type=int, default=None, help="median window (default: stripe.default_size(W))")
    ap.add_argument("--tbps", type=float, default=8.0, help="the memory rate of the traffic floor in TB/s")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-torch", action="store_true", help="skip the torch composition")
    ap.add_argument("--out", default=None, help="append the JSON lines here")
    args = ap.parse_args(argv)
    lines = []
    for shape in args.shapes.split(","):
        N, H, W = (int(v) for v in shape.split("x"))
        size = stripe.default_size(W) if args.size is None else args.size
        gen = torch.Generator(device="cuda").manual_seed(0)
        p = torch.rand(N, H, W, device="cuda", generator=gen)
        out = torch.empty_like(p)
        floor_ms = traffic_bytes(N, H, W, size) / (args.tbps * 1e12) * 1e3
        head = {"shape": [N, H, W], "size": size, "floor_ms": round(floor_ms, 4), "tbps": args.tbps,
                "device": torch.cuda.get_device_name(0)}
        whole = timed(lambda: stripe.remove_stripes(p, size=size, out=out), args.reps, args.windows, args.warmup)
        lines.append({"what": "remove_stripes", **whole, "ratio_to_floor": round(whole["ms"] / floor_ms, 2), **head})
        _abi.profile_enable(True)
        calls = args.reps * args.windows
        for _ in range(calls):
            stripe.remove_stripes(p, size=size, out=out)
        torch.cuda.synchronize()
        kernels = _abi.profile_collect()
        _abi.profile_enable(False)
        for name in ("stripe_sort_kernel", "stripe_median_kernel"):
            launches, ms = kernels[name]
            lines.append({"what": name, "ms": round(ms / calls, 4), "launches_per_call": launches / calls, "calls": calls, **head})
        if not args.no_torch:
            got = torch_remove_stripes(p, size)
            equal = bool(torch.equal(got.view(torch.int32), out.view(torch.int32)))
            del got
            composed = timed(lambda: torch_remove_stripes(p, size), 1, args.windows, 1)
            lines.append({"what": "torch_sort_unfold_median_scatter", **composed, "equal_bits_on_this_input": equal,
                          "ratio_to_remove_stripes": round(composed["ms"] / whole["ms"], 2), **head})
        del p, out
        torch.cuda.empty_cache()
    for line in lines:
        text = json.dumps(line)
        print(text, flush=True)
        if args.out:
            with open(args.out, "a") as handle:
                handle.write(text + "\n")


if __name__ == "__main__":
    main()
