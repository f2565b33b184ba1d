#!/usr/bin/env python3
"""TV-prox benchmark: one dual iteration of naf_tv_prox_step at 256^3 next to the same iteration written in torch ops, on the
same device in the same process.

    python tools/tvprox_bench.py
    python tools/tvprox_bench.py --size 256 512 --iters 20

Reported: device-event time of one iteration (median of `--windows` windows of `--iters` iterations after warm-up), the achieved
GB/s against the 52 bytes per voxel an iteration must move (seven arrays read: b, three planes of r, three of p; six written: three
of p, three of r_next), and the largest difference of the two results after one iteration.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

BYTES_PER_VOXEL = 4 * (7 + 6)


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


def _diff(f, a):
    """D_a f: f[v] - f[v - e_a], 0 at v_a = 0."""
    d = torch.zeros_like(f)
    n = f.shape[a]
    if n > 1:
        d.narrow(a, 1, n - 1).copy_(f.narrow(a, 1, n - 1) - f.narrow(a, 0, n - 1))
    return d


def torch_step(b, r, p, lam, momentum, nonneg):
    """The iteration of include/naf_hip.h V3 in elementwise torch ops (fp32); the inert planes of r and p are taken to be 0."""
    dt = torch.zeros_like(b)
    for a in range(3):
        n = b.shape[a]
        dt += r[a]
        if n > 1:
            dt.narrow(a, 0, n - 1).sub_(r[a].narrow(a, 1, n - 1))
    u = b - lam * dt
    if nonneg:
        u = torch.where(u < 0, torch.zeros_like(u), u)
    q = torch.stack([r[a] + (1.0 / (12.0 * lam)) * _diff(u, a) for a in range(3)])
    p_new = q / torch.clamp(torch.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2]), min=1.0)
    return p_new, p_new + momentum * (p_new - p)


def run(n, warmup, iters, windows, lam, momentum):
    from neuralvolumetricreconstructionformedicalimages_amd import _abi
    gen = torch.Generator(device="cuda").manual_seed(0)
    b = torch.rand((n, n, n), device="cuda", generator=gen)
    r = 2 * torch.rand((3, n, n, n), device="cuda", generator=gen) - 1
    p = 2 * torch.rand((3, n, n, n), device="cuda", generator=gen) - 1
    for t in (r, p):
        t[0][0], t[1][:, 0], t[2][:, :, 0] = 0, 0, 0
    lib = _abi.lib()
    dims = (n, n, n)

    def launch(r_in, p_io, r_out):
        _abi.check(lib.naf_tv_prox_step(_abi.ptr(b), _abi.ptr(r_in), _abi.ptr(p_io), _abi.ptr(r_out), *dims, lam, momentum, 1,
                                        _abi.stream_ptr()), "tv_prox_step")

    p_hip, r_hip = p.clone(), torch.empty_like(r)
    launch(r, p_hip, r_hip)
    want_p, want_r = torch_step(b, r, p, lam, momentum, True)
    mismatch = max(float((p_hip - want_p).abs().max()), float((r_hip - want_r).abs().max()))
    del want_p, want_r
    # the timed call: the library entry on preallocated buffers that alternate, as tv.tv_prox queues it
    state = {"r": r.clone(), "r_next": r_hip}

    def hip():
        launch(state["r"], p_hip, state["r_next"])
        state["r"], state["r_next"] = state["r_next"], state["r"]

    ops_state = {"r": r.clone(), "p": p.clone()}

    def ops():
        ops_state["p"], ops_state["r"] = torch_step(b, ops_state["r"], ops_state["p"], lam, momentum, True)

    t_hip = _time(hip, warmup, iters, windows)
    t_ops = _time(ops, warmup, iters, windows)
    return {"volume": [n] * 3, "lam": lam, "momentum": momentum,
            "hip_ms_per_iteration": round(t_hip[0], 4), "hip_ms_min_max": [round(t_hip[1], 4), round(t_hip[2], 4)],
            "torch_ms_per_iteration": round(t_ops[0], 4), "torch_ms_min_max": [round(t_ops[1], 4), round(t_ops[2], 4)],
            "speedup": round(t_ops[0] / t_hip[0], 2), "bytes_per_voxel_iteration": BYTES_PER_VOXEL,
            "hip_GB_per_s": round(BYTES_PER_VOXEL * n ** 3 / t_hip[0] * 1e-6, 1),
            "torch_GB_per_s_same_bytes": round(BYTES_PER_VOXEL * n ** 3 / t_ops[0] * 1e-6, 1),
            "one_iteration_max_abs_difference": mismatch}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, nargs="*", default=[256])
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--lam", type=float, default=0.1)
    ap.add_argument("--momentum", type=float, default=0.8)
    args = ap.parse_args()
    for n in args.size:
        print(json.dumps(run(n, args.warmup, args.iters, args.windows, args.lam, args.momentum)), flush=True)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
