#!/usr/bin/env python3
"""Host check of the gather transpose's enumeration: compiles tools/gather_host_check.cpp (the footprint rectangle, k-range and
corner weight of csrc/backproject_gather_device.h, driven by plain loops over voxels, views and pixels; the kernel of
csrc/backproject_gather.hip, its span table and its launch are not part of it) for the CPU with AddressSanitizer and UBSan and runs
it over the geometries of tests/test_backproject_gather_cpu.py.  For each it asserts that the header's candidate set holds every
(ray, sample, voxel) of a float64 enumeration of the scatter (positions and weights of tests/_backproject_oracle.py, weight != 0)
and of the float32 one, and prints how many pixels and samples a voxel visits.  The program is a stand-alone executable; nothing of
it is loaded into Python.  No GPU.

    python tools/gather_host_check.py
"""
import tempfile

import numpy as np

import host_check


def float64_triples(geo, rays):
    """(ray, sample, flat voxel) of every non-zero float64 weight of the scatter oracle."""
    import _backproject_oracle as B
    import _projector_oracle as O
    dims = tuple(int(v) for v in geo.nVoxel)
    r = np.asarray(rays, dtype=np.float32)
    step = np.float32(geo.accuracy * float(np.min(np.asarray(geo.dVoxel, dtype=np.float64))))
    t0, t1, _, n = O.segments(r, dims, geo.dVoxel, step)
    rr, kk = np.nonzero(np.arange(int(n.max()))[None, :] < n[:, None])
    a, b = t0[rr].astype(np.float64), t1[rr].astype(np.float64)
    t = a + (kk + 0.5) * ((b - a) / n[rr])
    p = r[rr, 0:3].astype(np.float64) + t[:, None] * r[rr, 3:6].astype(np.float64)
    idx, w = B.cell(dims, geo.dVoxel, p)
    out = []
    for c in range(8):
        bits = [(c >> 2) & 1, (c >> 1) & 1, c & 1]
        if any(bit and dims[ax] == 1 for ax, bit in enumerate(bits)):
            continue
        weight = np.prod([w[ax] if bit else 1 - w[ax] for ax, bit in enumerate(bits)], axis=0)
        vox = np.ravel_multi_index([idx[ax] + bit for ax, bit in enumerate(bits)], dims)
        keep = weight != 0
        out.append(np.stack([rr[keep], kk[keep], vox[keep]], 1))
    return np.concatenate(out)


def run(exe, geo, angles, rays, triples):
    import _backproject_gather_oracle as G
    dims, half, dv = G.grid(geo)
    W, H = int(geo.nDetector[0]), int(geo.nDetector[1])
    p0, d, seg, weight, n = G.spans(rays, dims, geo.dVoxel, geo.accuracy)
    spans = np.concatenate([p0, d, seg[:, None], weight[:, None], n[:, None].astype(np.float32)], 1)
    spans[n == 0] = 0
    grid, det = np.concatenate([half, dv]), np.array([*geo.dDetector, *geo.offDetector, geo.DSD])
    (res,), _ = host_check.run(exe, [*dims, W, H, len(angles), int(geo.mode == "parallel")],
                               [grid, det, G.poses(geo, angles), spans, (triples, np.int64)], [(np.int64, len(triples) + 2)])
    return res[:-2].astype(bool), int(res[-2]), int(res[-1])


def main():
    import _backproject_gather_oracle as G
    import _backproject_oracle as B
    from neuralvolumetricreconstructionformedicalimages_amd.geometry import ConeGeometry
    with tempfile.TemporaryDirectory() as workdir:
        exe = host_check.build("gather", workdir)
        for name, (data, angles) in sorted(G.geometries().items()):
            geo = ConeGeometry(data)
            dims = tuple(int(v) for v in geo.nVoxel)
            rays = B.case_rays(geo, angles)
            wide, single = float64_triples(geo, rays), G.scatter_triples(rays, dims, geo.dVoxel, geo.accuracy)
            held, pixels, samples = run(exe, geo, angles, rays, np.concatenate([wide, single]))
            per = int(np.prod(dims)) * len(angles)
            print(f"{name:22s}: {len(wide)} float64 and {len(single)} float32 non-zero terms, all {int(held.sum())} in the candidate "
                  f"set; per voxel and view {pixels / per:.1f} pixels, {samples / per:.1f} candidate samples")
            assert held.all(), (name, np.concatenate([wide, single])[~held][:10])
            # the header and its numpy restatement pick the same candidates
            ok, k_lo, k_hi = G.candidates(geo, angles, rays)
            assert samples == int(np.where(ok, k_hi - k_lo + 1, 0).sum()), name
        print("every geometry: the candidate set is a superset of the scatter's non-zero terms; no sanitizer report")


if __name__ == "__main__":
    main()
