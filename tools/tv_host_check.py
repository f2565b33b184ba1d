#!/usr/bin/env python3
"""Host check of the TV device code: compiles tools/tv_host_check.cpp (the per-voxel arithmetic of csrc/tv_device.h, fed by a plain
loop over the volume; the kernel's own staging and indexing in csrc/tv.hip is not part of it) for the CPU with AddressSanitizer and
UBSan, runs it over the test shapes and prints its largest difference from the float64 oracle of tests/_tv_oracle.py.  The GPU
tests' bounds are 4 x these figures (tests/test_hip_tv.py).  No GPU.

    python tools/tv_host_check.py
"""
import tempfile

import numpy as np

import host_check


def run(exe, args, volume):
    (out,), stdout = host_check.run(exe, args, [volume], [(np.float32, volume.size)])
    return out.reshape(volume.shape), [float(v) for v in stdout.split()]


def main():
    import _tv_oracle as T
    with tempfile.TemporaryDirectory() as workdir:
        exe = host_check.build("tv", workdir)
        worst_g = worst_tv = worst_g2 = 0.0
        for shape in T.SHAPES + T.GPU_SHAPES:
            for kind in T.KINDS:
                for eps in T.EPS:
                    x = T.volume(kind, shape)
                    g, (tv, g2) = run(exe, ["gradient", *shape, repr(eps)], x)
                    want = T.gradient(x, eps)
                    err = float(np.abs(g - want).max())
                    zero = T.constant_neighbourhood(x)
                    assert not g[zero].any(), (shape, kind, eps)
                    tv_want, g2_want = T.tv(x, eps), float((want * want).sum())
                    e_tv = abs(tv - tv_want) / x.size
                    e_g2 = abs(g2 - g2_want) / x.size
                    print(f"{shape} {kind:8s} eps {eps:g}: max|g| {np.abs(want).max():.3f}  max|g - oracle| {err:.3e}  "
                          f"|TV - oracle| / N {e_tv:.3e}  |sum g^2 - oracle| / N {e_g2:.3e}")
                    worst_g, worst_tv, worst_g2 = max(worst_g, err), max(worst_tv, e_tv), max(worst_g2, e_g2)
        print(f"gradient: largest |g - oracle| {worst_g:.3e}, largest |TV - oracle| / N {worst_tv:.3e}, "
              f"largest |sum g^2 - oracle| / N {worst_g2:.3e}")
        clean, noisy = T.noisy_phantom()
        for eps in T.EPS:
            got, (tv, g2) = run(exe, ["descent", *noisy.shape, repr(eps), repr(T.DESCENT_STEP), T.DESCENT_STEPS], noisy)
            want, tv_want, norm_want = T.descent(noisy, T.DESCENT_STEP, T.DESCENT_STEPS, eps)
            print(f"descent, {T.DESCENT_STEPS} steps of {T.DESCENT_STEP} from the noisy 32^3 phantom, eps {eps:g}: "
                  f"max|f - oracle| {np.abs(got - want).max():.3e}  TV before the last step {tv:.6f} vs {tv_want:.6f} "
                  f"(differs by {abs(tv - tv_want):.3e})  ||g|| {np.sqrt(g2):.6f} vs {norm_want:.6f} "
                  f"(differs by {abs(np.sqrt(g2) - norm_want):.3e})")


if __name__ == "__main__":
    main()
