#!/usr/bin/env python3
"""Host check of the TV-prox device code: compiles tools/tvprox_host_check.cpp (the per-voxel arithmetic of csrc/tvprox_device.h,
fed by a plain loop over the volume; the kernel's own staging and indexing in csrc/tvprox.hip is not part of it) for the CPU with
AddressSanitizer and UBSan, runs it over the step tests' shapes and inputs and prints its largest difference from the float64
oracle of tests/_tvprox_oracle.py, next to the difference of the oracle's own float32 form, which is where the GPU tests' bounds
come from (4 x those figures; tests/test_hip_tvprox.py).  No GPU.

    python tools/tvprox_host_check.py
"""
import tempfile

import numpy as np

import host_check


def run(exe, args, inputs, outputs):
    """`inputs`: arrays written to files and passed after `args`; `outputs`: shapes of the float32 files the program writes."""
    arrays, _ = host_check.run(exe, args, inputs, [(np.float32, int(np.prod(shape))) for shape in outputs])
    return [a.reshape(shape) for a, shape in zip(arrays, outputs)]


def main():
    import _tvprox_oracle as T
    with tempfile.TemporaryDirectory() as workdir:
        exe = host_check.build("tvprox", workdir)
        worst = {"host step": 0.0, "oracle f32 step": 0.0, "host primal": 0.0, "oracle f32 primal": 0.0}
        for shape in T.STEP_SHAPES:
            for lam in T.STEP_LAMBDAS:
                for nonneg in (False, True):
                    b, r, p_old = T.step_inputs(shape)
                    want_p, want_r = T.step(b, r, p_old, lam, T.STEP_MOMENTUM, nonneg)
                    own_p, own_r = T.step_f32(b, r, p_old, lam, T.STEP_MOMENTUM, nonneg)
                    p, r_next = run(exe, ["step", *shape, repr(lam), repr(T.STEP_MOMENTUM), int(nonneg)], [b, r, p_old],
                                    [(3,) + shape] * 2)
                    host = max(float(np.abs(p - want_p).max()), float(np.abs(r_next - want_r).max()))
                    own = max(float(np.abs(own_p - want_p).max()), float(np.abs(own_r - want_r).max()))
                    inert = max(float(np.abs(t[0][0]).max()) + float(np.abs(t[1][:, 0]).max()) + float(np.abs(t[2][:, :, 0]).max())
                                for t in (p, r_next))
                    assert inert == 0.0, (shape, lam, nonneg)
                    want_x = T.primal(b, r, lam, nonneg)
                    x, = run(exe, ["primal", *shape, repr(lam), int(nonneg)], [b, r], [shape])
                    host_x = float(np.abs(x - want_x).max())
                    own_x = float(np.abs(T.primal_f32(b, r, lam, nonneg) - want_x).max())
                    same = np.array_equal(p, own_p) and np.array_equal(r_next, own_r) and np.array_equal(x, T.primal_f32(b, r, lam, nonneg))
                    print(f"{shape} lam {lam:g} nonneg {int(nonneg)}: step, host {host:.3e}, oracle f32 {own:.3e};  primal, host "
                          f"{host_x:.3e}, oracle f32 {own_x:.3e};  host == oracle f32 bit for bit: {same}")
                    for key, v in (("host step", host), ("oracle f32 step", own), ("host primal", host_x), ("oracle f32 primal", own_x)):
                        worst[key] = max(worst[key], v)
        print("largest |. - float64 oracle|: " + ", ".join(f"{k} {v:.3e}" for k, v in worst.items()))


if __name__ == "__main__":
    main()
