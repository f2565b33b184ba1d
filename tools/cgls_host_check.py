#!/usr/bin/env python3
"""Host check of the CGLS device code: compiles tools/cgls_host_check.cpp (the per-element arithmetic of csrc/cgls_device.h, fed by
plain loops that add in the kernels' order; the kernels' own indexing in csrc/cgls.hip is not part of it) for the CPU with
AddressSanitizer and UBSan, runs it over the GPU tests' sizes, inputs and scalars (tests/_cgls_oracle.py) and asserts every bound
those tests assert: the weighted sums against the correctly rounded float64 sum, the two element-wise steps per element, and that
a breakdown or a stop leaves r, x and p bit for bit.  The program is never loaded into Python.  No GPU.

    python tools/cgls_host_check.py
"""
import tempfile

import numpy as np

import host_check


def run(exe, args, inputs, outputs):
    """The arrays of host_check.run: the program prints nothing."""
    return host_check.run(exe, args, inputs, outputs)[0]


def main():
    import _cgls_oracle as C
    f32, f64 = np.float32, np.float64
    with tempfile.TemporaryDirectory() as workdir:
        exe = host_check.build("cgls", workdir)
        worst = {"wdot": 0.0, "residual r": 0.0, "residual y": 0.0, "direction x": 0.0, "direction p": 0.0}
        for n in C.SIZES:
            r, q, w, x, p, s = C.step_inputs(n)
            for has_w in (1, 0):
                weights = w if has_w else None
                total, = run(exe, ["wdot", n, has_w], [r, w], [(f64, 1)])
                want = C.wsum(r, weights)
                assert abs(total[0] - want) <= C.wsum_bound(n, want), (n, has_w)
                worst["wdot"] = max(worst["wdot"], abs(total[0] - want) / max(C.wsum_bound(n, want), 1e-300))
                for gamma, delta, _ in C.LIVE_SCALARS:
                    r2, y, out = run(exe, ["residual", n, has_w, repr(gamma), repr(delta), 0], [r, q, w],
                                     [(f32, n), (f32, n), (f64, 2)])
                    want_r, want_y = C.residual_step(r, q, weights, gamma, delta)
                    bound_r, bound_y = C.residual_bounds(q, weights, gamma, delta, r2, y)
                    assert out[1] == 1.0 and abs(out[0] - want) <= C.wsum_bound(n, want)
                    assert np.all(np.abs(r2 - want_r) <= bound_r) and np.all(np.abs(y - want_y) <= bound_y), (n, has_w, gamma)
                    worst["residual r"] = max(worst["residual r"], float((np.abs(r2 - want_r) / bound_r).max()))
                    worst["residual y"] = max(worst["residual y"], float((np.abs(y - want_y) / np.maximum(bound_y, 1e-300)).max()))
                dead = [(g, d, 0) for g, d, _ in C.DEAD_SCALARS] + [(*C.LIVE_SCALARS[0][:2], 3)]
                spoiled = q.copy()
                spoiled[0] = np.inf
                for gamma, delta, stopped in dead:
                    r2, y, out = run(exe, ["residual", n, has_w, repr(gamma), repr(delta), stopped], [r, spoiled, w],
                                     [(f32, n), (f32, n), (f64, 2)])
                    assert out[1] == 0.0 and np.array_equal(r2, r) and np.array_equal(y, w * r if has_w else r), (n, gamma, delta)
            for gamma, delta, gamma_next in C.LIVE_SCALARS:
                x2, p2 = run(exe, ["direction", n, repr(gamma), repr(delta), repr(gamma_next), 0], [x, p, s], [(f32, n)] * 2)
                want_x, want_p = C.direction_step(x, p, s, gamma, delta, gamma_next)
                bound_x, bound_p = C.fma_bound(gamma / delta, p, x2), C.fma_bound(gamma_next / gamma, p, p2)
                assert np.all(np.abs(x2 - want_x) <= bound_x) and np.all(np.abs(p2 - want_p) <= bound_p), (n, gamma)
                worst["direction x"] = max(worst["direction x"], float((np.abs(x2 - want_x) / bound_x).max()))
                worst["direction p"] = max(worst["direction p"], float((np.abs(p2 - want_p) / bound_p).max()))
            spoiled = s.copy()
            spoiled[n // 2] = np.nan
            for gamma, delta, stopped in [(g, d, 0) for g, d, _ in C.DEAD_SCALARS] + [(*C.LIVE_SCALARS[0][:2], 3)]:
                x2, p2 = run(exe, ["direction", n, repr(gamma), repr(delta), 1.5, stopped], [x, p, spoiled], [(f32, n)] * 2)
                assert np.array_equal(x2, x) and np.array_equal(p2, p), (n, gamma, delta)
            print(f"n {n}: every bound holds", flush=True)
        print("no sanitizer report; largest |. - float64| / bound: " + ", ".join(f"{k} {v:.3e}" for k, v in worst.items()))


if __name__ == "__main__":
    main()
