#!/usr/bin/env python3
"""Host check of the MLP kernels' launch plan: compiles tools/step_plan_host_check.cpp (csrc/mlp_step_plan.h, the functions the
host drivers call) for the CPU with AddressSanitizer and UBSan and runs it as a process of its own over (flags, n_rays, n_samples)
cases.  plan() returns what it printed; tests/test_step_plan_cpu.py holds that to tests/_mlp16_oracle.py.  The program is never
loaded into Python.  No GPU.

    python tools/step_plan_host_check.py [flags n_rays n_samples]
"""
import collections
import functools
import os
import sys
import tempfile

sys.path.append(os.path.dirname(os.path.abspath(__file__)))          # tools/, for a caller that loads this file by its path
import host_check  # noqa: E402

Caps = collections.namedtuple("Caps", "forward forward_split backward backward16 train_max_rays max_samples_lds")
Plan = collections.namedtuple("Plan", "parts train_waves splits split_grid forward_grid16 forward_grid32 slabs16 slabs32 train_grid")

compiler = host_check.compiler                                       # such a caller asks the driver, not host_check
build = functools.partial(host_check.build, "step_plan")


def plan(exe, workdir, cases):
    """cases: (flags, n_rays, n_samples) triples -> (Caps, [Plan per case]).  A sanitizer report is an error."""
    path = os.path.join(workdir, "cases.txt")
    with open(path, "w") as f:
        f.write("".join(f"{a} {b} {c}\n" for a, b, c in cases))
    lines = host_check.run(exe, [path])[1].splitlines()
    head = lines[0].split()
    assert head[0] == "caps" and len(lines) == len(cases) + 1, (head, len(lines), len(cases))
    return Caps(*map(int, head[1:])), [Plan(*map(int, line.split())) for line in lines[1:]]


def main():
    case = tuple(int(v) for v in sys.argv[1:4]) if len(sys.argv) >= 4 else (0, 1024, 192)
    with tempfile.TemporaryDirectory() as workdir:
        caps, (p,) = plan(build(workdir), workdir, [case])
        print(caps)
        print(case, p)


if __name__ == "__main__":
    main()
