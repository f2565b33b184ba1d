"""What the drivers tools/*_host_check.py share: the host compiler, one flag list, the build of tools/<name>_host_check.cpp and the
run of the program it gives.  Such a program is a stand-alone executable with a main of its own, built with AddressSanitizer and
UBSan and run as a child process; nothing of it is ever loaded into Python.  A module, not a script.  No GPU.
"""
import os
import shutil
import subprocess
import sys

import numpy as np

TOOLS = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(TOOLS)
for _path in (os.path.join(REPO, "tests"), REPO):                  # the drivers import the package and the oracles of tests/
    if _path not in sys.path:
        sys.path.insert(0, _path)

# -ffp-contract=off as the library has it: a device header's arithmetic is compiled in the order written.  -fno-sanitize-recover=all:
# a UBSan finding ends the program with a non-zero exit as an AddressSanitizer one does, besides its text on stderr.
FLAGS = ["-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall"]


def compiler():
    return shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")


def build(name, workdir, defines=()):
    """Compiles tools/<name>_host_check.cpp into `workdir` -> the executable's path."""
    cxx = compiler()
    if cxx is None:
        raise RuntimeError("no host C++ compiler found")
    exe = os.path.join(workdir, name + "_host_check")
    subprocess.check_call([cxx, *FLAGS, *defines, os.path.join(TOOLS, name + "_host_check.cpp"), "-o", exe])
    return exe


def run(exe, args, inputs=(), outputs=()):
    """Runs `exe` as a child process with `args`, then one file per input, then one file per output, beside the executable.
    An input is an array, written as float32, or (array, dtype), or None for an absent one, passed as "-"; an output is (dtype, count).
    -> ([array per output], stdout).  A non-zero exit, any text on stderr (a sanitizer report) or a short output file is an error."""
    workdir = os.path.dirname(exe)
    paths = []
    for i, a in enumerate(inputs):
        if a is None:
            paths.append("-")
            continue
        a, dtype = a if isinstance(a, tuple) else (a, np.float32)
        paths.append(os.path.join(workdir, f"in{i}.bin"))
        np.ascontiguousarray(a, dtype=dtype).tofile(paths[-1])
    outs = [os.path.join(workdir, f"out{i}.bin") for i in range(len(outputs))]
    done = subprocess.run([exe, *[str(a) for a in args], *paths, *outs], capture_output=True, text=True)
    if done.returncode != 0 or done.stderr.strip():
        raise RuntimeError(f"{os.path.basename(exe)}: exit {done.returncode}: {done.stdout}\nsanitizer output:\n{done.stderr}")
    arrays = [np.fromfile(path, dtype=dtype, count=count) for path, (dtype, count) in zip(outs, outputs)]
    for a, (_, count) in zip(arrays, outputs):
        if a.size != count:
            raise RuntimeError(f"{os.path.basename(exe)}: an output of {a.size} elements, {count} expected")
    return arrays, done.stdout
