#!/usr/bin/env python3
"""Host check of the ctypes mirrors of the C ABI's structs: compiles tools/abi_layout_host_check.cpp, which includes
include/naf_hip.h and prints `sizeof` and every `offsetof` of its public structs, runs it as a process of its own, and holds three
descriptions of each struct against one another:
  - the field names in the header's text, in order (read here with a regular expression, so a field added to the header alone shows),
  - the names, offsets and size the C compiler reports through the program,
  - the names, `.offset`s and `ctypes.sizeof` of the matching class of _abi.py.
A field added, dropped, moved or retyped on any side makes them differ.  The program is never loaded into Python.  No GPU.

    python tools/abi_layout_host_check.py
"""
import ctypes
import functools
import os
import re
import sys
import tempfile

sys.path.append(os.path.dirname(os.path.abspath(__file__)))          # tools/, for a caller that loads this file by its path
import host_check  # noqa: E402

# struct of include/naf_hip.h -> its mirror in _abi.py
MIRRORS = {"naf_render_cfg": "RenderCfg", "naf_grad_buckets": "GradBuckets", "naf_table_adam": "TableAdam",
           "naf_scan_draw": "ScanDraw", "naf_detector": "Detector", "naf_next_draw": "NextDraw"}

compiler = host_check.compiler                                       # a caller asks the driver, not host_check
build = functools.partial(host_check.build, "abi_layout")


def header_structs(path=os.path.join(host_check.REPO, "include", "naf_hip.h")):
    """-> {struct: [field names in order]} for every `typedef struct <name> { ... } <name>;` of the header."""
    text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    out = {}
    for name, body in re.findall(r"typedef\s+struct\s+(\w+)\s*\{(.*?)\}\s*\1\s*;", text, flags=re.S):
        out[name] = [re.search(r"(\w+)\s*(\[[^\]]*\])?\s*$", declarator).group(1)
                     for declaration in body.split(";") if declaration.strip() for declarator in declaration.split(",")]
    return out


def compiled_structs(exe):
    """-> {struct: (size, [(field, offset) in order])} as the program prints them."""
    _, stdout = host_check.run(exe, [])
    out, current = {}, None
    for kind, name, number in (line.split() for line in stdout.splitlines()):
        if kind == "struct":
            current = out[name] = (int(number), [])
        else:
            current[1].append((name, int(number)))
    return out


def mirrored_struct(cls):
    """-> (size, [(field, offset) in order]) of a ctypes.Structure."""
    return ctypes.sizeof(cls), [(name, getattr(cls, name).offset) for name, *_ in cls._fields_]


def differences(exe, abi):
    """Every disagreement between the header's text, the compiled layout and the classes of `abi` (_abi.py), as lines of text."""
    header, compiled, found = header_structs(), compiled_structs(exe), []
    if set(header) != set(MIRRORS) or list(compiled) != list(MIRRORS):
        found.append(f"structs: header {sorted(header)}, program {sorted(compiled)}, mirrored {sorted(MIRRORS)}")
    for struct, cls in MIRRORS.items():
        size, fields = compiled.get(struct, (None, []))
        mirror_size, mirror_fields = mirrored_struct(getattr(abi, cls))
        if header.get(struct) != [name for name, _ in fields]:
            found.append(f"{struct}: the header names {header.get(struct)}, the program prints {[name for name, _ in fields]}")
        if (size, fields) != (mirror_size, mirror_fields):
            found.append(f"{struct}: compiled size {size} fields {fields}, _abi.{cls} size {mirror_size} fields {mirror_fields}")
    return found


def main():
    from neuralvolumetricreconstructionformedicalimages_amd import _abi
    with tempfile.TemporaryDirectory() as workdir:
        found = differences(build(workdir), _abi)
    for line in found:
        print(line)
    if not found:
        print(f"{len(MIRRORS)} structs: names, offsets and sizes agree between the header, the compiler and _abi.py")
    return 1 if found else 0


if __name__ == "__main__":
    sys.exit(main())
