#!/usr/bin/env python3
"""Compares two assembly listings of one translation unit, function by function (hipcc ... --cuda-device-only -S of
csrc/render_fused.hip before and after a change that must leave the machine code alone).  Per symbol it compares the instruction
text from the function's label to its end, the .amdhsa_kernel descriptor, the resource `.set` lines and the kernel's entry in the
amdgpu metadata.  The only normalisation: the running function number in local labels (.LBB<n>_, .Lfunc_end<n>, BB<n>_ in the loop
comments, ...), which follows the ORDER of the functions in the unit, and the column of the comment behind such a label.  It reads the two files and nothing else.

    python tools/compare_kernel_asm.py before.s after.s        exit 0: every function identical

--rename OLD=NEW (repeatable) reads the symbol NEW of after.s as OLD, for a kernel that the change renamed.
"""
import argparse
import re
import sys

LOCAL = re.compile(r"(\.L|\b)(BB|func_end|func_begin|JTI|tmp|CPI)\d+(?=_|\b)")


def functions(path, rename=()):
    """-> ({symbol: text}, kernel symbols, the .ident line)."""
    text = open(path).read()
    for old, new in rename:
        text = text.replace(new, old)
    meta_at = text.index("\t.amdgpu_metadata")
    body, meta = text[:meta_at], text[meta_at:]
    out, kernels = {}, set()
    starts = [(m.start(), m.group(1)) for m in re.finditer(r"^\t\.type\t(\S+),@function$", body, re.M)]
    for (at, name), (end, _) in zip(starts, starts[1:] + [(len(body), None)]):
        chunk = body[at:end]
        begin = chunk.rfind("; -- Begin function")           # the next function's .text / .section, .protected, .globl lines
        if begin != -1:
            lines = chunk[:chunk.rfind("\n", 0, begin) + 1].split("\n")
            while lines and (lines[-1] == "" or lines[-1].startswith(("\t.text", "\t.section\t.text"))):
                lines.pop()
            chunk = "\n".join(lines)
        elif "\t.p2alignl" in chunk:                         # the unit's last function: its padding, globals and compilation-unit id follow
            chunk = chunk[:chunk.index("\t.p2alignl")]
        out[name] = re.sub(r"[ \t]+;", " ;", LOCAL.sub(lambda m: m.group(1) + m.group(2), chunk))      # (the number's width moves the comment column)
        if "\t.amdhsa_kernel " + name in chunk:
            kernels.add(name)
    for entry in re.split(r"^  - ", meta[meta.index("amdhsa.kernels:"):meta.index("amdhsa.target:")], flags=re.M)[1:]:
        name = re.search(r"^    \.name:\s+(\S+)$", entry, re.M).group(1)
        out[name] += "\n; metadata\n" + entry
    ident = re.search(r"^\t\.ident\t(.*)$", text, re.M)
    return out, kernels, ident.group(1) if ident else "?"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("before")
    ap.add_argument("after")
    ap.add_argument("--rename", action="append", default=[], metavar="OLD=NEW")
    args = ap.parse_args()
    a, ka, ia = functions(args.before)
    b, kb, ib = functions(args.after, [r.split("=", 1) for r in args.rename])
    print("compiler:", ia if ia == ib else f"{ia} / {ib}")
    differ = sorted(n for n in a.keys() & b.keys() if a[n] != b[n])
    for label, names in (("only in " + args.before, sorted(a.keys() - b.keys())), ("only in " + args.after, sorted(b.keys() - a.keys())),
                         ("differ", differ)):
        for n in names:
            print(f"{label}: {n}")
    same = len(ka & kb) - len([n for n in differ if n in ka])
    print(f"{same} of {len(ka | kb)} kernels identical; {len(a.keys() | b.keys()) - len(ka | kb)} other functions, "
          f"{len([n for n in differ if n not in ka])} of them differ")
    return 0 if not differ and a.keys() == b.keys() and ia == ib else 1


if __name__ == "__main__":
    sys.exit(main())
