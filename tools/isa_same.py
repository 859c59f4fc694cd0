#!/usr/bin/env python3
"""Are the kernels of two device-assembly files the same code?  The check a refactor of the device side has to pass.

    hipcc <the Makefile's flags of FILE> --offload-arch=gfx950 --cuda-device-only -S FILE.hip -o before/FILE.s     (old tree)
    hipcc ...                                                                        -o after/FILE.s      (new tree)
    tools/isa_same.py before/FILE.s after/FILE.s [...more pairs]

Per kernel it compares the instruction stream (labels included, comments dropped) and the .amdhsa_* descriptor lines
(registers, LDS, scratch).  What a compilation unit's identity puts into the file (.file, .ident, the __hip_cuid symbol) and
the metadata notes are not code and are ignored.  Exit status 1 if a kernel is missing, new or different."""
import difflib
import re
import sys


def kernels(path):
    """{kernel name: [lines]} -- from the kernel's label to its .end_amdhsa_kernel (body, then descriptor)"""
    out, name, body = {}, None, []
    names = set()
    lines = open(path).read().split("\n")
    for ln in lines:
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", ln)
        if m:
            names.add(m.group(1))
    for ln in lines:
        s = ln.split(";")[0].rstrip()
        if not s.strip():
            continue
        m = re.match(r"(\S+):$", s)
        if m and m.group(1) in names:
            name, body = m.group(1), []
            out[name] = body
            continue
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", s)
        if m:
            name, body = m.group(1), out.setdefault(m.group(1), [])
        if name is None or re.match(r"\s*\.(file|ident|loc|cfi_|p2align|section|text|type|size|globl|protected|weak|set)\b", s):
            continue
        body.append(s)
        if s.strip() == ".end_amdhsa_kernel" or s.strip().startswith(".Lfunc_end"):
            name = None
    return out


def main():
    args = sys.argv[1:]
    if not args or len(args) % 2:
        sys.exit(__doc__)
    bad = 0
    for before, after in zip(args[::2], args[1::2]):
        a, b = kernels(before), kernels(after)
        for k in sorted(set(a) | set(b)):
            if k not in a or k not in b:
                print(f"{after}: {k}: only in {'the new' if k in b else 'the old'} file")
                bad += 1
            elif a[k] != b[k]:
                d = [x for x in difflib.unified_diff(a[k], b[k], lineterm="", n=0) if not x.startswith(("---", "+++", "@@"))]
                print(f"{after}: {k}: DIFFERENT ({len(d)} changed lines of {len(a[k])}), first: {d[:2]}")
                bad += 1
        print(f"{after}: {len(b)} kernels, {sum(1 for k in b if a.get(k) == b[k])} identical")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
