#!/usr/bin/env python3
"""Are two device listings the same code?  For refactors that must not touch a kernel.

    python tools/isa_same.py A.s B.s        # e.g. build/emsar_hip-hip-amdgcn-amd-amdhsa-gfx950.s of two trees

Compares PER KERNEL SYMBOL, not by position (moving host code changes the order in which templates are instantiated): the set of
symbols, each symbol's text (instructions, its kernel descriptor, its resource .set lines) and its entry of the metadata block
(registers, LDS, scratch, spills, arguments).  Assembler comments, the __hip_cuid_ lines and the function numbers inside local
labels (.LBB12_3 -> .LBB_3) are left out.  Prints the symbols that differ; exit status 0 = nothing differs.
"""
import re
import sys

LOCAL = re.compile(r"\.(LBB|Lfunc_end|Lfunc_begin|LJTI|Ltmp)\d+")
TEXT_SECTION = re.compile(r"\.section\s+\.text\.([^,\s]+)")


def lines_of(path):
    with open(path) as f:
        for raw in f:
            line = raw.split(";", 1)[0].rstrip()
            if line.strip() and "__hip_cuid_" not in line:
                yield LOCAL.sub(lambda m: "." + m.group(1) + "_", line)


def split(path):
    """({symbol: its lines of text}, {symbol: its lines of metadata})"""
    text, meta, sym, entry, in_meta = {}, {}, "<head>", None, False
    for line in lines_of(path):
        word = line.strip()
        if word == ".amdgpu_metadata":
            in_meta = True
        elif word == ".end_amdgpu_metadata":
            in_meta = False
        elif in_meta:
            if line.startswith("  - "):                 # the next kernel's entry; keyed by its .name below
                entry = []
                meta[len(meta)] = entry
            (entry if entry is not None and line.startswith("  ") else meta.setdefault("<meta head>", [])).append(line)
        else:
            m = TEXT_SECTION.search(line)
            if m:
                sym = m.group(1)
            elif word.startswith(".section") and not word.startswith(".section\t.rodata") and not word.startswith(".section .rodata"):
                sym = "<tail>"
            text.setdefault(sym, []).append(line)
    named = {}
    for key, entry in meta.items():
        name = next((l.split(":", 1)[1].strip() for l in entry if l.strip().startswith(".name:") and not l.startswith("      ")), key)
        named[name] = entry
    return text, named


def main(a, b):
    ta, ma = split(a)
    tb, mb = split(b)
    bad = 0
    for what, x, y in (("text", ta, tb), ("metadata", ma, mb)):
        for s in sorted(set(x) | set(y), key=str):
            if s not in x or s not in y:
                print("%s: %s only in %s" % (what, s, a if s in x else b))
                bad += 1
            elif x[s] != y[s]:
                first = next((i for i, (p, q) in enumerate(zip(x[s], y[s])) if p != q), min(len(x[s]), len(y[s])))
                print("%s: %s differs (%d against %d lines, first at line %d of the symbol)" % (what, s, len(x[s]), len(y[s]), first))
                bad += 1
    kernels = sum(1 for s in ma if not str(s).startswith("<"))
    print("%d kernels, %d symbols with text: %s" % (kernels, len(ta), "nothing differs" if not bad else "%d differences" % bad))
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
