#!/usr/bin/env python3
"""tools/isa_compare.py before.s after.s — compares the kernels of two gfx950 assembly dumps of one csrc/*.hip file (ptss_kernels.hip:
the kernels and launches, compiled as one translation unit over the layer headers ptwave.h .. ptshade.h; or one of the short kernel
files), made by hipcc with the shipped flags and --cuda-device-only -S (tools/isa_dump.sh has the command line), instruction by
instruction, after normalising symbol, label and comment text and dropping directives. Prints the summary kept as
profiles/*/isa_compare.txt."""
import re
import sys


def kernels(path):
    out, name, body = {}, None, []
    names = set()
    text = open(path).read().splitlines()
    for line in text:
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", line)
        if m:
            names.add(m.group(1))
    for line in text:
        m = re.match(r"^(\S+):", line)
        if m and m.group(1) in names:
            name, body = m.group(1), []
            continue
        if name is None:
            continue
        if re.match(r"^\.Lfunc_end", line):
            out[name] = body
            name = None
            continue
        s = re.sub(r";.*$", "", line).strip()
        if not s or s.startswith(".") and not s.startswith(".L") or re.match(r"^\.?[\w$.]+:$", s):
            continue   # comments, directives, labels
        s = re.sub(r"\.LBB\d+_\d+", "L", s)
        s = re.sub(r"_ZN?\w+", "SYM", s)
        out_line = re.sub(r"\s+", " ", s)
        body.append(out_line)
    return out


def main():
    before, after = kernels(sys.argv[1]), kernels(sys.argv[2])
    same = [k for k in before if k in after and before[k] == after[k]]
    differ = [k for k in before if k in after and before[k] != after[k]]
    missing = [k for k in before if k not in after]
    new = [k for k in after if k not in before]
    print(f"{len(same)} of {len(before)} existing kernel instantiations identical after normalising symbol, label and comment text; "
          f"{len(differ)} differ, {len(missing)} missing; {len(after)} kernels after ({len(new)} new)")
    for k in differ:
        print(f"differs: {k} {len(before[k])} -> {len(after[k])} instructions")
    for k in missing:
        print(f"missing: {k}")
    for k in new:
        print(f"new: {k} {len(after[k])} instructions")


if __name__ == "__main__":
    main()
