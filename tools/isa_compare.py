#!/usr/bin/env python3
"""tools/isa_compare.py before.s after.s [pairs.txt] — compares the kernels of two gfx950 assembly dumps of one csrc/*.hip file (ptss_kernels.hip:
the kernels and launches, compiled as one translation unit over the layer headers ptwave.h .. ptshade.h; or one of the short kernel
files), made by hipcc with the shipped flags and --cuda-device-only -S (tools/isa_dump.sh has the command line), instruction by
instruction, after normalising symbol, label and comment text and dropping directives. Prints the summary kept as
profiles/*/isa_compare.txt.

Kernels are paired by mangled name. pairs.txt, for a change that renames kernels or moves them between files (feed it the concatenated
dumps of the files concerned): lines of `old-name-substring new-name-substring`. A kernel missing after whose name holds the first is
compared against the new kernel whose name holds the second; each side of a pair must name exactly one kernel."""
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
    if len(sys.argv) > 3:
        pairs = [line.split() for line in open(sys.argv[3]) if line.strip() and not line.startswith("#")]
        moved_same = 0
        for old, successor in pairs:
            olds, news = [k for k in missing if old in k], [k for k in new if successor in k]
            if len(olds) != 1 or len(news) != 1:
                print(f"pair {old} {successor}: {len(olds)} missing and {len(news)} new kernels match, one of each wanted")
                continue
            missing.remove(olds[0])
            new.remove(news[0])
            if before[olds[0]] == after[news[0]]:
                moved_same += 1
                print(f"moved, identical: {olds[0]} -> {news[0]}")
            else:
                print(f"moved, differs: {olds[0]} -> {news[0]} {len(before[olds[0]])} -> {len(after[news[0]])} instructions")
        print(f"{len(pairs)} pairs: {moved_same} moved kernels identical; {len(missing)} kernels without a successor, {len(new)} without a predecessor")
    for k in missing:
        print(f"missing: {k}")
    for k in new:
        print(f"new: {k} {len(after[k])} instructions")


if __name__ == "__main__":
    main()
