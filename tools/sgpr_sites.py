#!/usr/bin/env python3
"""tools/sgpr_sites.py <kernel.s> [min-depth] — where the SGPR-operand VALU instructions of one kernel's assembly sit (tools/isa_dump.sh
writes the dump): one line per loop of the kernel (the compiler's own "Loop Header" comments name each block's loop and depth) with
the loop's VALU count, its SGPR-operand VALU count (the class of tools/isa_classes.py: twice the issue cost of a plain instruction,
tools/microbench/vgpr_banks.hip) and how many of those are plain copies `v_mov_b32 vN, sM`, followed by the instructions themselves.
Blocks outside every loop are summed as depth 0. The table kept as profiles/uniform/sgpr_operand_sites.txt is this output with the
loops named by hand."""
import collections
import re
import sys

path = sys.argv[1]
min_depth = int(sys.argv[2]) if len(sys.argv) > 2 else 0
sgpr = re.compile(r"(?<![\w\[])s\d+|s\[\d+:\d+\]|\bvcc\b|\bexec\b")
slow_prefix = ("v_cmp", "v_cndmask", "v_addc", "v_subb", "v_readlane", "v_writelane", "v_readfirstlane")

loops = collections.OrderedDict()   # header label -> dict
cur = ("-", 0)
label = None
lines = open(path).read().splitlines()
for n, raw in enumerate(lines, 1):
    m = re.match(r"^(\.LBB\d+_\d+):", raw)
    if m or re.match(r"^; %bb\.\d+:", raw):
        label = m.group(1) if m else None
        # the block's loop: named on this line, or — a loop header — on the comment lines that follow it
        h = re.search(r"in Loop: Header=(BB\d+_\d+) Depth=(\d+)", raw)
        own = None
        for k in range(n - 1, min(n + 8, len(lines))):
            if k > n - 1 and not lines[k].lstrip().startswith(";"):
                break
            mm = re.search(r"This (?:Inner )?Loop Header: Depth=(\d+)", lines[k])
            if mm:
                own = int(mm.group(1))
        if own is not None and label:
            cur = (label[2:], own)
        elif h:
            cur = (h.group(1), int(h.group(2)))
        else:
            cur = ("-", 0)
        continue
    ins = raw.split(";")[0].strip()
    m = re.match(r"(v_\w+)\b(.*)", ins)
    if not m:
        continue
    d = loops.setdefault(cur, {"valu": 0, "sites": [], "first": n})
    d["valu"] += 1
    op, rest = m.group(1), m.group(2)
    if not op.startswith(slow_prefix) and sgpr.search(rest):
        d["sites"].append((n, ins))

tot = sum(len(d["sites"]) for d in loops.values())
print("%s: %d SGPR-operand VALU instructions" % (path.split("/")[-1], tot))
for (head, depth), d in loops.items():
    if depth < min_depth or not d["sites"]:
        continue
    movs = sum(1 for _, i in d["sites"] if re.match(r"v_mov_b32_e32 v\d+, s\d+$", i))
    print("loop %-10s depth %d  line %5d  VALU %4d  SGPR-operand %3d  (v_mov v, s: %d)" % (head, depth, d["first"], d["valu"], len(d["sites"]), movs))
    for n, i in d["sites"]:
        print("      %5d  %s" % (n, i))
