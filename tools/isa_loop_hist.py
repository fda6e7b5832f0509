#!/usr/bin/env python3
"""Instruction mix of the loops of one kernel in a gfx950 assembly listing (hipcc -S
--cuda-device-only of a small TU that instantiates just that kernel: seconds instead of the
library's two minutes), the mix OUTSIDE its MFMA loops -- before the first, after the last -- and the
kernel's register / scratch / occupancy lines.  Usage: isa_loop_hist.py file.s <substring of the mangled kernel name>
[--brief: no per-opcode lists, MFMA loops only]"""
import collections
import re
import sys


def group(op):
    return ("mfma" if "mfma" in op else "valu" if op.startswith("v_") else "lds" if op.startswith("ds_")
            else "vmem" if op.startswith(("global_", "buffer_", "flat_", "scratch_")) else "salu" if op.startswith("s_") else op)


def count(lines):
    ops = collections.Counter()
    for x in lines:
        x = x.strip()
        if not x or x[0] in ";._" or x.endswith(":"):     # comments, directives, labels (the kernel's own: "_Z...: ; @...")
            continue
        ops[x.split()[0]] += 1
    return ops


def groups(ops):
    grp = collections.Counter()
    for k, v in ops.items():
        grp[group(k)] += v
    return dict(grp)


def main(path, key, brief=False):
    s = open(path).read().splitlines()
    start = next(i for i, l in enumerate(s) if re.match(r"^_Z\S*" + re.escape(key) + r"\S*:", l))
    end = next(i for i in range(start, len(s)) if s[i].startswith(".Lfunc_end"))
    body = s[start:end]
    print(s[start].split(":")[0], len(body), "lines")
    # the resource lines the compiler prints behind the kernel's code
    for l in s[end:end + 80]:
        if re.match(r"^; (NumVgprs|NumAgprs|TotalNumVgprs|NumSgprs|ScratchSize|Occupancy|LDSByteSize)\b", l):
            print("  ", l[2:])
        if l.startswith("_Z"):
            break
    labels = {}
    for i, l in enumerate(body):
        m = re.match(r"^(\.LBB\d+_\d+):", l)
        if m:
            labels[m.group(1)] = i
    loops = []
    for i, l in enumerate(body):
        m = re.search(r"(s_cbranch\w+|s_branch)\s+(\.LBB\d+_\d+)", l)
        if not (m and m.group(2) in labels and labels[m.group(2)] < i):
            continue
        a, b = labels[m.group(2)], i
        ops = count(body[a:b])
        loops.append((a, b, m.group(2), ops, sum(v for k, v in ops.items() if "mfma" in k)))
    mfma_loops = [(a, b) for a, b, _, _, nm in loops if nm]
    # Outside the k-loops: an enclosing loop that merely contains MFMA loops (a grid-stride or tile loop) is no k-loop --
    # the innermost ones count, i.e. those that contain no other MFMA loop
    inner = [(a, b) for a, b in mfma_loops if not any((a <= c and d <= b) and (a, b) != (c, d) for c, d in mfma_loops)]
    for a, b, label, ops, nm in loops:
        if brief and (a, b) not in inner:      # --brief: the k-loops alone (a backward branch around one is no k-loop)
            continue
        print("loop", label, "lines", b - a, "instructions", sum(ops.values()), "mfma", nm)
        if nm == 0:
            continue
        print("   groups:", groups(ops))
        if not brief:
            for k, v in sorted(ops.items(), key=lambda t: -t[1])[:40]:
                print("     %-28s %d" % (k, v))
    if inner:
        first, last = min(a for a, _ in inner), max(b for _, b in inner)
        for name, part in (("before the first MFMA loop", body[:first]), ("after the last MFMA loop", body[last + 1:])):
            ops = count(part)
            print(name + ":", sum(ops.values()), "instructions")
            print("   groups:", groups(ops))
            if not brief:
                for k, v in sorted(ops.items(), key=lambda t: -t[1])[:40]:
                    print("     %-28s %d" % (k, v))


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2], "--brief" in sys.argv[3:])
