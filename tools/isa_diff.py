#!/usr/bin/env python3
"""Compare two device-assembly dumps of one source file, kernel by kernel.

    hipcc ... --cuda-device-only -S conv_igemm.hip -o old.s        (the same flags as the Makefile, at both commits)
    python tools/isa_diff.py old.s new.s [--diff SYMBOL]

Prints the kernels that exist on one side only, how many common kernels have equal bodies, and for each one that differs the
register, LDS and scratch figures of its kernel descriptor and the instruction counts of both sides.  Bodies are compared after
assembler comments are stripped and basic-block / temporary labels are renumbered in order of appearance, so that a kernel whose
position in the file moved still compares equal.  --diff SYMBOL prints the unified diff of one kernel's normalised body.
A refactor of device code is checked with this before it is timed: equal bodies need no measurement.
"""
import difflib
import re
import sys

FIELDS = ("next_free_vgpr", "next_free_sgpr", "accum_offset", "group_segment_fixed_size", "private_segment_fixed_size")
LABEL = re.compile(r"\.L(?:BB|tmp|JTI|func_begin)[0-9_]+")


def kernels(path):
    """symbol -> (normalised body lines, descriptor fields)"""
    text = open(path).read()
    out = {}
    for m in re.finditer(r"^\t\.amdhsa_kernel (\S+)\n(.*?)^\t\.end_amdhsa_kernel", text, re.M | re.S):
        sym, desc = m.group(1), m.group(2)
        start = text.rindex("\n%s:" % sym, 0, m.start()) + 1
        names = {}
        body = []
        for line in text[start:m.start()].splitlines()[1:]:
            line = line.split(";")[0].strip()
            if not line or (line.startswith(".") and not line.startswith(".L")):   # directives (.p2align, .section ...) are not code
                continue
            body.append(LABEL.sub(lambda l: names.setdefault(l.group(0), ".L%d" % len(names)), line))
        fields = {f: int(re.search(r"\.amdhsa_%s (\d+)" % f, desc).group(1)) for f in FIELDS}
        out[sym] = (body, fields)
    return out


def count(body):
    return sum(1 for line in body if not line.endswith(":"))


def main(argv):
    if len(argv) < 3:
        sys.exit(__doc__)
    a, b = kernels(argv[1]), kernels(argv[2])
    if len(argv) == 5 and argv[3] == "--diff":
        sys.stdout.write("\n".join(difflib.unified_diff(a[argv[4]][0], b[argv[4]][0], argv[1], argv[2], lineterm="", n=2)) + "\n")
        return
    for name, x, y in (("first", a, b), ("second", b, a)):
        for sym in sorted(set(x) - set(y)):
            print("only in the %s: %s" % (name, sym))
    common = sorted(set(a) & set(b))
    differ = [s for s in common if a[s][0] != b[s][0]]
    print("%d kernels / %d kernels, %d common, %d equal bodies, %d differ" % (len(a), len(b), len(common), len(common) - len(differ), len(differ)))
    print("(per differing kernel: %s, instructions; first -> second)" % ", ".join(FIELDS))
    for sym in differ:
        fa, fb = a[sym][1], b[sym][1]
        figs = ["%d -> %d" % (fa[f], fb[f]) if fa[f] != fb[f] else str(fa[f]) for f in FIELDS]
        worse = any(fb[f] > fa[f] for f in FIELDS if f != "next_free_sgpr")
        print("%s %s\n    %s | %d -> %d" % ("WORSE" if worse else "     ", sym, " | ".join(figs), count(a[sym][0]), count(b[sym][0])))


if __name__ == "__main__":
    main(sys.argv)
