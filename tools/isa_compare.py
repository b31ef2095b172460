#!/usr/bin/env python3
"""Was a kernel only moved by renaming?  Per kernel of a unit whose device assembly differs between two source trees:
    kernel  instructions old -> new  metadata equal?  loops with transcendentals identical?  differing lines outside them

    python tools/isa_compare.py OLD_CSRC UNIT[:SCHED_VAR] ...      e.g. /tmp/parent/svbrdf_estimation_amd/csrc svbrdf_photo_fit:SCHED_PHOTO

Each unit is compiled twice with the Makefile's flags for it (tests/unit_build.compile_unit_asm: OLD_CSRC's source, then
this tree's) and read with tools/isa_stats.py.  "identical": same instructions, operands and registers included, in every loop
that holds a transcendental; the lines outside are counted from a diff of the remaining instruction lists.  No GPU needed.
"""
import difflib
import os
import pathlib
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_stats
import unit_build

META = ("next_free_vgpr", "next_free_sgpr", "group_segment_fixed_size", "private_segment_fixed_size", "ScratchSize", "Occupancy",
        "NumVgprs", "NumSgprs", "LDS Size")


def split(text, name):
    """(instruction count, metadata, [text of each loop with transcendentals], text of everything else) of one kernel"""
    _, meta, whole, counts, ins, ranges = isa_stats.analyse(text, name)
    line = lambda i: "%s %s" % (i[2], i[3]) if i[2] else i[1]
    hot = [(a, b) for (a, b), c in zip(ranges, counts) if c["trans"]]
    inside = lambda k: any(a <= k <= b for a, b in hot)
    return (whole["total"], {m: meta.get(m) for m in META}, [[line(i) for i in ins[a:b + 1]] for a, b in hot],
            [line(i) for k, i in enumerate(ins) if not inside(k)])


if __name__ == "__main__":
    old_csrc, holder = os.path.abspath(sys.argv[1]), tempfile.TemporaryDirectory(prefix="isa_compare_")
    tmp = pathlib.Path(holder.name)         # (removed with `holder`, when the program ends)
    for arg in sys.argv[2:]:
        unit, _, sched = arg.partition(":")
        new = unit_build.compile_unit_asm(tmp, unit, sched or None)
        old = unit_build.compile_unit_asm(tmp, os.path.join(old_csrc, unit + ".hip"), sched or None)
        for name in sorted(k for k in isa_stats.kernels(new) if not k.startswith("__hip_cuid")):
            o, n = split(old, name), split(new, name)
            if o == n:
                continue
            differ = lambda a, b: sum(1 for d in difflib.ndiff(a, b) if d[0] == "+")
            inside = differ(sum(o[2], []), sum(n[2], []))
            print("%-28s %-90s %5d -> %5d  metadata %s  %d hot loops %s  other lines that differ: %d" % (
                unit, name[:90], o[0], n[0], "equal" if o[1] == n[1] else "DIFFER %s %s" % (o[1], n[1]), len(n[2]),
                "identical" if o[2] == n[2] else "DIFFER in %d lines" % inside, differ(o[3], n[3])))
