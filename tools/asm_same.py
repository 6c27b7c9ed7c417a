#!/usr/bin/env python3
"""Are two device-assembly dumps of the frame kernels (`make -C deepterrainrl_amd/csrc asm`) the same program?
Lines that name the per-translation-unit symbol __hip_cuid_<hash> (a hash of the source text) are left out; any other difference is
printed (first few) and the exit status is 1.
Usage: tools/asm_same.py old.s new.s"""
import itertools, sys


def body(path):
    return [l.rstrip("\n") for l in open(path) if "__hip_cuid_" not in l]


a, b = body(sys.argv[1]), body(sys.argv[2])
diffs = [(i + 1, x, y) for i, (x, y) in enumerate(itertools.zip_longest(a, b)) if x != y]
if not diffs:
    print("identical: %d lines compared (%s, %s)" % (len(a), sys.argv[1], sys.argv[2]))
    sys.exit(0)
print("DIFFERENT: %d of %d / %d compared lines (%s, %s)" % (len(diffs), len(a), len(b), sys.argv[1], sys.argv[2]))
for i, x, y in diffs[:10]:
    print("  line %d:\n    < %s\n    > %s" % (i, x, y))
sys.exit(1)
