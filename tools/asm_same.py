#!/usr/bin/env python3
"""Are two device-assembly dumps of the frame kernels (`make -C deepterrainrl_amd/csrc asm`) the same program?
Lines that name the per-translation-unit symbol __hip_cuid_<hash> (a hash of the source text) are left out; any other difference is
printed (first few) and the exit status is 1.
Usage: tools/asm_same.py old.s new.s [--only SUBSTR]

--only SUBSTR compares just the functions whose mangled name contains SUBSTR (e.g. frame_kernel), label to .Lfunc_end: for a change that ADDS a kernel
to the translation unit and must leave the frame kernels alone. A function's position in the file numbers its local labels (.LBB<k>_<n>, .Lfunc_end<k>,
the "BB<k>_<n>" of loop comments), so <k> is masked; everything else must match line for line."""
import itertools, re, sys


def body(path):
    return [l.rstrip("\n") for l in open(path) if "__hip_cuid_" not in l]


def functions(lines, substr):
    out, name, buf = {}, None, []
    for l in lines:
        m = re.match(r"^([A-Za-z_][\w$.]*):", l)
        if name is None and m and substr in m.group(1) and not m.group(1).startswith(".L"):
            name, buf = m.group(1), []
        if name is not None:
            buf.append(re.sub(r"(\.LBB|\.Lfunc_end|\.Lfunc_begin|\bBB)\d+", r"\1<k>", l))
            if l.startswith(".Lfunc_end"):
                out[name] = buf; name = None
    return out


args = [x for x in sys.argv[1:] if not x.startswith("--")]
only = sys.argv[sys.argv.index("--only") + 1] if "--only" in sys.argv else None
if only:
    args = [x for x in args if x != only]
a, b = body(args[0]), body(args[1])
if only:
    fa, fb = functions(a, only), functions(b, only)
    if not fa or fa.keys() != fb.keys():
        print("DIFFERENT: functions matching %r: %s / %s" % (only, sorted(fa), sorted(fb)))
        sys.exit(1)
    print("functions compared: " + ", ".join("%s (%d lines)" % (k[:48], len(v)) for k, v in sorted(fa.items())))
    a = [l for k in sorted(fa) for l in fa[k]]; b = [l for k in sorted(fb) for l in fb[k]]
diffs = [(i + 1, x, y) for i, (x, y) in enumerate(itertools.zip_longest(a, b)) if x != y]
if not diffs:
    print("identical: %d lines compared (%s, %s)" % (len(a), args[0], args[1]))
    sys.exit(0)
print("DIFFERENT: %d of %d / %d compared lines (%s, %s)" % (len(diffs), len(a), len(b), args[0], args[1]))
for i, x, y in diffs[:10]:
    print("  line %d:\n    < %s\n    > %s" % (i, x, y))
sys.exit(1)
