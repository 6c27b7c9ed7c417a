#!/usr/bin/env python3
"""Are two device-assembly dumps of the frame kernels (`make -C deepterrainrl_amd/csrc asm`) the same program?
Lines that name the per-translation-unit symbol __hip_cuid_<hash> (a hash of the source text) are left out; any other difference is
printed (first few) and the exit status is 1.
Usage: tools/asm_same.py old.s new.s [--only SUBSTR[,SUBSTR...]]

--only compares just the functions whose mangled name contains one of the SUBSTRs (e.g. frame_kernel,kin_dyn_terms), label to .Lfunc_end: for a change that
moves the frame kernels to another translation unit, or adds a kernel to theirs, and must leave them alone. The functions of either file that were NOT compared
are listed. A function's position in the file numbers its local labels (.LBB<k>_<n>, .Lfunc_end<k>, the "BB<k>_<n>" of loop comments), so <k> is masked.

Two more things are numbered or laid out per translation unit and say nothing about the instructions: the .Lpost_getpc<n> labels of long branches (masked),
and the column of the trailing `;` comments, which moves with the width of the labels in front (the comparison is made with trailing comments removed;
comment-only lines stay, without their indentation). Everything else must match line for line."""
import itertools, re, sys


def normal(line):
    line = re.sub(r"\.Lpost_getpc\d+", ".Lpost_getpc<n>", line.rstrip("\n"))
    if line.lstrip().startswith(";"):
        return re.sub(r"\s+;", " ;", line.lstrip())   # (a comment-only line: kept, without its columns)
    return re.sub(r"\s*;[^\"]*$", "", line)          # (a `;` inside a quoted string is not a comment)


def body(path):
    return [normal(l) for l in open(path) if "__hip_cuid_" not in l]


def functions(lines):
    """mangled name -> lines (label to .Lfunc_end), the function's index <k> masked in its local labels"""
    out, name, buf = {}, None, []
    is_function = {m.group(1) for m in (re.match(r"^\s*\.type\s+([\w$.]+),@function", l) for l in lines) if m}
    for l in lines:
        m = re.match(r"^([A-Za-z_][\w$.]*):", l)
        if name is None and m and m.group(1) in is_function:
            name, buf = m.group(1), []
        if name is not None:
            buf.append(re.sub(r"(\.LBB|\.Lfunc_end|\.Lfunc_begin|\bBB)\d+", r"\1<k>", l))
            if l.startswith(".Lfunc_end"):
                out[name] = buf; name = None
    return out


def main(argv):
    args = [x for x in argv if not x.startswith("--")]
    only = argv[argv.index("--only") + 1].split(",") if "--only" in argv else None
    if only:
        args.remove(argv[argv.index("--only") + 1])
    a, b = body(args[0]), body(args[1])
    if only:
        fa, fb = functions(a), functions(b)
        wanted = lambda name: any(s in name for s in only)
        ka, kb = sorted(filter(wanted, fa)), sorted(filter(wanted, fb))
        for path, f in ((args[0], fa), (args[1], fb)):
            print("not compared in %s: %s" % (path, ", ".join(k[:48] for k in sorted(f) if not wanted(k)) or "(none)"))
        if not ka or ka != kb:
            print("DIFFERENT: functions matching %r: %s / %s" % (",".join(only), ka, kb))
            return 1
        print("functions compared: " + ", ".join("%s (%d lines)" % (k[:48], len(fa[k])) for k in ka))
        a = [l for k in ka for l in fa[k]]; b = [l for k in kb for l in fb[k]]
    diffs = [(i + 1, x, y) for i, (x, y) in enumerate(itertools.zip_longest(a, b)) if x != y]
    if not diffs:
        print("identical: %d lines compared (%s, %s)" % (len(a), args[0], args[1]))
        return 0
    print("DIFFERENT: %d of %d / %d compared lines (%s, %s)" % (len(diffs), len(a), len(b), args[0], args[1]))
    for i, x, y in diffs[:10]:
        print("  line %d:\n    < %s\n    > %s" % (i, x, y))
    return 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
