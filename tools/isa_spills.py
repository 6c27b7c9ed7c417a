#!/usr/bin/env python3
"""Static check of a hipcc -S dump: spill instructions per loop nest of one kernel.
Two kinds of spill are counted:
  scratch   scratch_* instructions (VGPRs spilled to scratch memory)
  wl / rl   SGPR spills to VGPR lanes: every v_writelane_b32 (the store), and every v_readlane_b32 whose source VGPR is the target of a v_writelane_b32
            of the same function (the reload; a v_readlane of any other VGPR is a broadcast of lane data and is not counted)
The VGPRs that v_writelane_b32 targets are the ones reserved for SGPR spills; they are listed with the totals.
Memory round trips: gload = global_load_* instructions, vmwait = s_waitcnt instructions that wait on vmcnt (each one a point where the wave may stand still for a
trip to memory: a chain of load, wait, load, wait shows as vmwait close to gload). lgkmwait = s_waitcnt instructions that wait on lgkmcnt (LDS and scalar-memory
round trips, counted the same way).
A loop's "own" columns count the blocks whose innermost loop it is, the "nest" columns add every loop nested in it (the substep loop of the frame kernel is the
depth-2 loop with the largest nest).
Usage: tools/isa_spills.py file.s kernel_substring"""
import re, sys, collections

COLS = ("instr", "valu", "salu", "scratch", "wl", "rl", "gload", "vmwait", "lgkmwait")


def parse(src, key):
    """(own, parents, depth, spill_vgprs) of the functions whose label contains `key`: own[loop header or "-"] = Counter of the blocks whose innermost loop it is,
    parents[loop header] = headers of the loops around it, depth[loop header], spill_vgprs = the v_writelane targets"""
    body = []; inside = False
    for line in open(src):
        if re.match(r"^[A-Za-z_][\w.$]*:", line) and not line.startswith(".L"):
            inside = key in line
        if inside: body.append(line)
    spill_vgprs = set()
    for line in body:
        m = re.match(r"\s*v_writelane_b32\s+(v\d+)\s*,", line)
        if m: spill_vgprs.add(m.group(1))
    own = collections.defaultdict(collections.Counter); parents = {}; depth = {"-": 0}
    cur = "-"; hdr = None
    for line in body:
        if line.startswith(".LBB") or line.startswith("; %bb"):
            m = re.search(r"in Loop: Header=(\S+) Depth=(\d+)", line)
            cur = m.group(1) if m else "-"
            if m: depth[cur] = int(m.group(2))
            hdr = None
            if line.startswith(".LBB") and not m:   # maybe a loop header: its comment lines follow (parent loops outermost first, then the header line)
                hdr = (line.split(":")[0][2:], [])
                m2 = re.search(r"Parent Loop (\S+) Depth=\d+", line)
                if m2: hdr[1].append(m2.group(1))
                m3 = re.search(r"Loop Header: Depth=(\d+)", line)
                if m3: cur = hdr[0]; depth[cur] = int(m3.group(1)); parents[cur] = list(hdr[1]); hdr = None
            continue
        if hdr is not None and line.lstrip().startswith(";"):
            m2 = re.search(r"Parent Loop (\S+) Depth=\d+", line)
            if m2: hdr[1].append(m2.group(1))
            m3 = re.search(r"Loop Header: Depth=(\d+)", line)
            if m3: cur = hdr[0]; depth[cur] = int(m3.group(1)); parents[cur] = list(hdr[1]); hdr = None
            continue
        s = line.strip()
        t = s.split(" ")[0] if s else ""
        if not re.match(r"^(v_|s_|ds_|global_|scratch_|flat_|buffer_)", t): continue
        hdr = None
        c = own[cur]
        c["instr"] += 1
        if t.startswith("v_"): c["valu"] += 1
        if t.startswith("s_"): c["salu"] += 1
        if t.startswith("scratch_"): c["scratch"] += 1
        if t.startswith("global_load_"): c["gload"] += 1
        if t == "s_waitcnt" and "vmcnt" in s: c["vmwait"] += 1
        if t == "s_waitcnt" and "lgkmcnt" in s: c["lgkmwait"] += 1
        if t == "v_writelane_b32": c["wl"] += 1
        if t == "v_readlane_b32":
            m = re.match(r"v_readlane_b32\s+\S+\s*,\s*(v\d+)\s*,", s)
            if m and m.group(1) in spill_vgprs: c["rl"] += 1
    return own, parents, depth, spill_vgprs


def main():
    src, key = sys.argv[1], sys.argv[2]
    own, parents, depth, spill_vgprs = parse(src, key)
    nest = collections.defaultdict(collections.Counter)
    for k, c in own.items():
        for a in [k] + parents.get(k, []): nest[a].update(c)
    tot = collections.Counter()
    for c in own.values(): tot.update(c)
    print("kernel *%s*: %d instr, %d VALU, %d SALU, %d scratch, %d v_writelane (SGPR spill stores), %d v_readlane of spill VGPRs (SGPR spill reloads), %d global loads, %d vmcnt waits, %d lgkmcnt waits"
          % ((key,) + tuple(tot[k] for k in COLS)))
    vs = sorted(spill_vgprs, key=lambda v: int(v[1:]))
    print("VGPRs reserved for SGPR spills: %d (%s)" % (len(vs), " ".join(vs)))
    print("%-12s %5s | %s | %s" % ("loop", "depth", " ".join("%8s" % k for k in COLS), " ".join("%8s" % k for k in COLS)))
    print("%-12s %5s | %-72s | %s" % ("", "", "own blocks", "nest (with the loops inside it)"))
    for k, c in sorted(nest.items(), key=lambda kv: -kv[1]["instr"])[:25]:
        if k == "-": continue
        print("%-12s %5d | %s | %s" % (k, depth.get(k, 0), " ".join("%8d" % own[k][x] for x in COLS), " ".join("%8d" % c[x] for x in COLS)))
    print("%-12s %5d | %s |" % ("(no loop)", 0, " ".join("%8d" % own["-"][x] for x in COLS)))


if __name__ == "__main__":
    main()
