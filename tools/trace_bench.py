#!/usr/bin/env python3
"""What does the frame trace cost?
GPU:  python tools/trace_bench.py > profiles/trace.txt   (docs/EXPERIMENTS.md 35)

(a) bench.py's configs[1] and configs[2] shapes (4096 dogs / 8192 raptors, xavier weights, the same seeds) under -terrain_gen= device, where RunFrames queues
    every frame without the host looking at the batch. Three legs -- no trace, 16 envs traced, every env traced (a ring of --ring rows) -- all batches built first,
    each pre-rolled to a stationary reset rate (bench.py's rule), then ALTERNATED inside one process: --rounds rounds (>= 3), every round times --steps frames of
    every leg in turn, ending in a device synchronise. Per leg: median, min, max M env-steps/s and the spread; each traced leg against the untraced one.
(b) the two reads of the fullest ring: TraceRead (page-locked staging, then the caller's arrays) and TraceReadDevice (the caller's device tensors), ms per call.
(c) the kernel against the rule on the host (DTRL_TRACE_FALLBACK=1) in the same batch, alternated, 16 and all envs traced, record and read.
--mode launches --leg none|sixteen|all runs 60 frames of configs[1] and nothing else: the workload of a kernel trace of its own, for the launch counts
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o t -- python tools/trace_bench.py --mode launches --leg none [--parent-lib PATH/libdtrl.so]"""
import argparse, os, sys, time
import numpy as np
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
import bench
import deepterrainrl_amd as da
from policy_slots_bench import older_library, preroll, sync, SEEDS

LEGS = (("no trace", 0), ("16 envs traced", 16), ("every env traced", -1))


def make(cfg, n, traced, ring, lib=None):
    b = (older_library(lib) if lib else da.BatchScenario)(cfg["arg_file"], n, data_root=bench.ROOT, extra_args=dict(SEEDS, terrain_gen="device"))
    b.SetPolicy(bench.xavier_weights(b.PolicyNumParams(), cfg["n_char"], cfg["frag"]), *bench.load_scale(cfg))
    if traced:
        b.Trace(None if traced < 0 else list(range(0, n, n // traced))[:traced], frames=ring)   # 16 envs: spread over the batch, so over both env groups
    return b


def timed(b, n, steps):
    sync(); t0 = time.perf_counter()
    b.RunFrames(steps)
    sync(); dt = time.perf_counter() - t0
    return n * steps * 20 / dt / 1e6


def report(label, v, unit="M env-steps/s", more=""):
    v = sorted(v); med = float(np.median(v))
    print("   %-44s median %8.3f  min %8.3f  max %8.3f %s  (spread %.2f %%%s)" % (label, med, v[0], v[-1], unit, 100 * (v[-1] - v[0]) / med if med else 0.0, more), flush=True)
    return med


def ms(fn, reps):
    out = []
    for _ in range(reps):
        sync(); t0 = time.perf_counter(); fn(); sync()
        out.append(1e3 * (time.perf_counter() - t0))
    return out


def rates(a):
    for c in (1, 2):
        cfg = bench.CONFIGS[c]; n = cfg["envs"]
        print("## (a) configs[%d]: %s, %d envs, device terrain, ring %d rows, %d rounds x %d frames per leg, alternating" % (c, cfg["arg_file"], n, a.ring, a.rounds, a.steps), flush=True)
        legs = ([("parent library, no trace", dict(traced=0, lib=a.parent_lib))] if a.parent_lib else []) + [(label, dict(traced=t)) for label, t in LEGS]
        batches = []
        for label, kw in legs:
            b = make(cfg, n, ring=a.ring, **kw)
            batches.append((label, b, preroll(b)))
        rate = {label: [] for label, _, _ in batches}
        for r in range(a.rounds):
            for label, b, _ in batches:
                rate[label].append(timed(b, n, a.steps))
        med = {label: report(label, rate[label], more="; pre-roll %d frames, %.1f resets/frame" % pr) for label, b, pr in batches}
        for label, _ in legs:
            if label != "no trace":
                print("   %s / no trace: %.4f" % (label, med[label] / med["no trace"]), flush=True)
        print("## (b) configs[%d]: the two reads of the ring, ms per call (%d calls each)" % (c, a.reads), flush=True)
        for label, b, _ in batches:
            if "traced" not in label:
                continue
            info = b.TraceInfo()
            rows = int(min(info["frames"], info["rows_written"].max()))
            mb = info["n_traced"] * rows * (info["width"] * 8 + 48) / 1e6
            report("%s: TraceRead, %d rows, %.1f MB" % (label, rows, mb), ms(lambda: b.TraceRead(), a.reads), "ms")
            report("%s: TraceReadDevice" % label, ms(lambda: b.TraceReadDevice(), a.reads), "ms")
        for _, b, _ in batches:
            b.close()


def fallback(a):
    cfg = bench.CONFIGS[1]; n = cfg["envs"]
    for label, t in LEGS[1:]:
        print("## (c) the kernels against DTRL_TRACE_FALLBACK=1: configs[1], %s, one batch, %d rounds x %d frames per leg, alternating" % (label, a.rounds, a.fallback_steps), flush=True)
        b = make(cfg, n, t, a.ring)
        preroll(b)
        rate = {"one launch of dtrl_trace_record": [], "the rule on the host (DTRL_TRACE_FALLBACK=1)": []}
        read = {k: [] for k in rate}
        for r in range(a.rounds):
            for k in rate:
                os.environ.pop("DTRL_TRACE_FALLBACK", None)
                if "FALLBACK" in k:
                    os.environ["DTRL_TRACE_FALLBACK"] = "1"
                rate[k].append(timed(b, n, a.fallback_steps))
                read[k] += ms(lambda: b.TraceRead(max_rows=min(a.ring, 8)), 1)
        os.environ.pop("DTRL_TRACE_FALLBACK", None)
        med = [report(k, v) for k, v in rate.items()]
        print("   kernel / host fallback: %.2f x" % (med[0] / med[1]), flush=True)
        med = [report("TraceRead of 8 rows, " + ("kernel" if "launch" in k else "host fallback"), v, "ms") for k, v in read.items()]
        print("   host fallback / kernel, read: %.2f x" % (med[1] / med[0]), flush=True)
        b.close()


def launches(a):
    cfg = bench.CONFIGS[1]
    b = make(cfg, cfg["envs"], dict(none=0, sixteen=16, all=-1)[a.leg], a.ring, lib=a.parent_lib or None)   # (--parent-lib: with --leg none only)
    b.RunFrames(60); sync()
    print("launch-count workload done: %d envs, 60 frames, device terrain, trace: %s%s" % (cfg["envs"], a.leg, ", parent library" if a.parent_lib else ""), flush=True)
    b.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default="", help="libdtrl.so built from the parent commit")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--ring", type=int, default=64, help="rows per traced env")
    ap.add_argument("--reads", type=int, default=5)
    ap.add_argument("--fallback-steps", type=int, default=10, help="frames per leg of (c): the host fallback copies per env")
    ap.add_argument("--mode", default="all", choices=["all", "rates", "fallback", "launches"])
    ap.add_argument("--leg", default="none", choices=["none", "sixteen", "all"], help="with --mode launches")
    a = ap.parse_args()
    if a.rounds < 3:
        ap.error("--rounds must be at least 3")
    sync()   # torch's HIP context first, as in bench.py (it does not come up behind the engine's)
    print("# tools/trace_bench.py --mode %s --rounds %d --steps %d --ring %d (GPU_MAX_HW_QUEUES=%s)" % (a.mode, a.rounds, a.steps, a.ring, os.environ["GPU_MAX_HW_QUEUES"]), flush=True)
    if a.mode == "launches":
        return launches(a)
    if a.mode != "fallback":
        rates(a)
    if a.mode != "rates":
        fallback(a)


if __name__ == "__main__":
    main()
