#!/usr/bin/env python3
"""What does the episode log cost?
GPU:  python tools/episode_log_bench.py [--parent-lib PATH/libdtrl.so] > profiles/episode_log.txt   (docs/EXPERIMENTS.md 36)

bench.py's configs[1] and configs[2] shapes (4096 dogs / 8192 raptors, the same seeds) under -terrain_gen= device, where RunFrames queues every frame without the
host looking at the batch, under the committed trained policy (few episodes end) and under the seeded xavier weights (many do). Legs -- the parent commit's
library (with --parent-lib), log off, log on, and the log through the host default (DTRL_EPISODE_LOG_FALLBACK=1: per-env copies behind a stream wait, --fallback-steps
frames a window) -- all batches built first, each pre-rolled to a stationary reset rate (bench.py's rule), then ALTERNATED inside one process: --rounds rounds
(>= 3), every round times --steps frames of every leg in turn, ending in a device synchronise, and drains the log behind the window. Per leg: median, min, max
M env-steps/s and the spread, each leg against `log off`; for the logged legs the rows per frame and the drain's ms per call.
--mode launches --leg off|on runs 60 frames of configs[1] and nothing else: the workload of a kernel trace of its own, for the launch counts and the launch's own
duration:  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o t -- python tools/episode_log_bench.py --mode launches --leg on"""
import argparse, os, sys, time
import numpy as np
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
import bench
import deepterrainrl_amd as da
from policy_slots_bench import older_library, preroll, sync, SEEDS

KNOB = "DTRL_EPISODE_LOG_FALLBACK"


def make(c, policy, capacity, lib=None):
    cfg = bench.CONFIGS[c]; n = cfg["envs"]
    b = (older_library(lib) if lib else da.BatchScenario)(cfg["arg_file"], n, data_root=bench.ROOT, extra_args=dict(SEEDS, terrain_gen="device"))
    if policy == "trained":
        b.LoadModel(os.path.join(REPO, bench.TRAINED_POLICY[c]))
    else:
        b.SetPolicy(bench.xavier_weights(b.PolicyNumParams(), cfg["n_char"], cfg["frag"]), *bench.load_scale(cfg))
    if capacity:
        b.EpisodeLog(capacity)
    return b


def timed(b, n, steps, fallback):
    os.environ.pop(KNOB, None)
    if fallback:
        os.environ[KNOB] = "1"
    sync(); t0 = time.perf_counter()
    b.RunFrames(steps)
    sync(); dt = time.perf_counter() - t0
    os.environ.pop(KNOB, None)
    return n * steps * 20 / dt / 1e6


def report(label, v, unit="M env-steps/s", more=""):
    v = sorted(v); med = float(np.median(v))
    print("   %-52s median %8.3f  min %8.3f  max %8.3f %s  (spread %.2f %%%s)" % (label, med, v[0], v[-1], unit, 100 * (v[-1] - v[0]) / med if med else 0.0, more), flush=True)
    return med


def rates(a):
    for c in (1, 2):
        for policy in ("trained", "xavier"):
            cfg = bench.CONFIGS[c]; n = cfg["envs"]
            print("## configs[%d]: %s, %d envs, %s policy, device terrain, rings of %d rows, %d rounds x %d frames per leg (fallback: %d), alternating"
                  % (c, cfg["arg_file"], n, policy, a.capacity, a.rounds, a.steps, a.fallback_steps), flush=True)
            legs = ([("parent library", dict(capacity=0, lib=a.parent_lib), False)] if a.parent_lib else []) + [("log off", dict(capacity=0), False), ("log on", dict(capacity=a.capacity), False),
                    ("log on, host default (%s=1)" % KNOB, dict(capacity=a.capacity), True)]
            batches = []
            for label, kw, fb in legs:
                b = make(c, policy, **kw)
                batches.append((label, b, fb, preroll(b)))
            rate = {label: [] for label, _, _, _ in batches}
            rows = {label: [] for label, _, _, _ in batches}
            drain_ms = {label: [] for label, _, _, _ in batches}
            for label, b, fb, _ in batches:
                if "log on" in label:
                    b.EpisodeLogDrain()                     # (the pre-roll's rows)
            for r in range(a.rounds):
                for label, b, fb, _ in batches:
                    steps = a.fallback_steps if fb else a.steps
                    rate[label].append(timed(b, n, steps, fb))
                    if "log on" in label:
                        t0 = time.perf_counter(); d = b.EpisodeLogDrain(); drain_ms[label].append(1e3 * (time.perf_counter() - t0))
                        rows[label].append((len(d["env"]) + d["lost"]) / float(steps))
            med = {label: report(label, rate[label], more="; pre-roll %d frames, %.1f resets/frame" % pr) for label, b, fb, pr in batches}
            for label, b, _, _ in batches:
                if label != "log off":
                    print("   %s / log off: %.4f" % (label, med[label] / med["log off"]), flush=True)
                if "log on" in label:
                    print("   %s: %.1f rows per frame; drain %.3f ms per call (median), %d rows lost" % (label, float(np.median(rows[label])), float(np.median(drain_ms[label])), b.EpisodeLogInfo()["lost"]), flush=True)
            for _, b, _, _ in batches:
                b.close()


def launches(a):
    b = make(1, a.policy, a.capacity if a.leg == "on" else 0, lib=a.parent_lib or None)   # (--parent-lib: with --leg off only)
    b.RunFrames(60); sync()
    n = len(b.EpisodeLogDrain()["env"]) if a.leg == "on" else 0
    print("launch-count workload done: %d envs, 60 frames, device terrain, %s policy, log %s%s, %d rows" % (bench.CONFIGS[1]["envs"], a.policy, a.leg, ", parent library" if a.parent_lib else "", n), flush=True)
    b.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default="", help="libdtrl.so built from the parent commit")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--capacity", type=int, default=65536, help="rows per ring")
    ap.add_argument("--fallback-steps", type=int, default=5, help="frames per window of the host-default leg: it copies per env")
    ap.add_argument("--mode", default="rates", choices=["rates", "launches"])
    ap.add_argument("--leg", default="off", choices=["off", "on"], help="with --mode launches")
    ap.add_argument("--policy", default="xavier", choices=["xavier", "trained"], help="with --mode launches")
    a = ap.parse_args()
    if a.rounds < 3:
        ap.error("--rounds must be at least 3")
    sync()   # torch's HIP context first, as in bench.py (it does not come up behind the engine's)
    print("# tools/episode_log_bench.py --mode %s --rounds %d --steps %d --capacity %d (GPU_MAX_HW_QUEUES=%s)" % (a.mode, a.rounds, a.steps, a.capacity, os.environ["GPU_MAX_HW_QUEUES"]), flush=True)
    return launches(a) if a.mode == "launches" else rates(a)


if __name__ == "__main__":
    main()
