#!/usr/bin/env python3
"""What does the push schedule cost, and what does dtrl_add_perturb in one launch save?
GPU:  python tools/push_schedule_bench.py --parent-lib PATH/libdtrl.so > profiles/push_schedule.txt   (docs/EXPERIMENTS.md, push schedule)

(a) bench.py's configs[1] shape (4096 dogs, args/dog_slopes_mixed_args.txt, xavier weights, the same seeds). Per terrain mode four legs, all batches built first,
    each pre-rolled to a stationary reset rate (bench.py's rule), then ALTERNATED inside one process: --rounds rounds (>= 3), every round times --steps frames of
    every leg in turn, ending in a device synchronise. Per leg: median, min, max M env-steps/s, the spread, and falls per frame inside the timed windows.
      parent library, no schedule      (--parent-lib: a build of the parent commit; left out when not given)
      this library, no schedule        (queues what the parent queues)
      this library, schedule, 0 N      (one launch of dtrl_push_schedule more per env group and frame, slots written, the workload unchanged: the launch's cost)
      this library, schedule, pushes   (the arg file's 50 .. 100 N for 0.1 .. 0.5 s every --wait frames: another workload -- more falls)
(b) dtrl_add_perturb for all 4096 envs: the one launch against the per-env copy loop it replaces (DTRL_PERTURB_FALLBACK=1) in the same library, alternated; wall
    time per call."""
import argparse, os, sys, time
import numpy as np
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
import bench
import deepterrainrl_amd as da
from policy_slots_bench import older_library, preroll, sync, SEEDS


def make(cfg, n, device_terrain, lib=None, schedule=None, wait=(30, 90)):
    extra = dict(SEEDS)
    if device_terrain:
        extra["terrain_gen"] = "device"
    b = (older_library(lib) if lib else da.BatchScenario)(cfg["arg_file"], n, data_root=bench.ROOT, extra_args=extra)
    b.SetPolicy(bench.xavier_weights(b.PolicyNumParams(), cfg["n_char"], cfg["frag"]), *bench.load_scale(cfg))
    if schedule == "zero":
        b.PushSchedule(wait, seed=7, force=(0.0, 0.0))
    elif schedule == "pushes":
        b.PushSchedule(wait, seed=7)
    return b


def rates(a):
    cfg = bench.CONFIGS[1]; n = cfg["envs"]
    for dev in (False, True):
        print("## (a) %s terrain: %s, %d envs, %d rounds x %d frames per leg, alternating; a push every %d .. %d frames" % ("device" if dev else "host", cfg["arg_file"], n, a.rounds, a.steps, a.wait[0], a.wait[1]), flush=True)
        legs = ([("parent library, no schedule", dict(lib=a.parent_lib))] if a.parent_lib else []) + [
            ("this library, no schedule", {}), ("this library, schedule, 0 N", dict(schedule="zero")), ("this library, schedule, pushes", dict(schedule="pushes"))]
        batches = []
        for label, kw in legs:
            b = make(cfg, n, dev, wait=tuple(a.wait), **kw)
            batches.append((label, b, preroll(b)))
        rate = {label: [] for label, _, _ in batches}
        falls = {label: 0 for label, _, _ in batches}
        for r in range(a.rounds):
            for label, b, _ in batches:
                r0 = b.EvalStats()["resets"]
                sync(); t0 = time.perf_counter()
                b.RunFrames(a.steps)
                sync(); dt = time.perf_counter() - t0
                rate[label].append(n * a.steps * 20 / dt / 1e6)
                falls[label] += b.EvalStats()["resets"] - r0
        med = {}
        for label, b, pr in batches:
            v = sorted(rate[label]); med[label] = float(np.median(v))
            print("   %-34s median %7.3f  min %7.3f  max %7.3f M env-steps/s  (spread %.2f %%; %.1f falls/frame; pre-roll %d frames)"
                  % (label, med[label], v[0], v[-1], 100 * (v[-1] - v[0]) / med[label], falls[label] / float(a.rounds * a.steps), pr[0]), flush=True)
        base = med[legs[0][0]]
        for label, _ in legs[1:]:
            print("   %s / %s: %.4f" % (label, legs[0][0], med[label] / base), flush=True)
        for label, b, _ in batches:
            if "schedule," in label:
                print("   %s: %d pushes" % (label, int(b.PushInfo()["pushes"].sum())), flush=True)
        for _, b, _ in batches:
            b.close()


def add_perturb(a):
    cfg = bench.CONFIGS[1]; n = cfg["envs"]
    print("## (b) dtrl_add_perturb for all %d envs, %d rounds x %d calls per leg, alternating" % (n, a.rounds, a.calls), flush=True)
    b = make(cfg, n, False)
    b.RunFrames(5)
    rng = np.random.RandomState(3)
    link = rng.randint(0, b.L, size=n).astype(np.int32); force = rng.uniform(-80, 80, size=(n, 2)); dur = rng.uniform(0.1, 0.4, size=n); lp = rng.uniform(-0.05, 0.05, size=(n, 2))
    times = {"one launch": [], "per-env copy loop (DTRL_PERTURB_FALLBACK=1)": []}
    for r in range(a.rounds):
        for label in times:
            os.environ.pop("DTRL_PERTURB_FALLBACK", None)
            if "FALLBACK" in label:
                os.environ["DTRL_PERTURB_FALLBACK"] = "1"
            for _ in range(a.calls):
                sync(); t0 = time.perf_counter()
                b.AddPerturb(link, force, dur, local_pos=lp)
                times[label].append(time.perf_counter() - t0)
    os.environ.pop("DTRL_PERTURB_FALLBACK", None)
    med = {}
    for label, v in times.items():
        v = sorted(v); med[label] = float(np.median(v))
        print("   %-48s median %10.3f ms  min %10.3f  max %10.3f" % (label, 1e3 * med[label], 1e3 * v[0], 1e3 * v[-1]), flush=True)
    k = list(times)
    print("   %s / %s: %.1f x" % (k[1], k[0], med[k[1]] / med[k[0]]), flush=True)
    b.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default="", help="libdtrl.so built from the parent commit")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=150)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--wait", type=int, nargs=2, default=[30, 90], metavar=("LO", "HI"))
    ap.add_argument("--only", default="", choices=["", "rates", "add_perturb"])
    a = ap.parse_args()
    if a.rounds < 3:
        ap.error("--rounds must be at least 3")
    sync()   # torch's HIP context first, as in bench.py (it does not come up behind the engine's)
    print("# tools/push_schedule_bench.py --rounds %d --steps %d --wait %d %d (GPU_MAX_HW_QUEUES=%s)" % (a.rounds, a.steps, a.wait[0], a.wait[1], os.environ["GPU_MAX_HW_QUEUES"]), flush=True)
    if a.only != "add_perturb":
        rates(a)
    if a.only != "rates":
        add_perturb(a)


if __name__ == "__main__":
    main()
