#!/usr/bin/env python3
"""What does the variant rescale cost?  GPU:  python tools/variant_rescale_bench.py > profiles/variant_rescale.txt   (docs/EXPERIMENTS.md 30)

bench.py's configs[1] and configs[2] shapes (4096 dogs on slopes_mixed, 8192 raptors on narrow_gaps, xavier weights, the same seeds) with -terrain_gen= device.
Per shape three legs, all batches built first, each pre-rolled to a stationary reset rate (bench.py's rule), then ALTERNATED inside one process: --rounds rounds
(>= 3), every round times --steps frames of every leg in turn, ending in a device synchronise. Per leg: median, min, max M env-steps/s and the spread.
  rescale       every env under its private record, mass and torque-limit factors from 0.8 .. 1.2 per episode (one launch of dtrl_variant_rescale more per group and frame)
  table redraw  the existing discrete form: 64 ScaledVariant models under seeded scales from the same ranges, VariantRedraw over the table (the yardstick)
  no variants   the plain batch
--mode trace --leg rescale|redraw|plain runs 60 frames of one leg of the dog shape and nothing else: the workload of a kernel trace of its own
  rocprofv3 --kernel-trace --stats -d DIR -o t -- python tools/variant_rescale_bench.py --mode trace --leg rescale"""
import argparse, os, sys, time
import numpy as np
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
import bench
import deepterrainrl_amd as da
from policy_slots_bench import preroll, sync, SEEDS

N_VARIANTS = 64
RANGE = (0.8, 1.2)
LEGS = ("rescale", "redraw", "plain")
LABEL = {"rescale": "rescale (private records)", "redraw": "table redraw (%d variants)" % N_VARIANTS, "plain": "no variants"}


def make(cfg, n, leg, seed=7):
    b = da.BatchScenario(cfg["arg_file"], n, data_root=bench.ROOT, extra_args=dict(SEEDS, terrain_gen="device"))
    b.SetPolicy(bench.xavier_weights(b.PolicyNumParams(), cfg["n_char"], cfg["frag"]), *bench.load_scale(cfg))
    if leg == "rescale":
        b.CreateVariants(1)
        b.VariantRescale(0, seed=seed, mass=RANGE, torque_lim=RANGE)
        b.Reset()
    elif leg == "redraw":
        b.CreateVariants(N_VARIANTS)
        rng = np.random.RandomState(seed)
        for v in range(1, N_VARIANTS):
            b.ScaledVariant(v, mass=float(rng.uniform(*RANGE)), torque_lim=float(rng.uniform(*RANGE)))
        b.AssignVariants(None, np.arange(n, dtype=np.int32) % N_VARIANTS)
        b.Reset()
        b.VariantRedraw(0, N_VARIANTS - 1, seed=seed)
    return b


def mode_rates(a):
    for c in a.configs:
        cfg = bench.CONFIGS[c]; n = cfg["envs"]
        print("## libdtrl.so, %s, %d envs, device terrain, %d rounds x %d frames per leg, alternating" % (cfg["arg_file"], n, a.rounds, a.steps), flush=True)
        batches = []
        for leg in LEGS:
            b = make(cfg, n, leg)
            batches.append((leg, b, preroll(b)))
        rate = {leg: [] for leg in LEGS}
        for r in range(a.rounds):
            for leg, b, _ in batches:
                sync(); t0 = time.perf_counter()
                b.RunFrames(a.steps)
                sync(); dt = time.perf_counter() - t0
                rate[leg].append(n * a.steps * 20 / dt / 1e6)
        med = {}
        for leg, b, pr in batches:
            v = sorted(rate[leg]); med[leg] = float(np.median(v))
            print("   %-28s median %7.3f  min %7.3f  max %7.3f M env-steps/s  (spread %.2f %%; pre-roll %d frames, %.1f resets/frame)"
                  % (LABEL[leg], med[leg], v[0], v[-1], 100 * (v[-1] - v[0]) / med[leg], pr[0], pr[1]), flush=True)
        print("   rescale / table redraw %.4f   rescale / no variants %.4f   table redraw / no variants %.4f"
              % (med["rescale"] / med["redraw"], med["rescale"] / med["plain"], med["redraw"] / med["plain"]), flush=True)
        info = batches[0][1].VariantRescaleInfo()
        print("   rescale: %d episode starts under drawn scales, most on one env %d" % (int(info["episodes"].sum()), int(info["episodes"].max())), flush=True)
        for _, b, _ in batches:
            b.close()


def mode_trace(a):
    cfg = bench.CONFIGS[1]
    b = make(cfg, cfg["envs"], a.leg)
    b.RunFrames(60)
    sync()
    b.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", default="rates", choices=["rates", "trace"])
    ap.add_argument("--leg", default="rescale", choices=list(LEGS), help="(trace) which leg")
    ap.add_argument("--configs", type=int, nargs="+", default=[1, 2], choices=sorted(bench.CONFIGS), help="bench.py config numbers (1: 4096 dogs, 2: 8192 raptors)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=150)
    a = ap.parse_args()
    if a.rounds < 3:
        ap.error("--rounds must be at least 3")
    sync()   # torch's HIP context first, as in bench.py (it does not come up behind the engine's)
    print("# tools/variant_rescale_bench.py --mode %s --rounds %d --steps %d (GPU_MAX_HW_QUEUES=%s)" % (a.mode, a.rounds, a.steps, os.environ["GPU_MAX_HW_QUEUES"]), flush=True)
    (mode_rates if a.mode == "rates" else mode_trace)(a)


if __name__ == "__main__":
    main()
