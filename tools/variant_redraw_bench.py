#!/usr/bin/env python3
"""What does the variant redraw cost?  GPU:  python tools/variant_redraw_bench.py > profiles/variant_redraw.txt   (docs/EXPERIMENTS.md, variant redraw)

bench.py's configs[1] shape (4096 dogs, args/dog_slopes_mixed_args.txt, xavier weights, the same seeds) with 64 model variants: variant 0 the nominal dog and 63
ScaledVariant tables under seeded torso-mass (0.7 .. 1.5) and torque-limit (0.6 .. 1.2) scales, the envs dealt e % 64 and reset. Per library (libdtrl.so, then
libdtrl_f32.so) four legs, all batches built first, each pre-rolled to a stationary reset rate (bench.py's rule), then ALTERNATED inside one process: --rounds rounds
(>= 3), every round times --steps frames of every leg in turn, ending in a device synchronise. Per leg: median, min, max M env-steps/s and the spread.
  host terrain,   static assignment      host terrain,   redraw on (the rule in the host's status loop, a slice upload per group-frame with a fall)
  device terrain, static assignment      device terrain, redraw on (one launch of dtrl_variant_redraw more per env group and frame)
--mode trace --leg static|redraw runs 60 frames of one device-terrain leg and nothing else: the workload of a kernel trace of its own
  rocprofv3 --kernel-trace --stats -d DIR -o t -- python tools/variant_redraw_bench.py --mode trace --leg redraw"""
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


def make(cfg, n, device_terrain, redraw, f32=False, seed=7):
    extra = dict(SEEDS)
    if device_terrain:
        extra["terrain_gen"] = "device"
    if f32:
        extra["physics_precision"] = "f32"
    b = da.BatchScenario(cfg["arg_file"], n, data_root=bench.ROOT, extra_args=extra)
    b.SetPolicy(bench.xavier_weights(b.PolicyNumParams(), cfg["n_char"], cfg["frag"]), *bench.load_scale(cfg))
    b.CreateVariants(N_VARIANTS)
    rng = np.random.RandomState(seed)
    for v in range(1, N_VARIANTS):
        b.ScaledVariant(v, mass={"torso": float(rng.uniform(0.7, 1.5))}, torque_lim=float(rng.uniform(0.6, 1.2)))
    b.AssignVariants(None, np.arange(n, dtype=np.int32) % N_VARIANTS)   # every leg starts from the same mixture
    b.Reset()
    if redraw:
        b.VariantRedraw(0, N_VARIANTS - 1, seed=seed)
    return b


def mode_rates(a):
    cfg = bench.CONFIGS[1]; n = cfg["envs"]
    for f32 in (False, True):
        print("## %s, %s, %d envs, %d variants, %d rounds x %d frames per leg, alternating" % ("libdtrl_f32.so" if f32 else "libdtrl.so", cfg["arg_file"], n, N_VARIANTS, a.rounds, a.steps), flush=True)
        batches = []
        for dev in (False, True):
            for redraw in (False, True):
                label = "%s terrain, %s" % ("device" if dev else "host", "redraw on" if redraw else "static assignment")
                b = make(cfg, n, dev, redraw, f32)
                batches.append((label, b, preroll(b)))
        rate = {label: [] for label, _, _ in batches}
        for r in range(a.rounds):
            for label, b, _ in batches:
                sync(); t0 = time.perf_counter()
                b.RunFrames(a.steps)
                sync(); dt = time.perf_counter() - t0
                rate[label].append(n * a.steps * 20 / dt / 1e6)
        med = {}
        for label, b, pr in batches:
            v = sorted(rate[label]); med[label] = float(np.median(v))
            print("   %-36s median %7.3f  min %7.3f  max %7.3f M env-steps/s  (spread %.2f %%; pre-roll %d frames, %.1f resets/frame)"
                  % (label, med[label], v[0], v[-1], 100 * (v[-1] - v[0]) / med[label], pr[0], pr[1]), flush=True)
        for k in (0, 2):
            print("   %s: redraw / static %.4f" % (batches[k][0].split(",")[0], med[batches[k + 1][0]] / med[batches[k][0]]), flush=True)
        for label, b, _ in batches:
            if "redraw" in label:
                info = b.VariantRedrawInfo()
                h = np.bincount(info["variant"], minlength=N_VARIANTS)
                print("   %s: %d draws, envs per variant min %d max %d" % (label, int(info["draws"].sum()), int(h.min()), int(h.max())), flush=True)
        for _, b, _ in batches:
            b.close()


def mode_trace(a):
    cfg = bench.CONFIGS[1]
    b = make(cfg, cfg["envs"], True, a.leg == "redraw")
    b.RunFrames(60)
    sync()
    b.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", default="rates", choices=["rates", "trace"])
    ap.add_argument("--leg", default="redraw", choices=["static", "redraw"], help="(trace) which device-terrain leg")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=150)
    a = ap.parse_args()
    if a.rounds < 3:
        ap.error("--rounds must be at least 3")
    sync()   # torch's HIP context first, as in bench.py (it does not come up behind the engine's)
    print("# tools/variant_redraw_bench.py --mode %s --rounds %d --steps %d (GPU_MAX_HW_QUEUES=%s)" % (a.mode, a.rounds, a.steps, os.environ["GPU_MAX_HW_QUEUES"]), flush=True)
    (mode_rates if a.mode == "rates" else mode_trace)(a)


if __name__ == "__main__":
    main()
