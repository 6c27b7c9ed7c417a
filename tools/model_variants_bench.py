#!/usr/bin/env python3
"""What do model variants cost?  GPU:  python tools/model_variants_bench.py --mode all > profiles/model_variants.txt   (docs/EXPERIMENTS.md 20)

bench.py's workloads and widths (4096 dogs on slopes_mixed, 8192 raptors on narrow_gaps, xavier weights, host terrain, the same seeds) under the protocol of
tools/policy_slots_bench.py: every comparison builds all of its batches first, pre-rolls each to a stationary reset rate, and then ALTERNATES them inside one
process, --rounds rounds (>= 3) of --steps frames each, ending in a device synchronise. Reported per configuration: median, min and max M env-steps/s and the
frame kernel's device time per launch (HIP events, dtrl_kernel_time_ms). The baseline is the plain batch: its kernels are the parent commit's, instruction
for instruction (tools/asm_same.py), so it stands for the parent.
  cost      plain batch / CreateVariants(1) (the indirection alone: every env in variant 0) / K = 8 / K = 64 / K = num_envs (one model per env) / K = 8 through the
            per-variant fallback (DTRL_VARIANTS_FALLBACK=1). Variants >= 1 are ScaledVariant draws: every body's mass and every torque limit x U(0.8, 1.2), seeded;
            envs round-robin over the variants
  counters  60 frames of the dog workload with --k variants (0 = none, -1 = one per env), the workload of a counter collection of its own, one K per process:
            rocprofv3 --pmc SQC_DCACHE_REQ SQC_DCACHE_MISSES --kernel-trace -d DIR -o pmc -- python tools/model_variants_bench.py --mode counters --k 8"""
import argparse, os, sys, time
import numpy as np
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
import bench
import deepterrainrl_amd as da
import policy_slots_bench as P


def draw_variants(b, k, seed=7):
    """variants 1 .. k - 1 of batch b: a seeded +-20 % draw of every body's mass and of the torque limits"""
    import json
    rng = np.random.RandomState(seed)
    with open(b.CharacterFile()) as f:
        names = [x["Name"] for x in json.load(f)["BodyDefs"]]
    for v in range(1, k):
        b.ScaledVariant(v, mass={nm: float(rng.uniform(0.8, 1.2)) for nm in names}, torque_lim=float(rng.uniform(0.8, 1.2)))


def make(cfg, n, k):
    """bench.py's batch; k = 0: no variants, else k variants, envs round-robin"""
    b = da.BatchScenario(cfg["arg_file"], n, data_root=bench.ROOT, extra_args=dict(P.SEEDS))
    b.SetPolicy(bench.xavier_weights(b.PolicyNumParams(), cfg["n_char"], cfg["frag"]), *bench.load_scale(cfg))
    if k:
        t0 = time.perf_counter()
        b.CreateVariants(k)
        draw_variants(b, k)
        b.AssignVariants(None, np.arange(n, dtype=np.int32) % k)
        b.load_s = time.perf_counter() - t0
    return b


def alternate(title, cfg, n, configs, a):
    """configs: [(label, k, env)]; env is set around the batch's creation AND its timed windows (the knobs are read per launch)"""
    print("## %s: %s, %d envs, %d rounds x %d frames per configuration, alternating" % (title, cfg["arg_file"], n, a.rounds, a.steps), flush=True)
    batches = []
    for label, k, env in configs:
        os.environ.update(env)
        b = make(cfg, n, k)
        pr = P.preroll(b)
        for key in env:
            del os.environ[key]
        batches.append((label, b, env, pr))
    rate = {label: [] for label, _, _, _ in batches}; kms = {label: [] for label, _, _, _ in batches}
    for r in range(a.rounds):
        for label, b, env, _ in batches:
            os.environ.update(env)
            b.KernelTimeMs()
            P.sync(); t0 = time.perf_counter()
            b.RunFrames(a.steps)
            P.sync(); dt = time.perf_counter() - t0
            for key in env:
                del os.environ[key]
            rate[label].append(n * a.steps * 20 / dt / 1e6)
            kms[label].append(b.KernelTimeMs()[0])
    for label, b, _, pr in batches:
        v = sorted(rate[label]); med = float(np.median(v))
        print("   %-44s median %7.3f  min %7.3f  max %7.3f M env-steps/s  (spread %.2f %%)  frame kernel %6.3f ms per launch  (pre-roll %d frames, %.1f resets/frame%s)"
              % (label, med, v[0], v[-1], 100 * (v[-1] - v[0]) / med, float(np.median(kms[label])), pr[0], pr[1], "; variants loaded in %.1f s" % b.load_s if hasattr(b, "load_s") else ""), flush=True)
        b.close()


def mode_cost(a):
    for c in (1, 2):
        cfg = bench.CONFIGS[c]; n = cfg["envs"]
        alternate("model variants against the plain batch", cfg, n,
                  [("plain batch (shipped kernels)", 0, {}), ("K = 1 (variant kernels, every env in variant 0)", 1, {}), ("K = 8", 8, {}), ("K = 64", 64, {}),
                   ("K = %d (one model per env)" % n, n, {}), ("K = 8, DTRL_VARIANTS_FALLBACK=1 (8 launches)", 8, {"DTRL_VARIANTS_FALLBACK": "1"})], a)


def mode_counters(a):
    """one K per process (--k; 0 = no variants, -1 = one per env), so that a counter pass attributes its launches to one configuration"""
    cfg = bench.CONFIGS[1]; n = cfg["envs"]
    b = make(cfg, n, n if a.k < 0 else a.k)
    b.RunFrames(60)
    b.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", default="all", choices=["all", "cost", "counters"])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=150)
    ap.add_argument("--k", type=int, default=8, help="(counters) number of variants, 0 = none, -1 = one per env")
    a = ap.parse_args()
    if a.rounds < 3:
        ap.error("--rounds must be at least 3")
    P.sync()   # torch's HIP context first, as in bench.py (it does not come up behind the engine's)
    print("# tools/model_variants_bench.py --mode %s --rounds %d --steps %d" % (a.mode, a.rounds, a.steps), flush=True)
    for m in (["cost"] if a.mode == "all" else [a.mode]):
        dict(cost=mode_cost, counters=mode_counters)[m](a)


if __name__ == "__main__":
    main()
