#!/usr/bin/env python3
"""What do policy slots cost?  GPU:  python tools/policy_slots_bench.py --mode all [--parent-lib DIR] > profiles/policy_slots.txt   (docs/EXPERIMENTS.md 18)

bench.py's workloads and widths (4096 dogs on slopes_mixed, 8192 raptors on narrow_gaps, xavier weights, host terrain, the same seeds). Every comparison builds all
of its batches first, pre-rolls each to a stationary reset rate (bench.py's rule), and then ALTERNATES them inside one process: --rounds rounds (>= 3), every
round times --steps frames of every configuration in turn, ending in a device synchronise. Reported per configuration: median, min and max M env-steps/s.
  k1        the price of the indirection: no slots (the shipped kernels) / CreateSlots(1) (the slot kernels, one slot) / -- with --parent-lib DIR, a directory that
            holds the parent commit's libdtrl.so -- the parent's library, same process
  sweep     K = 1, 2, 4, 8, 16 distinct weight sets (xavier seeds), envs round-robin over the slots
  fallback  K = 8: one launch of the slot kernels / per-slot launches of the shipped kernels (DTRL_SLOTS_FALLBACK=1)
  stats     dtrl_slot_stats (device reduction) / dtrl_eval_stats (D2H of every EnvState record) at 8192 raptors, per call, ending in a synchronise
  eval      tools/eval_policies.py's evaluate_many on 8 sets of weights (the three golden policies and xavier seeds) in one batch / 8 x learn_curve.evaluate; the per-model
            figures must be identical
  counters  60 frames of the dog workload with --k slots (0 = none), the workload of a counter collection of its own, one K per process:
            rocprofv3 --pmc FETCH_SIZE --kernel-trace -d DIR -o pmc -- python tools/policy_slots_bench.py --mode counters --k 8     (then tools/pmc_avg.py DIR)"""
import argparse, os, sys, time
import numpy as np
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
import bench
import deepterrainrl_amd as da

SEEDS = dict(terrain_seed=20260925, rand_seed=1)


def sync():
    import torch
    torch.cuda.synchronize()


def older_library(path):
    """BatchScenario on another build of libdtrl.so -- the parent commit's, which lacks the entry points this commit adds: those bind to a stub that is never called"""
    import ctypes

    class Stub:
        argtypes = restype = None

    class Tolerant(ctypes.CDLL):
        def __getattr__(self, name):
            try:
                return super().__getattr__(name)
            except AttributeError:
                if not name.startswith("dtrl_"):
                    raise
                return Stub()

    class Older(da.BatchScenario):
        def _library(self):
            keep = da.C.CDLL
            da.C.CDLL = Tolerant
            try:
                return da._bind(path)
            finally:
                da.C.CDLL = keep
    return Older


def make(cfg, n, k_slots, lib=None, explore=None):
    """bench.py's batch; k_slots = 0: no slots, else k_slots slots with distinct xavier weights, envs round-robin"""
    b = (older_library(lib) if lib else da.BatchScenario)(cfg["arg_file"], n, data_root=bench.ROOT, extra_args=dict(SEEDS))
    scale = bench.load_scale(cfg)
    if k_slots:
        b.CreateSlots(k_slots)
    b.SetPolicy(bench.xavier_weights(b.PolicyNumParams(), cfg["n_char"], cfg["frag"]), *scale)
    for s in range(1, k_slots):
        b.SlotSetPolicy(s, bench.xavier_weights(b.PolicyNumParams(), cfg["n_char"], cfg["frag"], seed=1234 + s), *scale)
    if k_slots:
        b.AssignSlots(None, np.arange(n, dtype=np.int32) % k_slots)
    return b


def preroll(b):
    done = 0; rates = []; r_prev = b.EvalStats()["resets"]
    while done < bench.PREROLL_MAX:
        b.RunFrames(bench.PREROLL_BLOCK); done += bench.PREROLL_BLOCK
        r = b.EvalStats()["resets"]; rates.append((r - r_prev) / float(bench.PREROLL_BLOCK)); r_prev = r
        if done >= bench.PREROLL_MIN and len(rates) >= 2 and rates[-1] > 0 and abs(rates[-1] - rates[-2]) <= 0.25 * max(rates[-1], rates[-2]):
            break
    b.RunFrames(10)
    return done, rates[-1]


def alternate(title, cfg, n, configs, a):
    """configs: [(label, make-kwargs, env)]; env is set around the batch's creation AND its timed windows (the knobs are read per launch)"""
    print("## %s: %s, %d envs, %d rounds x %d frames per configuration, alternating" % (title, cfg["arg_file"], n, a.rounds, a.steps), flush=True)
    batches = []
    for label, kw, env in configs:
        os.environ.update(env)
        b = make(cfg, n, **kw)
        pr = preroll(b)
        for k in env:
            del os.environ[k]
        batches.append((label, b, env, pr))
    rate = {label: [] for label, _, _, _ in batches}
    for r in range(a.rounds):
        for label, b, env, _ in batches:
            os.environ.update(env)
            sync(); t0 = time.perf_counter()
            b.RunFrames(a.steps)
            sync(); dt = time.perf_counter() - t0
            for k in env:
                del os.environ[k]
            rate[label].append(n * a.steps * 20 / dt / 1e6)
    out = {}
    for label, b, _, pr in batches:
        v = sorted(rate[label]); med = float(np.median(v))
        out[label] = med
        print("   %-44s median %7.3f  min %7.3f  max %7.3f M env-steps/s  (spread %.2f %%; pre-roll %d frames, %.1f resets/frame)" % (label, med, v[0], v[-1], 100 * (v[-1] - v[0]) / med, pr[0], pr[1]), flush=True)
        b.close()
    return out


def mode_k1(a):
    for c in (1, 2):
        cfg = bench.CONFIGS[c]
        configs = [("no slots (shipped kernels)", dict(k_slots=0), {}), ("CreateSlots(1) (slot kernels)", dict(k_slots=1), {})]
        if a.parent_lib:
            configs.append(("parent commit's library (shipped kernels)", dict(k_slots=0, lib=os.path.join(os.path.abspath(a.parent_lib), "libdtrl.so")), {}))
        alternate("K = 1 through the slot kernels against the shipped kernels", cfg, cfg["envs"], configs, a)


def mode_sweep(a):
    for c in (1, 2):
        cfg = bench.CONFIGS[c]
        alternate("K distinct weight sets, round-robin", cfg, cfg["envs"], [("K = %d" % k, dict(k_slots=k), {}) for k in (1, 2, 4, 8, 16)], a)


def mode_fallback(a):
    for c in (1, 2):
        cfg = bench.CONFIGS[c]
        alternate("K = 8, one launch against per-slot launches", cfg, cfg["envs"],
                  [("one launch (slot kernels)", dict(k_slots=8), {}), ("DTRL_SLOTS_FALLBACK=1 (8 launches, shipped kernels)", dict(k_slots=8), {"DTRL_SLOTS_FALLBACK": "1"})], a)


def mode_stats(a):
    cfg = bench.CONFIGS[2]; n = cfg["envs"]
    b = make(cfg, n, 8)
    b.RunFrames(60)
    t = {"SlotStats (8 slots: 8 calls)": [], "SlotStats (one slot: 1 call)": [], "EvalStats": []}
    for r in range(max(a.rounds, 5)):
        sync(); t0 = time.perf_counter(); [b.SlotStats(s) for s in range(8)]; sync(); t["SlotStats (8 slots: 8 calls)"].append(time.perf_counter() - t0)
        sync(); t0 = time.perf_counter(); b.SlotStats(3); sync(); t["SlotStats (one slot: 1 call)"].append(time.perf_counter() - t0)
        sync(); t0 = time.perf_counter(); b.EvalStats(); sync(); t["EvalStats"].append(time.perf_counter() - t0)
    print("## per-slot statistics at %d envs (%s), %d rounds, alternating; time per line, ending in a synchronise" % (n, cfg["arg_file"], len(t["EvalStats"])))
    for k, v in t.items():
        v = sorted(v)
        print("   %-32s median %8.3f ms  min %8.3f  max %8.3f" % (k, 1e3 * float(np.median(v)), 1e3 * v[0], 1e3 * v[-1]))
    b.close()


def mode_eval(a):
    import eval_policies, learn_curve
    gold = os.path.join(REPO, "tests", "golden", "policies")
    arg = learn_curve.CHARS["dog"]["evalf"]
    probe = da.BatchScenario(arg, 1, data_root=bench.ROOT)
    pols = [eval_policies.load_policy(probe, os.path.join(gold, m)) for m in ("dog_mace3_slopes_mixed_model.h5", "goat_mace3_cliffs_model.h5")]
    cfg = bench.CONFIGS[1]
    pols += [(bench.xavier_weights(probe.PolicyNumParams(), cfg["n_char"], cfg["frag"], seed=1234 + s), tuple(bench.load_scale(cfg))) for s in range(6)]
    probe.close()
    names = ["dog (trained)", "goat (trained, on the dog's scene)"] + ["xavier seed %d" % (1234 + s) for s in range(6)]
    tm, te = [], []
    for r in range(a.rounds):
        sync(); t0 = time.perf_counter(); many = learn_curve.evaluate_many(arg, bench.ROOT, pols, a.eval_envs, a.eval_frames); sync(); tm.append(time.perf_counter() - t0)
        sync(); t0 = time.perf_counter(); each = [learn_curve.evaluate(arg, bench.ROOT, w, norm, a.eval_envs, a.eval_frames) for w, norm in pols]; sync(); te.append(time.perf_counter() - t0)
    same = all(eval_policies.same(x, y) for x, y in zip(many, each))
    print("## 8 policies x %d envs x %d frames of %s (the raptor's golden policy is another net shape and cannot share a batch with these), %d rounds, alternating" % (a.eval_envs, a.eval_frames, arg, a.rounds))
    print("   one slotted batch (evaluate_many)      median %7.2f s  min %7.2f  max %7.2f" % (float(np.median(tm)), min(tm), max(tm)))
    print("   8 x learn_curve.evaluate               median %7.2f s  min %7.2f  max %7.2f" % (float(np.median(te)), min(te), max(te)))
    print("   per-model figures: %s" % ("identical" if same else "DIFFERENT"))
    for nme, r in zip(names, many):
        print("   %-36s speed %6.3f  falls_k %6.3f  avg_dist %8.3f  alive %5.3f  episodes %5d  cycles %6d" % (nme, r["speed"], r["falls_k"], r["avg_dist"], r["alive"], r["episodes"], r["cycles"]))
    if not same:
        sys.exit(1)


def mode_counters(a):
    """one K per process (--k; 0 = no slots), so that a counter pass attributes its launches to one configuration"""
    cfg = bench.CONFIGS[1]
    b = make(cfg, cfg["envs"], a.k)
    b.RunFrames(60)
    b.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", default="all", choices=["all", "k1", "sweep", "fallback", "stats", "eval", "counters"])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=150)
    ap.add_argument("--eval-envs", type=int, default=512)
    ap.add_argument("--eval-frames", type=int, default=300)
    ap.add_argument("--k", type=int, default=8, help="(counters) number of slots, 0 = none")
    ap.add_argument("--parent-lib", default="", help="directory with the parent commit's libdtrl.so (k1)")
    a = ap.parse_args()
    if a.rounds < 3:
        ap.error("--rounds must be at least 3")
    modes = dict(k1=mode_k1, sweep=mode_sweep, fallback=mode_fallback, stats=mode_stats, eval=mode_eval, counters=mode_counters)
    sync()   # torch's HIP context first, as in bench.py (it does not come up behind the engine's)
    print("# tools/policy_slots_bench.py --mode %s --rounds %d --steps %d" % (a.mode, a.rounds, a.steps), flush=True)
    for m in (["k1", "sweep", "fallback", "stats", "eval"] if a.mode == "all" else [a.mode]):
        modes[m](a)


if __name__ == "__main__":
    main()
