#!/usr/bin/env python3
"""What do terrain sets cost?  GPU:  python tools/terrain_sets_bench.py [--parent-lib DIR] > profiles/terrain_sets.txt   (docs/EXPERIMENTS.md, terrain sets)

bench.py's configs[1] shape (4096 dogs, args/dog_slopes_mixed_args.txt, xavier weights, the same seeds), once with -terrain_gen= device and once with host terrain.
Every comparison builds all of its batches first, pre-rolls each to a stationary reset rate (bench.py's rule), and then ALTERNATES them inside one process: --rounds
rounds (>= 3), every round times --steps frames of every configuration in turn, ending in a device synchronise. Per configuration: median, min, max M env-steps/s.
  no terrains                 the batch never calls CreateTerrains: the launches it always ran (device terrain: dtrl_terrain_boundary)
  parent commit's library     the same batch on the parent commit's libdtrl.so (--parent-lib DIR: a directory that holds it): what the no-terrain rate is held against
  terrains, all in terrain 0  CreateTerrains(4), every env left in terrain 0 (device terrain: dtrl_terrain_boundary_keyed, one type in every wavefront)
  four terrains mixed         slopes_mixed / narrow_gaps / cliffs_rugged / flat dealt e % 4 with restart (device terrain: the lanes of a wavefront part ways by type)
  ... DTRL_TERRAINS_FALLBACK=1  the same through the host default of Backend::TerrainBoundary (device terrain only; --fallback-steps frames per round: it is slow)
--mode trace --variant none|zero|mixed runs 60 frames of one device-terrain variant and nothing else: the workload of a kernel trace of its own
  rocprofv3 --kernel-trace --stats -d DIR -o t -- python tools/terrain_sets_bench.py --mode trace --variant mixed"""
import argparse, os, sys, time
import numpy as np
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
import bench
import deepterrainrl_amd as da
from policy_slots_bench import older_library, preroll, sync, SEEDS

TERRAINS = ["data/terrain/narrow_gaps.txt", "data/terrain/cliffs_rugged.txt", "data/terrain/flat.txt"]   # terrains 1 .. 3; terrain 0 is the arg file's slopes_mixed


def make(cfg, n, variant, extra, lib=None):
    """variant: none (no CreateTerrains) / zero (4 terrains, every env in terrain 0) / mixed (e % 4, with restart)"""
    b = (older_library(lib) if lib else da.BatchScenario)(cfg["arg_file"], n, data_root=bench.ROOT, extra_args=dict(SEEDS, **extra))
    b.SetPolicy(bench.xavier_weights(b.PolicyNumParams(), cfg["n_char"], cfg["frag"]), *bench.load_scale(cfg))
    if variant != "none":
        b.CreateTerrains(1 + len(TERRAINS))
        for t, f in enumerate(TERRAINS):
            b.SetTerrainFile(1 + t, f)
    if variant == "mixed":
        b.AssignTerrains(None, np.arange(n, dtype=np.int32) % (1 + len(TERRAINS)), restart=True)
    return b


def alternate(title, cfg, n, configs, a):
    """configs: [(label, make-kwargs, env, frames per round)]; env is set around the batch's creation AND its timed windows (the knob is read per launch)"""
    print("## %s: %s, %d envs, %d rounds, alternating" % (title, cfg["arg_file"], n, a.rounds), flush=True)
    batches = []
    for label, kw, env, steps in configs:
        os.environ.update(env)
        b = make(cfg, n, **kw)
        pr = preroll(b) if not env else (0, 0.0)
        if env:
            b.RunFrames(steps)
        for k in env:
            del os.environ[k]
        batches.append((label, b, env, steps, pr))
    rate = {c[0]: [] for c in batches}
    for r in range(a.rounds):
        for label, b, env, steps, _ in batches:
            os.environ.update(env)
            sync(); t0 = time.perf_counter()
            b.RunFrames(steps)
            sync(); dt = time.perf_counter() - t0
            for k in env:
                del os.environ[k]
            rate[label].append(n * steps * 20 / dt / 1e6)
    out = {}
    for label, b, _, steps, pr in batches:
        v = sorted(rate[label]); med = float(np.median(v)); out[label] = med
        print("   %-52s median %7.3f  min %7.3f  max %7.3f M env-steps/s  (%d frames per round; spread %.2f %%; pre-roll %d frames, %.1f resets/frame)"
              % (label, med, v[0], v[-1], steps, 100 * (v[-1] - v[0]) / med, pr[0], pr[1]), flush=True)
        b.close()
    return out


def mode_rates(a):
    cfg = bench.CONFIGS[1]; n = cfg["envs"]
    for name, extra in (("-terrain_gen= device", dict(terrain_gen="device")), ("host terrain", {})):
        configs = [("no terrains", dict(variant="none", extra=extra), {}, a.steps)]
        if a.parent_lib:
            configs.append(("parent commit's library (no terrains)", dict(variant="none", extra=extra, lib=os.path.join(os.path.abspath(a.parent_lib), "libdtrl.so")), {}, a.steps))
        configs.append(("terrains created, all envs in terrain 0", dict(variant="zero", extra=extra), {}, a.steps))
        configs.append(("four terrains mixed e % 4", dict(variant="mixed", extra=extra), {}, a.steps))
        if extra:
            configs.append(("four terrains mixed, DTRL_TERRAINS_FALLBACK=1", dict(variant="mixed", extra=extra), {"DTRL_TERRAINS_FALLBACK": "1"}, a.fallback_steps))
        out = alternate(name, cfg, n, configs, a)
        if a.parent_lib:
            print("   no terrains / parent commit's library: %.4f" % (out["no terrains"] / out["parent commit's library (no terrains)"]), flush=True)


def mode_trace(a):
    cfg = bench.CONFIGS[1]
    b = make(cfg, cfg["envs"], a.variant, dict(terrain_gen="device"))
    b.RunFrames(60)
    sync()
    b.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", default="rates", choices=["rates", "trace"])
    ap.add_argument("--variant", default="mixed", choices=["none", "zero", "mixed"], help="(trace) which batch")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=150)
    ap.add_argument("--fallback-steps", type=int, default=5)
    ap.add_argument("--parent-lib", default="", help="directory with the parent commit's libdtrl.so")
    a = ap.parse_args()
    if a.rounds < 3:
        ap.error("--rounds must be at least 3")
    sync()   # torch's HIP context first, as in bench.py (it does not come up behind the engine's)
    print("# tools/terrain_sets_bench.py --mode %s --rounds %d --steps %d" % (a.mode, a.rounds, a.steps), flush=True)
    (mode_rates if a.mode == "rates" else mode_trace)(a)


if __name__ == "__main__":
    main()
