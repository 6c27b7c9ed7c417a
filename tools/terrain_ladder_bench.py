#!/usr/bin/env python3
"""What does the terrain ladder cost?  GPU:  python tools/terrain_ladder_bench.py --parent-lib DIR > profiles/terrain_ladder.txt   (docs/EXPERIMENTS.md, terrain ladder)

bench.py's configs[1] shape (4096 dogs, args/dog_slopes_mixed_args.txt, xavier weights, the same seeds) with -terrain_gen= device and 8 terrains: the arg file's
slopes_mixed at lerp 0 as terrain 0 and seven lerp steps of data/terrain/slopes_mixed.txt behind it (SetTerrainFile(t, path, lerp=t/7)). Three legs, all batches
built first, each pre-rolled to a stationary reset rate (bench.py's rule), then ALTERNATED inside one process: --rounds rounds (>= 3), every round times --steps
frames of every leg in turn, ending in a device synchronise. Per leg: median, min, max M env-steps/s and the spread.
  (a) parent commit's library, terrains, no ladder   --parent-lib DIR: a directory that holds the parent commit's libdtrl.so (dtrl_terrain_boundary_keyed)
  (b) this commit, terrains, no ladder               the same launches: nothing moved for batches without a ladder
  (c) this commit, ladder on                         TerrainLadder(0, 7, --up-dist, --down-dist): dtrl_terrain_boundary_ladder in place of the keyed kernel
--mode trace --leg b|c runs 60 frames of one leg and nothing else: the workload of a kernel trace of its own
  rocprofv3 --kernel-trace --stats -d DIR -o t -- python tools/terrain_ladder_bench.py --mode trace --leg c"""
import argparse, os, sys, time
import numpy as np
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
import bench
import deepterrainrl_amd as da
from policy_slots_bench import older_library, preroll, sync, SEEDS

N_TERRAINS = 8
LADDER_FILE = "data/terrain/slopes_mixed.txt"


def make(cfg, n, a, ladder, lib=None):
    b = (older_library(lib) if lib else da.BatchScenario)(cfg["arg_file"], n, data_root=bench.ROOT, extra_args=dict(SEEDS, terrain_gen="device"))
    b.SetPolicy(bench.xavier_weights(b.PolicyNumParams(), cfg["n_char"], cfg["frag"]), *bench.load_scale(cfg))
    b.CreateTerrains(N_TERRAINS)
    for t in range(1, N_TERRAINS):
        b.SetTerrainFile(t, LADDER_FILE, lerp=t / float(N_TERRAINS - 1))
    b.AssignTerrains(None, np.arange(n, dtype=np.int32) % N_TERRAINS, restart=True)   # every leg starts from the same mixture
    if ladder:
        b.TerrainLadder(0, N_TERRAINS - 1, a.up_dist, a.down_dist)
    return b


def mode_rates(a):
    cfg = bench.CONFIGS[1]; n = cfg["envs"]
    legs = []
    if a.parent_lib:
        legs.append(("(a) parent commit's library, no ladder", dict(ladder=False, lib=os.path.join(os.path.abspath(a.parent_lib), "libdtrl.so"))))
    legs += [("(b) this commit, no ladder", dict(ladder=False)), ("(c) this commit, ladder on", dict(ladder=True))]
    print("## -terrain_gen= device, %s, %d envs, %d terrains, %d rounds x %d frames per leg, alternating" % (cfg["arg_file"], n, N_TERRAINS, a.rounds, a.steps), flush=True)
    batches = []
    for label, kw in legs:
        b = make(cfg, n, a, **kw)
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
        print("   %-42s median %7.3f  min %7.3f  max %7.3f M env-steps/s  (spread %.2f %%; pre-roll %d frames, %.1f resets/frame)"
              % (label, med[label], v[0], v[-1], 100 * (v[-1] - v[0]) / med[label], pr[0], pr[1]), flush=True)
    lb, lc = legs[-2][0], legs[-1][0]
    if a.parent_lib:
        print("   (b) / (a): %.4f" % (med[lb] / med[legs[0][0]]), flush=True)
    print("   (c) / (b): %.4f" % (med[lc] / med[lb]), flush=True)
    lad = batches[-1][1]
    info = lad.LadderInfo()
    print("   ladder leg: level histogram %s, ups %d, downs %d" % (np.bincount(lad.GetTerrains(), minlength=N_TERRAINS).tolist(), int(info["ups"].sum()), int(info["downs"].sum())), flush=True)
    for _, b, _ in batches:
        b.close()


def mode_trace(a):
    cfg = bench.CONFIGS[1]
    b = make(cfg, cfg["envs"], a, ladder=a.leg == "c")
    b.RunFrames(60)
    sync()
    b.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", default="rates", choices=["rates", "trace"])
    ap.add_argument("--leg", default="c", choices=["b", "c"], help="(trace) which leg")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=150)
    ap.add_argument("--up-dist", type=float, default=2.0)
    ap.add_argument("--down-dist", type=float, default=1.0)
    ap.add_argument("--parent-lib", default="", help="directory with the parent commit's libdtrl.so")
    a = ap.parse_args()
    if a.rounds < 3:
        ap.error("--rounds must be at least 3")
    sync()   # torch's HIP context first, as in bench.py (it does not come up behind the engine's)
    print("# tools/terrain_ladder_bench.py --mode %s --rounds %d --steps %d --up-dist %g --down-dist %g" % (a.mode, a.rounds, a.steps, a.up_dist, a.down_dist), flush=True)
    (mode_rates if a.mode == "rates" else mode_trace)(a)


if __name__ == "__main__":
    main()
