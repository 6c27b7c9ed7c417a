#!/usr/bin/env python3
"""A committed trained policy on a terrain ladder: T lerp steps of one terrain file as levels 0 .. T-1 (SetTerrainFile(t, path, lerp=t/(T-1)); level 0 is the
scene's own terrain at the same file's lerp 0), every env starting on level 0, and the envs climbing and descending by their own episodes (dtrl_terrain_ladder).
GPU:  python tools/terrain_ladder.py --char dog --levels 6 --envs 1024 --frames 600 --terrain-gen device
Prints, every --every frames, the level histogram and the ups and downs since the start; at the end the per-level dtrl_terrain_stats.
The model defaults to tests/golden/policies/<char>_mace3_*_model.h5 (with its '_scale.txt' next to it); the terrain file to the character's own."""
import argparse, glob, os, sys
import numpy as np
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
import deepterrainrl_amd as da
import eval_policies, learn_curve


def run(arg_file, root, terrain_file, policy, levels, n, frames, up_dist, down_dist, at_top=False, every=50, seed=777001, scenario=None, extra=None, out=print):
    """Returns [(frame, histogram [levels], ups, downs)] at every `every` frames and at the end, and the batch's per-level statistics."""
    args = {"terrain_seed": seed, "terrain_file": terrain_file}
    args.update(extra or {})
    b = (scenario or da.BatchScenario)(arg_file, n, data_root=root, extra_args=args)
    b.SetPolicy(policy[0], *policy[1])
    b.SetExplore(0, 0.0, 1.0, 0.0)
    b.CreateTerrains(levels)
    for t in range(1, levels):
        b.SetTerrainFile(t, terrain_file, lerp=t / float(levels - 1))
    b.TerrainLadder(0, levels - 1, up_dist, down_dist, at_top)
    rows = []
    out("%6s  %-*s %8s %8s" % ("frame", 7 * levels, "envs per level", "ups", "downs"))
    for f in range(1, frames + 1):
        b.Update(1.0 / 30.0)
        if f % every == 0 or f == frames:
            info = b.LadderInfo()
            hist = np.bincount(b.GetTerrains(), minlength=levels)
            rows.append((f, hist.tolist(), int(info["ups"].sum()), int(info["downs"].sum())))
            out("%6d  %s %8d %8d" % (f, "".join("%7d" % h for h in hist), rows[-1][2], rows[-1][3]))
    stats = [b.TerrainStats(t) for t in range(levels)]
    out("%6s %6s %9s %8s %7s %9s" % ("level", "envs", "episodes", "cycles", "resets", "avg_dist"))
    for t, s in enumerate(stats):
        out("%6d %6d %9d %8d %7d %9.3f" % (t, s["n_envs"], s["episodes"], s["cycles"], s["resets"], s["avg_dist"]))
    b.close()
    return rows, stats


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--char", default="dog", choices=sorted(learn_curve.CHARS))
    ap.add_argument("--root", default=os.path.join(REPO, "tests", "golden", "refdata"))
    ap.add_argument("--model", default="", help="model file (default: the character's committed policy under tests/golden/policies/)")
    ap.add_argument("--terrain", default="", help="terrain file whose parameter sets the levels blend (default: the character's own)")
    ap.add_argument("--levels", type=int, default=6)
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--frames", type=int, default=600)
    ap.add_argument("--every", type=int, default=50)
    ap.add_argument("--up-dist", type=float, default=10.0)
    ap.add_argument("--down-dist", type=float, default=3.0)
    ap.add_argument("--at-top", action="store_true", help="an env that passes the top level is dealt a level of the ladder at random")
    ap.add_argument("--seed", type=int, default=777001)
    ap.add_argument("--terrain-gen", default="device", choices=["host", "device"])
    a = ap.parse_args()
    if a.levels < 2:
        ap.error("--levels must be at least 2")
    c = learn_curve.CHARS[a.char]
    model = a.model or sorted(glob.glob(os.path.join(REPO, "tests", "golden", "policies", "%s_mace3_*_model.h5" % a.char)))[0]
    probe = da.BatchScenario(c["evalf"], 1, data_root=a.root)
    pol = eval_policies.load_policy(probe, model)
    probe.close()
    print("# %s on %d lerp steps of %s, %d envs, up_dist %g, down_dist %g, at_top %d, -terrain_gen= %s" % (os.path.basename(model), a.levels, a.terrain or c["terrain"], a.envs, a.up_dist, a.down_dist, a.at_top, a.terrain_gen))
    run(c["evalf"], a.root, a.terrain or c["terrain"], pol, a.levels, a.envs, a.frames, a.up_dist, a.down_dist, a.at_top, a.every, a.seed, extra={"terrain_gen": a.terrain_gen})


if __name__ == "__main__":
    main()
