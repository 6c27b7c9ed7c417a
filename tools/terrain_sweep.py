#!/usr/bin/env python3
"""One policy -- or none (the controller's FSM), or K policies -- over T terrain files in ONE poli_eval batch (terrain sets).
GPU:  python tools/terrain_sweep.py --char dog --model m.h5 data/terrain/flat.txt data/terrain/slopes_mixed.txt data/terrain/narrow_gaps.txt data/terrain/cliffs_rugged.txt
      python tools/terrain_sweep.py --char dog --slots a.h5 b.h5 -- data/terrain/flat.txt data/terrain/cliffs_rugged.txt          (K policies x T terrains)

T x --envs envs (K x T x --envs with --slots), dealt round-robin over the terrains (over the grid: env e runs policy e % K on terrain (e // K) % T) and restarted under
their terrain (dtrl_assign_terrains with restart), so every env begins as an env of a batch created with that terrain file begins. --frames outer frames, greedy.
Without --slots: per terrain dtrl_terrain_stats (envs, episodes, cycles, falls, average episode distance). With --slots: per cell the same figures from the per-env
getters (dtrl_get_cycle_info, the distance log). --dist-log FILE writes the distance log grouped by terrain (by cell), one line per group: "<terrain file>[ <model>]: d0, d1, ..."
A model is a Caffe HDF5 file with its '<model>_scale.txt' next to it; terrain files are resolved like -terrain_file= (relative to --root)."""
import argparse, os, sys
import numpy as np
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
import deepterrainrl_amd as da
import eval_policies, learn_curve


def sweep(arg_file, root, terrains, policies, n, frames, seed=777001, scenario=None, extra=None):
    """terrains: T terrain files; policies: [] (arg_file names no -policy_net=: the controller's FSM alone), or [(weights, norm)] (K = 1: no slots), or K of them (slots).
    Returns (cells, dist): cells[k][t] = dict(n_envs, episodes, cycles, falls, avg_dist), dist[k][t] = the episode distances of the cell's envs (env order, time order)."""
    T, K = len(terrains), max(1, len(policies))
    N = K * T * n
    args = {"terrain_seed": seed}
    args.update(extra or {})
    b = (scenario or da.BatchScenario)(arg_file, N, data_root=root, extra_args=args)
    if len(policies) > 1:
        b.CreateSlots(K)
    if policies:
        b.SetPolicy(policies[0][0], *policies[0][1])
    for k in range(1, len(policies)):
        b.SlotSetPolicy(k, policies[k][0], *policies[k][1])
    b.SetExplore(0, 0.0, 1.0, 0.0)
    e = np.arange(N, dtype=np.int32)
    slot, terr = e % K, (e // K) % T
    if len(policies) > 1:
        b.AssignSlots(None, slot)
    b.CreateTerrains(T + 1)                      # terrain 0 stays the arg file's; the swept files are terrains 1 .. T
    for t, f in enumerate(terrains):
        b.SetTerrainFile(1 + t, f)
    b.AssignTerrains(None, 1 + terr, restart=True)
    nc0, nr0 = (np.asarray(x).copy() for x in b.CycleInfo()[:2])
    for _ in range(frames):
        b.Update(1.0 / 30.0)
    nc, nr = (np.asarray(x) for x in b.CycleInfo()[:2])
    d, ids = b.GetDistLog()
    ids = np.asarray(ids, np.int64)
    cells = [[None] * T for _ in range(K)]; dist = [[None] * T for _ in range(K)]
    for k in range(K):
        for t in range(T):
            m = (slot == k) & (terr == t)
            dk = d[m[ids]]
            cells[k][t] = dict(n_envs=int(m.sum()), episodes=int(len(dk)), cycles=int((nc - nc0)[m].sum()), falls=int((nr - nr0)[m].sum()), avg_dist=float(dk.mean()) if len(dk) else float("nan"))
            dist[k][t] = dk
    if K == 1:                                   # the device reduction agrees with the per-env getters
        for t in range(T):
            st = b.TerrainStats(1 + t)
            assert (st["n_envs"], st["resets"] - st["n_envs"]) == (cells[0][t]["n_envs"], cells[0][t]["falls"]), (t, st, cells[0][t])
    b.close()
    return cells, dist


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--char", default="dog", choices=sorted(learn_curve.CHARS))
    ap.add_argument("--root", default=os.path.join(REPO, "tests", "golden", "refdata"))
    ap.add_argument("--arg-file", default="", help="the scene (default: the character's poli_eval scene; without a model args/sim_<char>_args.txt, which names no policy net)")
    ap.add_argument("--model", default="", help="one model file (default: no policy net, the FSM controller)")
    ap.add_argument("--slots", nargs="+", default=[], help="K model files: K policies x T terrains")
    ap.add_argument("--envs", type=int, default=256, help="envs per terrain (per cell)")
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--seed", type=int, default=777001)
    ap.add_argument("--terrain-gen", default="host", choices=["host", "device"])
    ap.add_argument("--dist-log", default="")
    ap.add_argument("terrains", nargs="+")
    a = ap.parse_args()
    files = a.slots or ([a.model] if a.model else [])
    arg = a.arg_file or (learn_curve.CHARS[a.char]["evalf"] if files else "args/sim_%s_args.txt" % a.char)   # without a model: the scene without a policy net
    pols = []
    if files:
        probe = da.BatchScenario(arg, 1, data_root=a.root)
        pols = [eval_policies.load_policy(probe, f) for f in files]
        probe.close()
    cells, dist = sweep(arg, a.root, a.terrains, pols, a.envs, a.frames, a.seed, extra={"terrain_gen": a.terrain_gen})
    names = [os.path.basename(f) for f in files] or ["(no policy net)"]
    print("%-28s %-32s %6s %8s %8s %6s %9s" % ("terrain", "policy", "envs", "episodes", "cycles", "falls", "avg_dist"))
    lines = []
    for t, tf in enumerate(a.terrains):
        for k, nm in enumerate(names):
            c = cells[k][t]
            print("%-28s %-32s %6d %8d %8d %6d %9.3f" % (os.path.basename(tf), nm, c["n_envs"], c["episodes"], c["cycles"], c["falls"], c["avg_dist"]))
            lines.append("%s%s: %s" % (tf, " " + nm if len(names) > 1 else "", ", ".join("%f" % x for x in dist[k][t])))
    if a.dist_log:
        with open(a.dist_log, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
