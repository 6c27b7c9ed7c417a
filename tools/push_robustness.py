#!/usr/bin/env python3
"""How hard a push does a trained policy survive?  GPU:  python tools/push_robustness.py --char dog   (and --char raptor)

ONE poli_eval batch runs the committed trained policy of the character (tests/golden/policies) greedily under a push schedule (BatchScenario.PushSchedule) whose
force magnitude is fixed at --force newtons, with a per-env scale (PushScale) over the grid --scales: --cell-envs envs per cell, env e in cell e % cells, every cell
on the SAME --cell-envs terrains (env e is reseeded with --seed + e // cells). Scale 0 is the unpushed control. The push STREAM of an env depends on its global id,
so the cells see different random links, directions and times of the same distribution; only the magnitude is swept. Per cell: pushes received, and falls per 1000
env-steps from the envs' reset counters."""
import argparse, os, sys, time
import numpy as np
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
import deepterrainrl_amd as da
import eval_policies, learn_curve
from robustness_sweep import MODELS


def sweep(char, scales, n, frames, seed, root, force, wait, duration, scenario=None, policy=None):
    """[(scale, dict(force, pushes, falls_k, n_envs))] in grid order"""
    K = len(scales)
    b = (scenario or learn_curve.SCENARIO)(learn_curve.CHARS[char]["evalf"], K * n, data_root=root, extra_args={"terrain_seed": seed})
    w, norm = policy if policy is not None else eval_policies.load_policy(b, os.path.join(REPO, "tests", "golden", "policies", MODELS[char]))
    b.SetPolicy(w, *norm)
    b.SetExplore(0, 0.0, 1.0, 0.0)
    cell = np.arange(K * n, dtype=np.int32) % K
    b.Reset(None, [seed + e // K for e in range(K * n)])           # the same n terrains for every cell
    b.PushScale(np.asarray(scales, np.float64)[cell])
    b.PushSchedule(wait, seed=seed, force=(force, force), duration=duration)
    r0 = np.asarray(b.CycleInfo()[1]).copy()
    b.RunFrames(frames)
    falls = np.asarray(b.CycleInfo()[1]) - r0
    pushes = b.PushInfo()["pushes"]
    out = []
    for k, s in enumerate(scales):
        m = cell == k
        out.append((s, dict(force=s * force, pushes=int(pushes[m].sum()), falls_k=1000.0 * float(falls[m].sum()) / (n * frames * 20.0), n_envs=int(m.sum()))))
    b.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--char", choices=sorted(MODELS), default="dog")
    ap.add_argument("--force", type=float, default=100.0, help="force magnitude at scale 1, N")
    ap.add_argument("--scales", default="0,0.5,1,1.5,2,3,4,6", help="per-cell scales of the force")
    ap.add_argument("--wait", type=int, nargs=2, default=[30, 90], metavar=("LO", "HI"), help="frames between two pushes of an env")
    ap.add_argument("--duration", type=float, nargs=2, default=[0.1, 0.3], metavar=("LO", "HI"), help="seconds")
    ap.add_argument("--cell-envs", type=int, default=256)
    ap.add_argument("--frames", type=int, default=600)
    ap.add_argument("--seed", type=int, default=777001)
    ap.add_argument("--data-root", default=os.path.join(REPO, "tests", "golden", "refdata"))
    ap.add_argument("--lib", default="", help="(CPU smoke runs only) bind the scenario to this build of the engine, e.g. tests/emul/libdtrl_emul.so")
    a = ap.parse_args()
    scenario = None
    if a.lib:
        class LibScenario(da.BatchScenario):
            def _library(self):
                return da._bind(os.path.abspath(a.lib))
        scenario = LibScenario
    scales = [float(x) for x in a.scales.split(",")]
    t0 = time.time()
    res = sweep(a.char, scales, a.cell_envs, a.frames, a.seed, a.data_root, a.force, tuple(a.wait), tuple(a.duration), scenario)
    print("# tools/push_robustness.py --char %s: %s greedy, %d cells x %d envs x %d frames in one batch, %.1f s; a push every %d .. %d frames for %.2f .. %.2f s" % (
        a.char, MODELS[a.char], len(res), a.cell_envs, a.frames, time.time() - t0, a.wait[0], a.wait[1], a.duration[0], a.duration[1]))
    print("   %8s %10s %10s %28s" % ("scale", "force, N", "pushes", "falls per 1000 env-steps"))
    for s, r in res:
        print("   %8.2f %10.1f %10d %28.3f" % (s, r["force"], r["pushes"], r["falls_k"]))


if __name__ == "__main__":
    main()
