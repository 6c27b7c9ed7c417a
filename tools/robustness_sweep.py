#!/usr/bin/env python3
"""How far does a trained policy survive a change of its character?  GPU:  python tools/robustness_sweep.py --char dog   (and --char raptor)

ONE poli_eval batch (model variants) runs the committed trained policy of the character (tests/golden/policies) greedily over a grid of main-body mass x
torque-limit scales: one variant per cell (cell 0,0 of the default grid is not special: the nominal model is the cell with both scales 1), --cell-envs envs per
cell, env e in cell e % cells, every cell on the SAME --cell-envs terrains (env e is reseeded with --seed + e // cells). The reset that reseeds also starts every
episode under the env's own model. Per cell, from dtrl_variant_stats: falls per 1000 env-steps and speed (m/s, distance covered over all episodes / time).
The main body is `torso` for the dog and the first body (`root`) for the raptor."""
import argparse, os, sys, time
import numpy as np
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
import deepterrainrl_amd as da
import eval_policies, learn_curve

MODELS = {"dog": "dog_mace3_slopes_mixed_model.h5", "raptor": "raptor_mace3_narrow_gaps_model.h5"}
BODY = {"dog": "torso", "raptor": "root"}


def sweep(char, masses, limits, n, frames, seed, root, scenario=None, policy=None):
    """[(mass scale, torque-limit scale, dict(falls_k, speed, episodes, cycles, n_envs))] in grid order (mass-major). policy: (weights, normalisers) in place of
    the committed trained net (tools/domain_randomisation.py)"""
    cells = [(m, t) for m in masses for t in limits]
    K = len(cells)
    arg = learn_curve.CHARS[char]["evalf"]
    b = (scenario or learn_curve.SCENARIO)(arg, K * n, data_root=root, extra_args={"terrain_seed": seed})
    w, norm = policy if policy is not None else eval_policies.load_policy(b, os.path.join(REPO, "tests", "golden", "policies", MODELS[char]))
    b.SetPolicy(w, *norm)
    b.SetExplore(0, 0.0, 1.0, 0.0)
    b.CreateVariants(K + 1)                                        # variant 0 stays the batch's own model and is not used: every cell is loaded the same way
    for k, (m, t) in enumerate(cells):
        b.ScaledVariant(k + 1, mass={BODY[char]: m}, torque_lim=t)
    cell = np.arange(K * n, dtype=np.int32) % K
    b.AssignVariants(None, cell + 1)
    b.Reset(None, [seed + e // K for e in range(K * n)])           # the same n terrains for every cell; episodes start under the env's own model
    x0 = b.PoseVel()[0][:, 0].copy()
    b.RunFrames(frames)
    d, ids = b.GetDistLog()
    ids = np.asarray(ids, np.int64)
    x1 = b.PoseVel()[0][:, 0]
    T = frames / 30.0
    out = []
    for k, (m, t) in enumerate(cells):
        st = b.VariantStats(k + 1)
        total = float(d[ids % K == k].sum()) + float((x1[cell == k] - x0[cell == k]).sum())
        falls = st["resets"] - st["n_envs"]                        # (the reseeding reset is counted by the engine; it is not a fall)
        out.append((m, t, dict(falls_k=1000.0 * falls / (n * frames * 20.0), speed=total / (n * T), episodes=st["episodes"], cycles=st["cycles"], n_envs=st["n_envs"])))
    b.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--char", choices=sorted(MODELS), default="dog")
    ap.add_argument("--mass", default="0.7,0.85,1,1.15,1.3,1.5", help="main-body mass scales")
    ap.add_argument("--torque", default="0.6,0.8,1,1.2", help="torque-limit scales")
    ap.add_argument("--cell-envs", type=int, default=128)
    ap.add_argument("--frames", type=int, default=300)
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
    masses = [float(x) for x in a.mass.split(",")]; limits = [float(x) for x in a.torque.split(",")]
    t0 = time.time()
    res = sweep(a.char, masses, limits, a.cell_envs, a.frames, a.seed, a.data_root, scenario)
    print("# tools/robustness_sweep.py --char %s: %s, %d cells x %d envs x %d frames in one batch, %.1f s; %s mass x torque limit" % (
        a.char, MODELS[a.char], len(res), a.cell_envs, a.frames, time.time() - t0, BODY[a.char]))
    for what, fmt in (("falls per 1000 env-steps", "%8.3f"), ("speed, m/s", "%8.3f")):
        key = "falls_k" if what.startswith("falls") else "speed"
        print("## %s (rows: %s mass scale; columns: torque-limit scale)" % (what, BODY[a.char]))
        print("   %8s " % "" + " ".join("%8.2f" % t for t in limits))
        for m in masses:
            print("   %8.2f " % m + " ".join(fmt % r[key] for mm, tt, r in res if mm == m))


if __name__ == "__main__":
    main()
