#!/usr/bin/env python3
"""Evaluate K model files side by side in ONE poli_eval batch (policy slots).  GPU:  python tools/eval_policies.py --char dog a.h5 b.h5 c.h5

K x --eval-envs envs, env e in slot e % K (round-robin: every slot's envs are spread over the launch), every model on the SAME --eval-envs terrains: env e is
reseeded with terrain seed --seed + e // K, the seed env e // K of a fresh tools/learn_curve.py evaluation batch is created with. Greedy, --eval-frames outer frames.
Per model the columns of learn_curve.py's evaluation (speed, falls_k, avg_dist, alive, episodes, cycles) -- the same numbers, bit for bit, as learn_curve.evaluate
gives for that model alone (--check runs those K single-policy evaluations as well, compares, and prints both wall times).
A model is a Caffe HDF5 file with its '<model>_scale.txt' next to it (BatchScenario.SlotLoadModel)."""
import argparse, os, sys, time
import numpy as np
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
import deepterrainrl_amd as da
import learn_curve

COLS = ("speed", "falls_k", "avg_dist", "alive", "episodes", "cycles")


evaluate_many = learn_curve.evaluate_many


def load_policy(b, model_file):
    """(weights, normalisers) of a model file, through the same readers SlotLoadModel uses."""
    import json
    from deepterrainrl_amd import caffe_hdf5
    w = caffe_hdf5.load_mace_weights(model_file, b.num_frags)
    scale = os.path.splitext(model_file)[0] + "_scale.txt"
    norm = (None,) * 4
    if os.path.exists(scale):
        j = json.load(open(scale))
        norm = tuple(None if j.get(k) is None else np.asarray(j[k], np.float64) for k in ("InputOffset", "InputScale", "OutputOffset", "OutputScale"))
    return w, norm


def same(a, b):
    return all((a[k] == b[k]) or (a[k] != a[k] and b[k] != b[k]) for k in COLS)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("models", nargs="+", help="Caffe HDF5 model files (at most 32)")
    ap.add_argument("--char", choices=sorted(learn_curve.CHARS), default="dog")
    ap.add_argument("--eval-envs", type=int, default=512)
    ap.add_argument("--eval-frames", type=int, default=300)
    ap.add_argument("--seed", type=int, default=777001)
    ap.add_argument("--data-root", default=os.path.join(REPO, "tests", "golden", "refdata"))
    ap.add_argument("--check", action="store_true", help="also run learn_curve.evaluate once per model; the figures must be identical; prints both wall times")
    ap.add_argument("--lib", default="", help="(CPU smoke runs only) bind the scenario to this build of the engine, e.g. tests/emul/libdtrl_emul.so")
    a = ap.parse_args()
    if a.lib:
        class LibScenario(da.BatchScenario):
            def _library(self):
                return da._bind(os.path.abspath(a.lib))
        learn_curve.SCENARIO = LibScenario
    arg_file = learn_curve.CHARS[a.char]["evalf"]
    probe = learn_curve.SCENARIO(arg_file, 1, data_root=a.data_root)
    pols = [load_policy(probe, m) for m in a.models]
    probe.close()
    t0 = time.time()
    res = evaluate_many(arg_file, a.data_root, pols, a.eval_envs, a.eval_frames, a.seed)
    t_many = time.time() - t0
    print("# %d models x %d envs x %d frames of %s in one batch: %.2f s" % (len(pols), a.eval_envs, a.eval_frames, arg_file, t_many))
    print("# %-48s %8s %8s %9s %7s %9s %9s" % (("model",) + COLS))
    for m, r in zip(a.models, res):
        print("  %-48s %8.3f %8.3f %9.3f %7.3f %9d %9d" % ((os.path.basename(m),) + tuple(r[k] for k in COLS)))
    if a.check:
        t0 = time.time()
        ref = [learn_curve.evaluate(arg_file, a.data_root, w, norm, a.eval_envs, a.eval_frames, a.seed) for w, norm in pols]
        t_each = time.time() - t0
        bad = [m for m, x, y in zip(a.models, res, ref) if not same(x, y)]
        print("# %d single-policy evaluations (one fresh batch each): %.2f s; one slotted batch: %.2f s; per-model figures %s" % (
            len(pols), t_each, t_many, "identical" if not bad else "DIFFER for " + ", ".join(bad)))
        if bad:
            sys.exit(1)


if __name__ == "__main__":
    main()
