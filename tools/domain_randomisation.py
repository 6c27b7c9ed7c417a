#!/usr/bin/env python3
"""Does training under a variant redraw give a sturdier policy?  GPU:  python tools/domain_randomisation.py --out profiles/variant_redraw_learning.txt

Runs the dog's schedule of tools/learn_curve.py (args/opt_args_train_mace.txt on slopes_mixed, 4096 envs, native trainer, overlapped, --iters iterations) twice
with the same seeds: once on the nominal model, once with train_loop.train(variants=...) -- a table of --variants models under seeded torso-mass and torque-limit
scales, every episode of every env under a model drawn afresh (BatchScenario.VariantRedraw). Both final nets are then evaluated greedily over the torso mass x
torque-limit grid of tools/robustness_sweep.py (one batch per net, one variant per cell, the same terrains in every cell and for both nets). Printed per cell:
falls per 1000 env-steps of both nets. --continuous adds a third run: train_loop.train(rescale=...), the torso mass and the torque limits drawn afresh from the
same two ranges at every episode of every env on the device (BatchScenario.VariantRescale, no table), evaluated over the same grid. A result to report, not a bar
to pass."""
import argparse, gc, os, sys, time
import numpy as np
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
import deepterrainrl_amd as da
from deepterrainrl_amd import train_loop
import learn_curve, robustness_sweep


def run(a):
    c = learn_curve.CHARS["dog"]
    spec = dict(count=a.variants, mass=tuple(a.mass_range), torque_lim=tuple(a.torque_range), seed=a.variant_seed, keep_nominal=a.keep_nominal, mass_body="torso")
    extra = dict({"terrain_file": c["terrain"]}, **({"trainer_num_init_samples": a.init_samples} if a.init_samples is not None else {}))
    lines = ["# tools/domain_randomisation.py: %s with -terrain_file= %s, %d envs, native trainer, overlapped, %d iterations, trainer seed %d; evaluation: %d envs per cell x %d frames, terrain seed %d; GPU_MAX_HW_QUEUES=%s"
             % (c["train"], c["terrain"], a.envs, a.iters, a.seed, a.cell_envs, a.eval_frames, a.eval_seed, os.environ["GPU_MAX_HW_QUEUES"]),
             "# redraw: %d variants, torso mass scale uniform in [%g, %g], torque-limit scale uniform in [%g, %g], variant seed %d, weight on the nominal model %g"
             % (a.variants, a.mass_range[0], a.mass_range[1], a.torque_range[0], a.torque_range[1], a.variant_seed, a.keep_nominal)]
    masses = [float(x) for x in a.mass.split(",")]; limits = [float(x) for x in a.torque.split(",")]
    grids = {}
    # (the rescale scales every body's mass by the one factor of the episode: per-link factors would scale each body on its own, and the grid varies the torso alone)
    cont = dict(mass=tuple(a.mass_range), torque_lim=tuple(a.torque_range), seed=a.variant_seed)
    if a.continuous:
        lines.append("# continuous: mass scale (every body) uniform in [%g, %g], torque-limit scale uniform in [%g, %g], drawn per episode, seed %d" % (*a.mass_range, *a.torque_range, a.variant_seed))
    # (--episode-limit: all runs alike, so that the redraw and the rescale keep drawing once the policy has stopped falling)
    limit = dict(frames=tuple(a.episode_limit), seed=a.variant_seed) if a.episode_limit else None
    if limit:
        lines.append("# episode limit: every episode ends after %d .. %d frames at the latest, drawn per episode, seed %d" % (*a.episode_limit, a.variant_seed))
    runs = [("nominal", None, None), ("redraw", spec, None)] + ([("continuous", None, cont)] if a.continuous else [])
    for name, variants, rescale in runs:
        t0 = time.time()
        st = train_loop.train(c["train"], a.data_root, a.envs, max_iters=a.iters, overlap=True, trainer=a.trainer, seed=a.seed, extra_args=extra, variants=variants, rescale=rescale, episode_limit=limit)
        line = "# %-8s training: %d frames, %d iterations, %d tuples, %.1f s, %.2f M env-steps/s" % (name, st["frames"], st["iters"], st["tuples"], time.time() - t0, st["env_steps_per_s"] / 1e6)
        if variants:
            line += "; %d draws, envs per variant at the end min %d max %d" % (int(st["variants"]["draws"].sum()), *(lambda h: (int(h.min()), int(h.max())))(np.bincount(st["variants"]["variant"], minlength=a.variants)))
        if rescale:
            line += "; %d episode starts under drawn scales" % int(st["rescale"]["episodes"].sum())
        if limit:
            line += "; %d episodes ended by the limit, %d by a fall" % (int(st["episode_limit"]["by_limit"].sum()), int(st["episode_limit"]["by_fall"].sum()))
        lines.append(line); print(line, flush=True)
        gc.collect()   # (the training batch hangs in train()'s closures: give its device memory back before the next batches are built)
        grids[name] = robustness_sweep.sweep("dog", masses, limits, a.cell_envs, a.eval_frames, a.eval_seed, a.data_root, None, policy=(st["weights"], st["offset_scale"]))
    for name, _, _ in runs:
        lines.append("## %s-trained net: falls per 1000 env-steps (rows: torso mass scale; columns: torque-limit scale)" % name)
        lines.append("   %8s " % "" + " ".join("%8.2f" % t for t in limits))
        for m in masses:
            lines.append("   %8.2f " % m + " ".join("%8.3f" % r["falls_k"] for mm, tt, r in grids[name] if mm == m))
    mean = {k: float(np.mean([r["falls_k"] for _, _, r in g])) for k, g in grids.items()}
    nom = {k: [r["falls_k"] for m, t, r in g if m == 1.0 and t == 1.0] for k, g in grids.items()}
    lines.append("# mean over the grid: %s; nominal cell (1, 1): %s" % (", ".join("%s-trained %.3f" % (k, v) for k, v in mean.items()),
                 ", ".join("%s-trained %.3f" % (k, v[0]) for k, v in nom.items() if v) or "not in the grid"))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=60000)
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--seed", type=int, default=0, help="trainer seed (both runs)")
    ap.add_argument("--variants", type=int, default=64)
    ap.add_argument("--variant-seed", type=int, default=11)
    ap.add_argument("--keep-nominal", type=float, default=0.25)
    ap.add_argument("--mass-range", type=float, nargs=2, default=[0.7, 1.5])
    ap.add_argument("--torque-range", type=float, nargs=2, default=[0.6, 1.2])
    ap.add_argument("--continuous", action="store_true", help="a third run trained under the variant rescale: scales drawn per episode from the two ranges, no table")
    ap.add_argument("--episode-limit", type=int, nargs=2, default=None, metavar=("LO", "HI"), help="every training run under an episode limit of LO .. HI frames (train_loop.train(episode_limit=...)): episodes, and with them the draws, keep coming under a policy that no longer falls")
    ap.add_argument("--mass", default="0.7,0.85,1,1.15,1.3,1.5", help="evaluation grid: torso mass scales")
    ap.add_argument("--torque", default="0.6,0.8,1,1.2", help="evaluation grid: torque-limit scales")
    ap.add_argument("--cell-envs", type=int, default=128)
    ap.add_argument("--eval-frames", type=int, default=300)
    ap.add_argument("--eval-seed", type=int, default=777001)
    ap.add_argument("--trainer", choices=["hip", "torch"], default="hip")
    ap.add_argument("--init-samples", type=int, default=None, help="(smoke runs only) override -trainer_num_init_samples=")
    ap.add_argument("--data-root", default=os.path.join(REPO, "tests", "golden", "refdata"))
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    lines = run(a)
    print("\n".join(lines))
    if a.out:
        open(a.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
