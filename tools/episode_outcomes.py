#!/usr/bin/env python3
"""Episode outcomes under the scales the episodes actually ran under.
GPU:  python tools/episode_outcomes.py [--envs 4096 --frames 600]

A committed trained policy under the continuous variant rescale (every episode of every env under a mass and a torque-limit scale drawn afresh on the device) and
an episode limit, run with RunFrames in chunks -- the host never looks at the batch between the frames of a chunk -- with one drain of the episode log per
chunk. Every row carries the draw number its episode's factors were drawn with (rescale_draw); VariantRescaleFactors recomputes the factors from it, and the
table below bins the episodes by their mass and torque_lim factor: episodes, fall share, mean distance and mean length per bin. This is the evaluation
tools/domain_randomisation.py --continuous does on a ScaledVariant grid because it cannot attribute an outcome to a draw."""
import argparse, os, sys
import numpy as np
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import deepterrainrl_amd as da

POLICY = {"dog": ("args/dog_slopes_mixed_args.txt", "tests/golden/policies/dog_mace3_slopes_mixed_model.h5"),
          "raptor": ("args/raptor_narrow_gaps_args.txt", "tests/golden/policies/raptor_mace3_narrow_gaps_model.h5")}


def run(a, scenario_cls=None, data_root=None):
    """-> (rows: dict of arrays over all drained episodes, factors [rows, 4, L], lost)"""
    arg, model = POLICY[a.character]
    b = (scenario_cls or da.BatchScenario)(arg, a.envs, data_root=data_root or os.path.join(REPO, "tests", "golden", "refdata"), extra_args=dict(terrain_seed=a.seed, rand_seed=1, terrain_gen="device"))
    b.LoadModel(os.path.join(REPO, model))
    b.CreateVariants(1)
    b.VariantRescale(base=0, seed=a.seed, mass=tuple(a.mass_range), torque_lim=tuple(a.torque_range))
    b.Reset()                                            # every env starts its first episode under drawn scales
    b.EpisodeLimit(tuple(a.limit), seed=a.seed)
    b.EpisodeLog(a.capacity)
    parts, lost, done = [], 0, 0
    while done < a.frames:
        k = min(a.chunk, a.frames - done)
        b.RunFrames(k); done += k
        d = b.EpisodeLogDrain()
        lost += d["lost"]
        parts.append(d)
    rows = {k: np.concatenate([p[k] for p in parts]) for k in parts[0] if k != "lost"}
    fac = b.VariantRescaleFactors(rows["env"], rows["rescale_draw"])
    b.close()
    return rows, fac, lost


def table(rows, fac, a, quantity, q):
    lo, hi = (a.mass_range, a.torque_range)[0 if quantity == "mass" else 1]
    f = fac[:, q, 0]                                     # (not per link: one factor for all links)
    edges = np.linspace(lo, hi, a.bins + 1)
    lines = ["%-12s %9s %10s %10s %11s" % (quantity + " factor", "episodes", "fall share", "mean dist", "mean frames")]
    for i in range(a.bins):
        m = (f >= edges[i]) & ((f < edges[i + 1]) | (i == a.bins - 1))
        n = int(m.sum())
        lines.append("%5.2f..%-5.2f %9d %10s %10s %11s" % (edges[i], edges[i + 1], n, *(("%.3f" % v) if n else "-" for v in
                     ((rows["cause"][m] == 1).mean() if n else 0, rows["dist"][m].mean() if n else 0, rows["frames"][m].mean() if n else 0))))
    return lines


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--character", default="dog", choices=sorted(POLICY))
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--frames", type=int, default=600)
    ap.add_argument("--chunk", type=int, default=50, help="frames per RunFrames call and drain")
    ap.add_argument("--capacity", type=int, default=65536, help="rows per ring of the episode log")
    ap.add_argument("--limit", type=int, nargs=2, default=[60, 120], metavar=("LO", "HI"), help="episode limit in frames")
    ap.add_argument("--mass-range", type=float, nargs=2, default=[0.7, 1.5])
    ap.add_argument("--torque-range", type=float, nargs=2, default=[0.6, 1.2])
    ap.add_argument("--bins", type=int, default=4)
    ap.add_argument("--seed", type=int, default=11)
    a = ap.parse_args(argv)
    rows, fac, lost = run(a)
    n = len(rows["env"])
    print("# tools/episode_outcomes.py: %s, %d envs, %d frames in chunks of %d, limit %d .. %d frames, mass x [%g, %g], torque_lim x [%g, %g]" % (a.character, a.envs, a.frames, a.chunk, *a.limit, *a.mass_range, *a.torque_range))
    print("# %d episodes drained (%d rows lost), %.3f ended by a fall, mean distance %.3f" % (n, lost, float((rows["cause"] == 1).mean()) if n else 0.0, float(rows["dist"].mean()) if n else 0.0))
    for quantity, q in (("mass", 0), ("torque_lim", 3)):
        print("\n".join(table(rows, fac, a, quantity, q)))


if __name__ == "__main__":
    main()
