#!/usr/bin/env python3
"""Record a rollout with the frame trace (include/dtrl.h dtrl_trace) and write it out for the reference's viewer.
GPU:  python tools/trace_export.py --arg-file args/dog_slopes_mixed_args.txt --model data/policies/dog/models/dog_mace3_slopes_mixed_model.h5 \
          --envs 64 --trace 0 5 9 --frames 300 --out out/trace

Runs a batch under a policy file for --frames frames with a trace on the chosen envs -- every frame queued at once, the host does not look at the batch in between
(RunFrames) -- and writes
  <out>.npz                        every named array of TraceRead (time, phase, q, qd, tau, row, need_reset, ... terrain, count, env_ids)
  <out>_env<e>_ep<k>.txt           per traced env and episode one motion file in the reference's own format, {"Motion": {"Loop": false, "Frames": [[1/30, q...], ...]}}
                                   (cMotion::Load, anim/Motion.cpp:109-171: a frame is its duration followed by the pose), which its viewer plays with -motion_file=
An env's rows are split into episodes behind every row with need_reset & 1: that row is the episode's last pose, the fallen one included."""
import argparse, json, os, sys
import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

FRAME_DT = 1.0 / 30.0


def split_episodes(need_reset):
    """[(first row, one past the last row)] of each episode: a cut behind every row with need_reset & 1"""
    out, start = [], 0
    for r, v in enumerate(need_reset):
        if int(v) & 1:
            out.append((start, r + 1)); start = r + 1
    if start < len(need_reset):
        out.append((start, len(need_reset)))
    return out


def motion_doc(q_rows, dt=FRAME_DT):
    """The reference's motion format: every frame is [duration, pose...]"""
    return {"Motion": {"Loop": False, "Frames": [[dt] + [float(x) for x in q] for q in q_rows]}}


def write_trace(tr, out):
    """tr: TraceRead's dict. Writes <out>.npz and the motion files; returns {env id: [motion file of episode 0, 1, ...]}"""
    d = os.path.dirname(os.path.abspath(out))
    os.makedirs(d, exist_ok=True)
    np.savez(out + ".npz", **{k: v for k, v in tr.items() if k not in ("vals", "ints")})
    files = {}
    for i, e in enumerate(tr["env_ids"]):
        c = int(tr["count"][i])
        files[int(e)] = []
        for k, (r0, r1) in enumerate(split_episodes(tr["need_reset"][i, :c])):
            path = "%s_env%d_ep%d.txt" % (out, int(e), k)
            with open(path, "w") as f:
                json.dump(motion_doc(tr["q"][i, r0:r1]), f)
            files[int(e)].append(path)
    return files


def record(b, frames, env_ids=None):
    """`frames` frames of batch b under a trace of env_ids (None: all), read back whole"""
    b.Trace(env_ids, frames=frames)
    if b.external:
        raise SystemExit("trace_export drives the batch itself: not with -policy_mode= external")
    b.RunFrames(frames)
    return b.TraceRead()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arg-file", required=True)
    ap.add_argument("--data-root", default=os.path.join(REPO, "tests", "golden", "refdata"))
    ap.add_argument("--model", default="", help="policy file for LoadModel (Caffe HDF5; its _scale.txt beside it); none: the arg file's own")
    ap.add_argument("--envs", type=int, default=16)
    ap.add_argument("--trace", type=int, nargs="*", default=None, help="env ids to trace (default: all)")
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--device-terrain", action="store_true")
    ap.add_argument("--out", required=True, help="path prefix of the files written")
    a = ap.parse_args()
    import deepterrainrl_amd as da
    b = da.BatchScenario(a.arg_file, a.envs, data_root=a.data_root, extra_args=dict(terrain_gen="device") if a.device_terrain else None)
    if a.model:
        b.LoadModel(a.model)
    tr = record(b, a.frames, a.trace)
    files = write_trace(tr, a.out)
    print("%s.npz: %d envs x up to %d rows" % (a.out, len(tr["env_ids"]), tr["q"].shape[1]))
    for e, fs in files.items():
        print("env %d: %d episodes -> %s" % (e, len(fs), ", ".join(os.path.basename(f) for f in fs)))
    b.close()


if __name__ == "__main__":
    main()
