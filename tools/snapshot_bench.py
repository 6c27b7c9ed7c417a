#!/usr/bin/env python3
"""What do env snapshots cost? (docs/EXPERIMENTS.md 15, profiles/r08_snapshot.txt)

Full-batch save, restore, all-to-all clone shift, export and import at the BASELINE widths (4096 dogs on slopes_mixed, 8192 raptors on narrow_gaps), each
as the median of --reps repetitions after warm-up: wall clock of the call, and for the calls that launch a kernel the device time of the launch (HIP events,
the library's dtrlx_snapshot_launch_ms hook). The same save and restore again through the Backend defaults built from one D2D copy per record and env
(DTRL_SNAPSHOT_FALLBACK=1), and one frame of the same batch for scale.

Usage: python tools/snapshot_bench.py [--reps 20] [--configs dog,raptor] [--fallback-reps 3]
"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import numpy as np  # noqa: E402

HBM_PEAK_GBS = 8000.0   # MI355X HBM3E peak


def timed(b, fn, reps, warm=3):
    wall, dev = [], []
    hook = b._lib.dtrlx_snapshot_launch_ms
    hook.restype = C.c_double; hook.argtypes = [C.c_void_p]
    for k in range(warm + reps):
        hook(b._h)
        t0 = time.perf_counter(); fn(); t1 = time.perf_counter()
        ms = hook(b._h)
        if k >= warm:
            wall.append((t1 - t0) * 1e3); dev.append(ms)
    return statistics.median(wall), statistics.median(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--fallback-reps", type=int, default=3)
    ap.add_argument("--configs", default="dog,raptor")
    a = ap.parse_args()
    import deepterrainrl_amd as da
    da.configure_hw_queues()
    from oracle import model as om
    import test_snapshot as T
    for name in a.configs.split(","):
        which, n = {"dog": (T.DOG, 4096), "raptor": (T.RAPTOR, 8192)}[name]
        b = T.make(da.BatchScenario, om, n, which)
        b.RunFrames(40)
        b.DrainTuples()
        b.KernelTimeMs()
        t0 = time.perf_counter(); b.RunFrames(20); frame_ms = (time.perf_counter() - t0) * 1e3 / 20
        b.DrainTuples()
        snap = b.SaveState()
        per_env = snap.bytes_per_env
        total_mb = per_env * n / 1e6
        rows = []
        keep = []

        def save():
            keep.append(b.SaveState())
            if len(keep) > 2:
                keep.pop(0).free()
        rows.append(("save, full batch",) + timed(b, save, a.reps))
        rows.append(("restore, full batch",) + timed(b, lambda: b.RestoreState(snap), a.reps))
        src = np.arange(0, n - 1, dtype=np.int32); dst = src + 1
        rows.append(("clone_envs, shift i -> i + 1 (staged: 2 launches)",) + timed(b, lambda: b.CloneEnvs(src, dst), a.reps))
        half = np.arange(0, n // 2, dtype=np.int32)
        rows.append(("clone_envs, lower half -> upper half (1 launch)",) + timed(b, lambda: b.CloneEnvs(half, half + n // 2), a.reps))
        blob = [None]

        def export():
            blob[0] = snap.export()
        rows.append(("export (device -> host blob)",) + timed(b, export, a.reps))
        imps = []

        def imp():
            imps.append(b.ImportState(blob[0]))
            if len(imps) > 2:
                imps.pop(0).free()
        rows.append(("import (host blob -> device)",) + timed(b, imp, a.reps))
        os.environ["DTRL_SNAPSHOT_FALLBACK"] = "1"
        rows.append(("save, copy-per-record fallback",) + timed(b, save, a.fallback_reps, warm=1))
        rows.append(("restore, copy-per-record fallback",) + timed(b, lambda: b.RestoreState(snap), a.fallback_reps, warm=1))
        del os.environ["DTRL_SNAPSHOT_FALLBACK"]
        print("== %s: %d envs, %d B per env in device memory (+ %d B host), %.1f MB per full-batch snapshot; one frame of this batch: %.2f ms wall"
              % (name, n, per_env, snap.host_bytes_per_env, total_mb, frame_ms))
        print("%-52s %12s %12s %14s %10s" % ("call (median of %d)" % a.reps, "wall ms", "launch ms", "GB/s (r + w)", "of HBM"))
        for what, w, d in rows:
            moved = 2 * total_mb / 1e3                       # GB read + written
            if "half" in what:
                moved /= 2
            if "shift" in what:
                moved *= 2
            if d > 0:
                bw = moved / (d * 1e-3)
                print("%-52s %12.3f %12.3f %14.0f %9.1f%%" % (what, w, d, bw, 100 * bw / HBM_PEAK_GBS))
            else:
                print("%-52s %12.3f %12s %14s %10s" % (what, w, "-", "-", "-"))
        sys.stdout.flush()
        for s in keep + imps + [snap]:
            s.free()
        b.close()


if __name__ == "__main__":
    main()
