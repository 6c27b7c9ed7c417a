"""The drop-in boundary: include/dtrl.h is plain C, include/BatchScenarioExp.h compiles inside the reference's own header tree and
drives frames, and the batch-level counterparts of cScenarioPoliEval::GetDistLog / ResetAvgDist, the tuple hand-over (host and device
destinations, overflow accounting) and the argument checks behave as the header says. CPU tests use the lane-loop build of the kernel
source (tests/emul); test_gpu_parity.py re-runs the behavioural ones through libdtrl.so on the GPU."""
import os
import struct
import subprocess

import numpy as np
import pytest

from conftest import EMUL_LIB, HIP_LIB, REFDATA, REPO, EmulScenario, dog_policy, pin_to_oracle

Scenario = EmulScenario   # the GPU twin points this at the product class
SHIM_DIR = os.path.join(REPO, "oracle", "_ref", "shim")   # built from tests/shim/*.cpp by oracle/_ref_build/shim.mk


def _hip_link_flags():
    return ["-L" + os.path.dirname(HIP_LIB), "-ldtrl", "-Wl,-rpath," + os.path.dirname(HIP_LIB), "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath,/opt/rocm/lib"]


def test_header_is_plain_c99_and_links(tmp_path):
    """include/dtrl.h must be consumable from C (the FFI a cgo / JNI / ctypes binding would see): compile with gcc -std=c99 -pedantic, link against
    the HIP library, call the entry points that need no device."""
    src = tmp_path / "use_dtrl.c"
    src.write_text(r'''
#include <stdio.h>
#include <string.h>
#include "dtrl.h"
int main(void)
{
	dtrl_batch* b = NULL;
	const char* argv[] = {"-character_file=", "does/not/exist.txt", "-char_ctrl=", "dog"};
	float strip[512]; int n = 0, found = 0, ntok = 0; double w = 0; char val[64];
	double prm[40]; int i;
	dtrl_status rc;
	for (i = 0; i < 40; ++i) prm[i] = 0;
	prm[0] = 4; prm[1] = 7; prm[2] = 0.5; prm[3] = 2; prm[4] = -2; prm[5] = -2;
	printf("version=%s\n", dtrl_version());
	rc = dtrl_create(argv, 4, 1, -1, &b);
	printf("create=%d handle=%s msg=%s\n", (int)rc, b ? "set" : "null", dtrl_last_error(NULL));
	rc = dtrl_terrain_build("gaps", prm, 7u, 20.0, strip, 512, &n, &w);
	printf("terrain=%d n=%d w=%.3f\n", (int)rc, n, w);
	rc = dtrl_args_parse_string(argv, 4, "char_ctrl", val, 64, &found, &ntok);
	printf("args=%d found=%d val=%s ntok=%d\n", (int)rc, found, val, ntok);
	return (sizeof(dtrl_status) == sizeof(int) && DTRL_TUPLE_EXP_ACTOR == 4u && rc == DTRL_OK) ? 0 : 1;
}
''')
    exe = tmp_path / "use_dtrl"
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I" + os.path.join(REPO, "include"), str(src), "-o", str(exe)] + _hip_link_flags(),
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    out = r.stdout
    assert "version=dtrl-mi355x" in out and "handle=null" in out and "terrain=0 n=2" in out and "found=1 val=dog ntok=4" in out
    # a missing data file is an I/O error with a message, never a crash; without a device the create path would say so instead
    assert "create=2" in out or "create=3" in out


def _write_policy(path, pol, n_out):
    desc, w, io, isc, oo, osc = pol
    with open(path, "wb") as f:
        f.write(struct.pack("<q", len(w)))
        f.write(np.asarray(w, np.float32).tobytes())
        for a in (io, isc, oo, osc):
            f.write(np.asarray(a, np.float64).tobytes())


def _run_shim(exe, tmp_path, om, frames=100, n_envs=12):
    pol = dog_policy(om)
    pfile = tmp_path / "policy.bin"
    _write_policy(pfile, pol, 90)
    r = subprocess.run([exe, REFDATA, "args/opt_args_train_mace.txt", str(n_envs), str(frames), str(pfile), "-terrain_seed=", "77", "-rand_seed=", "3"],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    return r.stdout.strip().splitlines(), pol


def _python_side(frames, n_envs, pol, scenario=None):
    """what the shim must reproduce: the same batch driven through the Python mirror"""
    b = (scenario or Scenario)("args/opt_args_train_mace.txt", n_envs, data_root=REFDATA, extra_args={"terrain_seed": 77, "rand_seed": 3})
    b.SetPolicy(pol[1], *pol[2:])
    b.SetExplore(True, 0.2, 0.025, 0.002)
    b.Reset()
    S, A = b.S, b.A
    buf_r, buf_f, buf_i = [], [], []
    lines = []
    total = 0
    for fr in range(frames):
        b.Update()
        r, fl, ids = b.DrainTuples()
        buf_r += list(r); buf_f += list(fl); buf_i += list(ids)
        if len(buf_r) >= 32:
            rows = np.array(buf_r, np.float64)
            sr = rows[:, 0].sum()
            ss = (rows[:, 1:1 + S] - 0.5 * rows[:, 1 + S + A:]).sum()
            sa = rows[:, 1 + S:1 + S + A].sum()
            h = 0
            for f_, i_ in zip(buf_f, buf_i):
                h ^= (int(f_) * 2654435761 + int(i_)) & 0xFFFFFFFF
            lines.append((fr, len(buf_r), sr, ss, sa, h))
            total += len(buf_r)
            buf_r, buf_f, buf_i = [], [], []
    return lines, total


def _check_shim_output(lines, py_lines, py_total):
    assert lines[0].startswith("name=Batch Exploration envs=12 S=283 A=30 O=90")
    got = [l for l in lines if l.startswith("frame=")]
    assert len(got) == len(py_lines) >= 1
    for l, (fr, n, sr, ss, sa, h) in zip(got, py_lines):
        kv = dict(x.split("=") for x in l.split())
        assert int(kv["frame"]) == fr and int(kv["tuples"]) == n and int(kv["flags_hash"]) == h
        for key, ref in (("reward_sum", sr), ("state_sum", ss), ("action_sum", sa)):
            assert abs(float(kv[key]) - ref) <= 1e-6 * max(1.0, abs(ref)), (l, key, ref)
    assert lines[-1] == "total=%d" % py_total


@pytest.mark.skipif(not os.path.exists(os.path.join(SHIM_DIR, "drive_shim_emul")), reason="oracle/_ref/shim/drive_shim_emul not built (needs the reference headers at build time)")
def test_shim_header_compiles_in_the_reference_tree_and_drives_frames(tmp_path, om):
    """include/BatchScenarioExp.h : cScenario built against the reference's own scenarios/Scenario.h, learning/ExpTuple.h, util/ArgParser.h, then
    100 outer frames through ParseArgs / Init / SetPolicy / Reset / Update / IsTupleBufferFull / GetTuples / ResetTupleBuffer."""
    r = subprocess.run(["make", "-C", os.path.join(REPO, "oracle", "_ref_build"), "shim"], capture_output=True, text=True)   # rebuilt where the reference tree exists
    assert r.returncode == 0, r.stderr[-3000:]
    lines, pol = _run_shim(os.path.join(SHIM_DIR, "drive_shim_emul"), tmp_path, om)
    py_lines, py_total = _python_side(100, 12, pol)
    _check_shim_output(lines, py_lines, py_total)


def run_eval_shim(exe, tmp_path, om, scenario, pool=6, max_episodes=14, max_cycles=100000, seed=4242):
    """include/BatchScenarioPoliEval.h driven like cOptScenarioPoliEval drives its pool (tests/shim/drive_shim_eval.cpp) vs the same protocol through the
    Python mirror: per-scene seeds (drawn by the reference's own cRand inside the shim), every fold of the record (episodes, cycles, running average
    distance), the dist log and the OutputResults line."""
    pol = dog_policy(om)
    pfile = tmp_path / "policy.bin"
    _write_policy(pfile, pol, 90)
    out_file = tmp_path / "eval_results.txt"
    r = subprocess.run([exe, REFDATA, "args/dog_slopes_mixed_args.txt", str(pool), str(max_episodes), str(max_cycles), str(pfile), str(seed), str(out_file), "-terrain_seed=", "77"],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    lines = r.stdout.strip().splitlines()
    seeds = [int(x) for x in lines[0].split("=")[1].split()]
    assert lines[0].startswith("seeds=") and len(seeds) == pool and len(set(seeds)) == pool
    assert lines[1] == "name=Batch Policy Evaluation pool=%d S=283 O=90" % pool
    # the same protocol through the Python mirror
    b = scenario("args/dog_slopes_mixed_args.txt", pool, data_root=REFDATA, extra_args={"terrain_seed": 77})
    b.SetPolicy(pol[1], *pol[2:])
    b.Reset(terrain_seeds=np.asarray(seeds, np.uint64))
    per_update = 10 * pool
    num_ep = num_cy = prev_cy = rec_ep = rec_cy = frames = 0
    rec_avg = 0.0
    folds = []
    while num_ep < max_episodes and num_cy < max_cycles:
        b.Update(); frames += 1
        st = b.EvalStats()
        num_cy = st["cycles"]; cur = st["episodes"]
        if cur >= per_update or cur + num_ep >= max_episodes:
            rec_avg = (rec_avg * rec_ep + st["avg_dist"] * cur) / max(rec_ep + cur, 1)      # cMathUtil::AddAverage
            rec_ep += cur; rec_cy += num_cy - prev_cy
            folds.append((frames, rec_ep, rec_cy, rec_avg))
            b.ResetAvgDist()
            num_ep += cur; prev_cy = num_cy
    got = [l for l in lines if l.startswith("fold ")]
    assert len(got) == len(folds) >= 1
    for l, (fr, ep, cy, avg) in zip(got, folds):
        kv = dict(x.split("=") for x in l.split()[1:])
        assert int(kv["frame"]) == fr and int(kv["episodes"]) == ep and int(kv["cycles"]) == cy and abs(float(kv["avg_dist"]) - avg) < 1e-6 * max(1.0, abs(avg)), (l, fr, ep, cy, avg)
    d, ids = b.GetDistLog()
    kv = dict(x.split("=") for x in lines[-1].split())
    assert int(kv["frames"]) == frames and int(kv["dist_log"]) == len(d) >= max_episodes and abs(float(kv["dist_sum"]) - d.sum()) < 1e-6 * max(1.0, abs(d.sum()))
    line = open(out_file).read()
    assert line == ", ".join("%f" % x for x in d) + "\n"            # std::to_string per entry, pool order
    return lines


@pytest.mark.skipif(not os.path.exists(os.path.join(SHIM_DIR, "drive_shim_eval_emul")), reason="oracle/_ref/shim/drive_shim_eval_emul not built (needs the reference headers at build time)")
def test_poli_eval_shim_compiles_in_the_reference_tree_and_runs_the_eval_loop(tmp_path, om):
    """include/BatchScenarioPoliEval.h : cScenario built against the reference's own scenarios/Scenario.h, util/ArgParser.h, util/Rand.h (VERDICT r2 missing #3)."""
    r = subprocess.run(["make", "-C", os.path.join(REPO, "oracle", "_ref_build"), "shim"], capture_output=True, text=True)   # rebuilt where the reference tree exists
    assert r.returncode == 0, r.stderr[-3000:]
    run_eval_shim(os.path.join(SHIM_DIR, "drive_shim_eval_emul"), tmp_path, om, Scenario)


def test_dist_log_avg_dist_and_output_results(da, om, tmp_path):
    """cScenarioPoliEval::RecordDistTraveled / GetDistLog / GetAvgDist / ResetAvgDist and cOptScenarioPoliEval::OutputResults over the batch."""
    m, _ = om.build_model("args/dog_slopes_mixed_args.txt", REFDATA)
    pol = dog_policy(om)
    n = 6
    b = Scenario("args/dog_slopes_mixed_args.txt", n, data_root=REFDATA, extra_args={"terrain_seed": 40})
    b.SetPolicy(pol[1], *pol[2:])
    es = [om.OracleEnv(m, terrain_seed=40 + i, rng_seed=0, env_id=i, policy=pol) for i in range(n)]
    for f in range(150):
        b.Update()
        for e in es:
            e.update()
        pin_to_oracle(b, es)   # every frame from a common state (conftest.pin_to_oracle): an episode's distance then agrees to the growth of its last frame
    d, ids = b.GetDistLog()
    st = b.EvalStats()
    assert len(d) == st["episodes"] >= 3 and np.all(np.diff(ids) >= 0)
    assert abs(d.mean() - st["avg_dist"]) < 1e-9
    # every env's first logged episode against the oracle's: an episode ends after a tumble (chaotic: rounding differences grow ~100x per
    # frame there, DESIGN 'Chaos note'), so the distance at the fall agrees closely, not bitwise; some envs stay in lock-step to the end
    n_first = n_tight = 0
    for i, e in enumerate(es):
        mine, theirs = d[ids == i], e.dist_log()
        if len(mine) and len(theirs):
            assert abs(mine[0] - theirs[0]) < 1.0, (i, mine, theirs)
            n_first += 1
            n_tight += abs(mine[0] - theirs[0]) < 1e-6
    assert n_first >= 3 and n_tight >= 1
    out = tmp_path / "dist.txt"
    b.OutputResults(str(out)); b.OutputResults(str(out))
    txt = out.read_text().splitlines()
    assert len(txt) == 2 and txt[0] == txt[1] == ", ".join("%f" % x for x in d)     # std::to_string == "%f"
    b.ResetAvgDist()
    st2 = b.EvalStats()
    assert st2["episodes"] == 0 and st2["avg_dist"] == 0 and st2["cycles"] == st["cycles"]
    assert len(b.GetDistLog()[0]) == len(d)                                         # the log is kept (cleared by Clear / Init only)
    for f in range(60):
        b.Update()
    st3 = b.EvalStats()
    d3, _ = b.GetDistLog()
    assert st3["episodes"] == len(d3) - len(d)


def test_tuple_ring_overflow_is_counted_never_silent(da, om):
    """The reference never loses a tuple; here a full ring drops rows but COUNTS them, so a caller that drains too rarely can tell."""
    pol = dog_policy(om)
    args = dict(terrain_seed=300, rand_seed=9)
    a = Scenario("args/opt_args_train_mace.txt", 8, data_root=REFDATA, extra_args=args)
    a.SetPolicy(pol[1], *pol[2:])
    total = 0
    for f in range(120):
        a.Update()
        total += len(a.DrainTuples()[0])
    sa = a.TupleStats()
    assert sa["dropped"] == 0 and sa["drained"] == total > 16 and sa["pending"] == 0 and sa["capacity"] == 32
    b = Scenario("args/opt_args_train_mace.txt", 8, data_root=REFDATA, extra_args=dict(args, tuple_ring_capacity=5))
    b.SetPolicy(pol[1], *pol[2:])
    b.RunFrames(120)
    sb = b.TupleStats()
    assert sb["capacity"] == 5 and sb["pending"] == 5 and sb["dropped"] == total - 5 and sb["drained"] == 0
    rows, fl, ids = b.DrainTuples()
    assert len(rows) == 5
    sb = b.TupleStats()
    assert sb["pending"] == 0 and sb["drained"] == 5 and sb["dropped"] == total - 5


def test_device_destination_drain_and_policy_hand_over_equal_the_host_calls(da, om):
    """dtrl_drain_tuples_device / dtrl_set_policy_device: same rows, same rollout as the host-pointer calls (on the lane-loop backend "device"
    memory is host memory; the GPU twin passes torch CUDA tensors)."""
    pol = dog_policy(om)
    args = dict(terrain_seed=31, rand_seed=2)
    a = Scenario("args/opt_args_train_mace.txt", 6, data_root=REFDATA, extra_args=args)
    b = Scenario("args/opt_args_train_mace.txt", 6, data_root=REFDATA, extra_args=args)
    a.SetPolicy(pol[1], *pol[2:])
    w = np.ascontiguousarray(pol[1], np.float32); nv = [np.ascontiguousarray(x, np.float64) for x in pol[2:]]
    b.SetPolicyDevice(w.ctypes.data, w.size, *[x.ctypes.data for x in nv])
    cap = 64
    rows = np.zeros((cap, b.W), np.float32); fl = np.zeros(cap, np.uint32); ids = np.zeros(cap, np.int32)
    n_tot = 0
    for f in range(90):
        a.Update(); b.Update()
        ra, fa, ia = a.DrainTuples()
        nb = b.DrainTuplesDevice(rows.ctypes.data, fl.ctypes.data, ids.ctypes.data, cap)
        assert nb == len(ra)
        assert np.array_equal(rows[:nb], ra) and np.array_equal(fl[:nb], fa) and np.array_equal(ids[:nb], ia)
        n_tot += nb
    assert n_tot >= 6
    assert np.array_equal(a.PoseVel()[0], b.PoseVel()[0])


def run_policy_hand_over_during_a_frame(scn, om, to_dev=None, n_envs=8, frames=40, stream_ptr=None):
    """dtrl_set_policy_device between dtrl_step_begin and dtrl_step_end does not wait for the frame: the weights go to the second buffer and the NEXT launch uses
    them -- the same rollout as handing them over after dtrl_step_end. Policies alternate every third frame so that a missed or early switch shows."""
    pol = dog_policy(om)
    rng = np.random.RandomState(12)
    w0 = np.ascontiguousarray(pol[1], np.float32)
    ws = [w0, (w0 * (1 + 0.05 * rng.normal(size=w0.size))).astype(np.float32), (w0 * (1 + 0.05 * rng.normal(size=w0.size))).astype(np.float32)]
    to_dev = to_dev or (lambda x: (x, x.ctypes.data))
    held = [to_dev(w) for w in ws]
    args = dict(terrain_seed=31, rand_seed=2)
    a = scn("args/opt_args_train_mace.txt", n_envs, data_root=REFDATA, extra_args=args)
    b = scn("args/opt_args_train_mace.txt", n_envs, data_root=REFDATA, extra_args=args)
    for x in (a, b):
        x.SetPolicy(pol[1], *pol[2:])
    a.UpdateBegin()
    for f in range(frames):
        k = (f // 3 + f // 9) % 3                              # (policy index and hand-over form both cycle with period 3: shift one against the other)
        if f % 3 == 0:                                      # frame f in flight on `a`: parked, effective from frame f + 1
            form = (f // 3) % 3
            if form == 0:
                a.SetPolicyDevice(held[k][1], w0.size)
            elif form == 1:
                a.SetPolicyDeviceOn(held[k][1], w0.size, stream_ptr)     # the same with the re-layout kernel on a stream of the caller's (None: the engine's)
            else:
                a.SetPolicyDeviceAsync(held[k][1], w0.size, stream_ptr)  # no host wait at all: the next launches wait for the re-layout kernel on the device
        a.UpdateEnd()
        b.Update()                                          # frame f on `b` with the weights frame f of `a` ran with
        if f % 3 == 0:
            b.SetPolicyDevice(held[k][1], w0.size)          # between frames: the waiting form
        pa, pb = a.PoseVel(), b.PoseVel()
        assert np.array_equal(pa[0], pb[0]) and np.array_equal(pa[1], pb[1]), f
        a.UpdateBegin()
    a.UpdateEnd()
    b.Update()
    ya, yb = a.PolicyOutput(), b.PolicyOutput()
    assert np.array_equal(a.PoseVel()[0], b.PoseVel()[0])
    assert np.abs(ya).max() > 0 and np.array_equal(ya, yb)


def test_policy_hand_over_during_a_frame(da, om):
    run_policy_hand_over_during_a_frame(Scenario, om)


def run_packed_drain_equals_plain_drain(scn, om, to_ptr=None, read=None, n_envs=10, cap=32, small=2, frames=120, every=3, ring_cap=None, extra_b=None,
                                        min_drain=0, min_multi_envs=0, min_carry=0):
    """dtrl_drain_tuples_packed: the rows of dtrl_drain_tuples sorted by env id (stable), flag word and GLOBAL env id appended, a header row with the
    count. Rows that do not fit the caller's block are CARRIED, not dropped: they stay in the ring, in order, in front of the newer rows, and a later
    drain hands them out -- a consumer with a small block (two rows here) receives every row of the big-block stream, each env's rows in time order.
    The width parameters (tests/test_gpu_handover_width.py): n_envs envs drained every `every` frames into blocks of `cap` (always fits) and `small` rows,
    rings of ring_cap rows, extra_b for the two packed batches; min_drain / min_multi_envs / min_carry are floors on the largest drain of `b`, on the envs with
    two or more rows in one drain of `b` and on the largest carry in a header of `c`. Returns what was reached."""
    pol = dog_policy(om)
    args = dict(terrain_seed=31, rand_seed=2, global_env_offset=100)
    if ring_cap is not None:
        args["tuple_ring_capacity"] = ring_cap
    a = scn("args/opt_args_train_mace.txt", n_envs, data_root=REFDATA, extra_args=args)
    b = scn("args/opt_args_train_mace.txt", n_envs, data_root=REFDATA, extra_args=dict(args, **(extra_b or {})))
    c = scn("args/opt_args_train_mace.txt", n_envs, data_root=REFDATA, extra_args=dict(args, **(extra_b or {})))
    for x in (a, b, c):
        x.SetPolicy(pol[1], *pol[2:])
    W = a.W
    if to_ptr is None:
        blk = np.zeros((cap + 1, W + 2), np.float32); blk_c = np.zeros((small + 1, W + 2), np.float32)
        to_ptr = lambda t: t.ctypes.data; read = lambda t: t
    else:
        import torch
        blk = torch.zeros((cap + 1, W + 2), dtype=torch.float32, device="cuda"); blk_c = torch.zeros((small + 1, W + 2), dtype=torch.float32, device="cuda")
    n_tot = n_multi = carried_max = drain_max = multi_envs_max = 0
    big, small_rows = [], []
    pending_c = 0
    for f in range(frames):
        for x in (a, b, c):
            x.Update()
        if f % every != every - 1:
            continue                                                   # drain every third frame (by default): several tuples per drain, some envs twice over time
        ra, fa, ia = a.DrainTuples(ring_cap)
        n = b.DrainTuplesPacked(to_ptr(blk), cap, want_count=True)
        h = read(blk)
        assert n == len(ra) and h[0, :3].view(np.int32).tolist() == [n, 0, 0]
        order = np.argsort(ia, kind="stable")
        assert np.array_equal(h[1:n + 1, :W], ra[order])
        meta = h[1:n + 1, W:].view(np.int32)
        assert np.array_equal(meta[:, 0], fa[order].astype(np.int32)) and np.array_equal(meta[:, 1], ia[order] + 100)
        n_tot += n; n_multi += n >= 2
        drain_max = max(drain_max, n)
        multi_envs_max = max(multi_envs_max, int((np.bincount(meta[:, 1] - 100, minlength=n_envs) >= 2).sum()))   # (from b's own id column)
        big.append(h[1:n + 1].copy())
        # a block with room for `small` rows only: the first rows in (env id, time) order of what is pending, the rest carried and counted in the header
        pending_c += n
        m = c.DrainTuplesPacked(to_ptr(blk_c), small, want_count=True)
        hc = read(blk_c)
        assert m == min(pending_c, small) and hc[0, :3].view(np.int32).tolist() == [m, 0, pending_c - m]
        pending_c -= m; carried_max = max(carried_max, int(hc[0, 2:3].view(np.int32)[0]))
        small_rows.append(hc[1:m + 1].copy())
        assert c.TupleStats()["pending"] == pending_c
    assert n_tot >= 12 and n_multi >= 3 and carried_max >= 2
    reached = dict(drain_max=drain_max, multi_envs_max=multi_envs_max, carried_max=carried_max, rows=n_tot)
    print("packed drain at %d envs: %s" % (n_envs, reached))
    assert drain_max > min_drain and multi_envs_max >= min_multi_envs and carried_max > min_carry, reached
    while pending_c > 0:                                                  # flush what the small block left behind
        m = c.DrainTuplesPacked(to_ptr(blk_c), small, want_count=True)
        assert m == min(pending_c, small)
        pending_c -= m
        small_rows.append(read(blk_c)[1:m + 1].copy())
    big, small_rows = np.concatenate(big), np.concatenate(small_rows)
    assert len(big) == len(small_rows) == n_tot
    ids_b, ids_s = big[:, W + 1].view(np.int32), small_rows[:, W + 1].view(np.int32)
    ob, os_ = np.argsort(ids_b, kind="stable"), np.argsort(ids_s, kind="stable")
    assert np.array_equal(ids_b[ob], ids_s[os_])
    assert np.array_equal(big[ob].view(np.int32), small_rows[os_].view(np.int32))   # every env: the same rows in the same (time) order (as bit patterns: a NaN equals itself)
    sb, sc = b.TupleStats(), c.TupleStats()
    assert sb["drained"] == n_tot and sb["dropped"] == 0 and sb["pending"] == 0
    assert sc["drained"] == n_tot and sc["dropped"] == 0 and sc["pending"] == 0
    return reached


def test_packed_drain_equals_plain_drain(da, om):
    run_packed_drain_equals_plain_drain(Scenario, om)


def run_packed_drain_of_a_full_ring(scn, om, to_ptr=None, read=None, n_envs=1100, ring=1500, block=1200, frames=40, more_frames=6, min_lost=256):
    """A packed drain of a ring that overflowed: header [block, lost, ring - block]. `a` is the twin with a ring that holds everything. Which rows of the frame
    that filled the ring got in is decided by the cursor atomics, so `b`'s rows are held to properties: sorted by env id across both drains, every row (with its
    flag word) a row of `a` of that env, none twice, each env's rows a subsequence of `a`'s in `a`'s order, and every row of the frames that ended before the ring
    was full present. Afterwards both batches run on and their streams agree again: cursor and counters were reset. Returns the rows lost."""
    pol = dog_policy(om)
    args = dict(terrain_seed=31, rand_seed=2, global_env_offset=100)
    big_ring = 8 * n_envs
    a = scn("args/opt_args_train_mace.txt", n_envs, data_root=REFDATA, extra_args=dict(args, tuple_ring_capacity=big_ring))
    b = scn("args/opt_args_train_mace.txt", n_envs, data_root=REFDATA, extra_args=dict(args, tuple_ring_capacity=ring))
    for x in (a, b):
        x.SetPolicy(pol[1], *pol[2:])
    W = a.W
    if to_ptr is None:
        blk = np.zeros((max(block, ring) + 1, W + 2), np.float32)
        to_ptr = lambda t: t.ctypes.data; read = lambda t: t
    else:
        import torch
        blk = torch.zeros((max(block, ring) + 1, W + 2), dtype=torch.float32, device="cuda")
    whole = 0                                                            # rows of `a` written by the frames that ended with the ring not yet full
    for f in range(frames):
        a.Update(); b.Update()
        pa = a.TupleStats()["pending"]
        if pa <= ring:
            whole = pa
    sa = a.TupleStats()
    total_a = sa["pending"]
    lost = total_a - ring
    print("full ring at %d envs: %d rows in the twin, ring of %d, %d lost, %d from whole frames" % (n_envs, total_a, ring, lost, whole))
    assert sa["dropped"] == 0 and sa["capacity"] == big_ring and lost >= min_lost and 0 < whole <= ring
    sb = b.TupleStats()
    assert (sb["capacity"], sb["pending"], sb["dropped"], sb["drained"]) == (ring, ring, lost, 0)
    ra, fa, ia = a.DrainTuples(big_ring)                                 # ring order: frame by frame
    assert len(ra) == total_a
    n1 = b.DrainTuplesPacked(to_ptr(blk), block, want_count=True)
    h1 = read(blk)[:block + 1].copy()
    assert n1 == block and h1[0, :3].view(np.int32).tolist() == [block, lost, ring - block]
    sb = b.TupleStats()
    assert (sb["pending"], sb["dropped"], sb["drained"]) == (ring - block, lost, block)
    n2 = b.DrainTuplesPacked(to_ptr(blk), block, want_count=True)
    h2 = read(blk)[:ring - block + 1].copy()
    assert n2 == ring - block and h2[0, :3].view(np.int32).tolist() == [ring - block, 0, 0]
    sb = b.TupleStats()
    assert (sb["pending"], sb["dropped"], sb["drained"]) == (0, lost, ring)
    out = np.concatenate([h1[1:], h2[1:]]).view(np.int32)                # bit patterns: rows, flag word, global env id
    ids_b = out[:, W + 1] - 100
    assert len(out) == ring and np.all(np.diff(ids_b) >= 0) and ids_b[0] >= 0 and ids_b[-1] < n_envs
    key = lambda row, flag: row.tobytes() + int(flag).to_bytes(4, "little", signed=True)
    rows_a = {}
    ra_i, fa_i = ra.view(np.int32), fa.astype(np.int32)
    for k in range(total_a):
        rows_a.setdefault(int(ia[k]), []).append(key(ra_i[k], fa_i[k]))
    got = set()
    at = {}
    for k in range(ring):
        e = int(ids_b[k]); kb = key(out[k, :W], out[k, W])
        mine = rows_a.get(e, [])
        j = at.get(e, 0)
        while j < len(mine) and mine[j] != kb:
            j += 1
        assert j < len(mine), "row %d of the drain (env %d) is no row of the twin behind that env's earlier rows" % (k, e)
        at[e] = j + 1                                                    # a subsequence in the twin's order; a row handed out twice would need a second match
        got.add((e, kb))
    assert len(got) == ring and len({(e, k) for e, v in rows_a.items() for k in v}) == total_a   # the twin's rows are distinct, so are the rows handed out
    for k in range(whole):
        assert (int(ia[k]), key(ra_i[k], fa_i[k])) in got, "row %d of the twin (env %d), written before the ring was full, is missing" % (k, ia[k])
    # both run on: the same stream again
    for f in range(more_frames):
        a.Update(); b.Update()
    ra, fa, ia = a.DrainTuples(big_ring)
    n = b.DrainTuplesPacked(to_ptr(blk), ring, want_count=True)
    h = read(blk)
    o = np.argsort(ia, kind="stable")
    assert n == len(ra) > 0 and h[0, :3].view(np.int32).tolist() == [n, 0, 0]
    assert np.array_equal(h[1:n + 1, :W].view(np.int32), ra[o].view(np.int32))
    meta = h[1:n + 1, W:].view(np.int32)
    assert np.array_equal(meta[:, 0], fa[o].astype(np.int32)) and np.array_equal(meta[:, 1], ia[o] + 100)
    sa, sb = a.TupleStats(), b.TupleStats()
    assert (sb["pending"], sb["dropped"], sb["drained"]) == (0, lost, ring + n) and sa["drained"] == total_a + n
    return lost


def run_pipelined_drain_equals_sequential(scn, om, to_ptr=None, read=None, n_envs=12, cap=48, frames=90, extra=None, extra_b=None):
    """dtrl_set_tuple_pipelining: UpdateEnd(f); UpdateBegin(f + 1); drain -> frame f's tuples from the ring frame f wrote, while frame f + 1 runs.
    The drained stream, frame by frame, equals that of the sequential protocol (Update(); drain) on a twin batch; nothing is lost or duplicated, the
    counters agree, plain drains work in the same place, and the mode cannot be left while a ring still holds rows."""
    pol = dog_policy(om)
    args = dict(terrain_seed=31, rand_seed=2, global_env_offset=7)
    args.update(extra or {})
    prev = os.environ.get("DTRL_GROUPS")
    os.environ["DTRL_GROUPS"] = "2"                     # two env groups (two streams) also at this batch size: UpdateEndBegin schedules per group
    try:
        a = scn("args/opt_args_train_mace.txt", n_envs, data_root=REFDATA, extra_args=args)
        b = scn("args/opt_args_train_mace.txt", n_envs, data_root=REFDATA, extra_args=dict(args, **(extra_b or {})))
    finally:
        if prev is None:
            del os.environ["DTRL_GROUPS"]
        else:
            os.environ["DTRL_GROUPS"] = prev
    for x in (a, b):
        x.SetPolicy(pol[1], *pol[2:])
    W = a.W
    if to_ptr is None:
        mk = lambda: np.zeros((cap + 1, W + 2), np.float32)
        to_ptr = lambda t: t.ctypes.data; read = lambda t: t
    else:
        import torch
        mk = lambda: torch.zeros((cap + 1, W + 2), dtype=torch.float32, device="cuda")
    blk_a, blk_b = mk(), mk()
    b.SetTuplePipelining(True)
    seq = []
    for f in range(frames):
        a.Update()
        n = a.DrainTuplesPacked(to_ptr(blk_a), cap, want_count=True)
        seq.append(read(blk_a)[:n + 1].copy())
    pip = []
    b.UpdateBegin()
    for f in range(frames):
        if f + 1 < frames and f % 2 == 0:
            b.UpdateEndBegin()                          # frame f done, frame f + 1 in flight (writing the other ring), no barrier between the env groups
        else:
            b.UpdateEnd()                               # the same with the barrier
            if f + 1 < frames:
                b.UpdateBegin()
        if f % 7 == 3:                                  # a plain drain in the same place hands out the same rows (host copy), in completion order
            r, fl, ids = b.DrainTuples()
            h = seq[f]; n = int(h[0, :1].view(np.int32)[0])
            o = np.argsort(ids, kind="stable")
            assert len(r) == n and np.array_equal(r[o], h[1:n + 1, :W]) and np.array_equal(ids[o] + 7, h[1:n + 1, W + 1].view(np.int32))
            pip.append(h)
            continue
        n = b.DrainTuplesPacked(to_ptr(blk_b), cap, want_count=True)
        pip.append(read(blk_b)[:n + 1].copy())
    total = 0
    for f in range(frames):
        assert np.array_equal(seq[f], pip[f]), f
        total += int(seq[f][0, :1].view(np.int32)[0])
    assert total >= 20
    sa, sb = a.TupleStats(), b.TupleStats()
    assert sa["drained"] == sb["drained"] == total and sb["dropped"] == 0 and sb["pending"] == 0
    qa, qb = a.PoseVel(), b.PoseVel()
    assert np.array_equal(qa[0], qb[0]) and np.array_equal(qa[1], qb[1])
    # leaving the mode while the idle ring still holds rows is refused (they would be stranded); an undrained ring is not lost, it is handed out two frames later
    for _ in range(40):
        b.UpdateBegin(); b.UpdateEnd()                  # nobody drains: both rings fill
    before = b.TupleStats()["drained"]
    with pytest.raises(Exception):
        b.SetTuplePipelining(False)
    n1 = len(b.DrainTuples()[0])                        # the ring of the last frame
    b.UpdateBegin(); b.UpdateEnd()
    n2 = len(b.DrainTuples()[0])                        # the other ring: what it held plus this frame's rows
    assert n1 > 0 and n2 > 0 and b.TupleStats()["drained"] == before + n1 + n2 and b.TupleStats()["dropped"] == 0
    b.SetTuplePipelining(False)
    b.Update(); b.DrainTuples()


def test_pipelined_drain_equals_sequential(da, om):
    run_pipelined_drain_equals_sequential(Scenario, om)


def test_pipelined_drain_equals_sequential_device_terrain(da, om):
    """The same protocol with -terrain_gen= device, where the frame boundary is queued work and the host never waits for a frame (the drain
    must follow the frame that wrote its ring on the DEVICE). The lane-loop backend is synchronous, so this checks the engine logic; the GPU twin in
    tests/test_gpu_parity.py runs a batch large enough for a frame to outlast the host."""
    run_pipelined_drain_equals_sequential(Scenario, om, extra={"terrain_gen": "device"})


def run_step_poll_keeps_the_tuple_stream(scn, om, n_envs=12, frames=80, work=None):
    """dtrl_step_poll between two dtrl_step_end_begin calls (groups that have finished are relaunched at once, into the ring just drained) does not change what
    is drained frame by frame, nor the trajectories; rings are refused while both are being written."""
    pol = dog_policy(om)
    args = dict(terrain_seed=31, rand_seed=2, tuple_ring="host")
    prev = os.environ.get("DTRL_GROUPS")
    os.environ["DTRL_GROUPS"] = "2"
    try:
        a = scn("args/opt_args_train_mace.txt", n_envs, data_root=REFDATA, extra_args=args)
        b = scn("args/opt_args_train_mace.txt", n_envs, data_root=REFDATA, extra_args=args)
    finally:
        if prev is None:
            del os.environ["DTRL_GROUPS"]
        else:
            os.environ["DTRL_GROUPS"] = prev
    for x in (a, b):
        x.SetPolicy(pol[1], *pol[2:])
    seq = []
    for f in range(frames):
        a.Update()
        r, fl, ids = a.DrainTuples(); o = np.argsort(ids, kind="stable")
        seq.append((r[o], fl[o], ids[o]))
    b.SetTuplePipelining(True)
    b.UpdateBegin()
    early = total = 0
    for f in range(frames):
        if f + 1 < frames:
            b.UpdateEndBegin()
        else:
            b.UpdateEnd()
        r, fl, ids = b.DrainTuples(); o = np.argsort(ids, kind="stable")
        assert np.array_equal(r[o], seq[f][0]) and np.array_equal(fl[o], seq[f][1]) and np.array_equal(ids[o], seq[f][2]), f
        total += len(r)
        if f + 2 < frames:
            if work is not None:
                work()                                   # (on the GPU: give the frame time to end, as a trainer's batch of Train() calls does)
            k = b.UpdatePoll()
            early += k
            if k:
                with pytest.raises(Exception):
                    b.DrainTuples()                      # both rings are being written now
                with pytest.raises(Exception):
                    b.UpdateEnd()
    assert total >= 20 and early >= 2
    qa, qb = a.PoseVel(), b.PoseVel()
    assert np.array_equal(qa[0], qb[0]) and np.array_equal(qa[1], qb[1])
    b.SetTuplePipelining(False)
    return early


def test_step_poll_keeps_the_tuple_stream(da, om):
    early = run_step_poll_keeps_the_tuple_stream(Scenario, om)
    assert early == 2 * 78                              # the lane-loop backend is synchronous: every poll finds both groups finished


def test_host_memory_tuple_ring_equals_the_device_ring(da, om):
    """-tuple_ring= host (rings in page-locked host memory, written by the kernels, drained without a queued copy) hands out the device ring's tuple stream:
    the pipelined protocol with plain and packed drains on the host ring vs the sequential protocol on the device ring."""
    run_pipelined_drain_equals_sequential(Scenario, om, extra_b={"tuple_ring": "host"})
    with pytest.raises(Exception):
        Scenario("args/opt_args_train_mace.txt", 2, data_root=REFDATA, extra_args={"tuple_ring": "pinned"})


def test_env_id_lists_are_validated(da):
    """dtrl_reset with more ids than envs / duplicates / negative counts must not overrun the engine's buffers."""
    b = Scenario("args/sim_dog_args.txt", 3, data_root=REFDATA, extra_args={"terrain_seed": 4})
    b.StepUpdates(5)
    q_before = b.PoseVel()[0]
    ids = np.array([2, 2, 2, 0, 0, 2, 2, 0, 2, 0, 2, 2], np.int32)      # 12 entries for a 3-env batch
    b.Reset(env_ids=ids)
    q = b.PoseVel()[0]
    assert np.array_equal(q[1], q_before[1]) and not np.array_equal(q[0], q_before[0]) and np.array_equal(q[0], q[2])
    with pytest.raises(da.DtrlError):
        b.Reset(env_ids=np.array([0, 3], np.int32))
    import ctypes as C
    assert b._lib.dtrl_reset(b._h, ids.ctypes.data_as(C.c_void_p), -5, None) == 1        # DTRL_ERR_ARG
    qq = np.zeros((3, b.D))
    assert b._lib.dtrl_get_pose_vel(b._h, None, -1, qq.ctypes.data_as(C.c_void_p), qq.ctypes.data_as(C.c_void_p)) == 1
    assert b._lib.dtrl_get_pose_vel(b._h, None, 4, qq.ctypes.data_as(C.c_void_p), qq.ctypes.data_as(C.c_void_p)) == 1
    b.StepUpdates(1)   # still alive
