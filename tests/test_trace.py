"""Frame trace (include/dtrl.h dtrl_trace): a ring of compact per-frame rows of chosen envs, written on the device behind the frame and the episode limit and in front
of everything that resets an env. The yardsticks are the per-env getters between frames (a row equals them bit for bit while the env's episode runs), a twin batch
stopped in front of the frame end (a fallen env's row is its last pose), the batch that never heard of a trace, and the records of the rules around it. Every
comparison is for equal bits. Runs on the lane-loop check build (the host default of Backend::TraceRecord / TraceGather); tests/test_gpu_trace.py points
`Scenario` of the helper modules at the product libraries (one launch of dtrl_trace_record per env group and frame, one of dtrl_trace_gather per read)."""
import json
import os
import sys

import numpy as np
import pytest

import test_episode_limit as E            # limit_batch, all_rules_batch, resets
import test_external_policy as X          # env_states / same_record / run_internal / replay_external
import test_model_variants as V           # with_variants / write_variants
import test_policy_slots as P             # slotted / policies / refused
import test_terrain_sets as T             # MODES, batch, with_policy, fill, assert_envs_equal
from conftest import REPO

sys.path.insert(0, os.path.join(REPO, "tools"))
import trace_export                       # noqa: E402

DOG, RAPTOR = T.DOG, T.RAPTOR
TRACED = [4, 0, 3]                        # unsorted, a strict subset of the 6 envs
INTS = ("row", "need_reset", "action_id", "state", "stance", "contact_bits", "num_cycles", "num_resets", "slot", "variant", "terrain")
VALS = ("time", "phase", "q", "qd", "tau")


def same(a, b):
    return np.asarray(a).tobytes() == np.asarray(b).tobytes()


def row_of(tr, i, r):
    """row r of listed env i as a dict of byte strings"""
    return {k: np.ascontiguousarray(tr[k][i, r]).tobytes() for k in VALS + INTS}


def getters(b, envs, keys):
    """What the host calls between frames show of the listed envs, under the trace's names. keys: {"slot" / "variant" / "terrain": getter} of the families the batch has."""
    q, qd = b.PoseVel(envs)
    _, tau = b.Torques(envs)
    state, phase, aid, _, _ = b.Ctrl(envs)
    nc, nr, _, _, _ = b.CycleInfo(envs)
    bits = (b.Contacts(envs).astype(np.int64) << np.arange(b.L)).sum(axis=1).astype(np.uint32).view(np.int32)
    st = X.env_states(b)[list(envs)]
    out = {"q": q, "qd": qd, "tau": tau, "state": state, "phase": phase, "action_id": aid, "contact_bits": bits, "num_cycles": nc.astype(np.int32), "num_resets": nr.astype(np.int32),
           "time": st["time"].astype(np.float64), "stance": st["stance"].astype(np.int32)}
    for k in ("slot", "variant", "terrain"):
        out[k] = np.asarray(keys[k](envs), np.int32) if k in keys else np.zeros(len(envs), np.int32)
    return out


def check_rows_equal_getters(b, keys, frames=30, traced=TRACED):
    """After each frame the new row of every traced env whose episode did not end equals the getters; returns how many rows were compared and how many ended an episode."""
    b.Trace(traced, frames=frames + 3)
    info = b.TraceInfo()
    assert info["n_traced"] == len(traced) and info["frames"] == frames + 3 and info["width"] == 3 * b.D + 2 and list(info["env_ids"]) == traced and not info["rows_written"].any()
    compared = ended = 0
    for f in range(frames):
        b.Update()
        tr = b.TraceRead()
        assert list(tr["env_ids"]) == traced and list(tr["count"]) == [f + 1] * len(traced) and tr["q"].shape == (len(traced), f + 1, b.D)
        g = getters(b, traced, keys)
        for i, e in enumerate(traced):
            assert tr["row"][i, f] == f
            if tr["need_reset"][i, f]:
                ended += 1
                continue
            for k in g:
                assert same(tr[k][i, f], g[k][i]), "frame %d env %d: %s of the row differs from the getter (%r, %r)" % (f, e, k, tr[k][i, f], g[k][i])
            compared += 1
    assert list(b.TraceInfo()["rows_written"]) == [frames] * len(traced)
    return compared, ended


# ---- 1. rows equal the getters ----
@pytest.mark.parametrize("mode", T.MODES, ids=T.MODE_IDS)
def test_rows_equal_getters_dog_with_variants_and_terrains(da, om, tmp_path, mode, n=6):
    """The dog (W = 71) under the xavier net with exploration on; model variants and terrain sets dealt over the envs, so that the two key columns are not all 0."""
    b = V.with_variants(om, DOG, n, V.write_variants(tmp_path, DOG), [e % 3 for e in range(n)], dict(terrain_seed=31, rand_seed=3, **mode))
    T.fill(b, T.four_walkable_files(DOG))
    b.AssignTerrains(None, [(e + 1) % 4 for e in range(n)], restart=True)
    assert b.TraceInfo()["width"] == 71
    compared, _ = check_rows_equal_getters(b, {"variant": b.GetVariants, "terrain": b.GetTerrains})
    assert compared >= 80
    tr = b.TraceRead()
    assert [list(tr[k][:, -1]) for k in ("slot", "variant", "terrain")] == [[0, 0, 0], [e % 3 for e in TRACED], [(e + 1) % 4 for e in TRACED]]


def test_rows_equal_getters_raptor_with_slots(da, om, n=6):
    """The raptor (W = 65, a stance leg) with two policy slots"""
    pols = P.policies(om, RAPTOR)[:2]
    b = P.slotted(RAPTOR, n, pols, [T.EXPLORE, T.EXPLORE], [e % 2 for e in range(n)], dict(terrain_seed=70, rand_seed=2))
    assert b.TraceInfo()["width"] == 65
    compared, _ = check_rows_equal_getters(b, {"slot": b.GetSlots})
    assert compared >= 80
    assert list(b.TraceRead()["slot"][:, -1]) == [e % 2 for e in TRACED]


def test_rows_equal_getters_fp32(da, om, n=6):
    """The fp32 library converts each value exactly, as its getters do"""
    b = T.with_policy(om, DOG, n, dict(terrain_seed=31, rand_seed=3, physics_precision="f32"))
    compared, _ = check_rows_equal_getters(b, {})
    assert compared >= 80
    q = b.TraceRead()["q"]
    assert same(q, q.astype(np.float32).astype(np.float64)) and np.abs(q).max() > 0


# ---- 2. a fallen env's row is its last pose ----
FALL = dict(terrain_seed=70, rand_seed=2)   # chosen on the check build: at least two of the traced envs fall inside 75 frames (asserted)


def fall_run(om, n=6, frames=75, extra=FALL):
    b = T.with_policy(om, DOG, n, dict(extra))
    b.Trace(TRACED, frames=frames)
    for _ in range(frames):
        b.Update()
    return b.TraceRead()


def test_a_fallen_envs_row_is_its_last_pose(da, om, n=6, frames=75):
    tr = fall_run(om, n, frames)
    fell = [(i, int(np.flatnonzero(tr["need_reset"][i] & 1)[0])) for i in range(len(TRACED)) if (tr["need_reset"][i] & 1).any()]
    print("first falls (listed env, row):", fell)
    assert len(fell) >= 2, "the run is meant to have at least two traced envs fall: pick another seed"
    for i, k in fell[:2]:
        e = TRACED[i]
        twin = T.with_policy(om, DOG, n, dict(FALL))
        for _ in range(k):
            twin.Update()
        assert twin.num_update_steps == 20
        twin.StepUpdates(20)                        # the frame's env-steps without its end: nothing resets
        q, qd = twin.PoseVel([e]); _, tau = twin.Torques([e])
        for name, v in (("q", q), ("qd", qd), ("tau", tau)):
            assert same(tr[name][i, k], v[0]), "env %d row %d: %s is not the pose the frame ended in" % (e, k, name)
        if k + 1 < frames:
            assert tr["num_resets"][i, k + 1] == tr["num_resets"][i, k] + 1, (e, k)
        twin.close()


# ---- 3. the ring ----
@pytest.mark.parametrize("mode", T.MODES, ids=T.MODE_IDS)
def test_ring_and_untouched_batch(da, om, mode, n=6, frames=11):
    extra = dict(terrain_seed=31, rand_seed=3, **mode)
    b, plain, full = (T.with_policy(om, DOG, n, extra) for _ in range(3))
    b.Trace(TRACED, frames=4)
    full.Trace(TRACED, frames=frames)
    for f in range(frames):
        b.Update(); plain.Update(); full.Update()
        tr = b.TraceRead()
        assert list(tr["count"]) == [min(f + 1, 4)] * 3 and list(b.TraceInfo()["rows_written"]) == [f + 1] * 3
    ref = full.TraceRead()
    tr = b.TraceRead()
    assert [list(r) for r in tr["row"]] == [[7, 8, 9, 10]] * 3
    for i in range(3):
        for r in range(4):
            assert row_of(tr, i, r) == row_of(ref, i, 7 + r), (i, r)
    two = b.TraceRead(max_rows=2)
    assert [list(r) for r in two["row"]] == [[9, 10]] * 3 and list(two["count"]) == [2] * 3
    assert all(row_of(two, i, r) == row_of(ref, i, 9 + r) for i in range(3) for r in range(2))
    one = b.TraceRead(env_ids=[3], max_rows=9)      # a subset, more rows asked for than the ring holds: rows beyond count stay as the caller left them
    assert list(one["count"]) == [4] and list(one["row"][0]) == [7, 8, 9, 10, 0, 0, 0, 0, 0] and row_of(one, 0, 3) == row_of(ref, 2, 10)
    # the trace reads state and writes only its own ring: every env, traced or not, is the env of a batch without a trace
    T.assert_envs_equal(b, plain, range(n), "traced batch against a batch without a trace")


# ---- 4. order against the rules ----
@pytest.mark.parametrize("mode", T.MODES, ids=T.MODE_IDS)
def test_row_carries_the_limits_need_reset(da, om, mode, n=6):
    """A limit of exactly 5 frames: the row of every fifth frame carries the truncation the limit wrote in front of the trace, and the reset counter rises behind it."""
    b = E.limit_batch(om, n, mode, frames=(5, 5))
    b.Trace(TRACED, frames=12)
    for _ in range(12):
        b.Update()
    tr = b.TraceRead()
    for i in range(3):
        assert [int(v) & 1 for v in tr["need_reset"][i]] == [0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0], tr["need_reset"][i]
        nr = tr["num_resets"][i]
        assert nr[5] == nr[4] + 1 and nr[10] == nr[9] + 1 and nr[4] == nr[0] and nr[9] == nr[5]
    info = b.EpisodeInfo(TRACED)
    assert list(info["by_limit"]) == [2, 2, 2] and list(info["by_fall"]) == [0, 0, 0]


@pytest.mark.parametrize("mode", T.MODES, ids=T.MODE_IDS)
def test_row_carries_the_keys_the_frame_ran_under(da, om, tmp_path, mode, n=E.N, frames=24):
    """Ladder, redraw, rescale, push schedule and limit in one batch: a row's terrain and variant are the keys in force BEFORE the boundary's rules ran (what the
    getters showed in front of the frame), also in the row that ends an episode; the next row carries the keys those rules moved the env to."""
    b = E.all_rules_batch(om, tmp_path, mode, n)
    traced = [69, 6, 64, 31, 0, 7]
    b.Trace(traced, frames=frames)
    moved = 0
    for f in range(frames):
        before = (b.GetTerrains(traced).copy(), b.GetVariants(traced).copy())
        b.Update()
        after = (b.GetTerrains(traced), b.GetVariants(traced))
        tr = b.TraceRead(max_rows=1)
        assert list(tr["row"][:, 0]) == [f] * len(traced)
        assert same(tr["terrain"][:, 0], before[0]) and same(tr["variant"][:, 0], before[1]), f
        ended = (tr["need_reset"][:, 0] & 1) != 0
        changed = (after[0] != before[0]) | (after[1] != before[1])
        assert not (changed & ~ended & (after[1] != before[1])).any(), "a variant moved without an episode end"
        moved += int((changed & ended).sum())
    assert moved >= 3, "the run is meant to move keys at episode ends"
    tr = b.TraceRead()
    assert same(tr["variant"][:, 1:][(tr["need_reset"][:, :-1] & 1) == 0], tr["variant"][:, :-1][(tr["need_reset"][:, :-1] & 1) == 0])   # a variant moves at an episode end alone
    rescaled = [i for i, e in enumerate(traced) if e in E.RESCALED]
    assert rescaled and all((tr["variant"][i] == 3 + traced[i]).all() for i in rescaled), "a private rescale key reads V + e"


# ---- 5. external policy mode ----
def test_external_trace_equals_internal(da, om, monkeypatch, n=8, frames=40):
    """Run A (internal) and its replay through the external hand-over: the two traces are equal row for row, though B's rows arrive in other ticks."""
    extra = dict(terrain_seed=70, rand_seed=2)
    made = []

    def traced_batch(da_, arg, n_, **kw):
        b = made_batch(da_, arg, n_, **kw)
        b.Trace(None, frames=4 * frames)
        made.append(b)
        return b
    made_batch = X.batch
    monkeypatch.setattr(X, "batch", traced_batch)
    rec, decisions, blind_from, _, a = X.run_internal(da, om, DOG, n, frames, extra)
    blind_from = dict(blind_from)
    compared, _, b = X.replay_external(da, om, DOG, n, frames, extra, rec, decisions, blind_from)   # (the replay lowers blind_from where it ran out of recorded decisions)
    assert made == [a, b] and b.external and compared > 0
    ta, tb = a.TraceRead(), b.TraceRead()
    assert list(ta["count"]) == [frames] * n and tb["count"].min() >= frames
    rows = 0
    for e in range(n):
        for f in range(min(frames, blind_from[e])):
            assert row_of(ta, e, f) == row_of(tb, e, f), "env %d row %d differs between the internal run and its external replay" % (e, f)
            rows += 1
    assert rows >= 0.9 * n * frames


def test_a_parked_env_writes_no_row(da, om, n=8, ticks=30):
    b = X.batch(da, DOG, n, policy_mode="external", terrain_seed=70, rand_seed=2)
    b.Trace([5, 1, 6], frames=ticks)
    table = b.ActionTable()
    written = np.zeros(3, np.int64)
    parked_ticks = 0
    for _ in range(ticks):
        b.Update()
        park, left = b.ExtEnvInfo([5, 1, 6])
        written += park == 0
        parked_ticks += int((park != 0).sum())
        assert list(b.TraceInfo()["rows_written"]) == list(written), (park, left)
        ids, _ = b.PendingActions(with_states=False)
        if len(ids):
            b.SupplyActions(ids, [0] * len(ids), np.array([table[0]] * len(ids)))
    assert parked_ticks >= 3 and written.min() >= 3
    tr = b.TraceRead()
    assert all(list(tr["row"][i, :written[i]]) == list(range(written[i])) for i in range(3))


# ---- 6. lifecycle and refusals ----
def test_lifecycle_and_refusals(da, om, n=6):
    b = T.with_policy(om, DOG, n, dict(terrain_seed=31, rand_seed=3))
    refused = lambda fn, *words: P.refused(da, fn, *words)
    assert b.TraceInfo()["n_traced"] == 0
    refused(lambda: b.TraceRead(env_ids=[0], max_rows=1), "no trace")
    refused(lambda: b.Trace([1, 2, 1], 4), "twice")
    refused(lambda: b.Trace([1, n], 4), "out of range")
    refused(lambda: b.Trace([-1], 4), "out of range")
    refused(lambda: b.Trace([1, 2], 0), "frames")
    refused(lambda: b.Trace(None, -3), "frames")
    assert b.TraceInfo()["n_traced"] == 0
    with pytest.raises(da.DtrlError, match="do(es)? not fit"):
        b.Trace(None, (1 << 31) - 1)
    assert b.TraceInfo()["n_traced"] == 0
    b.Trace(TRACED, 8)
    for _ in range(3):
        b.Update()
    refused(lambda: b.TraceRead(env_ids=[1], max_rows=1), "not traced")
    refused(lambda: b.TraceRead(env_ids=[n], max_rows=1), "out of range")
    b.UpdateBegin()
    for call in (lambda: b.Trace([0], 4), b.TraceOff, b.TraceInfo, b.TraceRead, lambda: b.TraceRead(max_rows=1)):
        refused(call, "frame is in flight")
    b.UpdateEnd()
    assert list(b.TraceInfo()["rows_written"]) == [4, 4, 4]
    # snapshot restore, clone and reset leave ring and counters as they were, and write no row
    before = b.TraceRead()
    snap = b.SaveState()
    b.Update()
    b.RestoreState(snap)
    b.CloneEnvs([1], [4])
    b.Reset([0, 3])
    b.Reset()
    after = b.TraceRead()
    assert list(after["count"]) == [5, 5, 5] and all(row_of(after, i, r) == row_of(before, i, r) for i in range(3) for r in range(4))
    snap.free()
    # a second call replaces the trace: counters from 0, another list, another ring
    b.Trace([2, 5], 3)
    info = b.TraceInfo()
    assert list(info["env_ids"]) == [2, 5] and info["frames"] == 3 and list(info["rows_written"]) == [0, 0] and list(b.TraceRead(max_rows=3)["count"]) == [0, 0]
    refused(lambda: b.TraceRead(env_ids=[4], max_rows=1), "not traced")
    b.Update()
    assert list(b.TraceRead()["row"][:, 0]) == [0, 0]
    b.Trace(None, 0)
    assert b.TraceInfo()["n_traced"] == 0
    b.Update()
    b.Trace([1], 2); b.TraceOff()
    assert b.TraceInfo()["n_traced"] == 0
    b.Trace(None, 2)
    assert list(b.TraceInfo()["env_ids"]) == list(range(n))


# ---- 7. export ----
def test_export_motion_files(da, om, tmp_path, n=6, frames=75):
    b = T.with_policy(om, DOG, n, dict(FALL))
    tr = trace_export.record(b, frames, TRACED)
    files = trace_export.write_trace(tr, str(tmp_path / "run"))
    z = np.load(str(tmp_path / "run.npz"))
    assert same(z["q"], tr["q"]) and list(z["env_ids"]) == TRACED
    assert sorted(files) == sorted(TRACED)
    for i, e in enumerate(TRACED):
        cuts = list(np.flatnonzero(tr["need_reset"][i] & 1))
        assert len(files[e]) == len(cuts) + (1 if not cuts or cuts[-1] != frames - 1 else 0)
        row = 0
        for path in files[e]:
            with open(path) as f:
                doc = json.load(f)
            assert set(doc) == {"Motion"} and doc["Motion"]["Loop"] is False
            for fr in doc["Motion"]["Frames"]:
                assert len(fr) == 23 + 1 and fr[0] == 1.0 / 30.0 and same(np.array(fr[1:]), tr["q"][i, row]), (e, row)
                row += 1
            if cuts and row - 1 in cuts:
                assert tr["need_reset"][i, row - 1] & 1          # a file ends with the episode's last pose
        assert row == frames
    assert sum(len(v) for v in files.values()) >= len(TRACED) + 2, "the run is meant to hold falls: several episodes per env"
