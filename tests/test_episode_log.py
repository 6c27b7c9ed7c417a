"""Episode log (include/dtrl.h dtrl_episode_log): one 64-byte row per ended episode, written on the device at the frame boundary behind the episode limit and the
trace and in front of every rule that moves a key or redraws a scale, into a ring per env group in page-locked host memory that the host drains without queueing
GPU work. The yardsticks are the calls that existed before, polled after every frame (EpisodeInfo for cause, length and distance; a trace of every env for the
cycle counter, need_reset and the keys; GetVariants / GetTerrains / VariantRescaleInfo before and after each boundary), an internal run replayed through the
external hand-over, a sequential run against one drained between UpdateBegin and UpdateEnd, and the batch that never heard of a log. Every comparison is for equal
bits. Runs on the lane-loop check build (the host default of Backend::EpisodeLog); tests/test_gpu_episode_log.py points `Scenario` of the helper modules at the
product libraries (one launch of dtrl_episode_log per env group and frame)."""
import os

import numpy as np
import pytest

import test_episode_limit as E            # limit_batch, all_rules_batch, HARD, RESCALED
import test_external_policy as X          # env_states / same_record / run_internal / replay_external
import test_policy_slots as P             # slotted / policies / refused
import test_terrain_sets as T             # MODES, with_policy
import test_variant_rescale as VR         # the loop test's settings
from conftest import REFDATA

DOG, RAPTOR = T.DOG, T.RAPTOR
N = E.N
FIELDS = ("env", "cause", "frames", "cycles", "boundary", "episode", "dist", "need_reset", "slot", "variant", "terrain", "rescale_draw")


def rows_of(d, skip=()):
    """the drained dict as a list of per-row tuples of (field, bytes)"""
    n = len(d["env"])
    assert all(len(d[k]) == n for k in FIELDS)
    return [tuple((k, np.ascontiguousarray(d[k][i]).tobytes()) for k in FIELDS if k not in skip) for i in range(n)]


def concat(parts):
    out = {k: np.concatenate([p[k] for p in parts]) for k in FIELDS}
    out["lost"] = sum(p["lost"] for p in parts)
    return out


def in_order(d):
    key = list(zip(d["boundary"].tolist(), d["env"].tolist()))
    return key == sorted(key) and len(set(key)) == len(key)


def pushed_batch(om, mode, limit=True, **more):
    """the scene of test_episode_limit.test_records_equal_the_rule_with_falls: 70 dogs, limits 4 .. 9, pushes of 1500 .. 3000 N"""
    return E.limit_batch(om, N, mode, limit=limit, min_perturb=E.HARD[0], max_perturb=E.HARD[1], min_pertrub_duration=0.1, max_perturb_duration=0.25, **more)


def pushed_run(b, frames, each_frame=None):
    for f in range(frames):
        if f % 2 == 0:
            b.ApplyRandForce(f)
        b.Update()
        if each_frame:
            each_frame(f)


# ---- 1. rows equal frame-by-frame polling ----
def check_rows_equal_polling(om, mode, prec, frames=30):
    b = pushed_batch(om, mode, **prec)
    b.EpisodeLog(4096)
    b.Trace(None, frames=frames + 2)
    info = b.EpisodeLogInfo()
    assert info["capacity"] == 4096 and info["n_groups"] >= 1 and info["written"] == 0 and info["lost"] == 0
    cycles0 = X.env_states(b)["num_cycles"].astype(np.int64).copy()
    ended = {k: 0 for k in range(N)}
    want = []
    prev = b.EpisodeInfo()

    def poll(f):
        nonlocal prev
        now = b.EpisodeInfo()
        for e in range(N):
            k = int(now["by_fall"][e] + now["by_limit"][e] - prev["by_fall"][e] - prev["by_limit"][e])
            assert k in (0, 1)
            if k:
                want.append(dict(env=e, cause=int(now["last_cause"][e]), frames=int(now["last_frames"][e]), dist=np.float64(now["last_dist"][e]), boundary=f, episode=ended[e]))
                ended[e] += 1
        prev = now
    pushed_run(b, frames, poll)
    tr = b.TraceRead()
    assert list(tr["env_ids"]) == list(range(N)) and list(tr["count"]) == [frames] * N
    for w in want:                                   # what the trace saw at that boundary: the cycle counter and the status record's need_reset
        e, f = w["env"], w["boundary"]
        w["cycles"] = int(tr["num_cycles"][e, f]) - int(cycles0[e])
        cycles0[e] = int(tr["num_cycles"][e, f])
        w["need_reset"] = int(tr["need_reset"][e, f])
        assert w["need_reset"] != 0
    got = b.EpisodeLogDrain()
    assert got["lost"] == 0 and in_order(got) and len(got["env"]) == len(want)
    for i, w in enumerate(want):                     # (the polling walks boundaries, then envs: the drain's order)
        for k in ("env", "cause", "frames", "cycles", "boundary", "episode", "need_reset"):
            assert int(got[k][i]) == w[k], (i, k, got[k][i], w)
        assert np.float64(got["dist"][i]).tobytes() == w["dist"].tobytes(), (i, got["dist"][i], w["dist"])
        assert (got["slot"][i], got["variant"][i], got["terrain"][i], got["rescale_draw"][i]) == (0, 0, 0, -1)
    for e in range(N):
        assert list(got["episode"][got["env"] == e]) == list(range(ended[e])), e
    cause, hi = got["cause"], got["env"] >= 64
    counts = dict(falls=int((cause == 1).sum()), limits=int((cause == 2).sum()), falls_hi=int(((cause == 1) & hi).sum()), limits_hi=int(((cause == 2) & hi).sum()))
    print(counts)
    assert counts["falls"] >= 10 and counts["limits"] >= 10 and counts["falls_hi"] >= 1 and counts["limits_hi"] >= 1, counts
    assert set(cause.tolist()) <= {1, 2}
    info = b.EpisodeLogInfo()
    assert info["written"] == len(want) and info["lost"] == 0 and b.EvalStats()["resets"] == len(want)
    assert len(b.EpisodeLogDrain()["env"]) == 0
    return got


@pytest.mark.parametrize("mode", T.MODES, ids=T.MODE_IDS)
def test_rows_equal_frame_by_frame_polling(da, om, mode):
    check_rows_equal_polling(om, mode, {})


def test_rows_equal_frame_by_frame_polling_fp32(da, om):
    check_rows_equal_polling(om, dict(terrain_gen="device"), dict(physics_precision="f32"))


def test_two_env_groups_merge_in_boundary_env_order(da, om, monkeypatch):
    """Two rings (envs 0 .. 34 and 35 .. 69): the drain merges them into the rows of the one-ring run, bit for bit"""
    one = check_rows_equal_polling(om, dict(terrain_gen="device"), {})
    monkeypatch.setenv("DTRL_GROUPS", "2")
    b = pushed_batch(om, dict(terrain_gen="device"))
    b.EpisodeLog(4096)
    assert b.EpisodeLogInfo()["n_groups"] == 2
    pushed_run(b, 30)
    assert rows_of(b.EpisodeLogDrain()) == rows_of(one)


# ---- 2. keys and draws are the episode's own ----
@pytest.mark.parametrize("mode", T.MODES, ids=T.MODE_IDS)
def test_keys_and_draws_are_the_episodes_own(da, om, tmp_path, mode, frames=24):
    """Ladder, redraw over 3 variants, rescale of every fifth env, push schedule and limits: a row carries the variant, the terrain and the draw number in force
    BEFORE the boundary that ended the episode, and the factors recomputed from its draw are the ones VariantRescaleInfo reported during the episode."""
    b = E.all_rules_batch(om, tmp_path, mode)
    b.EpisodeLog(1024)
    rows = moved = redrawn = 0
    for f in range(frames):
        before = (b.GetVariants().copy(), b.GetTerrains().copy(), b.VariantRescaleInfo())
        b.Update()
        after = (b.GetVariants(), b.GetTerrains(), b.VariantRescaleInfo())
        d = b.EpisodeLogDrain()
        assert (d["boundary"] == f).all() and in_order(d)
        for i, e in enumerate(d["env"]):
            assert d["variant"][i] == before[0][e] and d["terrain"][i] == before[1][e] and d["slot"][i] == 0, (f, e)
            private = e in E.RESCALED
            assert before[0][e] == (3 + e if private else before[0][e]) and (before[0][e] < 3) != private
            assert d["rescale_draw"][i] == (before[2]["episodes"][e] - 1 if private else -1), (f, e, d["rescale_draw"][i])
            if private:                               # the boundary drew the next episode's scales: the counter the calls show afterwards is one further
                assert after[2]["episodes"][e] == before[2]["episodes"][e] + 1 and d["rescale_draw"][i] != after[2]["episodes"][e] - 1
                redrawn += 1
            fac = b.VariantRescaleFactors([e], [d["rescale_draw"][i]])
            assert fac.shape == (1, 4, b.L) and fac.tobytes() == before[2]["factors"][e].tobytes(), (f, e)
            moved += int(after[0][e] != before[0][e] or after[1][e] != before[1][e])
        rows += len(d["env"])
    print(dict(rows=rows, keys_moved=moved, redrawn=redrawn))
    assert rows >= N and moved >= 3 and redrawn >= 3, "the run is meant to end episodes whose boundary moves a key or redraws the scales"
    assert (b.VariantRescaleFactors([1, 6], [-1, -1]) == 1.0).all()
    f0 = b.VariantRescaleFactors([1, 1, 6], [0, 1, 0])
    assert f0[0].tobytes() != f0[1].tobytes() and f0[0].tobytes() != f0[2].tobytes() and (f0[:, 0] >= 0.8).all() and (f0[:, 0] <= 1.2).all()


def test_rows_carry_the_slot(da, om, n=6, frames=12):
    """The raptor with two policy slots under a limit of 2 .. 4 frames"""
    pols = P.policies(om, RAPTOR)[:2]
    b = P.slotted(RAPTOR, n, pols, [T.EXPLORE, T.EXPLORE], [e % 2 for e in range(n)], dict(terrain_seed=70, rand_seed=2))
    b.EpisodeLimit((2, 4), seed=3)
    b.EpisodeLog(64)
    for _ in range(frames):
        b.Update()
    d = b.EpisodeLogDrain()
    assert len(d["env"]) >= 2 * n and list(d["slot"]) == [e % 2 for e in d["env"]] and not d["variant"].any() and not d["terrain"].any() and (d["rescale_draw"] == -1).all()


# ---- 3. the ring ----
@pytest.mark.parametrize("groups", ["1", "2"], ids=["one_group", "two_groups"])
@pytest.mark.parametrize("mode", T.MODES, ids=T.MODE_IDS)
def test_ring_keeps_the_last_rows_of_a_boundary(da, om, monkeypatch, mode, groups):
    """A fixed limit of 3 frames ends all 70 episodes in the boundary of index 2: 70 rows into rings of 4. Each group keeps the rows of its 4 highest env ids."""
    monkeypatch.setenv("DTRL_GROUPS", groups)
    G = int(groups)
    b = E.limit_batch(om, N, mode, frames=(3, 3))
    b.EpisodeLog(4)
    for f in range(4):
        b.Update()
        assert b.EpisodeLogInfo() == dict(capacity=4, n_groups=G, written=N if f >= 2 else 0, lost=N - 4 * G if f >= 2 else 0), f
    kept = sorted(e for g in range(G) for e in range(N * (g + 1) // G - 4, N * (g + 1) // G))
    first = b.EpisodeLogDrain(max_rows=3)
    assert list(first["env"]) == kept[:3] and first["lost"] == N - 4 * G
    rest = b.EpisodeLogDrain()
    assert list(rest["env"]) == kept[3:] and rest["lost"] == 0
    both = concat([first, rest])
    assert (both["boundary"] == 2).all() and (both["frames"] == 3).all() and (both["cause"] == 2).all() and not both["episode"].any()
    none = b.EpisodeLogDrain()
    assert len(none["env"]) == 0 and none["lost"] == 0 and b.EpisodeLogInfo()["written"] == N
    for _ in range(2):                                 # the next common end: ordinal 1, and the cursors count every row
        b.Update()
    d = b.EpisodeLogDrain()
    assert list(d["env"]) == kept and (d["episode"] == 1).all() and (d["boundary"] == 5).all() and d["lost"] == N - 4 * G
    assert b.EpisodeLogInfo() == dict(capacity=4, n_groups=G, written=2 * N, lost=2 * (N - 4 * G))


# ---- 4. listed starts and lifecycle ----
@pytest.mark.parametrize("mode", T.MODES, ids=T.MODE_IDS)
def test_listed_starts_and_lifecycle(da, om, mode, n=12):
    refused = lambda fn, *words: P.refused(da, fn, *words)
    b, never = (E.limit_batch(om, n, mode, frames=(5, 5)) for _ in range(2))
    refused(lambda: b.EpisodeLogDrain(), "no episode log")
    refused(lambda: b.EpisodeLog(-1), "dtrl_episode_log", "negative", "nothing changed")
    refused(lambda: b.VariantRescaleFactors([0], [0]), "no variant rescale")
    assert b.EpisodeLogInfo() == dict(capacity=0, n_groups=0, written=0, lost=0)
    b.EpisodeLog(64)
    b.Trace(None, frames=32)
    for _ in range(2):
        b.Update(); never.Update()
    # dtrl_reset in mid-episode: no row, and frames and cycles start over
    b.Reset([3, 3, 7]); never.Reset([3, 3, 7])
    assert b.EpisodeLogInfo()["written"] == 0
    c_reset = X.env_states(b)["num_cycles"][[3, 7]].astype(np.int64)
    for _ in range(3):
        b.Update(); never.Update()
    d = b.EpisodeLogDrain()                            # boundary 4: the ten envs that were not reset reach their 5 frames
    assert list(d["env"]) == [e for e in range(n) if e not in (3, 7)] and (d["frames"] == 5).all() and (d["boundary"] == 4).all()
    for _ in range(2):
        b.Update(); never.Update()
    d = b.EpisodeLogDrain()                            # boundary 6: the two that were, 5 frames behind the reset
    tr = b.TraceRead()
    assert list(d["env"]) == [3, 7] and list(d["frames"]) == [5, 5] and list(d["boundary"]) == [6, 6] and not d["episode"].any()
    assert list(d["cycles"]) == [int(tr["num_cycles"][e, 6]) - int(c) for e, c in zip((3, 7), c_reset)]
    # set and replace refuse a frame in flight; so does the info call
    b.UpdateBegin(); never.UpdateBegin()
    for call in (lambda: b.EpisodeLog(8), b.EpisodeLogOff, b.EpisodeLogInfo):
        refused(call, "frame is in flight")
    b.UpdateEnd(); never.UpdateEnd()
    # snapshot restore and clone leave the rings and the records alone
    for _ in range(2):
        b.Update(); never.Update()
    info = b.EpisodeLogInfo()
    assert info["written"] == n + 10                   # (boundary 9: the ten again)
    snap, snap2 = b.SaveState(), never.SaveState()
    b.RestoreState(snap); never.RestoreState(snap2)
    b.CloneEnvs([1], [4]); never.CloneEnvs([1], [4])
    snap.free(); snap2.free()
    assert b.EpisodeLogInfo() == info
    d = b.EpisodeLogDrain()
    assert list(d["env"]) == [e for e in range(n) if e not in (3, 7)] and (d["episode"] == 1).all() and (d["frames"] == 5).all()
    b.Update(); never.Update()                        # boundary 10: envs 3 and 7 count on where they were (frames 4 -> 5), a clone's target included
    b.Update(); never.Update()
    d = b.EpisodeLogDrain()
    assert list(d["env"]) == [3, 7] and list(d["frames"]) == [5, 5] and list(d["episode"]) == [1, 1] and list(d["boundary"]) == [11, 11]
    # replacing the log zeroes everything
    b.Update(); never.Update()
    b.EpisodeLog(16)
    assert b.EpisodeLogInfo() == dict(capacity=16, n_groups=info["n_groups"], written=0, lost=0) and len(b.EpisodeLogDrain()["env"]) == 0
    b.Update(); never.Update()
    b.Update(); never.Update()                        # (the limit's own count went on: its next common end is two boundaries on, the log's frames say 2)
    d = b.EpisodeLogDrain()
    assert list(d["env"]) == [e for e in range(n) if e not in (3, 7)] and (d["frames"] == 2).all() and not d["episode"].any() and (d["boundary"] == 1).all()
    # removing it, then frames: the batch equals the one that never had a log
    b.EpisodeLogOff()
    assert b.EpisodeLogInfo() == dict(capacity=0, n_groups=0, written=0, lost=0)
    refused(lambda: b.EpisodeLogDrain(), "no episode log")
    for _ in range(4):
        b.Update(); never.Update()
    sa, sb = X.env_states(b), X.env_states(never)
    for e in range(n):
        bad = X.same_record(sa[e], sb[e])
        assert bad is None, "env %d: EnvState.%s differs from the batch that never had a log" % (e, bad)


# ---- 5. external policy mode ----
def test_external_log_equals_internal(da, om, monkeypatch, n=16, frames=90):
    """Run A (internal) and its replay through the external hand-over: the two logs hold the same rows in every field but `boundary` (B's boundaries are ticks)."""
    extra = dict(terrain_seed=70, rand_seed=2)
    made = []

    def logged_batch(da_, arg, n_, **kw):
        b = made_batch(da_, arg, n_, **kw)
        b.EpisodeLog(1024)
        made.append(b)
        return b
    made_batch = X.batch
    monkeypatch.setattr(X, "batch", logged_batch)
    rec, decisions, blind_from, _, a = X.run_internal(da, om, DOG, n, frames, extra)
    blind_from = dict(blind_from)
    compared, _, b = X.replay_external(da, om, DOG, n, frames, extra, rec, decisions, blind_from)
    assert made == [a, b] and b.external and compared > 0
    da_, db = a.EpisodeLogDrain(), b.EpisodeLogDrain()
    assert in_order(da_) and in_order(db) and da_["lost"] == 0 and db["lost"] == 0
    ra, rb = rows_of(da_, skip=("boundary",)), rows_of(db, skip=("boundary",))
    same = 0
    for e in range(n):
        ia, ib = [i for i in range(len(ra)) if da_["env"][i] == e], [i for i in range(len(rb)) if db["env"][i] == e]
        done = 0
        for k, i in enumerate(ia):
            done += int(da_["frames"][i])
            assert int(da_["boundary"][i]) == done - 1          # internal: a boundary per frame
            if done > blind_from[e]:
                break
            assert k < len(ib) and ra[i] == rb[ib[k]], "env %d episode %d differs between the internal run and its external replay" % (e, k)
            assert int(db["boundary"][ib[k]]) >= int(da_["boundary"][i])
            same += 1
    print(dict(internal=len(ra), external=len(rb), compared=same))
    assert same >= 3, "the run is meant to end episodes inside the compared frames"


def test_a_parked_env_counts_no_frame(da, om, n=8, ticks=60):
    b = X.batch(da, DOG, n, policy_mode="external", terrain_seed=70, rand_seed=2, min_perturb=E.HARD[0], max_perturb=E.HARD[1], min_pertrub_duration=0.1, max_perturb_duration=0.25)
    b.EpisodeLog(256)
    table = b.ActionTable()
    completed = np.zeros((ticks, n), bool)
    for t in range(ticks):
        if t % 2 == 0:
            b.ApplyRandForce(t)                        # hard pushes: the dog falls within the run
        b.Update()
        park, _ = b.ExtEnvInfo()
        completed[t] = park == 0
        ids, _ = b.PendingActions(with_states=False)
        if len(ids):
            b.SupplyActions(ids, [0] * len(ids), np.array([table[0]] * len(ids)))
    d = b.EpisodeLogDrain()
    first = {}
    for i, e in enumerate(d["env"]):
        first.setdefault(int(e), i)
    parked = 0
    for e, i in first.items():                         # an env's first row: the frames it completed up to that tick, not the ticks
        t = int(d["boundary"][i])
        assert int(d["frames"][i]) == int(completed[:t + 1, e].sum()) and completed[t, e], (e, t)
        parked += t + 1 - int(d["frames"][i])
    print(dict(rows=len(d["env"]), envs=len(first), parked_ticks=parked))
    assert len(first) >= 2 and parked >= 2, "the run is meant to end episodes of envs that were parked for some ticks"


# ---- 6. in flight ----
@pytest.mark.parametrize("mode", T.MODES, ids=T.MODE_IDS)
def test_drain_while_a_frame_is_in_flight(da, om, mode, frames=14):
    seq, b = (pushed_batch(om, mode) for _ in range(2))
    seq.EpisodeLog(1024); b.EpisodeLog(1024)
    pushed_run(seq, frames)
    want = seq.EpisodeLogDrain()
    parts = []
    for f in range(frames):
        if f % 2 == 0:
            b.ApplyRandForce(f)
        b.UpdateBegin()
        d = b.EpisodeLogDrain()                        # no error, no wait: what has been published -- rows of completed boundaries only
        assert (d["boundary"] <= f).all() and in_order(d)
        parts.append(d)
        b.UpdateEnd()
        d = b.EpisodeLogDrain()
        assert (d["boundary"] == f).all()
        parts.append(d)
    got = concat(parts)
    assert len(want["env"]) >= 10 and got["lost"] == 0 and rows_of(got) == rows_of(want)


# ---- 7. the training loop ----
LOOP_TRAINER = dict(trainer_device="cpu", trainer_lib=os.path.join(os.path.dirname(__file__), "emul", "libdtrl_trainer_emul.so"))   # (the GPU twin: the native trainer on the device)


def loop_run(**more):
    from deepterrainrl_amd import train_loop
    extra = {"terrain_seed": 3, "trainer_num_init_samples": 10, "trainer_replay_mem_size": 512, "trainer_freeze_target_iters": 4,
             "init_exp_rate": 0.3, "init_exp_base_rate": 0.1, "trainer_init_input_offset_scale": "false"}
    kw = dict(num_envs=32, seed=1, scenario_cls=VR.Scenario, trainer="hip", extra_args=extra, max_frames=12, log_every=4, episode_limit=dict(frames=(2, 5), seed=3), **LOOP_TRAINER)
    kw.update(more)
    return train_loop.train(VR.V.TRAIN, REFDATA, **kw)


@pytest.mark.parametrize("overlap", [False, True], ids=["sequential", "overlapped"])
def test_train_loop_logs_episodes(da, om, overlap):
    out = loop_run(episode_log=256, overlap=overlap)
    tot = out["episode_log"]
    resets = out["log"][-1][4]["resets"]
    print(dict(tot=tot, resets=resets, log=[entry[5] for entry in out["log"]]))
    assert out["frames"] == 12 and tot["lost"] == 0 and tot["episodes"] >= 32 * 2
    assert tot["episodes"] == resets                   # (the last log entry's EvalStats: frame 12 is a log frame, and no frame is in flight behind it)
    per = [entry[5] for entry in out["log"]]
    assert len(per) == 3 and sum(p["episodes"] for p in per) == tot["episodes"] and all(2 <= p["mean_frames"] <= 5 and 0.0 <= p["fall_share"] <= 1.0 and np.isfinite(p["mean_dist"]) for p in per)
    plain = loop_run(overlap=overlap)
    assert "episode_log" not in plain and all(len(entry) == 5 for entry in plain["log"])
    assert np.asarray(plain["weights"]).tobytes() == np.asarray(out["weights"]).tobytes(), "the log changed what was trained"


# ---- 8. the outcomes tool ----
def test_episode_outcomes_tool(da, om, n=8, frames=20):
    """tools/episode_outcomes.py on a tiny shape: every drained episode ran under its private record, the factors recomputed from the rows' draws lie in the
    ranges, and the two tables count every episode once."""
    import argparse
    import sys
    from conftest import REPO
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import episode_outcomes
    a = argparse.Namespace(character="dog", envs=n, frames=frames, chunk=5, capacity=256, limit=[3, 6], mass_range=[0.7, 1.5], torque_range=[0.6, 1.2], bins=4, seed=11)
    rows, fac, lost = episode_outcomes.run(a, scenario_cls=T.Scenario, data_root=REFDATA)
    k = len(rows["env"])
    assert lost == 0 and k >= n * (frames // 6) and fac.shape[:2] == (k, 4)
    assert (rows["variant"] == 1 + rows["env"]).all() and (rows["rescale_draw"] >= 0).all() and (rows["rescale_draw"] == rows["episode"]).all()
    assert (fac[:, 0] >= 0.7).all() and (fac[:, 0] <= 1.5).all() and (fac[:, 3] >= 0.6).all() and (fac[:, 3] <= 1.2).all() and (fac[:, 1:3] == 1.0).all()
    for quantity, q in (("mass", 0), ("torque_lim", 3)):
        lines = episode_outcomes.table(rows, fac, a, quantity, q)
        assert len(lines) == 1 + a.bins and sum(int(l.split()[1]) for l in lines[1:]) == k, lines
