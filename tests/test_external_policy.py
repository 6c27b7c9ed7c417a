"""External policy mode (`-policy_mode= external`): envs park at their decisions, the caller supplies the actions (include/dtrl.h dtrl_pending_actions ...).
Runs on the lane-loop check build of the kernel source (tests/emul); tests/test_gpu_external_policy.py points `batch` / `Scenario` at the product library."""
import os

import numpy as np
import pytest

import test_host_and_emul as H
from conftest import REFDATA, EmulScenario, dog_policy, emul_f32_scenario

Scenario = EmulScenario   # the GPU twin points this at the product class


def batch(da, arg, n, **extra):
    if extra.get("physics_precision") == "f32" and Scenario is EmulScenario:
        return emul_f32_scenario(arg, n, data_root=REFDATA, extra_args=extra)
    return Scenario(arg, n, data_root=REFDATA, extra_args=extra)


DOG, RAPTOR, TRAIN = "args/dog_slopes_mixed_args.txt", "args/raptor_narrow_gaps_args.txt", "args/opt_args_train_mace.txt"
EXT_FIELDS = ("ext_park", "ext_steps_left")


def policy_for(om, arg):
    return H.raptor_policy(om) if "raptor" in arg else dog_policy(om)


def env_states(b):
    """Every env's whole EnvState record (q, qd, torques, action, FSM, timers, contact cache, counters, episode statistics ...) as a structured array."""
    s = b.SaveState()
    try:
        return s.env_state()
    finally:
        s.free()


def same_record(a, b, skip=()):
    """Field by field and byte by byte (a NaN equals itself); returns the first field that differs, or None."""
    for name in a.dtype.names:
        if name not in skip and a[name].tobytes() != b[name].tobytes():
            return name
    return None


def ground_key(b, e):
    segs, nb = b.GroundWindow(e)
    return [(mn, mx, h.tobytes()) for mn, mx, h in segs], nb


def observe(b, envs):
    st = env_states(b)
    ps = b.RecordPoliState()
    return {e: (st[e].copy(), ps[e].copy(), ground_key(b, e)) for e in envs}


def run_internal(da, om, arg, n, frames, extra, exp_scenario=False):
    """Run A: internal mode, exploration off. Per frame: every env's observation; per env: the net's decisions the per-frame record can see, and the frame from
    which the env has to be left out (two decisions in one frame, or a decision in the frame whose end reset the env: the record shows only the later event)."""
    b = batch(da, arg, n, **extra)
    pol = policy_for(om, arg)
    b.SetPolicy(pol[1], *pol[2:])
    b.SetExplore(0, 0.0, 1.0, 0.0)
    rec, tuples = [], {e: [] for e in range(n)}
    decisions = {e: [] for e in range(n)}
    blind_from = {e: frames + 1 for e in range(n)}
    nc0 = np.zeros(n, np.int64); nr0 = np.zeros(n, np.int64)
    reset_before = np.ones(n, bool)          # Exp: the first decision after Init / a reset is the queued random action, served without asking
    for f in range(frames):
        b.Update()
        rec.append(observe(b, range(n)))
        nc, nr, _, _, prm = b.CycleInfo()
        _, _, aid, _, _ = b.Ctrl()
        for e in range(n):
            d = int(nc[e] - nc0[e])
            if exp_scenario:
                d -= int(nr[e] - nr0[e])     # the cycle cScenarioExp closes at a fall (frame_end) is not a decision
                if reset_before[e] and d > 0:
                    d -= 1                   # ... nor is the commanded first action
                    reset_before[e] = False
            if d > 1 or (d == 1 and nr[e] != nr0[e]):
                blind_from[e] = min(blind_from[e], f)
            elif d == 1:
                decisions[e].append((int(aid[e]), prm[e].copy()))
            if nr[e] != nr0[e]:
                reset_before[e] = True
        nc0, nr0 = nc, nr
        if exp_scenario:
            rows, fl, ids = b.DrainTuples()
            for r, x, e in zip(rows, fl, ids):
                tuples[int(e)].append((r.tobytes(), int(x)))
    return rec, decisions, blind_from, tuples, b


def replay_external(da, om, arg, n, frames, extra, rec, decisions, blind_from, exp_scenario=False, flags_of=None):
    """Run B: the same arguments plus -policy_mode= external; at env e's k-th request it gets run A's k-th recorded decision. Whenever an env completes frame f
    it is compared with run A after frame f. Returns (compared env-frames, tuples per env, batch)."""
    b = batch(da, arg, n, policy_mode="external", **extra)
    table = b.ActionTable()
    frames_done = np.zeros(n, int); k = np.zeros(n, int)
    tuples = {e: [] for e in range(n)}
    compared = 0
    for tick in range(4 * frames):
        if frames_done.min() >= frames:
            break
        b.Update()
        park, left = b.ExtEnvInfo()
        assert np.all((park == 1) | ((park == 0) & (left == 0))), (park, left)   # after a tick an env is parked or has completed its frame
        done = [e for e in range(n) if park[e] == 0]
        obs = observe(b, done)
        for e in done:
            f = frames_done[e]
            frames_done[e] += 1
            if f >= frames or f >= blind_from[e]:
                continue
            sa, pa, ga = rec[f][e]
            sb, pb, gb = obs[e]
            bad = same_record(sa, sb, skip=EXT_FIELDS)
            assert bad is None, "env %d frame %d (tick %d): EnvState.%s differs from the internal run" % (e, f, tick, bad)
            assert pa.tobytes() == pb.tobytes(), "env %d frame %d: policy state differs" % (e, f)
            assert ga == gb, "env %d frame %d: ground window differs" % (e, f)
            assert sb["ext_park"] == 0 and sb["ext_steps_left"] == 0
            compared += 1
        if exp_scenario:
            rows, fl, ids = b.DrainTuples()
            for r, x, e in zip(rows, fl, ids):
                tuples[int(e)].append((r.tobytes(), int(x)))
        ids, _ = b.PendingActions(with_states=False)
        if len(ids):
            aids, prms = [], []
            for e in ids:
                if k[e] < len(decisions[e]):
                    a, p = decisions[e][k[e]]
                else:                                   # beyond what run A recorded (the env is ahead of the slowest one, or was left out): any valid row
                    a, p = 0, table[0]
                    blind_from[e] = min(blind_from[e], frames_done[e])
                k[e] += 1
                aids.append(a); prms.append(p)
            fl = None if flags_of is None else [flags_of(int(e)) for e in ids]
            b.SupplyActions(ids, aids, np.array(prms), fl)
    assert frames_done.min() >= frames, ("envs did not get through their frames", frames_done)
    return compared, tuples, b


REPLAY_CASES = [
    pytest.param(DOG, dict(terrain_seed=70, rand_seed=2), id="dog_slopes_mixed"),
    pytest.param(RAPTOR, dict(terrain_seed=70, rand_seed=2), id="raptor_narrow_gaps"),
    pytest.param(DOG, dict(terrain_seed=70, rand_seed=2, physics_precision="f32"), id="dog_fp32"),
    pytest.param(DOG, dict(terrain_seed=70, rand_seed=2, terrain_gen="device"), id="dog_device_terrain"),
]


@pytest.mark.parametrize("arg,extra", REPLAY_CASES)
def test_replay_internal_run_bit_for_bit(da, om, arg, extra, n=16, frames=90):
    """Run A (internal, xavier policy, exploration off, PoliEval: falls and resets included) replayed through the external hand-over: every env, at the end of each
    of its frames, is the env of run A after that frame -- the whole EnvState record, the policy state and the ground window, bit for bit. An env whose decisions
    the per-frame record of run A cannot tell apart is left out from that frame on; at most 5 % of the envs may be."""
    rec, decisions, blind_from, _, a = run_internal(da, om, arg, n, frames, extra)
    left_out = sum(1 for e in range(n) if blind_from[e] <= frames)
    assert left_out <= 0.05 * n, ("run A: too many envs with unseen decisions, pick another terrain seed", blind_from)
    assert a.EvalStats()["resets"] > 0 and min(len(d) for d in decisions.values()) >= 3, "the run is meant to cover falls, resets and several decisions per env"
    compared, _, b = replay_external(da, om, arg, n, frames, extra, rec, decisions, dict(blind_from))
    assert compared >= 0.95 * n * frames, compared
    s = b.ExtStats()
    assert s["env_frames_total"] >= n * frames and s["env_steps_total"] >= n * frames * b.num_update_steps


def test_exp_scenario_tuples_equal(da, om, n=16, frames=90):
    """The same replay on the MACE training scene (cScenarioExp): the tuples B writes on the device -- rows and flag words, per env in order, the cycles served by
    the queued random first action included -- are run A's. A second external run supplies flag words and finds them in its rows."""
    extra = dict(terrain_seed=74, rand_seed=2)   # (terrain seeds 70 - 72 each leave one env of run A with a decision in the frame that ends in its reset; 73 - 75 none)
    rec, decisions, blind_from, ta, _ = run_internal(da, om, TRAIN, n, frames, extra, exp_scenario=True)
    left_out = sum(1 for e in range(n) if blind_from[e] <= frames)
    assert left_out <= 0.05 * n, ("run A: too many envs with unseen decisions, pick another terrain seed", blind_from)
    bf = dict(blind_from)
    compared, tb, _ = replay_external(da, om, TRAIN, n, frames, extra, rec, decisions, bf, exp_scenario=True)
    assert compared >= 0.95 * n * frames, compared
    total = 0
    for e in range(n):
        if blind_from[e] <= frames:
            continue
        assert tb[e][:len(ta[e])] == ta[e], "env %d: tuples differ (%d / %d rows)" % (e, len(tb[e]), len(ta[e]))
        total += len(ta[e])
    assert total >= 3 * n
    assert all(x & 6 == 0 for e in range(n) for _, x in ta[e])   # (the cycle the commanded first action starts is the episode's warm-up cycle: it shapes the states, its own tuple is not recorded)
    # supplied flag words appear in the rows: env e's decisions all carry F_e
    want = lambda e: (0, 2, 4, 6)[e % 4]
    _, tf, _ = replay_external(da, om, TRAIN, n, 40, extra, rec, decisions, {e: 0 for e in range(n)}, exp_scenario=True, flags_of=want)
    for e in range(n):
        got = {x & 6 for _, x in tf[e]}
        assert got <= {want(e)}, (e, got)
        assert not tf[e] or want(e) in got, (e, got, len(tf[e]))
    assert {x & 6 for e in range(n) for _, x in tf[e]} == {0, 2, 4, 6} and sum(1 for e in range(n) if tf[e]) >= n // 2


def test_first_decision_against_oracle_forward(da, om, n=8):
    """The states handed out are the policy states the internal run recorded, bit for bit; the oracle's forward on them, supplied as (argmax fragment, its parameters),
    gives the controller parameters of the internal run's in-kernel forward within 1e-14 of the largest net output (test_policy_output_vs_oracle_forward's bound)."""
    extra = dict(terrain_seed=70, rand_seed=2)
    pol = dog_policy(om)
    m, _ = om.build_model(DOG, REFDATA)
    a = batch(da, DOG, n, **extra)
    a.SetPolicy(pol[1], *pol[2:]); a.SetExplore(0, 0.0, 1.0, 0.0)
    a.Update()
    assert np.array_equal(a.CycleInfo()[0], np.ones(n)), "one decision per env in the first frame"
    b = batch(da, DOG, n, policy_mode="external", **extra)
    b.Update()
    ids, states = b.PendingActions()
    assert np.array_equal(ids, np.arange(n))
    assert np.array_equal(states, a.RecordPoliState())
    assert np.array_equal(states, b.RecordPoliState())
    o = om.OracleEnv(m, terrain_seed=70, rng_seed=2, env_id=0, policy=pol)
    nf, fs = a.num_frags, a.frag_size
    aids, prms, ymax = [], [], []
    for i in range(n):
        y = o.nn_eval(states[i])[-a.nn_out:]
        k = int(np.argmax(y[:nf]))
        aids.append(k); prms.append(y[nf + k * fs: nf + (k + 1) * fs]); ymax.append(np.abs(y).max())
    b.SupplyActions(ids, aids, np.array(prms))
    b.Update()
    park, left = b.ExtEnvInfo()
    assert not park.any() and not left.any()
    _, _, aid_a, prm_a, _ = a.Ctrl()
    _, _, aid_b, prm_b, _ = b.Ctrl()
    assert np.array_equal(aid_a, aid_b)
    for i in range(n):
        err = np.abs(prm_a[i] - prm_b[i]).max()
        print("env %d: |params(internal) - params(external, oracle forward)| = %.3e, bound %.3e" % (i, err, 1e-14 * ymax[i]))
        assert err <= 1e-14 * ymax[i], (i, err, ymax[i])


def scripted(b, by_env=False):
    """by_env: the env's id is added to the label. Envs that start alike on level ground hand out the same state and, under the plain form, take the same rows
    until the terrain ahead of them differs -- a whole batch can walk one trajectory; with the id in the label they part at the first decision."""
    table = b.ActionTable()

    def policy(ids, states):
        lab = (np.abs(states[:, 200:]).sum(axis=1) * 1000).astype(np.int64)   # a function of the state alone (by_env: and of the env): the same state gets the same row
        lab = (lab + ids if by_env else lab) % len(table)
        return lab.astype(np.int32), table[lab]
    return policy


def test_liveness_and_accounting(da, om, n=64, ticks=200):
    """A scripted policy, 64 envs, 200 ticks: no delivered action is left unconsumed by the next tick; an env nobody answers stays put bit for bit while the others
    go on; the device's env-step count is the sum of what the envs' clocks say; awaiting + ready never exceeds the batch."""
    b = batch(da, DOG, n, policy_mode="external", terrain_seed=5, rand_seed=3)
    policy = scripted(b)
    dt_step = (1.0 / 30.0) / b.num_update_steps
    st = env_states(b)
    implied = 0
    mute, mute_from, mute_to = 5, 60, 90
    frozen = None
    for t in range(ticks):
        park0, left0 = b.ExtEnvInfo()
        b.Update()
        s = b.ExtStats()
        assert s["ready"] == 0, "tick %d: %d delivered actions were not consumed" % (t, s["ready"])
        assert s["awaiting"] + s["ready"] <= n
        st1 = env_states(b)
        for e in range(n):
            if st1[e]["num_resets"] != st[e]["num_resets"]:
                implied += left0[e] if left0[e] > 0 else b.num_update_steps      # the env completed its frame (fell) and was reset: its clock restarted
            else:
                implied += int(round((st1[e]["time"] - st[e]["time"]) / dt_step))
        assert s["env_steps_total"] == implied, (t, s, implied)
        ids, states = b.PendingActions()
        assert len(ids) == s["awaiting"] and np.all(np.diff(ids) > 0)
        if mute_from <= t < mute_to and mute in ids:
            if frozen is None:
                frozen = (st1[mute].copy(), b.RecordPoliState([mute]).copy(), t)
            else:
                assert same_record(frozen[0], st1[mute]) is None and np.array_equal(frozen[1], b.RecordPoliState([mute]))
            keep = ids != mute
            ids, states = ids[keep], states[keep]
        if len(ids):
            b.SupplyActions(ids, *policy(ids, states))
        st = st1
    assert frozen is not None and frozen[2] < mute_to - 10, "the muted env was meant to wait for several ticks"
    assert st["time"][mute] != frozen[0]["time"] or st["num_resets"][mute] != frozen[0]["num_resets"], "the muted env goes on once it is answered"
    s = b.ExtStats()
    assert s["env_frames_total"] > n * ticks * 0.8 and s["env_steps_total"] > 0


def full_state(b):
    n = b.num_envs
    return env_states(b), b.RecordPoliState(), [ground_key(b, e) for e in range(n)], b.ExtEnvInfo()


def assert_same_full(x, y):
    assert same_record(x[0], y[0]) is None, same_record(x[0], y[0])
    assert np.array_equal(x[1], y[1]) and x[2] == y[2]
    assert np.array_equal(x[3][0], y[3][0]) and np.array_equal(x[3][1], y[3][1])


@pytest.mark.parametrize("extra", [dict(), dict(terrain_gen="device")], ids=["host_terrain", "device_terrain"])
def test_snapshots_carry_park_state_and_delivered_actions(da, om, extra, n=16):
    """Saved mid-run with some envs awaiting and some holding a delivered action: after a restore -- and after an export / import -- the same 20 ticks with the
    same rows end in the same bits. A blob of one mode is refused by a batch of the other, by name."""
    b = batch(da, DOG, n, policy_mode="external", terrain_seed=5, rand_seed=3, **extra)
    policy = scripted(b)

    def go(ticks):
        for _ in range(ticks):
            ids, states = b.PendingActions()
            if len(ids):
                b.SupplyActions(ids, *policy(ids, states))
            b.Update()
    b.Update()
    go(14)
    # every second awaiting env gets its action now: the snapshot holds awaiting envs, ready envs and envs in between frames
    for _ in range(40):
        ids, states = b.PendingActions()
        if len(ids) >= 2:
            break
        go(1)
    assert len(ids) >= 2
    half = ids[::2]
    aid, prm = policy(ids, states)
    b.SupplyActions(half, aid[::2], prm[::2])
    park, _ = b.ExtEnvInfo()
    assert (park == 1).any() and (park == 2).any()
    snap = b.SaveState()
    at_save = full_state(b)
    go(20)
    first = full_state(b)
    assert same_record(at_save[0], first[0]) is not None
    b.RestoreState(snap)
    assert_same_full(at_save, full_state(b))
    go(20)
    assert_same_full(first, full_state(b))
    blob = snap.export()
    hdr = np.frombuffer(blob[:da.SNAP_HEADER_DTYPE.itemsize], da.SNAP_HEADER_DTYPE)[0]
    assert int(hdr["policy_mode"]) == 1
    snap2 = b.ImportState(blob)
    b.RestoreState(snap2)
    go(20)
    assert_same_full(first, full_state(b))
    # the other mode
    c = batch(da, DOG, n, terrain_seed=5, rand_seed=3, **extra)
    with pytest.raises(da.DtrlError, match="policy_mode"):
        c.ImportState(blob)
    blob_c = c.SaveState().export()
    assert int(np.frombuffer(blob_c[:da.SNAP_HEADER_DTYPE.itemsize], da.SNAP_HEADER_DTYPE)[0]["policy_mode"]) == 0
    with pytest.raises(da.DtrlError, match="policy_mode"):
        b.ImportState(blob_c)
    # an edited blob: the new fields are range-checked like the other indices
    bad = bytearray(blob)
    snap.env_state(bad)["ext_park"][0] = 7
    with pytest.raises(da.DtrlError, match="ext_park"):
        b.ImportState(bad)
    bad = bytearray(blob)
    snap.env_state(bad)["ext_steps_left"][0] = 1000
    with pytest.raises(da.DtrlError, match="ext_steps_left"):
        b.ImportState(bad)


def test_refusals(da, om, n=4):
    """Every misuse is DTRL_ERR_ARG with a message naming the cause, and changes nothing."""
    pol = dog_policy(om)
    b = batch(da, DOG, n, policy_mode="external", terrain_seed=5, rand_seed=3)
    assert b.external and b.n_opt == b.frag_size and b.n_labels >= 1
    before = full_state(b)
    ids, _ = b.PendingActions()
    assert len(ids) == 0                                    # nothing has run yet
    row = b.ActionTable()[:1]
    with pytest.raises(da.DtrlError, match="not awaiting"):
        b.SupplyActions([0], [0], row)
    for call, name in ((lambda: b.StepUpdates(1), "dtrl_step_updates"), (lambda: b.RunFrames(1), "dtrl_run_frames"), (lambda: b.UpdatePoll(), "dtrl_step_poll"),
                       (lambda: b.UpdateEndBegin(), "dtrl_step_end_begin"), (lambda: b.SetTuplePipelining(True), "dtrl_set_tuple_pipelining"),
                       (lambda: b.SetPolicy(pol[1], *pol[2:]), "dtrl_set_policy"),
                       (lambda: b.LoadScale(os.path.join(REFDATA, "data/policies/dog/models/dog_mace3_slopes_mixed_model_scale.txt")), "dtrl_load_scale_file")):
        with pytest.raises(da.DtrlError, match=name + ".*policy_mode= external"):
            call()
    assert_same_full(before, full_state(b))
    b.Update()
    ids, _ = b.PendingActions()
    assert np.array_equal(ids, np.arange(n))
    before = full_state(b)
    for bad_ids, bad_lab, what in (([0, 0], [0, 0], "listed twice"), ([0, n], [0, 0], "out of range"), ([0, 1], [0, 99], "action_id")):
        with pytest.raises(da.DtrlError, match=what):
            b.SupplyActions(bad_ids, bad_lab, np.repeat(row, 2, axis=0))
    b.SupplyActions([1], [0], row)
    with pytest.raises(da.DtrlError, match="not awaiting.*env 1.*nothing applied"):
        b.SupplyActions([0, 1], [0, 0], np.repeat(row, 2, axis=0))       # env 1 already has its action: env 0 must not get one either
    park, _ = b.ExtEnvInfo()
    assert list(park) == [1, 2, 1, 1]
    b.UpdateBegin()
    for call in (b.PendingActions, lambda: b.SupplyActions([0], [0], row), b.ExtStats, b.ExtEnvInfo):
        with pytest.raises(da.DtrlError, match="dtrl_step_end"):
            call()                                                       # refused, not waited for, while a tick is in flight
    b.UpdateEnd()
    # the new calls on an internal batch
    c = batch(da, DOG, n, terrain_seed=5, rand_seed=3)
    assert not c.external
    for call in (c.PendingActions, lambda: c.SupplyActions([0], [0], row), c.ExtStats, c.ExtEnvInfo):
        with pytest.raises(da.DtrlError, match="internal policy mode"):
            call()
    # Q and CACLA controllers, and a misspelt mode, at create
    for arg, word in (("args/opt_args_train_q.txt", "dog.*Q controller"), ("args/opt_args_train_cacla.txt", "dog_cacla.*CACLA controller")):
        with pytest.raises(da.DtrlError, match=r"\(1\).*" + word):       # DTRL_ERR_ARG
            batch(da, arg, n, policy_mode="external")
    with pytest.raises(da.DtrlError, match=r"\(1\).*policy_mode"):
        batch(da, DOG, n, policy_mode="outside")


def test_run_external_host_callable(da, om, n=16):
    """deepterrainrl_amd.external.run_external with a Python callable goes through the host calls."""
    from deepterrainrl_amd.external import run_external
    b = batch(da, DOG, n, policy_mode="external", terrain_seed=5, rand_seed=3)
    r = run_external(b, scripted(b), 40)
    assert r["decisions"] >= n and r["rejected"] == 0 and r["env_steps_total"] > 30 * n * b.num_update_steps
    assert np.isfinite(b.PoseVel()[0]).all()
    c = batch(da, DOG, n, terrain_seed=5, rand_seed=3)
    with pytest.raises(ValueError):
        run_external(c, scripted(c), 1)


class HostArrays:
    """The arrays of the device calls on the lane-loop build, where "device" memory is host memory; the GPU twin passes the same four operations on torch tensors."""
    @staticmethod
    def full(shape, value, dtype):
        return np.full(shape, value, dtype)

    @staticmethod
    def ptr(t):
        return t.ctypes.data

    @staticmethod
    def read(t):
        return t

    @staticmethod
    def write(t, values):
        t[:len(values)] = values


def run_hand_over_at_width(da, om, n=2304, ticks=20, arrays=HostArrays):
    """dtrl_pending_actions / dtrl_pending_actions_device above 1024 envs (a chunk of three envs per thread of the collection at 2304), tick by tick against
    ExtEnvInfo and RecordPoliState: the ids are the awaiting envs in ascending order, the states their policy states (float32 of them in the device call); a `cap`
    below the number awaiting -- 1, 1000, awaiting - 1: it cuts the list inside one thread's chunk -- hands out exactly the first `cap` of them and leaves the
    arrays behind `cap` as they were. One batch is driven through the host calls, one through the device calls, with the same float-rounded rows: equal at the end.
    Returns (smallest, largest) number of awaiting envs seen."""
    import ctypes
    mk = lambda: batch(da, DOG, n, policy_mode="external", terrain_seed=9, rand_seed=1)
    bd, bh = mk(), mk()
    table = bh.ActionTable()
    S = bh.S
    ID_SENT, ST_SENT = -7, -12345.0
    ids_t = arrays.full(n, ID_SENT, np.int32); st_t = arrays.full((n, S), ST_SENT, np.float32)
    lab_t = arrays.full(n, 0, np.int32); prm_t = arrays.full((n, bd.n_opt), 0.0, np.float32)
    ids_h = np.empty(n, np.int32); st_h = np.empty((n, S), np.float64)
    seen, cut = [], {"one": 0, "thousand": 0, "all_but_one": 0}

    def device_call(cap, want_ids, want_st32):
        arrays.write(ids_t, np.full(n, ID_SENT, np.int32)); arrays.write(st_t, np.full((n, S), ST_SENT, np.float32))
        m = bd.PendingActionsDevice(arrays.ptr(ids_t), arrays.ptr(st_t), cap)
        assert m == min(len(want_ids), cap)
        gi, gs = arrays.read(ids_t), arrays.read(st_t)
        assert np.array_equal(gi[:m], want_ids[:m]) and np.array_equal(gs[:m], want_st32[:m])
        assert np.all(gi[m:] == ID_SENT) and np.all(gs[m:] == ST_SENT), "written behind cap"
        return m

    def host_call(cap, want_ids, want_st):
        ids_h[:] = ID_SENT; st_h[:] = ST_SENT
        m = ctypes.c_int(-1)
        bh._chk(bh._lib.dtrl_pending_actions(bh._h, da._p(ids_h), da._p(st_h), int(cap), ctypes.byref(m)))
        m = m.value
        assert m == min(len(want_ids), cap)
        assert np.array_equal(ids_h[:m], want_ids[:m]) and np.array_equal(st_h[:m], want_st[:m])
        assert np.all(ids_h[m:] == ID_SENT) and np.all(st_h[m:] == ST_SENT), "written behind cap"

    for t in range(ticks):
        bd.Update(); bh.Update()
        park, _ = bh.ExtEnvInfo()
        assert np.array_equal(park, bd.ExtEnvInfo()[0]), t
        want_ids = np.flatnonzero(park == 1).astype(np.int32)
        awaiting = len(want_ids)
        seen.append(awaiting)
        if awaiting == 0:
            continue
        want_st = bh.RecordPoliState(want_ids)
        assert np.array_equal(want_st, bd.RecordPoliState(want_ids)), t
        want_st32 = want_st.astype(np.float32)
        for name, cap in (("one", 1), ("thousand", 1000), ("all_but_one", awaiting - 1)):
            if 0 < cap < awaiting:
                device_call(cap, want_ids, want_st32)
                host_call(cap, want_ids, want_st)
                cut[name] += 1
        host_call(n, want_ids, want_st)
        m = device_call(n, want_ids, want_st32)
        # the same float-rounded rows to both: a function of the handed-out float32 state alone
        lab = ((np.abs(want_st32[:, 200:].astype(np.float64)).sum(axis=1) * 1000).astype(np.int64) % len(table)).astype(np.int32)
        prm = (table[lab] * (1.0 + 0.01 * np.sin(want_st32[:, 200:201].astype(np.float64)))).astype(np.float32)   # not a table row: exercises the float -> real conversion
        arrays.write(lab_t, lab); arrays.write(prm_t, prm)
        assert bd.SupplyActionsDevice(arrays.ptr(ids_t), m, arrays.ptr(lab_t), arrays.ptr(prm_t), 0) == 0
        bh.SupplyActions(want_ids, lab, prm.astype(np.float64))
    print("hand-over at %d envs: awaiting per tick %s, cutting caps used %s" % (n, seen, cut))
    assert any(0 < k < 1024 for k in seen) and any(k > 1024 for k in seen), seen      # a sparse subset, and more than one env per thread of the collection
    assert cut["one"] >= 2 and cut["thousand"] >= 1 and cut["all_but_one"] >= 2, cut
    assert_same_full(full_state(bd), full_state(bh))
    assert bd.ExtStats() == bh.ExtStats()
    return min(k for k in seen if k > 0), max(seen)


def test_hand_over_at_width(da, om):
    """The reference logic and floors of run_hand_over_at_width on the lane-loop build, at the width of the GPU twin (tests/test_gpu_handover_width.py): about 25 s."""
    lo, hi = run_hand_over_at_width(da, om)
    assert 0 < lo < 1024 < hi
