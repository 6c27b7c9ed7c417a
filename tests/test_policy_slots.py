"""Policy slots (include/dtrl.h dtrl_slots_create ...): several policies in one batch, one per env. The yardstick is always the single-policy path: env e of a
K-slot batch, sitting in slot s, must equal -- bit for bit, every field of its EnvState record, its policy state, its ground window and build count -- env e of a
single-policy batch of the same size, arguments and seeds that runs slot s's policy and exploration.
Runs on the lane-loop check build of the kernel source (tests/emul: the per-key default of Backend::LaunchKeyed); tests/test_gpu_policy_slots.py points `Scenario`
at the product library (one launch of the slot kernels)."""
import numpy as np
import pytest

import test_external_policy as X          # env_states / same_record / ground_key / observe: helpers that take a batch
import test_host_and_emul as H
from conftest import REFDATA, EmulScenario, dog_policy, emul_f32_scenario, trained_policy

Scenario = EmulScenario   # the GPU twin points this at the product class

DOG, RAPTOR, TRAIN = "args/dog_slopes_mixed_args.txt", "args/raptor_narrow_gaps_args.txt", "args/opt_args_train_mace.txt"
# (enable, rate, temp, base_rate) per slot: one greedy, two exploring with different rates
EXPLORE = [(1, 0.5, 0.25, 0.1), (0, 0.0, 1.0, 0.0), (1, 0.9, 2.0, 0.3)]


def batch(arg, n, **extra):
    if extra.get("physics_precision") == "f32" and Scenario is EmulScenario:
        return emul_f32_scenario(arg, n, data_root=REFDATA, extra_args=extra)
    return Scenario(arg, n, data_root=REFDATA, extra_args=extra)


def policies(om, arg):
    """Three policies of the scene's character: two xavier seeds and the committed trained net."""
    if "raptor" in arg:
        a = H.raptor_policy(om)
        return [a, (a[0], om.xavier_weights(a[0], 77)) + a[2:], trained_policy(om, "raptor")]
    a = dog_policy(om)
    return [a, dog_policy(om, seed=99), trained_policy(om, "dog")]


def single(arg, n, pol, explore, extra):
    b = batch(arg, n, **extra)
    b.SetPolicy(pol[1], *pol[2:])
    b.SetExplore(*explore)
    return b


def slotted(arg, n, pols, explores, assign, extra):
    b = batch(arg, n, **extra)
    b.CreateSlots(len(pols))
    b.SetPolicy(pols[0][1], *pols[0][2:])
    b.SetExplore(*explores[0])
    for s in range(1, len(pols)):
        b.SlotSetPolicy(s, pols[s][1], *pols[s][2:])
        b.SlotSetExplore(s, *explores[s])
    b.AssignSlots(None, assign)
    assert list(b.GetSlots()) == list(assign)
    return b


def assert_envs_equal(bs, ref, envs, what):
    """Envs `envs` of batch bs against the same envs of batch ref."""
    envs = list(envs)
    if not envs:
        return
    oa, ob = X.observe(bs, envs), X.observe(ref, envs)
    for e in envs:
        (sa, pa, ga), (sb, pb, gb) = oa[e], ob[e]
        bad = X.same_record(sa, sb)
        assert bad is None, "%s: env %d: EnvState.%s differs from the single-policy run" % (what, e, bad)
        assert pa.tobytes() == pb.tobytes(), "%s: env %d: policy state differs" % (what, e)
        assert ga == gb, "%s: env %d: ground window / build count differs" % (what, e)


EQUAL_CASES = [(DOG, dict(terrain_seed=11)), (RAPTOR, dict(terrain_seed=5)), (DOG, dict(terrain_seed=11, terrain_gen="device")), (RAPTOR, dict(terrain_seed=5, terrain_gen="device"))]
EQUAL_IDS = ["dog", "raptor", "dog_device_terrain", "raptor_device_terrain"]


def run_equals_single_policy(om, arg, extra, n=12, frames=45):
    pols = policies(om, arg)
    assign = [e % 3 for e in range(n)]
    bs = slotted(arg, n, pols, EXPLORE, assign, extra)
    refs = [single(arg, n, pols[s], EXPLORE[s], extra) for s in range(3)]
    c0 = X.env_states(bs)["num_cycles"].copy()
    for f in range(frames):
        bs.Update()
        for s in range(3):
            refs[s].Update()
            assert_envs_equal(bs, refs[s], [e for e in range(n) if assign[e] == s], "frame %d slot %d" % (f, s))
    st = X.env_states(bs)
    for s in range(3):   # otherwise the comparison shows nothing
        assert any(st["num_cycles"][e] > c0[e] for e in range(n) if assign[e] == s), "no env of slot %d made a decision" % s
    assert st["num_resets"].sum() >= 1, "the run saw no reset"
    return bs


@pytest.mark.parametrize("arg,extra", EQUAL_CASES, ids=EQUAL_IDS)
def test_equals_single_policy_runs(da, om, arg, extra):
    """1. 12 envs round-robin over 3 slots (two xavier seeds and the trained net; one greedy, two exploring at different rates), 45 frames: about three decisions per
    env, several resets. Every frame, every env equals its single-policy run."""
    run_equals_single_policy(om, arg, extra)


def drain_into(b, tuples):
    rows, fl, ids = b.DrainTuples()
    for r, x, e in zip(rows, fl, ids):
        tuples[int(e)].append((r.tobytes(), int(x)))


def test_exp_scenario_tuples(da, om, n=12, frames=45):
    """2. The MACE training scene (cScenarioExp), 2 slots with different nets and exploration: per env, the drained rows and flag words are the single-policy
    run's, in order."""
    extra = dict(terrain_seed=74, rand_seed=2)
    pols = policies(om, TRAIN)[:2]
    exps = [EXPLORE[0], EXPLORE[2]]
    assign = [e % 2 for e in range(n)]
    bs = slotted(TRAIN, n, pols, exps, assign, extra)
    refs = [single(TRAIN, n, pols[s], exps[s], extra) for s in range(2)]
    ts = {e: [] for e in range(n)}
    tr = [{e: [] for e in range(n)} for _ in range(2)]
    for f in range(frames):
        bs.Update(); drain_into(bs, ts)
        for s in range(2):
            refs[s].Update(); drain_into(refs[s], tr[s])
    total = 0
    for e in range(n):
        assert ts[e] == tr[assign[e]][e], "env %d (slot %d): tuples differ (%d / %d rows)" % (e, assign[e], len(ts[e]), len(tr[assign[e]][e]))
        total += len(ts[e])
    assert total >= n, total
    for s in range(2):
        assert_envs_equal(bs, refs[s], [e for e in range(n) if assign[e] == s], "end, slot %d" % s)
        assert sum(len(ts[e]) for e in range(n) if assign[e] == s) > 0, "slot %d wrote no tuple" % s
    # the two slots did explore differently: slot 1 (rate 0.9) marks more of its rows as exploratory than slot 0 would have
    assert any(x & 6 for e in range(n) for _, x in ts[e])


def test_alias_follows_slot0(da, om, n=12, frames=36, switch=12):
    """3. Slot 1 is an alias of slot 0 with exploration off, slot 0 explores. A SetPolicy on slot 0 between frames is seen by both: the result equals two
    single-policy runs making the same call."""
    extra = dict(terrain_seed=11)
    p0, p1 = policies(om, DOG)[:2]
    bs = batch(DOG, n, **extra)
    bs.CreateSlots(2)
    bs.SetPolicy(p0[1], *p0[2:]); bs.SetExplore(*EXPLORE[0])
    bs.SlotAlias(1, 0); bs.SlotSetExplore(1, *EXPLORE[1])
    assign = [e % 2 for e in range(n)]
    bs.AssignSlots(None, assign)
    refs = [single(DOG, n, p0, EXPLORE[0], extra), single(DOG, n, p0, EXPLORE[1], extra)]
    c_switch = None
    for f in range(frames):
        if f == switch:
            for b in [bs] + refs:
                b.SetPolicy(p1[1], *p1[2:])
            c_switch = X.env_states(bs)["num_cycles"].copy()
        bs.Update()
        for s in range(2):
            refs[s].Update()
            assert_envs_equal(bs, refs[s], [e for e in range(n) if assign[e] == s], "frame %d slot %d" % (f, s))
    st = X.env_states(bs)
    for s in range(2):
        assert any(st["num_cycles"][e] > c_switch[e] for e in range(n) if assign[e] == s), "no env of slot %d decided under the new weights" % s


def test_reassignment_mid_run(da, om, n=12, frames=40, at=20):
    """4. Four envs move from slot 0 to slot 1 at frame 20: from then on they equal a single-policy run whose policy and exploration are switched at that frame."""
    extra = dict(terrain_seed=11)
    pols = policies(om, DOG)[:2]
    exps = [EXPLORE[0], EXPLORE[2]]
    assign = [e % 2 for e in range(n)]
    moved = [0, 2, 4, 6]
    bs = slotted(DOG, n, pols, exps, assign, extra)
    ref = single(DOG, n, pols[0], exps[0], extra)
    c_at = None
    for f in range(frames):
        if f == at:
            bs.AssignSlots(moved, [1] * len(moved))
            assert list(bs.GetSlots(moved)) == [1] * len(moved)
            ref.SetPolicy(pols[1][1], *pols[1][2:]); ref.SetExplore(*exps[1])
            c_at = X.env_states(bs)["num_cycles"].copy()
        bs.Update(); ref.Update()
        assert_envs_equal(bs, ref, moved if f >= at else [e for e in range(n) if assign[e] == 0], "frame %d" % f)
    st = X.env_states(bs)
    assert any(st["num_cycles"][e] > c_at[e] for e in moved), "no moved env made a decision in its new slot"


def test_snapshots_and_clones_keep_the_assignment(da, om, n=8, frames=12):
    """5. The assignment is batch state. An env of slot 0 cloned onto an env of slot 1 continues under slot 1 -- it equals the same state transplanted (a blob:
    blobs carry no assignment) onto that env in a single-policy batch of slot 1's policy. Restoring a snapshot taken before a reassignment, and a reset, leave the
    assignment as it was set."""
    extra = dict(terrain_seed=11)
    pols = policies(om, DOG)[:2]
    exps = [EXPLORE[0], EXPLORE[2]]
    assign = [e % 2 for e in range(n)]
    bs = slotted(DOG, n, pols, exps, assign, extra)
    ref = single(DOG, n, pols[1], exps[1], extra)
    for f in range(frames):
        bs.Update(); ref.Update()
    snap = bs.SaveState([0])
    blob = snap.export(); snap.free()
    bs.CloneEnvs([0], [1])
    assert list(bs.GetSlots()) == assign
    s = ref.ImportState(blob); ref.RestoreState(s, [1]); s.free()
    assert_envs_equal(bs, ref, [1], "after the clone")
    c0 = X.env_states(bs)["num_cycles"][1]
    for f in range(2 * frames):
        bs.Update(); ref.Update()
        assert_envs_equal(bs, ref, [1, 3], "frame %d after the clone" % f)
    assert X.env_states(bs)["num_cycles"][1] > c0, "the clone made no decision"
    before = bs.SaveState()
    bs.AssignSlots([2, 4], [1, 1])
    want = list(assign); want[2] = want[4] = 1
    bs.RestoreState(before); before.free()
    assert list(bs.GetSlots()) == want
    bs.Reset([2, 3])
    assert list(bs.GetSlots()) == want


def check_slot_stats(b, n_slots):
    st = X.env_states(b)
    slots = b.GetSlots()
    ev = b.EvalStats()
    tot = dict(n_envs=0, episodes=0, cycles=0, resets=0); dist = 0.0
    for s in range(n_slots):
        got = b.SlotStats(s)
        assert got == b.SlotStats(s), "slot %d: two calls differ" % s           # (floats compared as values of identical bits: no NaN here)
        assert np.float64(got["avg_dist"]).tobytes() == np.float64(b.SlotStats(s)["avg_dist"]).tobytes()
        m = slots == s
        ep = int(st["num_episodes"][m].sum())
        assert (got["n_envs"], got["episodes"], got["cycles"], got["resets"]) == (int(m.sum()), ep, int(st["num_cycles"][m].sum()), int(st["num_resets"][m].sum())), (s, got)
        want = float((st["avg_dist"][m].astype(np.float64) * st["num_episodes"][m]).sum() / ep) if ep else 0.0
        assert abs(got["avg_dist"] - want) <= 1e-12 * abs(want), (s, got["avg_dist"], want)
        for k in tot:
            tot[k] += got[k]
        dist += got["avg_dist"] * got["episodes"]
    assert (tot["n_envs"], tot["episodes"], tot["cycles"], tot["resets"]) == (b.num_envs, ev["episodes"], ev["cycles"], ev["resets"])
    want = ev["avg_dist"]
    got = dist / tot["episodes"] if tot["episodes"] else 0.0
    assert abs(got - want) <= 1e-12 * abs(want), (got, want)
    return tot


def test_slot_stats(da, om, n=12, frames=45):
    """6. dtrl_slot_stats: the integers are the sums over the slot's envs taken from the EnvState records, avg_dist is within 1e-12 relative (another summation
    order), two calls give identical bytes, and summed over the slots it is dtrl_eval_stats."""
    pols = policies(om, DOG)
    b = slotted(DOG, n, pols, EXPLORE, [e % 3 for e in range(n)], dict(terrain_seed=11))
    for f in range(frames):
        b.Update()
    tot = check_slot_stats(b, 3)
    assert tot["cycles"] > 0 and tot["episodes"] > 0, tot


def refused(da, fn, *words):
    with pytest.raises(da.DtrlError) as ei:
        fn()
    msg = str(ei.value)
    assert "(1)" in msg, msg                                       # DTRL_ERR_ARG
    for w in words:
        assert w in msg, (w, msg)


def test_refusals(da, om, n=4):
    """7. Every refusal is DTRL_ERR_ARG with the reason in the message."""
    p0, p1 = policies(om, DOG)[:2]
    b = batch(DOG, n, policy_mode="external")
    refused(da, lambda: b.CreateSlots(2), "external")
    b = batch("args/sim_dog_args.txt", n)
    refused(da, lambda: b.CreateSlots(2), "policy_net")
    b = batch(DOG, n, terrain_seed=11)
    refused(da, lambda: b.AssignSlots(None, [0] * n), "dtrl_slots_create")       # no slots yet
    refused(da, lambda: b.CreateSlots(0), "n_slots")
    refused(da, lambda: b.CreateSlots(33), "n_slots")
    b.SetPolicy(p0[1], *p0[2:])
    b.UpdateBegin()
    refused(da, lambda: b.CreateSlots(3), "dtrl_step_begin", "dtrl_step_end")
    b.UpdateEnd()
    b.CreateSlots(3)
    b.CreateSlots(3)                                                             # the same count again is accepted
    refused(da, lambda: b.CreateSlots(4), "already", "3")
    b.UpdateBegin()
    refused(da, lambda: b.AssignSlots(None, [0] * n), "dtrl_step_begin")
    refused(da, lambda: b.SlotSetPolicy(1, p1[1], *p1[2:]), "dtrl_step_begin")
    refused(da, lambda: b.SlotAlias(1, 0), "dtrl_step_begin")
    b.UpdateEnd()
    refused(da, lambda: b.SlotSetPolicy(3, p1[1], *p1[2:]), "slot 3", "out of range")
    refused(da, lambda: b.SlotSetExplore(-1, 0, 0, 1, 0), "out of range")
    refused(da, lambda: b.SlotStats(3), "out of range")
    refused(da, lambda: b.AssignSlots(None, [0, 3, 0, 0]), "slot 3", "out of range")
    refused(da, lambda: b.AssignSlots(None, [0, 1, 0, 0]), "slot 1", "empty")
    assert list(b.GetSlots()) == [0] * n                                         # all or nothing
    refused(da, lambda: b.SlotAlias(1, 1), "itself")
    refused(da, lambda: b.SlotAlias(1, 2), "slot 2", "empty")
    refused(da, lambda: b.SlotAlias(0, 1), "slot 0")
    refused(da, lambda: b.SlotSetPolicy(1, p1[1][:-1], *p1[2:]), "weight count")
    b.SlotAlias(1, 0); b.SlotAlias(2, 1)
    refused(da, lambda: b.SlotAlias(1, 2), "itself")                             # ... through another alias
    refused(da, lambda: b.AssignSlots([0, n], [1, 1]), "env id", "out of range")
    refused(da, lambda: b.AssignSlots([-1], [1]), "env id", "out of range")
    refused(da, lambda: b.GetSlots([n]), "out of range")
    b.AssignSlots([1, 3], [1, 2])
    assert list(b.GetSlots()) == [0, 1, 0, 2]
    b.Update()


def test_slot_stats_waits_for_a_frame_in_flight(da, om, n=4):
    """7b. The one asymmetry between slots and variants: between UpdateBegin and UpdateEnd dtrl_slot_stats is not refused -- it waits for the frame and
    answers, every env counted once -- where dtrl_variant_stats is refused (test_model_variants.test_refusals). AssignSlots in the same window is refused."""
    b = slotted(DOG, n, policies(om, DOG)[:2], EXPLORE[:2], [e % 2 for e in range(n)], dict(terrain_seed=11))
    b.UpdateBegin()
    got = [b.SlotStats(s) for s in range(2)]
    refused(da, lambda: b.AssignSlots(None, [0] * n), "dtrl_step_begin")
    b.UpdateEnd()
    assert got[0]["n_envs"] + got[1]["n_envs"] == n, got


def test_batch_without_slots_launches_as_before(da, om, n=6, frames=30):
    """8. A batch that never calls CreateSlots does not enter the slot path: per frame the backend's launch counter advances by the group's one frame launch, plus
    -- on the check build, whose counter sees the 0-step launches too -- one compact reset launch in a frame that ended with a fall. The same batch with three
    slots shows what the counter would have seen on the per-slot path."""
    emul = Scenario is EmulScenario
    pols = policies(om, DOG)
    extra = dict(terrain_seed=11)
    b = single(DOG, n, pols[0], EXPLORE[0], extra)
    bs = slotted(DOG, n, pols, EXPLORE, [e % 3 for e in range(n)], extra)
    b.KernelTimeMs(); bs.KernelTimeMs()
    r0 = X.env_states(b)["num_resets"].sum()
    slot_launches = 0
    for f in range(frames):
        b.Update(); bs.Update()
        r1 = X.env_states(b)["num_resets"].sum()
        assert b.KernelTimeMs()[1] == 1 + (1 if (emul and r1 != r0) else 0), "frame %d" % f
        r0 = r1
        slot_launches += bs.KernelTimeMs()[1]
    assert slot_launches >= (3 * frames if emul else frames)


def test_train_loop_greedy_envs(da, om, n=24, k=6, frames=40):
    """train_loop.train(greedy_envs=k): the last k envs sit in an alias of slot 0 with exploration off -- their tuples carry no exploration flag, the trainer is
    fed the other envs' tuples only, and their statistics come back from SlotStats. (The loop's host logic: lane-loop build only.)"""
    from conftest import _emul_scenario_cls
    from deepterrainrl_amd import train_loop
    seen = []

    class Recording(_emul_scenario_cls()):
        def DrainTuples(self, cap=None):
            out = super().DrainTuples(cap)
            seen.append((out[1].copy(), out[2].copy()))
            return out

    st = train_loop.train(TRAIN, REFDATA, num_envs=n, max_frames=frames, trainer_device="cpu", scenario_cls=Recording, greedy_envs=k,
                          extra_args={"terrain_seed": 3, "trainer_num_init_samples": 100000, "trainer_replay_mem_size": 4096, "init_exp_rate": 0.9, "init_exp_base_rate": 0.5, "trainer_init_input_offset_scale": "false"})
    fl = np.concatenate([f for f, _ in seen]); ids = np.concatenate([i for _, i in seen])
    greedy = ids >= n - k
    assert greedy.sum() > 0 and (~greedy).sum() > 0
    assert np.all(fl[greedy] & 6 == 0), "a greedy env wrote an exploration tuple"
    assert np.any(fl[~greedy] & 6 != 0), "the exploring envs did not explore"
    assert st["tuples"] == int((~greedy).sum()), (st["tuples"], int((~greedy).sum()), int(greedy.sum()))
    assert st["greedy"]["n_envs"] == k and st["greedy"]["cycles"] > 0 and st["greedy"]["falls_k"] >= 0.0
