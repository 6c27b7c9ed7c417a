"""Push schedule (include/dtrl.h dtrl_push_schedule): random external pushes at per-env random times, drawn on the device from a counter stream of (seed, global
env id, the env's own counter) and written into the env's perturbation slot at its frame boundary. The yardsticks are a pure-Python restatement of the stream and
of the rule (push_step), the writer that existed before (dtrl_add_perturb: a batch WITHOUT a schedule that is handed every reported push by hand must run bit for
bit like the scheduled one), the oracle's add_perturb, and a batch that never heard of a schedule. dtrl_add_perturb itself -- now one launch over one row per env
-- is held to one call per row in list order, which is what its sequential loop did.
Runs on the lane-loop check build (the host defaults of Backend::PushSchedule and Backend::PerturbScatter); tests/test_gpu_push_schedule.py points `Scenario` at
the product library (one launch of dtrl_push_schedule per env group and frame, one launch of dtrl_perturb_scatter per dtrl_add_perturb).

An env "fell in a frame" where its reset counter went up over the frame: dtrl_get_flags' fallen bit is computed from the state as it stands, and the boundary's
reset has cleared that by the time the host can look."""
import math
import os

import numpy as np
import pytest

import test_external_policy as X          # env_states / same_record / observe
import test_model_variants as V           # with_variants / write_variants / geometry_doc / refused
import test_policy_slots as P             # slotted / single / policies / drain_into
import test_terrain_ladder as LD          # plain_batch
import test_terrain_sets as T             # MODES, batch, with_policy, assert_envs_equal
from conftest import REFDATA, EmulScenario

Scenario = EmulScenario   # the GPU twin points this (and the helpers' own) at the product class

DOG, TRAIN, SIM = T.DOG, X.TRAIN, "args/sim_dog_args.txt"
M64 = (1 << 64) - 1
PUSH_CONST = 0x9054ED1            # the schedule's own constant (the ladder's is 0x1ADDE2, the redraw's 0x5EDBA77)
STEP = 0xD1342543DE82EF95
L_DOG = 21
# hard pushes: 34 kg of dog under 250 .. 500 N for 0.1 .. 0.25 s goes down often enough for the 40 frames of these tests to see falls after pushes
WAIT, FORCE, DUR, SEED = (1, 3), (250.0, 500.0), (0.1, 0.25), 7


# ---- the stream and the rule, written from their description ----
def tg_mix(x):
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


class PyPush:
    """Record of every env, and the rule at a frame boundary."""
    def __init__(self, n, wait=WAIT, force=FORCE, dur=DUR, seed=SEED, L=L_DOG, base=0, scale=None):
        self.n, self.wait_rng, self.force, self.dur, self.seed, self.L, self.base = n, wait, force, dur, seed & M64, L, base
        self.scale = [1.0] * n if scale is None else [float(s) for s in scale]
        self.wait, self.ctr, self.pushes = [0] * n, [0] * n, [0] * n
        self.last_link, self.last_f, self.last_dur = [-1] * n, [(0.0, 0.0)] * n, [0.0] * n
        self.starts_after_push = 0
        for e in range(n):
            self.start(e)

    def u(self, e):
        key = tg_mix(tg_mix(self.seed) ^ ((PUSH_CONST + self.base + e) & M64))
        bits = tg_mix((key + self.ctr[e] * STEP) & M64)
        self.ctr[e] += 1
        return float(bits >> 11) * 2.0 ** -53

    def draw_wait(self, e):
        lo, hi = self.wait_rng
        return min(lo + int(math.floor(self.u(e) * (hi - lo + 1))), hi)

    def start(self, e):
        if self.scale[e] == 0:
            return
        self.wait[e] = self.draw_wait(e)

    def boundary(self, e, fell):
        """True: env e was pushed in this boundary"""
        if self.scale[e] == 0:
            return False
        if fell:
            self.starts_after_push += self.pushes[e] > 0
            self.start(e)
            return False
        self.wait[e] -= 1
        if self.wait[e] > 0:
            return False
        link = min(int(math.floor(self.u(e) * self.L)), self.L - 1)
        d = []
        for _ in range(3):
            sgn = -1.0 if self.u(e) < 0.5 else 1.0
            d.append(sgn * self.u(e))
        nrm = math.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
        if nrm == 0:
            d[0], nrm = 1.0, 1.0
        mag = self.scale[e] * (self.force[0] + self.u(e) * (self.force[1] - self.force[0]))
        f = (mag * d[0] / nrm, mag * d[1] / nrm)
        dur = self.dur[0] + self.u(e) * (self.dur[1] - self.dur[0])
        self.last_link[e], self.last_f[e], self.last_dur[e] = link, f, dur
        self.pushes[e] += 1
        self.wait[e] = self.draw_wait(e)
        return True


def resets(b):
    return np.asarray(b.CycleInfo()[1]).copy()


def check_equals_rule(b, rule, what, envs=None):
    info = b.PushInfo(envs)
    envs = range(rule.n) if envs is None else envs
    assert list(info["wait"]) == [rule.wait[e] for e in envs], (what, info["wait"], rule.wait)
    assert list(info["pushes"]) == [rule.pushes[e] for e in envs], (what, info["pushes"], rule.pushes)
    assert list(info["last_link"]) == [rule.last_link[e] for e in envs], (what, info["last_link"], rule.last_link)
    # the four doubles, exactly: every operation of the rule is one correctly rounded double operation on both sides
    assert info["last_force"].tobytes() == np.array([rule.last_f[e] for e in envs], np.float64).tobytes(), (what, info["last_force"], rule.last_f)
    assert info["last_dur"].tobytes() == np.array([rule.last_dur[e] for e in envs], np.float64).tobytes(), (what, info["last_dur"], rule.last_dur)


def push_batch(om, n, mode, schedule=True, scale=None, terrain_seed=31, seed=SEED, wait=WAIT, **more):
    """n dogs, xavier policy under T.EXPLORE, the schedule turned on"""
    b = T.with_policy(om, DOG, n, dict(terrain_seed=terrain_seed, rand_seed=3, **mode, **more))
    if scale is not None:
        b.PushScale(scale)
    if schedule:
        b.PushSchedule(wait, seed=seed, force=FORCE, duration=DUR)
    return b


def step_with_rule(b, rule):
    """One frame of b; the rule at every env's boundary. Returns (fell, pushed) per env."""
    r0 = resets(b)
    b.Update()
    fell = resets(b) > r0
    pushed = np.array([rule.boundary(e, bool(fell[e])) for e in range(rule.n)])
    return fell, pushed


# ---- 1. records equal the rule ----
@pytest.mark.parametrize("mode", T.MODES, ids=T.MODE_IDS)
def test_records_equal_the_rule(da, om, mode, n=12, frames=40, **more):
    b = push_batch(om, n, mode, **more)
    rule = PyPush(n, base=int(more.get("global_env_offset", 0)))
    check_equals_rule(b, rule, "at creation")
    assert all(WAIT[0] <= w <= WAIT[1] for w in rule.wait) and rule.ctr == [1] * n
    falls = 0
    for f in range(frames):
        p0 = list(rule.pushes)
        fell, pushed = step_with_rule(b, rule)
        check_equals_rule(b, rule, "frame %d" % f)
        falls += int(fell.sum())
        for e in range(n):   # no push at an episode start
            assert not (fell[e] and rule.pushes[e] != p0[e]), (f, e)
    got = dict(pushes=sum(rule.pushes), fewest=min(rule.pushes), falls=falls, starts_after_push=rule.starts_after_push, links=len(set(rule.last_link)))
    print(got)
    # wait <= 3: every env is pushed at least every third boundary it does not fall in
    assert min(rule.pushes) >= 5 and falls >= 1 and rule.starts_after_push >= 1 and len(set(rule.last_link)) >= 4, got
    st = X.env_states(b)
    assert all(0 <= l < L_DOG for l in rule.last_link)
    assert all(math.hypot(*f) <= FORCE[1] * (1 + 1e-12) for f in rule.last_f)   # (x and y of a 3-vector of at most that length)
    assert np.isfinite(st["q"]).all()


# ---- 2. replay: the schedule's writer against dtrl_add_perturb and the frame kernels ----
def dynamic_state(b):
    q, qd = b.PoseVel()
    cnt, rid, lam = b.ContactCache()
    return [q, qd, cnt, rid, lam] + list(b.Ctrl())


@pytest.mark.parametrize("mode", T.MODES, ids=T.MODE_IDS)
def test_replay_through_add_perturb(da, om, mode, n=12, frames=40):
    """Batch A runs under a schedule; batch B, same seeds, without one: after each frame B is handed every push A reports, through dtrl_add_perturb. Pose, velocity,
    contact cache, controller state, the whole EnvState record and the drained tuples are bit-identical, through falls. (pert_lp is left out of the record
    comparison: AddPerturb rotates a zero offset and may store -0.0 where the schedule stores 0.0; both are the same offset to every reader.)"""
    extra = dict(terrain_seed=74, rand_seed=2, **mode)
    pol = T.policy_for(om, TRAIN)

    def make():
        b = T.batch(TRAIN, n, **extra)
        b.SetPolicy(pol[1], *pol[2:]); b.SetExplore(*T.EXPLORE)
        return b
    a, b = make(), make()
    a.PushSchedule(WAIT, seed=SEED, force=FORCE, duration=DUR)
    ta, tb = {e: [] for e in range(n)}, {e: [] for e in range(n)}
    p0, r0, replayed = np.zeros(n, np.int32), resets(a), 0
    for f in range(frames):
        a.Update(); b.Update()
        P.drain_into(a, ta); P.drain_into(b, tb)
        info = a.PushInfo()
        rose = np.nonzero(info["pushes"] > p0)[0].astype(np.int32)
        p0 = info["pushes"].copy()
        if len(rose):
            b.AddPerturb(info["last_link"][rose], info["last_force"][rose], info["last_dur"][rose], env_ids=rose)
            replayed += len(rose)
        for x, y, name in zip(dynamic_state(a), dynamic_state(b), ("q", "qd", "cache count", "cache ids", "cache lambda", "state", "phase", "action", "params", "targets")):
            assert x.tobytes() == y.tobytes(), "frame %d: %s differs" % (f, name)
        sa, sb = X.env_states(a), X.env_states(b)
        for e in range(n):
            bad = X.same_record(sa[e], sb[e], skip=("pert_lp",))
            assert bad is None, "frame %d env %d: EnvState.%s differs" % (f, e, bad)
            assert np.array_equal(sa["pert_lp"][e], sb["pert_lp"][e]), (f, e)   # (equal as numbers)
    assert ta == tb, "the drained tuples differ"
    falls = int((resets(a) - r0).sum())
    print(dict(replayed=replayed, falls=falls, tuples=sum(len(v) for v in ta.values())))
    assert replayed >= n and falls >= 1 and sum(len(v) for v in ta.values()) >= 1


# ---- 3. against the oracle ----
def test_scheduled_push_vs_oracle(da, om):
    """One scheduled push on a product env against an oracle env given add_perturb with the push as reported; tolerance and horizon of
    tests/test_host_and_emul.py::test_perturbation_force_vs_oracle. Env 0 is held out (scale 0) and follows the unpushed oracle."""
    m, _ = om.build_model(SIM, REFDATA)
    e, e0 = om.OracleEnv(m, terrain_seed=5), om.OracleEnv(m, terrain_seed=5)
    b = T.batch(SIM, 2, terrain_seed=5)
    b.PushScale([0.0], env_ids=[0])
    b.PushSchedule((1, 1), seed=3, force=(60.0, 90.0), duration=(0.04, 0.06))
    b.StepUpdates(30); e.step(30); e0.step(30)      # the boundary behind these env-steps pushes env 1
    info = b.PushInfo()
    assert list(info["pushes"]) == [0, 1] and info["last_link"][0] == -1
    b.PushSchedule((1, 0))                           # one push only
    link, force, dur = int(info["last_link"][1]), tuple(info["last_force"][1]), float(info["last_dur"][1])
    assert 0 <= link < L_DOG and 0.04 <= dur <= 0.06 and 0 < math.hypot(*force) <= 90.0
    e.add_perturb(link, (0.0, 0.0), force, dur)
    for k in range(80):
        b.StepUpdates(1); e.step(1); e0.step(1)
        q, qd = b.PoseVel(); qo, qdo = e.pose_vel(); qu, _ = e0.pose_vel()
        assert np.abs(q[1] - qo).max() < 1e-9 and np.abs(qd[1] - qdo).max() < 1e-7, k
        assert np.abs(q[0] - qu).max() < 1e-9
    assert np.abs(q[1] - qu).max() > 1e-4, np.abs(q[1] - qu).max()    # and the push did something
    assert list(b.PushInfo()["pushes"]) == [0, 1]                     # the removed schedule pushed no more


# ---- 4. scale 0, and scale as a factor ----
@pytest.mark.parametrize("mode", T.MODES, ids=T.MODE_IDS)
def test_held_out_envs_equal_a_batch_without_schedule(da, om, mode, n=12, frames=40):
    scale = [0.0 if e % 2 == 0 else 1.0 for e in range(n)]
    a = push_batch(om, n, mode, scale=scale)
    ref = push_batch(om, n, mode, schedule=False)
    out, inn = [e for e in range(n) if e % 2 == 0], [e for e in range(n) if e % 2]
    r0 = resets(a)
    for f in range(frames):
        a.Update(); ref.Update()
        T.assert_envs_equal(a, ref, out, "frame %d" % f)
        info = a.PushInfo(out)
        assert not info["wait"].any() and not info["pushes"].any() and (info["last_link"] == -1).all() and not info["last_force"].any(), (f, info)
    sa, sr = X.env_states(a), X.env_states(ref)
    assert all(sa["q"][e].tobytes() != sr["q"][e].tobytes() for e in inn), "a pushed env ran like its unpushed twin"
    assert a.PushInfo(inn)["pushes"].min() >= 5
    assert (resets(a) - r0)[out].sum() >= 0 and (resets(a) - r0).sum() >= 1


def test_scale_multiplies_the_force_and_nothing_else(da, om, n=3):
    """Env e of two batches is at the same stream position: the batch with scales (2, 0.5, 3) reports the forces of the batch with scale 1 times its scale -- exactly
    for the powers of two, within one rounding of the product (2 ulp) for 3 -- and the same link, duration and wait."""
    one, two = T.batch(SIM, n, terrain_seed=5), T.batch(SIM, n, terrain_seed=5)
    factors = np.array([2.0, 0.5, 3.0])
    two.PushScale(factors)
    for b in (one, two):
        b.PushSchedule((1, 1), seed=11, force=(50.0, 100.0), duration=(0.1, 0.5))
        b.StepUpdates(2)
    i1, i2 = one.PushInfo(), two.PushInfo()
    assert list(i1["pushes"]) == [1] * n == list(i2["pushes"])
    for key in ("wait", "last_link", "last_dur"):
        assert i1[key].tobytes() == i2[key].tobytes(), key
    want = i1["last_force"] * factors[:, None]
    assert np.array_equal(i2["last_force"][:2], want[:2]), (i2["last_force"], want)
    assert np.abs(i2["last_force"][2] - want[2]).max() <= 2 * np.spacing(np.abs(want[2]).max())
    s1, s2 = X.env_states(one), X.env_states(two)
    assert np.array_equal(s2["pert_f"][:2], s1["pert_f"][:2] * factors[:2, None]) and np.array_equal(s1["pert_dur"], s2["pert_dur"])
    assert np.array_equal(s1["pert_link"], i1["last_link"])


# ---- 5. resets, removal, batch state, shards ----
@pytest.mark.parametrize("mode", T.MODES, ids=T.MODE_IDS)
def test_batch_state_resets_and_removal(da, om, mode, n=12, frames=12):
    b = push_batch(om, n, mode)
    rule = PyPush(n)
    for _ in range(frames):
        step_with_rule(b, rule)
    check_equals_rule(b, rule, "after %d frames" % frames)
    # snapshots, restores and clones leave the records alone and carry the slot
    b.AddPerturb(3, (10.0, 5.0), 9.0, env_ids=[0])          # a long push, in flight on env 0 whatever the schedule does next
    snap = b.SaveState()
    slot0 = {k: X.env_states(b)[k][0].copy() for k in ("pert_link", "pert_f", "pert_dur", "pert_time")}
    for _ in range(4):
        step_with_rule(b, rule)
    b.RestoreState(snap); snap.free()
    check_equals_rule(b, rule, "after RestoreState")
    st = X.env_states(b)
    assert all(st[k][0].tobytes() == v.tobytes() for k, v in slot0.items()), "the restore did not bring the slot back"
    b.CloneEnvs([0], [5])
    check_equals_rule(b, rule, "after CloneEnvs")
    st = X.env_states(b)
    assert all(st[k][5].tobytes() == st[k][0].tobytes() for k in slot0), "the clone did not carry the slot"
    # dtrl_reset: a new wait once per env, however often it is listed; the reset clears the slot
    b.Reset([2, 2, 5, 2])
    rule.start(2); rule.start(5)
    check_equals_rule(b, rule, "after Reset([2, 2, 5, 2])")
    assert X.env_states(b)["pert_link"][5] == -1
    b.Reset()
    for e in range(n):
        rule.start(e)
    check_equals_rule(b, rule, "after Reset()")
    # a terrain restart starts the listed envs over
    b.CreateTerrains(2)
    b.SetTerrainFile(1, T.FLAT)
    b.AssignTerrains([0, 1, 4, 1], [1, 1, 1, 1], restart=True)
    for e in (0, 1, 4):
        rule.start(e)
    check_equals_rule(b, rule, "after AssignTerrains(restart=True)")
    for _ in range(4):
        step_with_rule(b, rule)
    check_equals_rule(b, rule, "frames after the restart")
    # removal keeps records and counters; the batch then runs without pushes; back on, the counters go on
    b.PushSchedule((1, 0))
    kept = b.PushInfo()
    for _ in range(4):
        b.Update()
    after = b.PushInfo()
    assert all(kept[k].tobytes() == after[k].tobytes() for k in kept), "a removed schedule moved a record"
    b.PushSchedule(WAIT, seed=SEED, force=FORCE, duration=DUR)
    for e in range(n):
        rule.start(e)
    check_equals_rule(b, rule, "schedule back on")
    for _ in range(4):
        step_with_rule(b, rule)
    check_equals_rule(b, rule, "frames after the schedule came back")


@pytest.mark.parametrize("mode", T.MODES, ids=T.MODE_IDS)
def test_shard_invariance(da, om, mode, n=8, frames=30):
    """8 envs in one batch against two batches of 4, the second with the global-id offset the sharding glue passes at creation."""
    whole, lo, hi = push_batch(om, n, mode), push_batch(om, 4, mode), push_batch(om, 4, mode, global_env_offset=4)
    for _ in range(frames):
        for b in (whole, lo, hi):
            b.Update()
    iw, il, ih = whole.PushInfo(), lo.PushInfo(), hi.PushInfo()
    for key in iw:
        assert iw[key].tobytes() == il[key].tobytes() + ih[key].tobytes(), key
    assert il["pushes"].min() >= 3 and ih["pushes"].min() >= 3
    ow, ol, oh = X.observe(whole, range(n)), X.observe(lo, range(4)), X.observe(hi, range(4))
    for g in range(n):
        (sa, pa, ga), (sb, pb, gb) = ow[g], (ol[g] if g < 4 else oh[g - 4])
        bad = X.same_record(sa, sb)
        assert bad is None, "global env %d: EnvState.%s differs between the shard and the whole batch" % (g, bad)
        assert pa.tobytes() == pb.tobytes() and ga == gb, g


# ---- 6. combinations ----
def end_of(b):
    info = b.PushInfo()
    return X.env_states(b), b.RecordPoliState(), [X.ground_key(b, e) for e in range(b.num_envs)], {k: v.tobytes() for k, v in info.items()}, info


def assert_same_end(x, y, what):
    for e in range(len(x[0])):
        bad = X.same_record(x[0][e], y[0][e])
        assert bad is None, "%s: env %d: EnvState.%s differs" % (what, e, bad)
    assert x[1].tobytes() == y[1].tobytes(), "%s: policy states differ" % what
    assert x[2] == y[2], "%s: ground windows / build counts differ" % what
    assert x[3] == y[3], "%s: push records differ" % what


@pytest.mark.parametrize("mode", T.MODES, ids=T.MODE_IDS)
def test_with_policy_slots(da, om, mode, n=12, frames=30):
    """Three slots under a schedule: every env equals its single-policy run under the same schedule (the push stream depends on the global env id alone)."""
    extra = dict(terrain_seed=11, **mode)
    pols = P.policies(om, DOG)
    assign = [e % 3 for e in range(n)]
    bs = P.slotted(DOG, n, pols, P.EXPLORE, assign, extra)
    refs = [P.single(DOG, n, pols[s], P.EXPLORE[s], extra) for s in range(3)]
    for b in [bs] + refs:
        b.PushSchedule(WAIT, seed=SEED, force=FORCE, duration=DUR)
    for f in range(frames):
        bs.Update()
        for s in range(3):
            refs[s].Update()
    for s in range(3):
        envs = [e for e in range(n) if assign[e] == s]
        P.assert_envs_equal(bs, refs[s], envs, "slot %d" % s)
        ia, ib = bs.PushInfo(envs), refs[s].PushInfo(envs)
        assert all(ia[k].tobytes() == ib[k].tobytes() for k in ia), s
    assert bs.PushInfo()["pushes"].min() >= 3 and X.env_states(bs)["num_resets"].sum() >= 1


def run_with_variants_and_redraw(om, tmp_path, mode, n=12, frames=30):
    paths = V.write_variants(tmp_path, DOG)
    b = V.with_variants(om, DOG, n, paths, [e % 3 for e in range(n)], dict(terrain_seed=31, rand_seed=3, **mode))
    b.VariantRedraw(0, 2, seed=5)
    b.PushSchedule(WAIT, seed=SEED, force=FORCE, duration=DUR)
    rule = PyPush(n)
    for f in range(frames):
        step_with_rule(b, rule)
    check_equals_rule(b, rule, "variants + redraw")
    return end_of(b) + (b.VariantRedrawInfo(),)


@pytest.mark.parametrize("mode", T.MODES, ids=T.MODE_IDS)
def test_with_model_variants_and_redraw(da, om, tmp_path, mode):
    """Variants, their redraw and the schedule in one batch: the records equal the rule, falls redraw variants, and a second run gives the same bits."""
    x, y = run_with_variants_and_redraw(om, tmp_path, mode), run_with_variants_and_redraw(om, tmp_path, mode)
    assert_same_end(x, y, "run after run")
    assert x[5]["draws"].sum() >= 1 and list(x[5]["variant"]) == list(y[5]["variant"]), x[5]


def run_with_ladder(om, mode, n=12, frames=30):
    b = LD.plain_batch(om, n, mode)
    b.AssignTerrains(None, [e % 3 for e in range(n)], restart=True)
    b.TerrainLadder(0, 2, up_dist=2.0, down_dist=1.5)
    b.PushSchedule(WAIT, seed=SEED, force=FORCE, duration=DUR)
    rule = PyPush(n)
    for f in range(frames):
        step_with_rule(b, rule)
    check_equals_rule(b, rule, "ladder")
    return end_of(b) + (list(b.GetTerrains()),)


@pytest.mark.parametrize("mode", T.MODES, ids=T.MODE_IDS)
def test_with_terrain_ladder(da, om, mode):
    x, y = run_with_ladder(om, mode), run_with_ladder(om, mode)
    assert_same_end(x, y, "run after run")
    assert x[5] == y[5]


# ---- 7. refusals ----
def test_refusals(da, om, n=4):
    """Every refusal is DTRL_ERR_ARG, names its cause and changes nothing."""
    nan, inf = float("nan"), float("inf")
    b = T.with_policy(om, DOG, n, dict(terrain_seed=11))
    V.refused(da, lambda: b.PushInfo(), "no push schedule")
    V.refused(da, lambda: b.PushSchedule((0, 3)), "min_wait", "at least 1")
    V.refused(da, lambda: b.PushSchedule((-2, 3)), "min_wait", "at least 1")
    V.refused(da, lambda: b.PushSchedule((1, 3), force=(-1.0, 5.0)), "min_force", "non-negative")
    V.refused(da, lambda: b.PushSchedule((1, 3), force=(1.0, inf)), "max_force", "finite")
    V.refused(da, lambda: b.PushSchedule((1, 3), duration=(-0.1, 0.2)), "min_dur", "non-negative")
    V.refused(da, lambda: b.PushSchedule((1, 3), duration=(0.1, inf)), "max_dur", "finite")
    V.refused(da, lambda: b.PushSchedule((1, 3), force=(9.0, 5.0)), "min_force exceeds max_force")
    V.refused(da, lambda: b.PushSchedule((1, 3), duration=(0.3, 0.2)), "min_dur exceeds max_dur")
    V.refused(da, lambda: b.PushInfo(), "no push schedule")            # none of the refused calls turned it on
    V.refused(da, lambda: b.PushScale([1.0, -1.0], env_ids=[0, 1]), "scale", "non-negative")
    V.refused(da, lambda: b.PushScale([nan], env_ids=[0]), "scale", "finite")
    V.refused(da, lambda: b.PushScale([inf], env_ids=[0]), "scale", "finite")
    V.refused(da, lambda: b.PushScale([1.0], env_ids=[n]), "out of range")
    V.refused(da, lambda: b.PushInfo(), "no push schedule")            # all or nothing: the refused scales allocated nothing
    b.UpdateBegin()
    V.refused(da, lambda: b.PushSchedule((1, 3)), "dtrl_push_schedule", "frame is in flight")
    V.refused(da, lambda: b.PushScale([1.0], env_ids=[0]), "dtrl_push_scale", "frame is in flight")
    b.UpdateEnd()
    b.PushSchedule((2, 2), seed=3)                                      # NaN ranges: the batch's -min_perturb= ... arguments (50 .. 100 N, 0.1 .. 0.5 s)
    V.refused(da, lambda: b.PushSchedule((1, 3), force=(9.0, 5.0)), "min_force exceeds max_force")   # a refused replacement leaves the schedule in place
    assert list(b.PushInfo()["wait"]) == [2] * n
    b.Update(); b.Update()
    info = b.PushInfo()
    assert list(info["pushes"]) == [1] * n, info
    assert all(0.1 <= d <= 0.5 for d in info["last_dur"]) and all(math.hypot(*f) <= 100.0 for f in info["last_force"])
    V.refused(da, lambda: b.PushInfo([n]), "out of range")
    b.UpdateBegin()
    V.refused(da, lambda: b.PushInfo(), "dtrl_push_info", "frame is in flight")
    b.UpdateEnd()
    x = X.batch(da, DOG, n, terrain_seed=11, policy_mode="external")
    V.refused(da, lambda: x.PushSchedule((1, 3)), "policy_mode= external", "not frames")


# ---- 8. dtrl_add_perturb in one launch ----
def perturb_rows(n, rows, seed=4):
    rng = np.random.RandomState(seed)
    env = rng.randint(0, n, size=rows).astype(np.int32)
    env[[5, 40, rows - 1]] = 17                              # one env named three times: its last row wins
    link = rng.randint(0, L_DOG, size=rows).astype(np.int32)
    force = rng.uniform(-80, 80, size=(rows, 2)); lp = rng.uniform(-0.1, 0.1, size=(rows, 2)); dur = rng.uniform(0.0, 0.4, size=rows)
    return env, link, force, lp, dur


def perturb_batch(om, tmp_path, n):
    paths = V.write_variants(tmp_path, DOG) + [V.write_doc(tmp_path, "geom.txt", V.geometry_doc())]
    b = V.with_variants(om, DOG, n, paths, [e % 4 for e in range(n)], dict(terrain_seed=11))
    b.Update()
    return b


def test_add_perturb_equals_row_by_row(da, om, tmp_path, n=70, rows=110):
    """70 envs over four variants (one with another root body angle), 110 random rows with offsets, env 17 named three times: one call with all rows leaves every
    env's record as one call per row in list order does -- what the sequential loop of the call did before it became a launch. The last row wins."""
    env, link, force, lp, dur = perturb_rows(n, rows)
    a, b = perturb_batch(om, tmp_path, n), perturb_batch(om, tmp_path, n)
    a.AddPerturb(link, force, dur, local_pos=lp, env_ids=env)
    for i in range(rows):
        b.AddPerturb(link[i:i + 1], force[i:i + 1], dur[i:i + 1], local_pos=lp[i:i + 1], env_ids=env[i:i + 1])
    sa, sb = X.env_states(a), X.env_states(b)
    for e in range(n):
        bad = X.same_record(sa[e], sb[e])
        assert bad is None, "env %d: EnvState.%s differs" % (e, bad)
    assert sa["pert_link"][17] == link[rows - 1] and sa["pert_dur"][17] == dur[rows - 1] and np.array_equal(sa["pert_f"][17], force[rows - 1])
    touched = sorted(set(env.tolist()))
    assert all(sa["pert_link"][e] == (link[np.nonzero(env == e)[0][-1]] if e in touched else -1) for e in range(n))
    assert len(touched) >= 40 and (sa["pert_lp"][touched] != 0).any()
    # a bad row stops the list where the loop stopped: the rows in front of it are applied
    c = perturb_batch(om, tmp_path, 4)
    with pytest.raises(da.DtrlError):
        c.AddPerturb([1, 99, 2], [(1.0, 0.0)] * 3, [0.5] * 3, env_ids=[0, 1, 2])
    assert list(X.env_states(c)["pert_link"]) == [1, -1, -1, -1]


def test_apply_rand_force_goes_through_the_launch(da, om, n=6):
    """dtrl_apply_rand_force is unchanged: what it draws reaches the slots through the same call."""
    b = T.batch(SIM, n, terrain_seed=2, min_perturb=200, max_perturb=300, min_pertrub_duration=0.05, max_perturb_duration=0.1)
    b.ApplyRandForce(11)
    st = X.env_states(b)
    mag = np.hypot(st["pert_f"][:, 0], st["pert_f"][:, 1])
    assert (st["pert_link"] >= 0).all() and (mag <= 300.0).all() and (mag > 0).all() and ((st["pert_dur"] >= 0.05) & (st["pert_dur"] <= 0.1)).all()
    assert not st["pert_lp"].any() and not st["pert_time"].any()


# ---- 9. the training loop ----
def run_train_loop_with_pushes(max_iters, max_frames, **more):
    from deepterrainrl_amd import train_loop
    extra = {"terrain_seed": 3, "trainer_num_init_samples": 30, "trainer_replay_mem_size": 512, "trainer_freeze_target_iters": 4,
             "init_exp_rate": 0.3, "init_exp_base_rate": 0.1, "trainer_init_input_offset_scale": "false"}
    kw = dict(num_envs=32, seed=1, scenario_cls=Scenario, trainer="hip", extra_args=extra, max_iters=max_iters, max_frames=max_frames, **more)
    out = train_loop.train(TRAIN, REFDATA, pushes=dict(wait=(2, 5), force=(100.0, 200.0), duration=(0.05, 0.1), seed=4, hold_out=[0, 3]), greedy_envs=4, **kw)
    info = out["pushes"]
    print(dict(frames=out["frames"], iters=out["iters"], pushes=int(info["pushes"].sum())))
    assert info["hold_out"] == [0, 3, 28, 29, 30, 31], info["hold_out"]          # the listed envs and the greedy ones
    assert not info["pushes"][info["hold_out"]].any() and info["pushes"][[1, 2, 4, 27]].min() >= 2, info["pushes"]
    assert np.all(np.isfinite(out["weights"]))
    with pytest.raises(ValueError, match="unknown keys"):
        train_loop.train(TRAIN, REFDATA, pushes=dict(wait=(2, 5), every=3), **kw)
    return out, kw


def test_train_loop_with_pushes(da, om):
    lib = os.path.join(os.path.dirname(__file__), "emul", "libdtrl_trainer_emul.so")
    out, kw = run_train_loop_with_pushes(None, 30, trainer_device="cpu", trainer_lib=lib)
    assert out["frames"] >= 30
    from deepterrainrl_amd import train_loop
    kw = dict(kw, max_frames=12)
    x, y = train_loop.train(TRAIN, REFDATA, pushes=None, **kw), train_loop.train(TRAIN, REFDATA, **kw)
    assert "pushes" not in x and x["weights"].tobytes() == y["weights"].tobytes() and x["tuples"] == y["tuples"]


# ---- 10. the tool ----
def test_push_robustness_tool(da, om, n=2, frames=40):
    """tools/push_robustness.py's sweep(): three magnitudes in one batch -- the unpushed cell gets no push, the others do, and every cell reports its envs."""
    import sys
    from conftest import REPO, trained_policy
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import push_robustness
    scn = Scenario if not T.is_emul() else (lambda *a, **k: EmulScenario(*a, **k))
    pol = trained_policy(om, "dog")
    res = push_robustness.sweep("dog", [0.0, 1.0, 4.0], n, frames, 777001, REFDATA, 100.0, (3, 6), (0.1, 0.3), scenario=scn, policy=(pol[1], tuple(pol[2:])))
    assert [s for s, _ in res] == [0.0, 1.0, 4.0] and all(r["n_envs"] == n for _, r in res)
    assert res[0][1]["pushes"] == 0 and res[0][1]["force"] == 0.0
    assert all(r["pushes"] >= n and r["force"] == s * 100.0 for s, r in res[1:]), res      # (a wait of at most 6 boundaries, 40 frames)
