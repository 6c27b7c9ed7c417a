"""Episode limits (include/dtrl.h dtrl_episode_limit): an env's episode ends after a per-episode drawn number of frame boundaries or at a distance, as if the env
had fallen, by a rule that runs on the device in front of every other frame-boundary rule. The yardsticks are a pure-Python restatement of the draw and of the
rule (episode_limit_step), a twin batch WITHOUT a limit that is handed every truncation through dtrl_reset (it must run bit for bit like the limited one), the
batch that never heard of a limit, and the records of the rules behind it (ladder, redraw, rescale, push schedule). Every comparison is for equal bits.
70 envs throughout: two 64-thread blocks with the second partial, and a split into two env groups at a non-zero e0.
Runs on the lane-loop check build (the host default of Backend::EpisodeLimit); tests/test_gpu_episode_limit.py points `Scenario` at the product libraries (one
launch of dtrl_episode_limit per env group and frame).

An env "fell in a frame" of the exp scenario where a drained tuple of that frame carries DTRL_TUPLE_FAIL for it: a truncation records no tuple."""
import math

import numpy as np
import pytest

import test_external_policy as X          # env_states / same_record / observe
import test_model_variants as V           # with_variants / write_variants / refused
import test_push_schedule as R            # tg_mix, PyPush
import test_terrain_sets as T             # MODES, batch, with_policy, assert_envs_equal

DOG, SIM = T.DOG, "args/sim_dog_args.txt"
M64 = (1 << 64) - 1
EPISODE_CONST = 0xE9150DE          # the limit's own constant (ladder 0x1ADDE2, redraw 0x5EDBA77, rescale 0x5CA1ED, push 0x9054ED1)
STEP = 0xD1342543DE82EF95
N, LIMITS, SEED = 70, (4, 9), 5
PRECISIONS = [dict(), dict(physics_precision="f32")]
PRECISION_IDS = ["f64", "f32"]
INFO_INTS = ("frames", "limit", "by_fall", "by_limit", "last_frames", "last_cause")


# ---- the draw and the rule, written from their description ----
class PyEpisode:
    """Record of every env, and the rule at a frame boundary. last_dist[e] is None where the test could not see the root x the episode ended at."""
    def __init__(self, n, frames=LIMITS, dist=None, seed=SEED, spawn_x=0.0, base=0, on=None, start=True):
        self.n, self.spawn_x, self.base = n, spawn_x, base
        self.on = [1] * n if on is None else list(on)
        self.frames, self.limit, self.draws = [0] * n, [0] * n, [0] * n
        self.last_frames, self.last_cause, self.by_fall, self.by_limit = [0] * n, [0] * n, [0] * n, [0] * n
        self.last_dist = [0.0] * n
        self.settings(frames, dist, seed, start)

    def settings(self, frames, dist, seed, start=True):
        self.rng, self.max_dist, self.seed = (0, 0) if frames is None else frames, math.inf if dist is None else dist, seed & M64
        if start:
            for e in range(self.n):
                self.start(e)

    def draw(self, e):
        lo, hi = self.rng
        if hi == 0:
            self.limit[e] = 0
            return
        key = R.tg_mix(R.tg_mix(self.seed) ^ ((EPISODE_CONST + self.base + e) & M64))
        bits = R.tg_mix((key + self.draws[e] * STEP) & M64)
        self.draws[e] += 1
        u = float(bits >> 11) * 2.0 ** -53
        self.limit[e] = min(lo + int(math.floor(u * (hi - lo + 1))), hi)

    def start(self, e):
        if self.on[e]:
            self.frames[e] = 0
            self.draw(e)

    def boundary(self, e, fell, root_x=None):
        """0, or the cause (2 frame limit, 3 distance) for which env e's episode is ended in this boundary"""
        if not self.on[e]:
            return 0
        self.frames[e] += 1
        dist = None if root_x is None else root_x - self.spawn_x
        cause = 0
        if fell:
            cause = 1
        elif self.limit[e] > 0 and self.frames[e] >= self.limit[e]:
            cause = 2
        elif dist is not None and dist >= self.max_dist:
            cause = 3
        if not cause:
            return 0
        if cause == 1:
            self.by_fall[e] += 1
        else:
            self.by_limit[e] += 1
        self.last_frames[e], self.last_dist[e], self.last_cause[e] = self.frames[e], dist, cause
        self.frames[e] = 0
        self.draw(e)
        return 0 if cause == 1 else cause


def check_equals_rule(b, rule, what, envs=None):
    info = b.EpisodeInfo(envs)
    envs = range(rule.n) if envs is None else envs
    for key in INFO_INTS:
        assert list(info[key]) == [getattr(rule, key)[e] for e in envs], (what, key, info[key], getattr(rule, key))
    for i, e in enumerate(envs):   # the double, exactly, where the test saw the root x
        if rule.last_dist[e] is not None:
            assert np.float64(info["last_dist"][i]).tobytes() == np.float64(rule.last_dist[e]).tobytes(), (what, e, info["last_dist"][i], rule.last_dist[e])
    return info


def resets(b):
    return np.asarray(b.CycleInfo()[1]).copy()


def root_x(b):
    return b.PoseVel()[0][:, 0].copy()


def limit_batch(om, n, mode, limit=True, frames=LIMITS, dist=None, seed=SEED, scenario="exp", terrain_seed=31, **more):
    """n dogs on slopes_mixed, xavier policy under T.EXPLORE, in the exp scenario unless told otherwise; the limit turned on"""
    b = T.with_policy(om, DOG, n, dict(terrain_seed=terrain_seed, rand_seed=3, scenario=scenario, **mode, **more))
    if limit:
        b.EpisodeLimit(frames, dist, seed)
    return b


def fails_of(da, b, n, into=None):
    """Drain b's tuples: which envs have one with DTRL_TUPLE_FAIL (into: per-env lists the rows and flags are appended to)"""
    rows, fl, ids = b.DrainTuples()
    fell = np.zeros(n, bool)
    for r, x, e in zip(rows, fl, ids):
        if int(x) & da.TUPLE_FAIL:
            fell[int(e)] = True
        if into is not None:
            into[int(e)].append((r.tobytes(), int(x)))
    return fell


# ---- 1. records equal the rule ----
@pytest.mark.parametrize("prec", PRECISIONS, ids=PRECISION_IDS)
@pytest.mark.parametrize("mode", T.MODES, ids=T.MODE_IDS)
def test_records_equal_the_rule_under_the_net(da, om, mode, prec, n=N, frames=40, **more):
    """Scene A: the exp scenario under the seeded xavier weights, limits 4 .. 9 frames. EpisodeInfo after every frame equals the rule fed with the env's observed
    falls, and the reset counter rises exactly where the env fell or the rule ended its episode.
    Measured on the check build: under these weights the earliest fall of the 70 envs comes 41 frames after a reset (both terrain modes, 60 frames), so under
    limits of at most 9 frames NO episode of this scene ends by a fall, however many frames run: 402 episodes end by the limit, 0 by a fall. The scene is kept as
    it is and asserts the limit's side; test_records_equal_the_rule_with_falls is the same scene under pushes hard enough to bring the dog down inside 9 frames,
    where both endings are asserted."""
    b = limit_batch(om, n, mode, **prec, **more)
    rule = PyEpisode(n, base=int(more.get("global_env_offset", 0)))
    check_equals_rule(b, rule, "at creation")
    assert all(LIMITS[0] <= l <= LIMITS[1] for l in rule.limit) and rule.draws == [1] * n and len(set(rule.limit)) >= 4
    for f in range(frames):
        r0 = resets(b)
        b.Update()
        fell = fails_of(da, b, n)
        ended = np.array([rule.boundary(e, bool(fell[e])) != 0 for e in range(n)])
        for e in range(n):
            rule.last_dist[e] = None if (fell[e] or ended[e]) else rule.last_dist[e]
        assert list(resets(b) - r0) == list((fell | ended).astype(np.int64)), (f, resets(b) - r0, fell, ended)
        info = check_equals_rule(b, rule, "frame %d" % f)
        assert np.isfinite(info["last_dist"]).all()
    got = dict(by_fall=sum(rule.by_fall), by_limit=sum(rule.by_limit), by_fall_hi=sum(rule.by_fall[64:]), by_limit_hi=sum(rule.by_limit[64:]))
    print(got)
    assert got["by_limit"] >= 10 and got["by_limit_hi"] >= 1, got
    assert b.EvalStats()["resets"] == got["by_fall"] + got["by_limit"]


@pytest.mark.parametrize("prec", PRECISIONS, ids=PRECISION_IDS)
@pytest.mark.parametrize("mode", T.MODES, ids=T.MODE_IDS)
def test_fsm_dog_resets_at_exactly_its_drawn_limits(da, om, mode, prec, n=N, frames=30):
    """Scene B: the FSM dog on flat ground does not fall: every env resets at exactly the boundaries its drawn limits name, back to the spawn x."""
    b = T.batch(SIM, n, terrain_seed=5, **mode, **prec)
    spawn = root_x(b)
    assert len(set(spawn.tolist())) == 1
    b.EpisodeLimit(LIMITS, seed=SEED)
    rule = PyEpisode(n, spawn_x=float(spawn[0]))
    for f in range(frames):
        r0, x0 = resets(b), root_x(b)
        b.Update()
        ended = np.array([rule.boundary(e, False) != 0 for e in range(n)])
        for e in range(n):
            if ended[e]:
                rule.last_dist[e] = None
        assert list(resets(b) - r0) == list(ended.astype(np.int64)), f
        x1 = root_x(b)
        assert (x1[ended] == spawn[ended]).all() and (x1[~ended] > x0[~ended]).all(), f
        info = check_equals_rule(b, rule, "frame %d" % f)
        assert (info["last_dist"][ended] > 0).all()
    assert sum(rule.by_fall) == 0 and min(rule.by_limit) >= frames // LIMITS[1] and len(set(rule.last_frames)) >= 4


# ---- 2. a truncation is a reset ----
HARD = (1500.0, 3000.0)


def run_twins(da, om, mode, n=N, frames=30, pushes=None, **more):
    """Batch X under limits; twin Y, same seeds, without: after every frame Y is handed the envs X truncated at that boundary through dtrl_reset, and everything
    of all n envs is compared. An env fell in a frame where Y's reset counter rose by itself (X's rises for truncations too); a FAIL tuple is always such a fall (a
    fall in an episode's warm-up cycle records no tuple). last_dist is the root x Y shows before its reset, minus the spawn x. Returns the rule."""
    if pushes is not None:
        more = dict(more, min_perturb=pushes[0], max_perturb=pushes[1], min_pertrub_duration=0.1, max_perturb_duration=0.25)
    x, y = limit_batch(om, n, mode, **more), limit_batch(om, n, mode, limit=False, **more)
    rule = PyEpisode(n, spawn_x=float(root_x(x)[0]))
    tx, ty = {e: [] for e in range(n)}, {e: [] for e in range(n)}
    for f in range(frames):
        r0 = resets(y)
        if pushes is not None and f % 2 == 0:      # the same random push for an env of X and its twin (dtrl_apply_rand_force: a function of seed and env id)
            x.ApplyRandForce(f); y.ApplyRandForce(f)
        x.Update(); y.Update()
        fell = (resets(y) - r0) > 0
        failed = fails_of(da, x, n, tx)
        assert (fails_of(da, y, n, ty) == failed).all() and not (failed & ~fell).any(), f
        yx = root_x(y)
        ids = [e for e in range(n) if rule.boundary(e, bool(fell[e]), None if fell[e] else float(yx[e])) != 0]
        if ids:
            y.Reset(ids)
        check_equals_rule(x, rule, "frame %d" % f)
        T.assert_envs_equal(x, y, range(n), "frame %d" % f)
        for a, c, name in zip(x.CycleInfo(), y.CycleInfo(), ("cycles", "resets", "cycle COM", "cycle time", "params")):
            assert a.tobytes() == c.tobytes(), "frame %d: CycleInfo %s differs" % (f, name)
        assert tx == ty, "frame %d: the drained tuples differ" % f
    got = dict(by_fall=sum(rule.by_fall), by_limit=sum(rule.by_limit), by_fall_hi=sum(rule.by_fall[64:]), by_limit_hi=sum(rule.by_limit[64:]), tuples=sum(len(v) for v in tx.values()))
    print(got)
    return got


@pytest.mark.parametrize("mode", T.MODES, ids=T.MODE_IDS)
def test_a_truncation_is_a_reset(da, om, mode):
    """The whole EnvState record (pose, velocity, contact cache, counters), the policy state, the ground window, CycleInfo and the drained tuples -- rows and flag
    words -- of all 70 envs are equal bit for bit over the whole run, so no tuple of X carries a begin state from before a truncation (Y's dtrl_reset dropped it)."""
    got = run_twins(da, om, mode)
    assert got["by_limit"] >= N and got["by_limit_hi"] >= 1, got


@pytest.mark.parametrize("prec", PRECISIONS, ids=PRECISION_IDS)
@pytest.mark.parametrize("mode", T.MODES, ids=T.MODE_IDS)
def test_records_equal_the_rule_with_falls(da, om, mode, prec):
    """Scene A with every env pushed by 1500 .. 3000 N every other frame (dtrl_apply_rand_force on both twins), which brings the dog down inside 9 frames: at
    least 10 episodes end by a fall and at least 10 by the limit, some of each in the second 64-thread block; a fall wins over a limit reached in the same frame."""
    got = run_twins(da, om, mode, pushes=HARD, **prec)
    assert got["by_fall"] >= 10 and got["by_limit"] >= 10 and got["by_fall_hi"] >= 1 and got["by_limit_hi"] >= 1, got


# ---- 3. distance limit and poli_eval ----
@pytest.mark.parametrize("mode", T.MODES, ids=T.MODE_IDS)
def test_distance_limit_and_poli_eval(da, om, mode, n=N, frames=45, dist=0.75):
    """poli_eval under the trained net with a distance limit alone: cause 3 at the first boundary with root_x - spawn_x >= max_dist (RootX after the previous frame
    is short of it, after this one the env stands at the spawn x again), and the episode bookkeeping a fall does: an ended episode with num_cycles >= 1 is in the
    distance log once with last_dist and counts in EvalStats; one ended before the env's first cycle is in neither; avg_dist is the running mean of the env's own
    log entries in the library's `real`.
    Measured on the check build: the cycle counter stands at 1 after an env's first env-step and no reset takes it back, so no frame boundary ever sees an env in
    front of its first cycle (467 episodes ended by the distance, 0 of them early): the test keeps the distinction and cannot exercise the early side."""
    b = T.with_policy(om, DOG, n, dict(terrain_seed=31, rand_seed=3, **mode), trained=True)
    spawn = float(root_x(b)[0])
    b.EpisodeLimit(dist=dist, seed=SEED)
    info = b.EpisodeInfo()
    assert not info["limit"].any() and not info["frames"].any()          # no frame limit: nothing drawn
    want = {e: [] for e in range(n)}
    early = cut = 0
    for f in range(frames):
        x0, i0 = root_x(b), b.EpisodeInfo()
        b.Update()
        x1, i1, cycles = root_x(b), b.EpisodeInfo(), b.CycleInfo()[0]
        for e in range(n):
            ended_by = int(i1["by_limit"][e] - i0["by_limit"][e]), int(i1["by_fall"][e] - i0["by_fall"][e])
            assert sum(ended_by) <= 1 and i1["limit"][e] == 0
            if sum(ended_by) == 0:
                assert x1[e] - spawn < dist and i1["frames"][e] == i0["frames"][e] + 1, (f, e)
                continue
            assert x1[e] == spawn and i1["frames"][e] == 0 and i1["last_frames"][e] == i0["frames"][e] + 1, (f, e)
            if ended_by[0]:
                cut += 1
                assert i1["last_cause"][e] == 3 and i1["last_dist"][e] >= dist and x0[e] - spawn < dist, (f, e, i1["last_dist"][e], x0[e])
            else:
                assert i1["last_cause"][e] == 1, (f, e)
            if cycles[e] >= 1:                                            # (the reset leaves the cycle counter alone: this is what frame_end saw)
                want[e].append(float(i1["last_dist"][e]))
            else:
                early += 1
    d, ids = b.GetDistLog()
    got = {e: [] for e in range(n)}
    for v, e in zip(d, ids):
        got[int(e)].append(float(v))
    assert got == want, "the distance log is not the recorded episodes"
    st = X.env_states(b)
    for e in range(n):
        avg = 0.0
        for k, v in enumerate(want[e]):
            avg = (k * avg + v) / (k + 1.0)
        assert st["num_episodes"][e] == len(want[e]) and float(st["avg_dist"][e]) == avg, (e, st["avg_dist"][e], avg)
    logged = sum(len(v) for v in want.values())
    print(dict(cut=cut, early=early, logged=logged))
    assert b.EvalStats()["episodes"] == logged
    assert cut >= n and logged >= n, (cut, early, logged)


# ---- 4. held-out envs ----
@pytest.mark.parametrize("mode", T.MODES, ids=T.MODE_IDS)
def test_held_out_envs_equal_a_batch_without_limit(da, om, mode, n=N, frames=24):
    a, ref = limit_batch(om, n, mode, limit=False), limit_batch(om, n, mode, limit=False)
    out, inn = [e for e in range(n) if e % 3 == 0], [e for e in range(n) if e % 3]
    a.EpisodeLimitEnvs(0, env_ids=out)                                   # before the limit exists
    a.EpisodeLimit(LIMITS, seed=SEED)
    for f in range(frames):
        a.Update(); ref.Update()
        T.assert_envs_equal(a, ref, out, "frame %d" % f)
        info = a.EpisodeInfo(out)
        assert not any(v.any() for v in info.values()), (f, info)
    assert a.EpisodeInfo(inn)["by_limit"].min() >= frames // LIMITS[1]
    sa, sr = X.env_states(a), X.env_states(ref)
    assert all(sa["q"][e].tobytes() != sr["q"][e].tobytes() for e in inn), "a limited env ran like its unlimited twin"


# ---- 5. shard invariance ----
@pytest.mark.parametrize("mode", T.MODES, ids=T.MODE_IDS)
def test_shard_invariance(da, om, mode, n=N, frames=24):
    """Envs 35 .. 69 of a 70-env batch against a 35-env batch created with the global-id offset the sharding glue passes."""
    h = n // 2
    whole, hi = limit_batch(om, n, mode), limit_batch(om, h, mode, global_env_offset=h)
    for _ in range(frames):
        whole.Update(); hi.Update()
    iw, ih = whole.EpisodeInfo(list(range(h, n))), hi.EpisodeInfo()
    for key in iw:
        assert iw[key].tobytes() == ih[key].tobytes(), key
    assert ih["by_limit"].min() >= frames // LIMITS[1]
    ow, oh = X.observe(whole, range(h, n)), X.observe(hi, range(h))
    for g in range(h, n):
        (sa, pa, ga), (sb, pb, gb) = ow[g], oh[g - h]
        bad = X.same_record(sa, sb)
        assert bad is None, "global env %d: EnvState.%s differs between the shard and the whole batch" % (g, bad)
        assert pa.tobytes() == pb.tobytes() and ga == gb, g


# ---- 6. every rule at once ----
RESCALED = [e for e in range(N) if e % 5 == 1]
PUSH_WAIT = (20, 30)


def all_rules_batch(om, tmp_path, mode, n=N):
    """Terrain sets under a ladder, model variants under a redraw, a rescale of every fifth env, a push schedule and the episode limit"""
    paths = V.write_variants(tmp_path, DOG)
    b = V.with_variants(om, DOG, n, paths, [e % 3 for e in range(n)], dict(terrain_seed=31, rand_seed=3, **mode))
    T.fill(b, T.four_walkable_files(DOG))
    b.AssignTerrains(None, [(e // 3) % 3 for e in range(n)], restart=True)
    b.TerrainLadder(0, 2, up_dist=2.0, down_dist=1.5)
    b.VariantRedraw(0, 2, seed=5)
    b.VariantRescale(base=0, env_ids=RESCALED, seed=9, mass=(0.8, 1.2), kp=(0.9, 1.1))
    b.PushSchedule(PUSH_WAIT, seed=R.SEED, force=R.FORCE, duration=R.DUR)
    b.EpisodeLimit(LIMITS, seed=SEED)
    return b


def all_rules_records(b):
    rec = {"terrain": list(b.GetTerrains()), "variant": list(b.GetVariants())}
    for name, info in (("ladder", b.LadderInfo()), ("redraw", b.VariantRedrawInfo()), ("rescale", b.VariantRescaleInfo()), ("push", b.PushInfo()), ("episode", b.EpisodeInfo())):
        rec.update((name + " " + k, v.tobytes()) for k, v in info.items() if hasattr(v, "tobytes"))
    return rec


def run_all_rules(om, tmp_path, mode, n=N, frames=24):
    b = all_rules_batch(om, tmp_path, mode, n)
    spawn = float(root_x(b)[0])
    push = R.PyPush(n, wait=PUSH_WAIT)
    cut = 0
    for f in range(frames):
        r0, e0 = resets(b), b.EpisodeInfo()
        d0, s0 = b.VariantRedrawInfo()["draws"].copy(), b.VariantRescaleInfo()["episodes"].copy()
        b.Update()
        rose, e1 = resets(b) - r0, b.EpisodeInfo()
        ended = (e1["by_limit"] - e0["by_limit"]) > 0
        assert list(rose) == list((e1["by_limit"] - e0["by_limit"]) + (e1["by_fall"] - e0["by_fall"])), f
        d1, s1, mark = b.VariantRedrawInfo()["draws"], b.VariantRescaleInfo()["episodes"], b.LadderInfo()["mark_x"]
        for e in range(n):                                               # for every rule behind the limit, an env it ended is an env whose episode ended
            push.boundary(e, bool(rose[e]))
            if ended[e]:
                cut += 1
                assert mark[e] == spawn, (f, e, mark[e])
                assert (s1[e] - s0[e], d1[e] - d0[e]) == ((1, 0) if e in RESCALED else (0, 1)), (f, e)
        R.check_equals_rule(b, push, "push schedule, frame %d" % f)      # (a truncated env drew a new wait and was not pushed)
    assert cut >= n
    return X.env_states(b), b.RecordPoliState(), [X.ground_key(b, e) for e in range(n)], all_rules_records(b)


def assert_same_run(x, y, what):
    for e in range(len(x[0])):
        bad = X.same_record(x[0][e], y[0][e])
        assert bad is None, "%s: env %d: EnvState.%s differs" % (what, e, bad)
    assert x[1].tobytes() == y[1].tobytes(), "%s: policy states differ" % what
    assert x[2] == y[2], "%s: ground windows / build counts differ" % what
    for k in x[3]:
        assert x[3][k] == y[3][k], "%s: %s differs" % (what, k)


@pytest.mark.parametrize("mode", T.MODES, ids=T.MODE_IDS)
def test_every_rule_at_once(da, om, tmp_path, mode):
    """A truncated env draws a variant or its scales, draws a push wait and has its ladder mark at the spawn x at that boundary."""
    run_all_rules(om, tmp_path, mode)


# ---- 6b. the listed episode starts under every rule at once ----
HELD_OUT = 33


def env_records(rec, e, n=N):
    """env e's part of all_rules_records: a key list, or n equal runs of bytes"""
    return {k: (v[e] if isinstance(v, list) else v[len(v) // n * e:len(v) // n * (e + 1)]) for k, v in rec.items()}


def run_listed_starts(om, tmp_path, mode, n=N):
    """dtrl_reset, dtrl_assign_terrains(restart) and an env coming into the limit, each between frames of a batch under all five rules (8 frames in all):
    every call moves, once, exactly the records of the listed envs that its episode start names; all other records keep their bytes."""
    b = all_rules_batch(om, tmp_path, mode, n)
    spawn = float(root_x(b)[0])
    b.EpisodeLimitEnvs(0, env_ids=[HELD_OUT])                            # (its record stays: one draw, at the limit's creation)
    push, rule = R.PyPush(n, wait=PUSH_WAIT), PyEpisode(n, spawn_x=spawn)
    rule.on[HELD_OUT] = 0

    def frames(k):
        for _ in range(k):
            r0, e0 = resets(b), b.EpisodeInfo()
            b.Update()
            rose, fell = resets(b) - r0, (b.EpisodeInfo()["by_fall"] - e0["by_fall"]) > 0
            for e in range(n):
                push.boundary(e, bool(rose[e]))
                rule.boundary(e, bool(fell[e]))
                rule.last_dist[e] = None
            R.check_equals_rule(b, push, "push schedule, in a frame")
            check_equals_rule(b, rule, "episode limit, in a frame")

    def started(call, listed, moved, draws):
        """One call: `moved` names the record families an episode start of this kind may move; draws: the listed envs draw a variant or their scales"""
        before = all_rules_records(b)
        call()
        after = all_rules_records(b)
        for e in range(n):
            x, y = env_records(before, e), env_records(after, e)
            for k in x:
                if e not in listed or k.split()[0] not in moved:
                    assert x[k] == y[k], ("env %d: %s moved" % (e, k), listed)
        info = {name: get() for name, get in (("redraw", b.VariantRedrawInfo), ("rescale", b.VariantRescaleInfo), ("ladder", b.LadderInfo))}
        was = {name: np.frombuffer(before[name], np.int32) for name in ("redraw draws", "rescale episodes")}
        for e in listed:
            rescaled = e in RESCALED
            assert info["redraw"]["draws"][e] - was["redraw draws"][e] == (1 if draws and not rescaled else 0), e
            assert info["rescale"]["episodes"][e] - was["rescale episodes"][e] == (1 if draws and rescaled else 0), e
            if "ladder" in moved:
                assert info["ladder"]["mark_x"][e] == spawn, (e, info["ladder"]["mark_x"][e])
            if "push" in moved:
                push.start(e)
            rule.start(e)
        R.check_equals_rule(b, push, "push schedule, after the call")     # (once per listed env, however often it is listed; nothing of any other env)
        check_equals_rule(b, rule, "episode limit, after the call")

    frames(3)
    draws = ("variant", "redraw", "rescale", "ladder", "push", "episode")
    started(lambda: b.Reset([2, 2, 65, 2]), (2, 65), draws, True)
    started(lambda: b.Reset([66]), (66,), draws, True)                   # (an env under a private record of the rescale, in the second block)
    frames(2)
    started(lambda: b.AssignTerrains([0, 1, 68, 1], [2, 0, 1, 2], restart=True), (0, 1, 68), ("terrain", "ladder", "push", "episode"), False)
    assert [int(t) for t in b.GetTerrains([0, 1, 68])] == [2, 2, 1]
    frames(2)
    rule.on[HELD_OUT] = 1
    started(lambda: b.EpisodeLimitEnvs([1, 1], env_ids=[HELD_OUT, 8]), (HELD_OUT,), ("episode",), False)   # (env 8 was in: nothing starts)
    frames(1)
    return X.env_states(b), b.RecordPoliState(), [X.ground_key(b, e) for e in range(n)], all_rules_records(b)


@pytest.mark.parametrize("mode", T.MODES, ids=T.MODE_IDS)
def test_listed_starts_under_every_rule(da, om, tmp_path, mode):
    """Each listed episode start moves every rule's records of the listed envs once, in the rule's own way -- a reset draws the variant or the scales, a terrain
    restart does not, an env coming into the limit starts its episode record alone -- and leaves every other env's records byte for byte where they were."""
    run_listed_starts(om, tmp_path, mode)


# ---- 7. batch state and lifecycle ----
@pytest.mark.parametrize("mode", T.MODES, ids=T.MODE_IDS)
def test_batch_state_and_lifecycle(da, om, mode, n=N, frames=8):
    b = limit_batch(om, n, mode)
    rule = PyEpisode(n)

    def run(k):
        for _ in range(k):
            b.Update()
            fell = fails_of(da, b, n)
            for e in range(n):
                rule.boundary(e, bool(fell[e]))
                rule.last_dist[e] = None
    run(frames)
    check_equals_rule(b, rule, "after %d frames" % frames)
    # a snapshot restore leaves the records alone: they stand where the frame behind the snapshot left them
    snap = b.SaveState()
    run(1)
    b.RestoreState(snap); snap.free()
    check_equals_rule(b, rule, "after RestoreState")
    # dtrl_reset: a new record start once per env, however often it is listed
    b.Reset([2, 2, 65, 2])
    rule.start(2); rule.start(65)
    check_equals_rule(b, rule, "after Reset([2, 2, 65, 2])")
    # a terrain restart starts the record
    b.CreateTerrains(2)
    b.SetTerrainFile(1, T.FLAT)
    b.AssignTerrains([0, 1, 68, 1], [1, 1, 1, 1], restart=True)
    for e in (0, 1, 68):
        rule.start(e)
    check_equals_rule(b, rule, "after AssignTerrains(restart=True)")
    run(4)
    check_equals_rule(b, rule, "frames after the restart")
    # replacing the limit keeps the counters and draws new limits
    b.EpisodeLimit((2, 3), seed=SEED + 1)
    rule.settings((2, 3), None, SEED + 1)
    check_equals_rule(b, rule, "limit replaced")
    assert all(2 <= l <= 3 for l in rule.limit) and sum(rule.by_limit) >= n
    run(4)
    check_equals_rule(b, rule, "frames under the new limit")
    # an env that comes in while the limit runs starts a record at that call; one that goes out keeps its record
    b.EpisodeLimitEnvs(0, env_ids=[7, 66])
    rule.on[7] = rule.on[66] = 0
    run(3)
    b.EpisodeLimitEnvs([1, 1, 1], env_ids=[7, 66, 8])                    # (env 8 was in: nothing starts)
    rule.on[7] = rule.on[66] = 1
    rule.start(7); rule.start(66)
    check_equals_rule(b, rule, "envs 7 and 66 back in")
    # removing the limit stops truncations and keeps the counters; the batch then runs like one that never had a limit
    b.EpisodeLimit()
    kept = b.EpisodeInfo()
    twin = limit_batch(om, n, mode, limit=False)
    snap = b.SaveState()
    blob = snap.export(); snap.free()
    s2 = twin.ImportState(blob); twin.RestoreState(s2); s2.free()
    b.DrainTuples(); twin.DrainTuples()
    tb, tt = {e: [] for e in range(n)}, {e: [] for e in range(n)}
    for f in range(10):
        r0 = resets(b)
        b.Update(); twin.Update()
        fell = fails_of(da, b, n, tb); fails_of(da, twin, n, tt)
        assert list(resets(b) - r0) == list(fell.astype(np.int64)), "a removed limit ended an episode"
        T.assert_envs_equal(b, twin, range(n), "frame %d after the removal" % f)
    assert tb == tt
    after = b.EpisodeInfo()
    assert all(kept[k].tobytes() == after[k].tobytes() for k in kept), "a removed limit moved a record"


# ---- 8. refusals ----
def test_refusals(da, om, n=4):
    """Every refusal is DTRL_ERR_ARG, names its cause and changes nothing."""
    nan, inf = float("nan"), float("inf")
    b = T.with_policy(om, DOG, n, dict(terrain_seed=11))
    V.refused(da, lambda: b.EpisodeInfo(), "no episode limit")
    b.EpisodeLimit()                                                      # removing what is not there allocates nothing
    V.refused(da, lambda: b.EpisodeInfo(), "no episode limit")
    b.EpisodeLimit((3, 6), seed=2)
    before = b.EpisodeInfo()

    def unchanged(what):
        after = b.EpisodeInfo()
        assert all(before[k].tobytes() == after[k].tobytes() for k in before), what
    for frames, dist, words in (((-1, 5), None, ("min_frames", "negative")), ((6, 3), None, ("exceeds max_frames",)), ((0, 5), None, ("exactly one",)),
                                ((3, 6), nan, ("NaN",)), (None, nan, ("NaN",))):
        V.refused(da, lambda: b.EpisodeLimit(frames, dist), "dtrl_episode_limit", "nothing changed", *words)
        unchanged((frames, dist))
    V.refused(da, lambda: b.EpisodeLimitEnvs([1, 0], env_ids=[0, n]), "out of range", "nothing changed")
    V.refused(da, lambda: b.EpisodeInfo([n]), "out of range")
    b.Update()
    before = b.EpisodeInfo()
    assert list(before["frames"]) == [1] * n and all(3 <= l <= 6 for l in before["limit"])   # the refused replacements left the limit in place
    b.UpdateBegin()
    V.refused(da, lambda: b.EpisodeLimit((1, 2)), "dtrl_episode_limit", "frame is in flight")
    V.refused(da, lambda: b.EpisodeLimitEnvs(0), "dtrl_episode_limit_envs", "frame is in flight")
    V.refused(da, lambda: b.EpisodeInfo(), "dtrl_episode_info", "frame is in flight")
    b.UpdateEnd()
    after = b.EpisodeInfo()
    assert list(after["frames"]) == [2] * n and after["limit"].tobytes() == before["limit"].tobytes()
    b.EpisodeLimit(dist=-1.0)                                             # no frame limit and a distance <= 0: removed
    b.Update()
    assert list(b.EpisodeInfo()["frames"]) == [2] * n
    x = X.batch(da, DOG, n, terrain_seed=11, policy_mode="external")
    V.refused(da, lambda: x.EpisodeLimit((3, 6)), "policy_mode= external", "ticks")
    V.refused(da, lambda: x.EpisodeInfo(), "no episode limit")


# ---- 9. the training loop ----
def test_setup_episode_limit_holds_the_greedy_envs_out(da, om, n=8):
    from deepterrainrl_amd import train_loop
    b = limit_batch(om, n, {}, limit=False)
    held = train_loop.setup_episode_limit(b, dict(frames=(2, 3), seed=4, hold_out=[1]), greedy_envs=2)
    assert held == {"hold_out": [1, 6, 7]}
    for _ in range(6):
        b.Update()
    info = b.EpisodeInfo()
    assert not info["by_limit"][[1, 6, 7]].any() and not info["limit"][[1, 6, 7]].any() and info["by_limit"][[0, 2, 3, 4, 5]].min() >= 1, info
    with pytest.raises(ValueError, match="unknown keys"):
        train_loop.setup_episode_limit(b, dict(frames=(2, 3), every=3))
    with pytest.raises(ValueError, match="or dist= is required"):
        train_loop.setup_episode_limit(b, dict(seed=3))
