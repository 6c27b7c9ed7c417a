"""Terrain ladder (include/dtrl.h dtrl_terrain_ladder): envs climb and descend a range of the batch's terrain set by their own episodes, at the frame boundary, in
front of the env's terrain work. The yardstick uses only calls that existed before: a second batch WITHOUT a ladder whose caller finds out per frame what every
env's frame will end like (SaveState / Update / RestoreState / StepUpdates), runs a pure-Python copy of the rule and moves the envs with AssignTerrains.
Every comparison is bit for bit: every field of the EnvState record, the policy state, the ground window and its build count.
Runs on the lane-loop check build (the host default of Backend::TerrainBoundary with -terrain_gen= device); tests/test_gpu_terrain_ladder.py points `Scenario`
at the product library (one launch of dtrl_terrain_boundary_ladder per env group and frame)."""
import numpy as np
import pytest

import test_external_policy as X          # env_states / same_record / observe / the recorded-decision replay
import test_model_variants as V
import test_policy_slots as P
import test_terrain_sets as T             # batches, terrain files, SlideWatch, assert_envs_equal, refused
from conftest import EmulScenario

Scenario = EmulScenario   # the GPU twin points this (and the helpers' own) at the product class

UPDATE_STEPS = 20         # env-steps of one outer frame (the dog's and the raptor's num_update_steps)


def plain_batch(om, n, mode, seed=31, trained=False, deal=None, **more):
    """dog, xavier policy under T.EXPLORE (or the trained net), the four walkable terrains; envs dealt over them with restart when `deal` is given"""
    b = T.fill(T.with_policy(om, T.DOG, n, dict(terrain_seed=seed, rand_seed=3, **mode, **more), trained), T.four_walkable_files(T.DOG))
    if deal is not None:
        b.AssignTerrains(None, deal, restart=True)
    return b


def root_x(b):
    return b.PoseVel()[0][:, 0].copy()


def resets(b):
    return np.asarray(b.CycleInfo()[1]).copy()


class PyLadder:
    """The rule, written from its description: levels, marks and counters of every env, and how often what happened."""
    def __init__(self, lo, hi, up_dist, down_dist, spawn_x, levels, marks):
        self.lo, self.hi, self.up, self.down, self.spawn = lo, hi, float(up_dist), float(down_dist), float(spawn_x)
        self.k = [int(x) for x in levels]
        self.mark = [float(x) for x in marks]
        self.ups, self.downs = [0] * len(self.k), [0] * len(self.k)
        self.promotions = self.demotions = self.held = 0
        self.promoted_at = {}

    def boundary(self, e, x, fell, frame=0):
        """mode 0: env e ends a frame at root x, fallen or not"""
        k = self.k[e]
        if k < self.lo or k > self.hi:
            return
        if fell:
            if x - self.mark[e] < self.down:
                if k > self.lo:
                    self.k[e] = k - 1; self.downs[e] += 1; self.demotions += 1
                else:
                    self.held += 1
            self.mark[e] = self.spawn
        elif x - self.mark[e] >= self.up:
            if k < self.hi:
                self.k[e] = k + 1; self.ups[e] += 1; self.promotions += 1
                self.promoted_at.setdefault(e, frame)
            else:
                self.held += 1
            self.mark[e] = float(x)


def check_ladder_equals_rule(a, rule, what):
    info = a.LadderInfo()
    assert list(a.GetTerrains()) == rule.k, what
    assert info["mark_x"].tobytes() == np.asarray(rule.mark, np.float64).tobytes(), (what, info["mark_x"], rule.mark)
    assert list(info["ups"]) == rule.ups and list(info["downs"]) == rule.downs, what


def hand_frame(b, rule, frame):
    """One frame of the batch without a ladder, the caller doing the ladder's work with calls that existed before it. Returns which envs fell."""
    snap = b.SaveState()
    r0 = resets(b)
    b.Update()
    fell = resets(b) > r0
    x_upd = root_x(b)                       # the root x at the frame's end -- of the envs that did not fall (the others have been reset)
    b.RestoreState(snap)
    b.StepUpdates(UPDATE_STEPS)             # the frame's env-steps without its end: nobody is reset, q[0] is the root x at the fall
    x_end = root_x(b)
    assert x_end[~fell].tobytes() == x_upd[~fell].tobytes()
    b.RestoreState(snap); snap.free()
    before = list(rule.k)
    for e in range(b.num_envs):
        rule.boundary(e, x_end[e], bool(fell[e]), frame)
    moved = [e for e in range(b.num_envs) if rule.k[e] != before[e]]
    if moved:
        b.AssignTerrains(moved, [rule.k[e] for e in moved], restart=False)
    b.Update()
    return fell


def run_against_hand_driven(make, lo, hi, up_dist, down_dist, frames, what, floors=True):
    """Batch A = make() with a ladder against batch B = make() driven by hand, compared after every frame. Returns (A, the Python rule)."""
    a, b = make(), make()
    n = a.num_envs
    x0 = root_x(b)
    a.TerrainLadder(lo, hi, up_dist, down_dist)
    rule = PyLadder(lo, hi, up_dist, down_dist, x0[0], b.GetTerrains(), x0)
    check_ladder_equals_rule(a, rule, what + ": at creation")
    watch = T.SlideWatch(b)
    seam_prev = list(watch.seam0)
    slid_after_promotion = set()
    for f in range(frames):
        a.Update()
        fell = hand_frame(b, rule, f)
        check_ladder_equals_rule(a, rule, "%s: frame %d" % (what, f))
        T.assert_envs_equal(a, b, range(n), "%s: frame %d" % (what, f))
        watch.look()
        seam_now = [T.seam(b, e) for e in range(n)]
        for e in range(n):   # a slide (not the fall's fresh window) of an env promoted in this boundary or an earlier one
            if seam_now[e] != seam_prev[e] and not fell[e] and e in rule.promoted_at:
                slid_after_promotion.add(e)
        seam_prev = seam_now
    assert np.all(x0 == x0[0]), "the envs do not spawn at one x"
    if floors:   # the run must not pass empty (counted on B's side)
        got = dict(promotions=rule.promotions, demotions=rule.demotions, held=rule.held, slid_after_promotion=sorted(slid_after_promotion), slid=sorted(watch.slid))
        print(what, got)
        assert rule.promotions >= 5 and rule.demotions >= 5, got
        assert rule.held >= 1, got
        assert slid_after_promotion and slid_after_promotion <= watch.slid, got
    return a, rule


# ---- 1. the ladder equals the caller doing it by hand ----
# (the issue's starting values -- 45 frames, up_dist 1.0, down_dist 0.5 -- gave 38 promotions but 2 demotions and no slide on the check build: the dog covers 0.13 m
# a frame, so its window first slides around frame 70 and every env sits at the top by frame 30. Longer distances and more frames; the floors are the issue's.)
HAND = dict(n=24, frames=100, up_dist=2.0, down_dist=1.5)


@pytest.mark.parametrize("mode", T.MODES, ids=T.MODE_IDS)
def test_ladder_equals_hand_driven(da, om, mode):
    """24 dogs under the xavier policy with exploration, dealt e % 4 over four terrains, ladder 0 .. 3, at_top = 0: after every frame levels, marks, counters, states,
    policy states and windows equal the hand-driven batch's. The rule's own counts show promotions, demotions, an env held at an end and a promoted env whose window
    slid afterwards."""
    n = HAND["n"]
    run_against_hand_driven(lambda: plain_batch(om, n, mode, deal=[e % 4 for e in range(n)]), 0, 3, HAND["up_dist"], HAND["down_dist"], HAND["frames"], "hand-driven")


# ---- 2. envs off the ladder are untouched ----
@pytest.mark.parametrize("mode", T.MODES, ids=T.MODE_IDS)
def test_envs_off_the_ladder_are_untouched(da, om, mode, n=12, frames=30):
    deal = [e % 4 for e in range(n)]
    a = plain_batch(om, n, mode, deal=deal)
    ref = plain_batch(om, n, mode, deal=deal)
    gone = plain_batch(om, n, mode, deal=deal)
    a.TerrainLadder(1, 2, 0.3, 0.5)
    gone.TerrainLadder(1, 2, 0.3, 0.5)
    gone.TerrainLadder(1, 0, 0.3, 0.5)                     # lo > hi: removed again, the levels stay
    assert list(gone.GetTerrains()) == deal
    T.refused(da, lambda: gone.LadderInfo(), "dtrl_ladder_info", "dtrl_terrain_ladder")
    for f in range(frames):
        a.Update(); ref.Update(); gone.Update()
    off = [e for e in range(n) if deal[e] in (0, 3)]
    T.assert_envs_equal(a, ref, off, "envs off the ladder")
    assert [int(t) for t in a.GetTerrains(off)] == [deal[e] for e in off]
    info = a.LadderInfo()
    assert not info["ups"][off].any() and not info["downs"][off].any()
    assert info["ups"].sum() + info["downs"].sum() > 0, "no env on the ladder moved"
    T.assert_envs_equal(gone, ref, range(n), "a batch whose ladder was removed")   # no ladder: the parent's states
    assert list(gone.GetTerrains()) == deal
    gone.UpdateBegin()
    assert list(gone.GetTerrains()) == deal                # (without a ladder: valid at any time, as before)
    gone.UpdateEnd()


# ---- 3. resets and restart ----
@pytest.mark.parametrize("mode", T.MODES, ids=T.MODE_IDS)
def test_resets_and_restart(da, om, mode, n=8, frames=12):
    a = plain_batch(om, n, mode, deal=[e % 4 for e in range(n)])
    spawn = root_x(a)[0]
    a.TerrainLadder(0, 3, 0.4, 0.5)
    for f in range(frames):
        a.Update()
    x = root_x(a)
    assert np.any(x != spawn)
    i0, lv0 = a.LadderInfo(), list(a.GetTerrains())
    a.Reset([1, 2])
    a.AssignTerrains([3], [lv0[3]], restart=True)
    a.AssignTerrains([4, 5], [lv0[5], lv0[4]], restart=False)
    i1 = a.LadderInfo()
    want = i0["mark_x"].copy()
    want[[1, 2, 3]] = spawn
    want[[4, 5]] = x[[4, 5]]
    assert i1["mark_x"].tobytes() == want.tobytes(), (i1["mark_x"], want)
    assert list(i1["ups"]) == list(i0["ups"]) and list(i1["downs"]) == list(i0["downs"])       # in none of the three do the counters move
    lv0[4], lv0[5] = lv0[5], lv0[4]
    assert list(a.GetTerrains()) == lv0
    assert root_x(a)[1] == spawn and root_x(a)[3] == spawn
    a.Update()


# ---- 4. at_top = 1 ----
def at_top_batch(om, n, mode, **more):
    b = plain_batch(om, n, mode, seed=9, trained=True, **more)
    b.TerrainLadder(1, 2, 0.3, 0.5, at_top=True)
    g0 = more.get("global_env_offset", 0)
    b.AssignTerrains(None, [1 + (g0 + e) % 2 for e in range(n)], restart=True)
    return b


@pytest.mark.parametrize("mode", T.MODES, ids=T.MODE_IDS)
def test_at_top_draws(da, om, mode, n=12, frames=40):
    """Ladder 1 .. 2 of four terrains with at_top: the levels stay on the ladder, the draw did run (an env went up more often than the ladder has steps and down),
    two runs give the same levels, and shards [0, 7) and [7, 12) with their global offsets equal the one batch env by env."""
    whole, again = at_top_batch(om, n, mode), at_top_batch(om, n, mode)
    lo, hi = at_top_batch(om, 7, mode), at_top_batch(om, 5, mode, global_env_offset=7)
    seen = set()
    for f in range(frames):
        for b in (whole, again, lo, hi):
            b.Update()
        lv = list(whole.GetTerrains())
        assert all(1 <= k <= 2 for k in lv), lv
        assert lv == list(again.GetTerrains()) and lv == list(lo.GetTerrains()) + list(hi.GetTerrains()), "frame %d" % f
        seen.update(lv)
    info = whole.LadderInfo()
    assert seen == {1, 2} and np.any(info["ups"] - info["downs"] > 1), (info["ups"], info["downs"])   # more net ups than steps: the top was passed through the draw
    T.assert_envs_equal(whole, again, range(n), "run after run")
    ow, ol, oh = X.observe(whole, range(n)), X.observe(lo, range(7)), X.observe(hi, range(5))
    for g in range(n):
        (sa, pa, ga), (sb, pb, gb) = ow[g], (ol[g] if g < 7 else oh[g - 7])
        bad = X.same_record(sa, sb)
        assert bad is None, "global env %d: EnvState.%s differs between the shard and the whole batch" % (g, bad)
        assert pa.tobytes() == pb.tobytes() and ga == gb, g
    il, ih = lo.LadderInfo(), hi.LadderInfo()
    for key in ("mark_x", "ups", "downs"):
        assert info[key].tobytes() == np.concatenate([il[key], ih[key]]).tobytes(), key


# ---- 5. key ownership ----
@pytest.mark.parametrize("mode", T.MODES, ids=T.MODE_IDS)
def test_key_ownership(da, om, mode, n=12, frames=20):
    a = plain_batch(om, n, mode, deal=[e % 4 for e in range(n)])
    a.TerrainLadder(0, 3, 0.3, 0.5)
    for f in range(frames):
        a.Update()
    lv = list(a.GetTerrains())
    assert lv != [e % 4 for e in range(n)], "no level moved"
    new = {2: (lv[2] + 1) % 4, 7: (lv[7] + 2) % 4}
    a.AssignTerrains(list(new), list(new.values()))
    want = [new.get(e, lv[e]) for e in range(n)]
    assert list(a.GetTerrains()) == want                     # every other env's level is what the ladder left, not what the host array last held
    stats = [a.TerrainStats(t) for t in range(4)]
    assert sum(s["n_envs"] for s in stats) == n and [s["n_envs"] for s in stats] == [want.count(t) for t in range(4)]
    T.check_terrain_stats(a)
    # batch state: a restore brings back the envs, not the levels or the records
    snap = a.SaveState()
    for f in range(10):
        a.Update()
    lv1, i1 = list(a.GetTerrains()), a.LadderInfo()
    a.RestoreState(snap); snap.free()
    i2 = a.LadderInfo()
    assert list(a.GetTerrains()) == lv1 and all(i1[k].tobytes() == i2[k].tobytes() for k in i1)
    a.Update()
    assert sum(a.TerrainStats(t)["n_envs"] for t in range(4)) == n


# ---- 6. combinations ----
def run_with_slots(om, mode, n=12, frames=30):
    pols = P.policies(om, T.DOG)

    def make():
        b = T.fill(P.slotted(T.DOG, n, pols, P.EXPLORE, [e % 3 for e in range(n)], dict(terrain_seed=31, rand_seed=3, **mode)), T.four_walkable_files(T.DOG))
        b.AssignTerrains(None, [e % 4 for e in range(n)], restart=True)
        return b
    a, rule = run_against_hand_driven(make, 0, 3, 0.5, 0.5, frames, "ladder x policy slots", floors=False)
    assert rule.promotions + rule.demotions >= 3, (rule.promotions, rule.demotions)


def run_with_variants(om, tmp_path, mode, n=12, frames=30):
    paths = V.write_variants(tmp_path, T.DOG)

    def make():
        b = T.fill(V.with_variants(om, T.DOG, n, paths, [e % 3 for e in range(n)], dict(terrain_seed=31, rand_seed=3, **mode)), T.four_walkable_files(T.DOG))
        b.AssignTerrains(None, [e % 4 for e in range(n)], restart=True)
        return b
    a, rule = run_against_hand_driven(make, 0, 3, 0.5, 0.5, frames, "ladder x model variants", floors=False)
    assert rule.promotions + rule.demotions >= 3, (rule.promotions, rule.demotions)


def run_with_external_policy(da, om, mode, n=16, frames=60):
    """The recorded-decision replay of test_external_policy with a ladder in both runs: run A internal, run B external gets A's decisions; whenever an env completes
    frame f it equals run A after frame f (state, policy state, window) -- with the levels moving on both sides."""
    extra = dict(terrain_seed=70, rand_seed=2, **mode)
    made = []
    real_batch = X.batch

    def batch_with_ladder(da_, arg_, n_, **ex):
        b = real_batch(da_, arg_, n_, **ex)
        T.fill(b, T.four_walkable_files(T.DOG)).AssignTerrains(None, [e % 4 for e in range(n_)])
        b.TerrainLadder(0, 3, 0.5, 0.5)
        made.append(b)
        return b
    X.batch = batch_with_ladder
    try:
        rec, decisions, blind_from, _, a = X.run_internal(da, om, T.DOG, n, frames, extra)
        compared, _, b = X.replay_external(da, om, T.DOG, n, frames, extra, rec, decisions, blind_from)
    finally:
        X.batch = real_batch
    assert len(made) == 2 and b.external
    assert compared >= n * frames // 2, compared
    info = a.LadderInfo()
    assert info["ups"].sum() >= 3 and info["downs"].sum() >= 1, (info["ups"], info["downs"])
    ib = b.LadderInfo()
    assert ib["ups"].sum() >= 3
    assert all(0 <= k <= 3 for k in b.GetTerrains())


@pytest.mark.parametrize("mode", T.MODES, ids=T.MODE_IDS)
def test_ladder_with_policy_slots(da, om, mode):
    run_with_slots(om, mode)


@pytest.mark.parametrize("mode", T.MODES, ids=T.MODE_IDS)
def test_ladder_with_model_variants(da, om, tmp_path, mode):
    run_with_variants(om, tmp_path, mode)


@pytest.mark.parametrize("mode", T.MODES, ids=T.MODE_IDS)
def test_ladder_with_external_policy(da, om, mode):
    run_with_external_policy(da, om, mode)


# ---- 7. refusals ----
def test_refusals(da, om, tmp_path, n=4):
    pol = T.policy_for(om, T.DOG)
    b = T.batch(T.DOG, n, terrain_seed=11)
    b.SetPolicy(pol[1], *pol[2:])
    T.refused(da, lambda: b.TerrainLadder(0, 1, 1.0, 0.5), "dtrl_terrain_ladder", "dtrl_terrains_create")   # no terrain set
    T.refused(da, lambda: b.LadderInfo(), "dtrl_ladder_info", "dtrl_terrains_create")
    b.CreateTerrains(3)
    b.SetTerrainFile(2, T.FLAT)
    T.refused(da, lambda: b.LadderInfo(), "dtrl_ladder_info", "no terrain ladder")
    T.refused(da, lambda: b.TerrainLadder(0, 2, 1.0, 0.5), "terrain 1", "empty")                              # an empty terrain inside [lo, hi]
    T.refused(da, lambda: b.TerrainLadder(0, 3, 1.0, 0.5), "out of range")
    T.refused(da, lambda: b.TerrainLadder(-1, 0, 1.0, 0.5), "out of range")
    b.SetTerrainFile(1, T.SLOPES)
    T.refused(da, lambda: b.TerrainLadder(0, 2, 0.0, 0.5), "up_dist")
    T.refused(da, lambda: b.TerrainLadder(0, 2, -1.0, 0.5), "up_dist")
    T.refused(da, lambda: b.TerrainLadder(0, 2, 1.0, -0.1), "down_dist")
    T.refused(da, lambda: b._chk(b._lib.dtrl_terrain_ladder(b._h, 0, 2, 1.0, 0.5, 2)), "at_top")
    b.UpdateBegin()
    T.refused(da, lambda: b.TerrainLadder(0, 2, 1.0, 0.5), "dtrl_terrain_ladder", "dtrl_step_begin")          # a frame in flight
    b.UpdateEnd()
    b.TerrainLadder(0, 2, 1.0, 0.5)
    b.TerrainLadder(1, 2, 2.0, 0.0, at_top=True)                                                              # replaced
    assert not b.LadderInfo()["ups"].any()
    b.UpdateBegin()
    T.refused(da, lambda: b.GetTerrains(), "dtrl_get_terrains", "dtrl_step_begin")                            # with a ladder: the last completed boundary
    T.refused(da, lambda: b.LadderInfo(), "dtrl_ladder_info", "dtrl_step_begin")
    T.refused(da, lambda: b.AssignTerrains(None, [0] * n), "dtrl_assign_terrains", "dtrl_step_begin")
    b.UpdateEnd()
    T.refused(da, lambda: b.LadderInfo([n]), "env id", "out of range")
    assert len(b.LadderInfo([0, 2])["mark_x"]) == 2
    # the spawn x is the batch's: -char_init_pos_x= moves it, and creation puts every mark there. (Model variants whose spawn x differ are refused by name; no
    # variant can be made to differ today -- the default pose comes from the batch's state file and -char_init_pos_x= from its arguments, which every variant shares --
    # so that refusal has no case here; test_ladder_with_model_variants holds the accepted side.)
    v = T.batch(T.DOG, n, terrain_seed=11, char_init_pos_x=0.5)
    v.CreateTerrains(2); v.SetTerrainFile(1, T.FLAT)
    v.TerrainLadder(0, 1, 1.0, 0.5)
    assert np.all(v.LadderInfo()["mark_x"] == 0.5) and np.all(root_x(v) == 0.5), v.LadderInfo()["mark_x"]


def test_terrain_ladder_tool(da, om, n=6, frames=40):
    """tools/terrain_ladder.py's run(): the committed dog policy on three lerp steps of slopes_mixed; the printed histogram counts every env, the counters only grow."""
    import os
    import sys
    from conftest import REFDATA, REPO, trained_policy
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import terrain_ladder
    pol = trained_policy(om, "dog")
    scn = T.Scenario if not T.is_emul() else (lambda *a, **k: EmulScenario(*a, **k))
    lines = []
    rows, stats = terrain_ladder.run(T.DOG, REFDATA, T.SLOPES_MIXED, (pol[1], tuple(pol[2:])), 3, n, frames, 0.5, 0.5, every=10, seed=5, scenario=scn, out=lines.append)
    assert [r[0] for r in rows] == [10, 20, 30, 40] and all(sum(r[1]) == n for r in rows)
    assert all(a[2] <= b[2] and a[3] <= b[3] for a, b in zip(rows, rows[1:])) and rows[-1][2] >= n
    assert sum(s["n_envs"] for s in stats) == n and len(lines) == 1 + 4 + 1 + 3
