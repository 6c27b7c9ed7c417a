"""Terrain sets (include/dtrl.h dtrl_terrains_create ...): several terrains in one batch, one per env. The yardsticks are the paths that existed before: a batch
CREATED with a terrain file (restart), the curriculum call dtrl_set_terrain_lerp (no restart), and the batch that puts all its envs into one terrain (independence).
Every comparison is bit for bit: every field of the EnvState record, the policy state, the ground window and its build count.
Runs on the lane-loop check build of the kernel source (tests/emul: the host default of Backend::TerrainBoundary with -terrain_gen= device);
tests/test_gpu_terrain_sets.py points `Scenario` at the product library (one launch of dtrl_terrain_boundary_keyed)."""
import json
import os

import numpy as np
import pytest

import test_external_policy as X          # env_states / same_record / ground_key / observe: helpers that take a batch
import test_host_and_emul as H
import test_model_variants as V           # variant character files
import test_policy_slots as P             # three policies per character
from conftest import REFDATA, REPO, EmulScenario, dog_policy, emul_f32_scenario, trained_policy

Scenario = EmulScenario   # the GPU twin points this at the product class

DOG, RAPTOR = "args/dog_slopes_mixed_args.txt", "args/raptor_narrow_gaps_args.txt"
EXPLORE = (1, 0.5, 0.25, 0.1)
TDIR = "data/terrain/"
FLAT, SLOPES, SLOPES_MIXED, NARROW_GAPS, CLIFFS = (TDIR + f for f in ("flat.txt", "slopes.txt", "slopes_mixed.txt", "narrow_gaps.txt", "cliffs_rugged.txt"))
MODES = [dict(), dict(terrain_gen="device")]
MODE_IDS = ["host_terrain", "device_terrain"]


def is_emul():
    return Scenario is EmulScenario


def batch(arg, n, **extra):
    if extra.get("physics_precision") == "f32" and is_emul():
        return emul_f32_scenario(arg, n, data_root=REFDATA, extra_args=extra)
    return Scenario(arg, n, data_root=REFDATA, extra_args=extra)


def policy_for(om, arg):
    return H.raptor_policy(om) if "raptor" in arg else dog_policy(om)


def own_file(arg):
    return NARROW_GAPS if "raptor" in arg else SLOPES_MIXED


def four_files(arg):
    """[terrain 0 = the arg file's own (None), 1, 2, 3]: flat / slopes_mixed / narrow_gaps / cliffs_rugged in the order that leaves the scene's own terrain at 0."""
    return [None] + [f for f in (SLOPES_MIXED, NARROW_GAPS, CLIFFS, FLAT) if f != own_file(arg)]


def four_walkable_files(arg):
    """The same with `slopes` in place of `cliffs_rugged`: no committed policy gets far enough on the cliffs for a window to slide within a test's frames."""
    return [SLOPES if f == CLIFFS else f for f in four_files(arg)]


def with_policy(om, arg, n, extra, trained=False):
    """xavier weights (falls every second or two: many resets), or the committed trained net of the character with mild exploration (runs: windows slide)"""
    b = batch(arg, n, **extra)
    pol = trained_policy(om, "raptor" if "raptor" in arg else "dog") if trained else policy_for(om, arg)
    b.SetPolicy(pol[1], *pol[2:])
    b.SetExplore(*((1, 0.2, 0.25, 0.1) if trained else EXPLORE))
    return b


def fill(b, files):
    b.CreateTerrains(len(files))
    assert b.num_terrains == len(files) and list(b.GetTerrains()) == [0] * b.num_envs
    for t in range(1, len(files)):
        assert not b.TerrainInfo(t)["filled"]
        b.SetTerrainFile(t, files[t])
        assert b.TerrainInfo(t)["filled"]
    return b


def seam(b, e):
    """Where env e's two segments meet: the spawn window's middle until the window slides."""
    segs, _ = b.GroundWindow(e)
    return segs[1][0]


class SlideWatch:
    """Which envs' windows have slid at some frame: looked at after every frame, because a fall puts the window back around the spawn point."""
    def __init__(self, b):
        self.b, self.n = b, b.num_envs
        self.seam0 = [seam(b, e) for e in range(self.n)]
        self.slid = set()

    def look(self):
        self.slid.update(e for e in range(self.n) if e not in self.slid and seam(self.b, e) != self.seam0[e])


def assert_envs_equal(bs, ref, envs, what):
    envs = list(envs)
    oa, ob = X.observe(bs, envs), X.observe(ref, envs)
    for e in envs:
        (sa, pa, ga), (sb, pb, gb) = oa[e], ob[e]
        bad = X.same_record(sa, sb)
        assert bad is None, "%s: env %d: EnvState.%s differs" % (what, e, bad)
        assert pa.tobytes() == pb.tobytes(), "%s: env %d: policy state differs" % (what, e)
        assert ga == gb, "%s: env %d: ground window / build count differs" % (what, e)


# ---- 1. restart equals creation ----
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("arg", [DOG, RAPTOR], ids=["dog", "raptor"])
def test_restart_equals_creation(da, om, arg, mode, n=48):
    """48 envs dealt e % 3 over {the arg file's terrain, narrow_gaps, cliffs_rugged} with restart: right after the call every env's window (counts, ranges, heights,
    build count) is env e's of a batch CREATED with that terrain file at the same terrain seed and env-id base. Independent of the new boundary path's arithmetic:
    the yardstick never heard of terrain sets."""
    extra = dict(terrain_seed=21, global_env_offset=7, **mode)
    files = [None, NARROW_GAPS, CLIFFS]
    a = fill(batch(arg, n, **extra), files)
    assign = [e % 3 for e in range(n)]
    a.AssignTerrains(None, assign, restart=True)
    assert list(a.GetTerrains()) == assign
    for t in range(3):
        ref = batch(arg, n, **(dict(extra, terrain_file=files[t]) if files[t] else extra))
        for e in range(n):
            if assign[e] == t:
                assert X.ground_key(a, e) == X.ground_key(ref, e), "env %d (terrain %d): the restarted window is not the created one" % (e, t)
                assert X.ground_key(a, e)[1] == (2 if mode else -1)
    if arg == DOG:   # different terrains did give different ground
        assert X.ground_key(a, 0)[0] != X.ground_key(a, 1)[0] and X.ground_key(a, 1)[0] != X.ground_key(a, 2)[0]


def test_restart_after_frames_equals_creation(da, om, n=12, frames=20):
    """The same after the batch has run: windows slid and were rebuilt, streams advanced, build counts grew -- restart still gives creation's windows."""
    for mode in MODES:
        extra = dict(terrain_seed=21, **mode)
        a = fill(with_policy(om, DOG, n, extra), [None, NARROW_GAPS])
        for _ in range(frames):
            a.Update()
        rc0 = X.env_states(a)["rng_ctr"].copy()
        a.AssignTerrains(list(range(0, n, 2)), [1] * (n // 2), restart=True)
        ref = batch(DOG, n, **dict(extra, terrain_file=NARROW_GAPS))
        st = X.env_states(a)
        for e in range(0, n, 2):
            assert X.ground_key(a, e) == X.ground_key(ref, e), e
            assert st["rng_ctr"][e] >= rc0[e] > 0, "the exploration counter of env %d was rewound" % e
        a.Update()


# ---- 2. no restart equals the curriculum path ----
def two_set_file(tmp_path, arg):
    """The scene's own terrain file with a second, harder parameter set behind the first: something for a lerp to blend."""
    with open(os.path.join(REFDATA, own_file(arg))) as f:
        doc = json.load(f)
    hard = dict(doc["Params"][0])
    for k, v in hard.items():
        if k.endswith("WMax") or k.endswith("H0Max") or k == "SlopeDeltaRange":
            hard[k] = v * 1.5
    assert hard != doc["Params"][0]
    doc["Params"] = [doc["Params"][0], hard]
    p = tmp_path / "two_sets.txt"
    p.write_text(json.dumps(doc))
    return str(p)


CURRICULUM_SEED = {"host_terrain": 11, "device_terrain": 7}   # chosen on the check build so that a window slides (asserted below)


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_no_restart_equals_curriculum_step(da, om, tmp_path, mode, n=12, frames=150):
    """Terrain 1 = the batch's own (two-set) terrain file at lerp 0.7, all envs assigned to it without restart, against a second batch that called
    dtrl_set_terrain_lerp(0.7): after 150 frames EnvState, policy states, windows, build counts and EvalStats are equal. At least one window slid."""
    path = two_set_file(tmp_path, DOG)
    extra = dict(terrain_seed=CURRICULUM_SEED[MODE_IDS[MODES.index(mode)]], terrain_file=path, **mode)
    a = with_policy(om, DOG, n, extra)
    b = with_policy(om, DOG, n, extra)
    a.CreateTerrains(2)
    a.SetTerrainFile(1, path, 0.7)
    a.AssignTerrains(None, [1] * n)
    b.SetTerrainParamsLerp(0.7)
    i0, i1 = a.TerrainInfo(0), a.TerrainInfo(1)
    assert i0["type"] == i1["type"] == "slopes_mixed" and i0["params"].tobytes() != i1["params"].tobytes()
    assert_envs_equal(a, b, range(n), "after the assignment")      # the window in place stays
    watch = SlideWatch(a)
    for f in range(frames):
        a.Update(); b.Update()
        watch.look()
    assert_envs_equal(a, b, range(n), "after %d frames" % frames)
    assert a.EvalStats() == b.EvalStats()
    assert watch.slid, "no window slid: the comparison saw no segment built under the new terrain"
    if mode:
        assert any(X.ground_key(a, e)[1] > 2 for e in range(n))
    c = with_policy(om, DOG, n, extra)                                # (the lerp did change the ground that was built)
    for f in range(frames):
        c.Update()
    assert any(X.ground_key(a, e) != X.ground_key(c, e) for e in range(n))


# ---- 3. envs are independent ----
def dist_sum_in_reduction_order(x, mask):
    """sum of x[e] over the envs of `mask`, in the order Backend::SlotReduce adds them: env order on the check build; on the device per wavefront of 64 envs a
    butterfly (lane i + lane i ^ 32, then ^ 16 ...), the wavefronts in order (n <= 256: one workgroup, one pass)."""
    v = np.where(mask, x, 0.0).astype(np.float64)
    if is_emul():
        s = 0.0
        for e in np.nonzero(mask)[0]:
            s += float(v[e])
        return s
    assert len(v) <= 256
    v = np.concatenate([v, np.zeros(256 - len(v))])
    total = 0.0
    for w in range(4):
        r = v[64 * w:64 * w + 64].copy()
        d = 32
        while d > 0:
            r = r[:d] + r[d:2 * d]
            d //= 2
        total = (0.0 + float(r[0])) if w == 0 else total + float(r[0])   # (a wavefront without a member adds 0.0: the same bits)
    return total


def check_terrain_stats(b):
    """dtrl_terrain_stats == the sums over the member envs from the per-env getters, exactly; two calls return the same bits; over the terrains it is dtrl_eval_stats."""
    n = b.num_envs
    st = X.env_states(b)
    nc, nr = b.CycleInfo()[:2]
    ter = b.GetTerrains()
    tot = dict(n_envs=0, episodes=0, cycles=0, resets=0)
    out = []
    for t in range(b.num_terrains):
        got, again = b.TerrainStats(t), b.TerrainStats(t)
        assert got == again and np.float64(got["avg_dist"]).tobytes() == np.float64(again["avg_dist"]).tobytes()
        m = ter == t
        ep = int(st["num_episodes"][m].sum())
        assert (got["n_envs"], got["episodes"], got["cycles"], got["resets"]) == (int(m.sum()), ep, int(np.asarray(nc)[m].sum()), int(np.asarray(nr)[m].sum())), (t, got)
        ds = dist_sum_in_reduction_order(st["avg_dist"].astype(np.float64) * st["num_episodes"].astype(np.float64), m)
        want = ds / float(ep) if ep else 0.0
        assert np.float64(got["avg_dist"]).tobytes() == np.float64(want).tobytes(), (t, got["avg_dist"], want)
        for k in tot:
            tot[k] += got[k]
        out.append(got)
    ev = b.EvalStats()
    assert (tot["n_envs"], tot["episodes"], tot["cycles"], tot["resets"]) == (n, ev["episodes"], ev["cycles"], ev["resets"])
    return out


def mixed_batch(om, arg, n, files, assign, extra, trained=False):
    b = fill(with_policy(om, arg, n, extra, trained), files)
    b.AssignTerrains(None, assign, restart=True)
    return b


def run_envs_are_independent(om, arg, mode, n=96, seed=31):   # (the seed: chosen on the check build so that the conditions asserted below hold)
    frames = 150 if "raptor" in arg else 120
    extra = dict(terrain_seed=seed, rand_seed=3, **mode)
    files = four_walkable_files(arg)
    assign = [e % 4 for e in range(n)]
    a = mixed_batch(om, arg, n, files, assign, extra, trained=True)
    refs = [mixed_batch(om, arg, n, files, [t] * n, extra, trained=True) for t in range(4)]
    watch = SlideWatch(a)
    resets0 = [a.TerrainStats(t)["resets"] for t in range(4)]      # (the restart's own reset is counted by the engine; it is not a fall)
    for f in range(frames):
        a.Update()
        for r in refs:
            r.Update()
        watch.look()
    for t in range(4):
        assert_envs_equal(a, refs[t], [e for e in range(n) if assign[e] == t], "terrain %d" % t)
    stats = check_terrain_stats(a)
    for t in range(4):
        envs = [e for e in range(n) if assign[e] == t]
        assert stats[t]["resets"] - resets0[t] >= 1, "terrain %d saw no reset" % t
        assert watch.slid & set(envs), "terrain %d saw no slid window" % t
        if mode:
            assert any(X.ground_key(a, e)[1] > 2 for e in envs)
    da, ia = a.GetDistLog()
    for t in range(4):   # the distance log, env by env (both terrain modes: the default's ring writes included)
        dr, ir = refs[t].GetDistLog()
        for e in range(t, n, 4):
            assert da[ia == e].tobytes() == dr[ir == e].tobytes(), "dist log of env %d" % e
    return a


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("arg", [DOG, RAPTOR], ids=["dog", "raptor"])
def test_envs_are_independent(da, om, arg, mode):
    """96 envs, 4 terrains mixed e % 4 with restart, 120 frames (raptor 150): env e equals env e of the batch that put ALL envs into terrain e % 4 the same way;
    TerrainStats equals the sums over the member envs. Every terrain saw a reset and a slid window."""
    run_envs_are_independent(om, arg, mode)


# ---- 4. composition ----
def run_with_slots(om, arg, mode, n=12, frames=40):
    """Terrains x policy slots: env e runs slot e % 3 on terrain (e // 3) % 2; it equals env e of the 3-slot batch whose envs all sit in that terrain."""
    extra = dict(terrain_seed=11, **mode)
    pols = P.policies(om, arg)
    slots = [e % 3 for e in range(n)]
    terr = [(e // 3) % 2 for e in range(n)]
    files = [None, CLIFFS]
    plain_slots = P.slotted(arg, n, pols, P.EXPLORE, slots, extra)
    zero = fill(P.slotted(arg, n, pols, P.EXPLORE, slots, extra), files)           # terrains exist, every env in terrain 0
    a = fill(P.slotted(arg, n, pols, P.EXPLORE, slots, extra), files)
    a.AssignTerrains(None, terr, restart=True)
    refs = []
    for t in range(2):
        r = P.slotted(arg, n, pols, P.EXPLORE, slots, extra)
        fill(r, files).AssignTerrains(None, [t] * n, restart=True)
        refs.append(r)
    late = fill(batch(arg, n, **extra), files)                                     # the other order: terrains first, then slots
    late.CreateSlots(3)
    for f in range(frames):
        for b in [a, zero, plain_slots] + refs:
            b.Update()
    for t in range(2):
        assert_envs_equal(a, refs[t], [e for e in range(n) if terr[e] == t], "slots x terrains, terrain %d" % t)
    assert_envs_equal(zero, plain_slots, range(n), "terrains present, all envs in terrain 0")
    assert [zero.SlotStats(s) for s in range(3)] == [plain_slots.SlotStats(s) for s in range(3)]
    st = X.env_states(a)
    assert st["num_cycles"].sum() > n and st["num_resets"].sum() >= 1
    # per-cell figures from the per-env getters
    for s in range(3):
        for t in range(2):
            assert sum(1 for e in range(n) if slots[e] == s and terr[e] == t) == 2


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_terrains_with_policy_slots(da, om, mode):
    run_with_slots(om, DOG, mode)


def run_with_variants(om, tmp_path, arg, mode, n=12, frames=40):
    extra = dict(terrain_seed=11, **mode)
    paths = V.write_variants(tmp_path, arg)
    var = [e % 3 for e in range(n)]
    terr = [(e // 3) % 2 for e in range(n)]
    files = [None, CLIFFS]

    def make(t_assign):
        b = V.with_variants(om, arg, n, paths, var, extra)
        if t_assign is not None:
            fill(b, files)
            if any(t_assign):
                b.AssignTerrains(None, t_assign, restart=True)
        return b
    plain_var, zero = make(None), make([0] * n)
    a = make(terr)
    refs = []
    for t in range(2):
        r = V.with_variants(om, arg, n, paths, var, extra)
        fill(r, files).AssignTerrains(None, [t] * n, restart=True)
        refs.append(r)
    for f in range(frames):
        for b in [a, zero, plain_var] + refs:
            b.Update()
    for t in range(2):
        assert_envs_equal(a, refs[t], [e for e in range(n) if terr[e] == t], "variants x terrains, terrain %d" % t)
    assert_envs_equal(zero, plain_var, range(n), "terrains present, all envs in terrain 0")
    assert [zero.VariantStats(v) for v in range(3)] == [plain_var.VariantStats(v) for v in range(3)]
    assert X.env_states(a)["num_cycles"].sum() > n


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_terrains_with_model_variants(da, om, tmp_path, mode):
    run_with_variants(om, tmp_path, DOG, mode)


def run_with_external_policy(da, om, arg, mode, n=16, frames=90):
    """Terrains + external policy mode, the recorded-decision replay of test_external_policy: run A is INTERNAL with mixed terrains, run B external with the same
    terrains gets A's decisions; whenever an env completes frame f it equals run A after frame f. The envs are assigned WITHOUT restart (the replay's bookkeeping
    starts from the counters of a fresh batch): an env's terrain shows from its first fall or slide on."""
    extra = dict(terrain_seed=70, rand_seed=2, **mode)   # (test_external_policy's replay case)
    files = [None, CLIFFS]
    terr = [e % 2 for e in range(n)]
    made = []
    real_batch = X.batch

    def batch_with_terrains(da_, arg_, n_, **ex):
        b = real_batch(da_, arg_, n_, **ex)
        fill(b, files).AssignTerrains(None, terr)
        made.append(b)
        return b
    X.batch = batch_with_terrains
    try:
        rec, decisions, blind_from, _, a = X.run_internal(da, om, arg, n, frames, extra)
        compared, _, b = X.replay_external(da, om, arg, n, frames, extra, rec, decisions, blind_from)
    finally:
        X.batch = real_batch
    assert len(made) == 2 and b.external and list(b.GetTerrains()) == terr
    assert compared >= n * frames // 2, compared
    # against the single-terrain internal batches, per env
    for t in range(2):
        r = with_policy(om, arg, n, extra)
        r.SetExplore(0, 0.0, 1.0, 0.0)
        fill(r, files).AssignTerrains(None, [t] * n)
        for f in range(frames):
            r.Update()
        assert_envs_equal(a, r, [e for e in range(n) if terr[e] == t], "internal run A, terrain %d" % t)
        if t == 0:
            assert any(X.ground_key(a, e) != X.ground_key(r, e) for e in range(n) if terr[e] == 1), "no env of terrain 1 has built ground of its own"


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_terrains_with_external_policy(da, om, mode):
    run_with_external_policy(da, om, DOG, mode)


# ---- 5. batch state ----
def slope_stat(h):
    """mean |dh| between neighbouring vertices without the jumps (gaps, steps): 0 on a flat terrain"""
    d = np.abs(np.diff(np.asarray(h, np.float64)))
    return float(d[d < 0.05].mean())


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_batch_state(da, om, mode, n=8, frames=140):
    """The assignment is batch state: snapshot save / restore / clone / export-import and Reset leave it as it was set. A window restored into an env under
    another terrain builds its next segment under the env's CURRENT terrain: a window saved under `slopes` and restored into envs of `flat` grows flat."""
    extra = dict(terrain_seed=17, terrain_file=SLOPES, **mode)
    a = fill(with_policy(om, DOG, n, extra, trained=True), [None, FLAT])
    assign = [0, 1] * (n // 2)
    a.AssignTerrains(None, assign, restart=True)
    for f in range(3):
        a.Update()
    snap = a.SaveState()
    want = [1, 0] * (n // 2)
    a.AssignTerrains(None, want)                              # no restart: the windows stay
    a.RestoreState(snap)
    assert list(a.GetTerrains()) == want
    blob = snap.export(); snap.free()
    s2 = a.ImportState(blob); a.RestoreState(s2); s2.free()
    assert list(a.GetTerrains()) == want
    a.CloneEnvs([0], [3])                                     # env 0 (now flat) -> env 3 (slopes): the window moves, the terrain stays
    assert list(a.GetTerrains()) == want
    a.Reset([6])
    assert list(a.GetTerrains()) == want
    seam0 = {e: seam(a, e) for e in range(n)}
    before = {e: a.GroundWindow(e)[0] for e in range(n)}
    checked = {0: set(), 1: set()}
    for f in range(frames):
        a.Update()
        for e in range(n):
            if e in checked[want[e]] or seam(a, e) == seam0[e]:
                continue
            new = a.GroundWindow(e)[0][1][2]                   # the window has just slid forward: its max segment was built after the restore
            if want[e] == 1:
                assert slope_stat(new) == 0.0, "env %d sits in the flat terrain, its new segment is not flat" % e
            else:
                assert slope_stat(new) > 1e-3, "env %d sits in the slopes terrain, its new segment is flat" % e
            checked[want[e]].add(e)
    assert list(a.GetTerrains()) == want
    assert checked[0] and checked[1], checked
    # the saved windows themselves were of the OTHER terrain
    assert slope_stat(before[0][0][2]) > 1e-3 and slope_stat(before[1][0][2]) == 0.0


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_two_shards_equal_one_process(da, om, mode, n=12, frames=40):
    """Local env ids: shards [0, 7) and [7, 12) with their global offsets, each dealing ITS envs by global id, equal the one batch env by env."""
    extra = dict(terrain_seed=9, rand_seed=3, **mode)
    files = [None, NARROW_GAPS, CLIFFS]
    whole = mixed_batch(om, DOG, n, files, [e % 3 for e in range(n)], extra)
    lo = mixed_batch(om, DOG, 7, files, [g % 3 for g in range(0, 7)], extra)
    hi = mixed_batch(om, DOG, 5, files, [g % 3 for g in range(7, 12)], dict(extra, global_env_offset=7))
    assert list(hi.GetTerrains([0, 1])) == [7 % 3, 8 % 3]
    for f in range(frames):
        whole.Update(); lo.Update(); hi.Update()
    ow, ol, oh = X.observe(whole, range(n)), X.observe(lo, range(7)), X.observe(hi, range(5))
    for g in range(n):
        (sa, pa, ga), (sb, pb, gb) = ow[g], (ol[g] if g < 7 else oh[g - 7])
        bad = X.same_record(sa, sb)
        assert bad is None, "global env %d: EnvState.%s differs between the shard and the whole batch" % (g, bad)
        assert pa.tobytes() == pb.tobytes() and ga == gb, g
    assert X.env_states(whole)["num_resets"].sum() >= 1


# ---- 6. refusals and the idle rule ----
def refused(da, fn, *words, code="(1)"):
    with pytest.raises(da.DtrlError) as ei:
        fn()
    msg = str(ei.value)
    assert code in msg, msg                                        # DTRL_ERR_ARG unless stated
    for w in words:
        assert w in msg, (w, msg)


def test_refusals(da, om, tmp_path, n=4):
    pol = policy_for(om, DOG)
    b = batch(DOG, n, terrain_seed=11)
    b.SetPolicy(pol[1], *pol[2:])
    for fn in (lambda: b.AssignTerrains(None, [0] * n), lambda: b.SetTerrainFile(1, NARROW_GAPS), lambda: b.SetTerrainParams(1, "flat", np.zeros(40)),
               lambda: b.GetTerrains(), lambda: b.TerrainStats(0), lambda: b.TerrainInfo(0)):
        refused(da, fn, "dtrl_terrains_create")                    # no terrains yet
    refused(da, lambda: b.CreateTerrains(0), "n_terrains")
    refused(da, lambda: b.CreateTerrains(n + 1), "n_terrains")
    b.UpdateBegin()
    refused(da, lambda: b.CreateTerrains(3), "dtrl_step_begin", "dtrl_step_end")
    b.UpdateEnd()
    b.CreateTerrains(3)
    b.CreateTerrains(3)                                            # the same count again is accepted
    refused(da, lambda: b.CreateTerrains(2), "already", "3 terrains")
    refused(da, lambda: b.SetTerrainFile(3, NARROW_GAPS), "terrain 3", "out of range")
    refused(da, lambda: b.SetTerrainFile(-1, NARROW_GAPS), "out of range")
    refused(da, lambda: b.SetTerrainFile(0, NARROW_GAPS), "terrain 0", "own terrain")
    refused(da, lambda: b.SetTerrainParams(0, "flat", np.zeros(40)), "terrain 0", "own terrain")
    refused(da, lambda: b.TerrainStats(3), "terrain 3", "out of range")
    refused(da, lambda: b.TerrainInfo(3), "terrain 3", "out of range")
    refused(da, lambda: b.AssignTerrains(None, [0, 3, 0, 0]), "terrain 3", "out of range")
    refused(da, lambda: b.AssignTerrains(None, [0, 1, 0, 0]), "terrain 1", "empty")
    assert list(b.GetTerrains()) == [0] * n                        # all or nothing
    refused(da, lambda: b.SetTerrainFile(1, str(tmp_path / "missing.txt")), "terrain 1", "missing.txt", code="(2)")   # DTRL_ERR_IO
    bad = tmp_path / "bad_type.txt"
    bad.write_text(json.dumps({"Type": "moguls", "Params": []}))
    refused(da, lambda: b.SetTerrainFile(1, str(bad)), "terrain 1", "moguls")
    refused(da, lambda: b.SetTerrainParams(1, "moguls", np.zeros(40)), "terrain 1", "moguls")
    refused(da, lambda: b.AssignTerrains(None, [0, 1, 0, 0]), "terrain 1", "empty")    # a refused fill leaves the terrain empty
    b.SetTerrainFile(1, NARROW_GAPS)
    b.SetTerrainFile(2, CLIFFS)
    prm = b.TerrainInfo(2)["params"].copy()
    b.SetTerrainParams(2, "flat", np.zeros(40))
    assert b.TerrainInfo(2)["type"] == "flat" and not b.TerrainInfo(2)["params"].any()
    b.SetTerrainParams(2, "cliffs", prm)                           # the same from memory
    assert b.TerrainInfo(2)["params"].tobytes() == prm.tobytes()
    assert b.TerrainInfo(2)["type"] == "cliffs" and b.TerrainInfo(1)["type"] == "narrow_gaps" and b.TerrainInfo(0)["type"] == "slopes_mixed"
    b.UpdateBegin()
    refused(da, lambda: b.AssignTerrains(None, [0] * n), "dtrl_assign_terrains", "dtrl_step_begin")
    refused(da, lambda: b.AssignTerrains(None, [1] * n, restart=True), "dtrl_step_begin")
    refused(da, lambda: b.SetTerrainFile(1, NARROW_GAPS), "dtrl_terrain_set_file", "dtrl_step_begin")
    refused(da, lambda: b.SetTerrainParams(1, "flat", np.zeros(40)), "dtrl_step_begin")
    refused(da, lambda: b.TerrainStats(1), "dtrl_terrain_stats", "dtrl_step_begin")
    assert list(b.GetTerrains()) == [0] * n                        # (valid at any time)
    b.UpdateEnd()
    refused(da, lambda: b.AssignTerrains([0, n], [1, 1]), "env id", "out of range")
    refused(da, lambda: b.AssignTerrains([-1], [1]), "env id", "out of range")
    refused(da, lambda: b.GetTerrains([n]), "out of range")
    b.AssignTerrains([1, 3], [1, 2])
    assert list(b.GetTerrains()) == [0, 1, 0, 2]
    b.Update()
    # NOT refused with slots, variants or external mode, in either order
    s = batch(DOG, n, terrain_seed=11); s.SetPolicy(pol[1], *pol[2:]); s.CreateSlots(2); s.CreateTerrains(2)
    s = batch(DOG, n, terrain_seed=11); s.SetPolicy(pol[1], *pol[2:]); s.CreateTerrains(2); s.CreateSlots(2)
    v = batch(DOG, n, terrain_seed=11); v.CreateVariants(2); v.CreateTerrains(2)
    v = batch(DOG, n, terrain_seed=11); v.CreateTerrains(2); v.CreateVariants(2)
    x = batch(DOG, n, terrain_seed=11, policy_mode="external"); x.CreateTerrains(2)


def test_terrain_zero_follows_the_curriculum(da, om, tmp_path, n=6):
    """dtrl_set_terrain_lerp on a batch with terrains rewrites entry 0 and moves the envs in terrain 0 alone."""
    path = two_set_file(tmp_path, DOG)
    for mode in MODES:
        b = fill(with_policy(om, DOG, n, dict(terrain_seed=11, terrain_file=path, **mode)), [None, FLAT])
        b.AssignTerrains([1, 3], [1, 1])
        p0 = b.TerrainInfo(0)["params"].copy()
        b.SetTerrainParamsLerp(1.0)
        p1 = b.TerrainInfo(0)["params"]
        assert p0.tobytes() != p1.tobytes() and b.TerrainInfo(1)["type"] == "flat"
        ref = with_policy(om, DOG, n, dict(terrain_seed=11, terrain_file=path, **mode))
        ref.SetTerrainParamsLerp(1.0)
        for f in range(100):
            b.Update(); ref.Update()
        # (envs 1 and 3 build flat ground from their first slide on: they part from the reference run; the others are the reference run)
        assert_envs_equal(b, ref, [0, 2, 4, 5], "envs in terrain 0")


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_batch_without_terrains_launches_as_before(da, om, mode, n=6, frames=30):
    """A batch that never calls CreateTerrains: per frame the launch counter advances as it always did, and after F frames it equals, bit for bit, a batch with
    terrains whose envs all stayed in terrain 0 -- which itself launches no frame kernel more."""
    emul = is_emul()
    extra = dict(terrain_seed=11, **mode)
    b = with_policy(om, DOG, n, extra)
    bt = fill(with_policy(om, DOG, n, extra), [None, CLIFFS])
    b.KernelTimeMs(); bt.KernelTimeMs()
    r0 = X.env_states(b)["num_resets"].sum()
    for f in range(frames):
        b.Update(); bt.Update()
        r1 = X.env_states(b)["num_resets"].sum()
        # (device terrain: the 0-step reset launch is queued every frame; the check build's counter sees it)
        want = 1 + (1 if emul and (mode or r1 != r0) else 0)
        assert b.KernelTimeMs()[1] == want and bt.KernelTimeMs()[1] == want, "frame %d" % f
        r0 = r1
    assert_envs_equal(b, bt, range(n), "terrains present, all envs in terrain 0")
    assert b.EvalStats() == bt.EvalStats()


def test_queued_behind_unfinished_frames(da, om, n=12, frames=25):
    """Frames queued without a host wait -- -terrain_gen= device under dtrl_step_end_begin (the boundary work and the next frame are queued behind the frame, the
    host waits for nothing), and host terrain with dtrl_step_poll relaunching groups early (host tuple ring) -- then, right behind them, set_file + assign: they take
    effect only after those frames. Build counts and windows equal the synchronous order (Update() frame by frame). While a group is a frame ahead, assign is refused."""
    files = [None, NARROW_GAPS]

    def finish(b):
        b.SetTerrainFile(1, CLIFFS)
        b.AssignTerrains(list(range(0, n, 2)), [1] * (n // 2))
        for f in range(frames):
            b.Update()
    for extra in (dict(terrain_seed=11, terrain_gen="device"), dict(terrain_seed=11, tuple_ring="host")):
        a = fill(with_policy(om, DOG, n, extra), files)
        s = fill(with_policy(om, DOG, n, extra), files)
        for f in range(frames):
            s.Update()
        polled = 0
        if "tuple_ring" in extra:
            a.SetTuplePipelining(True)
        a.UpdateBegin()
        for f in range(frames - 1):
            a.UpdateEndBegin()
            if "tuple_ring" in extra:
                a.DrainTuples()
            k = a.UpdatePoll()
            polled += k
            refused(da, lambda: a.AssignTerrains(None, [0] * n), "dtrl_assign_terrains", "dtrl_step_begin")
            refused(da, lambda: a.SetTerrainFile(1, CLIFFS), "dtrl_step_begin")
        a.UpdateEndBegin()      # no poll behind this one: a polled group is a frame ahead, and dtrl_step_end wants the groups level
        a.UpdateEnd()
        s.Update()              # (frames + 1 frames on both sides)
        if "tuple_ring" in extra and not is_emul():
            print("dtrl_step_poll relaunched %d groups early" % polled)
        finish(a); finish(s)
        assert_envs_equal(a, s, range(n), "queued against synchronous")
        if "terrain_gen" in extra:
            assert any(X.ground_key(a, e)[1] > 2 for e in range(0, n, 2))


def test_terrain_sweep_tool(da, om, n=3, frames=40):
    """tools/terrain_sweep.py's sweep(): 2 policies x 2 terrains in one batch, per-cell figures from the per-env getters; with one policy (and with none: the FSM scene)
    the per-terrain device reduction agrees with them (asserted inside sweep)."""
    import sys
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import terrain_sweep
    scn = Scenario if not is_emul() else (lambda *a, **k: EmulScenario(*a, **k))
    pols = [(p[1], tuple(p[2:])) for p in P.policies(om, DOG)[:2]]
    for pp, arg in (([], "args/sim_dog_args.txt"), (pols[:1], DOG), (pols, DOG)):
        cells, dist = terrain_sweep.sweep(arg, REFDATA, [FLAT, CLIFFS], pp, n, frames, seed=5, scenario=scn)
        assert len(cells) == max(1, len(pp)) and all(len(row) == 2 for row in cells)
        for row, drow in zip(cells, dist):
            for c, d in zip(row, drow):
                assert c["n_envs"] == n and c["cycles"] > 0 and c["episodes"] == len(d)
    assert sum(c["falls"] for row in cells for c in row) >= 1
