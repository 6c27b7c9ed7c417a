"""Variant rescale (include/dtrl.h dtrl_variant_rescale): envs under a private model record draw continuous mass and motor scales at each episode start, in front
of the reset launch, by counter-based draws that depend on (seed, global env id, the env's episode number) alone. The yardsticks are a pure-Python restatement
of the draw and the character loader itself: the private record must hold the bits ScaledVariant under the reported factors loads.
Runs on the lane-loop check build (the host default of Backend::VariantRescale, the per-key default of Backend::LaunchKeyed); tests/test_gpu_variant_rescale.py
points `Scenario` at the product library (one launch of dtrl_variant_rescale per env group and frame)."""
import json
import os

import numpy as np
import pytest

import test_external_policy as X          # env_states / same_record / observe
import test_model_variants as V           # batch / policy_for / write_variants / assert_envs_equal / refused
import test_terrain_sets as T             # MODES
from conftest import REFDATA, EmulScenario

Scenario = EmulScenario   # the GPU twin points this (and the helpers' own) at the product class

DOG, RAPTOR = V.DOG, V.RAPTOR
M64 = (1 << 64) - 1
RESCALE_CONST = 0x5CA1ED          # the rescale's own constant (the redraw's is 0x5EDBA77)
QUANT = ("mass", "kp", "kd", "torque_lim")
# wide ranges: dogs with weak, soft motors fall early (the xavier dogs of the nominal model fall around frame 40)
RANGES = dict(mass=(0.6, 2.0), kp=(0.3, 1.2), kd=(0.5, 1.5), torque_lim=(0.1, 1.0))
# found by running the check build: under RANGES, rescale seed 7 and this terrain seed, env 3 of 6 falls in frame 17 (counted from 0) in both terrain modes. No env
# fell within three frames of a Reset at any of the terrain seeds 1 .. 39 tried (the fall rule needs about half a second of simulated time), so the three frames
# that must hold a fall and a redraw follow WARM frames that are compared like them
TERRAIN_SEED, RESCALE_SEED, WARM, FALL_ENV = 1, 7, 16, 3


# ---- the rule, written from its description ----
def tg_mix(x):
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def py_factors(seed, gid, n, L, ranges=RANGES, per_link=()):
    """factors [4][L] of global env `gid` in its episode n"""
    key = tg_mix(tg_mix(seed & M64) ^ ((RESCALE_CONST + gid) & M64))
    out = np.ones((4, L))
    for q, name in enumerate(QUANT):
        lo, hi = ranges.get(name) or (1.0, 1.0)
        for j in range(L):
            idx = n * 4 * L + q * L + (j if name in per_link else 0)
            u = float(tg_mix((key + idx * 0xD1342543DE82EF95) & M64) >> 11) * 2.0 ** -53
            out[q, j] = lo + u * (hi - lo)
    return out


def same_bits(a, b):
    return np.asarray(a, np.float64).tobytes() == np.asarray(b, np.float64).tobytes()


def resets(b):
    return np.asarray(b.CycleInfo()[1]).copy()


def rescaled(om, arg, n, mode, per_link=("mass", "kp"), ranges=RANGES, seed=RESCALE_SEED, env_ids=None, n_variants=1, reset=True, terrain_seed=TERRAIN_SEED, **more):
    """n characters, xavier policy under V.EXPLORE, a variant table, the rescale over `env_ids` (all by default) on base 0, then Reset: every episode starts drawn"""
    b = V.batch(arg, n, terrain_seed=terrain_seed, rand_seed=3, **mode, **more)
    pol = V.policy_for(om, arg)
    b.SetPolicy(pol[1], *pol[2:])
    b.SetExplore(*V.EXPLORE)
    b.CreateVariants(n_variants)
    b.VariantRescale(0, env_ids=env_ids, seed=seed, per_link=per_link, **ranges)
    if reset:
        b.Reset()
    return b


def check_factors(b, per_link, ranges=RANGES, seed=RESCALE_SEED, base=0, what=""):
    """The reported factors of every env under its private key are the restatement's at episodes - 1, bit for bit, and inside their ranges."""
    info = b.VariantRescaleInfo()
    L = b.L
    for e in range(b.num_envs):
        if info["key"][e] != b.num_variants + e or info["episodes"][e] == 0:
            assert same_bits(info["factors"][e], np.ones((4, L))), (what, e)
            continue
        want = py_factors(seed, base + e, int(info["episodes"][e]) - 1, L, ranges, per_link)
        assert same_bits(info["factors"][e], want), (what, e, info["factors"][e], want)
        for q, name in enumerate(QUANT):
            lo, hi = ranges.get(name) or (1.0, 1.0)
            assert np.all(info["factors"][e][q] >= lo) and np.all(info["factors"][e][q] <= hi), (what, e, name)
            if name not in per_link:
                assert len(set(info["factors"][e][q])) == 1, (what, e, name)
    return info


# ---- 1. the rule against the restatement ----
@pytest.mark.parametrize("mode", T.MODES, ids=T.MODE_IDS)
def test_factors_equal_the_restatement(da, om, mode, n=6, frames=20):
    per_link = ("mass", "kp")
    ranges = dict(RANGES, kd=(1.3, 1.3))           # lo == hi: exactly that factor
    a = rescaled(om, DOG, n, mode, per_link=per_link, ranges=ranges, reset=False)
    info = check_factors(a, per_link, ranges, what="joined, no episode yet")
    assert list(info["key"]) == [1 + e for e in range(n)] and list(a.GetVariants()) == [1 + e for e in range(n)] and list(info["episodes"]) == [0] * n
    assert info["base"] == 0 and info["seed"] == RESCALE_SEED and info["per_link"] == per_link and info["ranges"] == {k: tuple(map(float, v)) for k, v in ranges.items()}
    a.Reset()
    info = check_factors(a, per_link, ranges, what="after Reset")
    assert list(info["episodes"]) == [1] * n
    assert np.all(info["factors"][:, 2, :] == 1.3)
    assert len({f.tobytes() for f in info["factors"]}) == n                      # every env its own draw
    assert all(len(set(info["factors"][e][0])) == a.L for e in range(n))       # per-link masses differ link by link
    # the uniform / per-link switch of one quantity leaves every other quantity's factors where they were (and the switched one's link 0)
    u = rescaled(om, DOG, n, mode, per_link=("mass",), ranges=ranges)
    fu = check_factors(u, ("mass",), ranges, what="kp uniform")["factors"]
    assert same_bits(fu[:, [0, 2, 3], :], info["factors"][:, [0, 2, 3], :]) and same_bits(fu[:, 1, 0], info["factors"][:, 1, 0])
    assert not same_bits(fu[:, 1, :], info["factors"][:, 1, :])
    # a second episode draws at n + 1: a fall (found by running: TERRAIN_SEED), and Reset naming an env twice counts once
    r0 = resets(a)
    for f in range(frames):
        a.Update()
    fell = resets(a) - r0
    info = check_factors(a, per_link, ranges, what="after %d frames" % frames)
    assert list(info["episodes"]) == list(1 + fell) and fell.sum() >= 1, (info["episodes"], fell)
    a.Reset([2, 2, 5])
    info2 = check_factors(a, per_link, ranges, what="after Reset([2, 2, 5])")
    assert list(info2["episodes"] - info["episodes"]) == [1 if e in (2, 5) else 0 for e in range(n)]


@pytest.mark.parametrize("mode", T.MODES, ids=T.MODE_IDS)
def test_shard_invariance(da, om, mode, n=6, frames=20):
    """6 envs in one batch against two batches of 3, the second with the global-id offset the sharding glue passes at creation: factors and trajectories, bitwise."""
    whole = rescaled(om, DOG, n, mode)
    lo = rescaled(om, DOG, 3, mode)
    hi = rescaled(om, DOG, 3, mode, global_env_offset=3)
    for _ in range(frames):
        for b in (whole, lo, hi):
            b.Update()
    iw, il, ih = check_factors(whole, ("mass", "kp")), check_factors(lo, ("mass", "kp")), check_factors(hi, ("mass", "kp"), base=3)
    assert list(iw["episodes"]) == list(il["episodes"]) + list(ih["episodes"]) and iw["episodes"].max() >= 2, (iw["episodes"], il["episodes"], ih["episodes"])
    assert same_bits(iw["factors"], np.concatenate([il["factors"], ih["factors"]]))
    ow, ol, oh = X.observe(whole, range(n)), X.observe(lo, range(3)), X.observe(hi, range(3))
    for g in range(n):
        (sa, pa, ga), (sb, pb, gb) = ow[g], (ol[g] if g < 3 else oh[g - 3])
        bad = X.same_record(sa, sb)
        assert bad is None, "global env %d: EnvState.%s differs between the shard and the whole batch" % (g, bad)
        assert pa.tobytes() == pb.tobytes() and ga == gb, g
        assert same_bits(whole.VariantScalars(g)[0]["mass"], (lo if g < 3 else hi).VariantScalars(g % 3)[0]["mass"])


# ---- 2. the records against the loader ----
def names_of(arg):
    doc = V.nominal_doc(arg)
    return [b["Name"] for b in doc["BodyDefs"]], [p["Name"] for p in doc["PDControllers"]]


def load_scaled(b, v, factors, arg):
    """variant v of b = the character file under the factors [4][L], through the JSON loader"""
    bodies, joints = names_of(arg)
    by = lambda names, row: {nm: float(f) for nm, f in zip(names, row)}
    b.ScaledVariant(v, mass=by(bodies, factors[0]), kp=by(joints, factors[1]), kd=by(joints, factors[2]), torque_lim=by(joints, factors[3]))


def assert_scalars_equal(a, ea, b, eb, what):
    (sa, ta), (sb, tb) = a.VariantScalars(ea), b.VariantScalars(eb)
    for k in sa:
        assert same_bits(sa[k], sb[k]), (what, k, sa[k], sb[k])
    assert same_bits(ta, tb), (what, "total_mass", ta, tb)


def transplant(a, e, dst):
    """env e of `a` as it stands into slot e of `dst`, through a blob"""
    s = a.SaveState([e])
    blob = s.export(); s.free()
    t = dst.ImportState(blob)
    dst.RestoreState(t, [e]); t.free()


def run_records_equal_the_loader(om, arg, mode, n=6, warm=WARM, frames=3, terrain_seed=TERRAIN_SEED, fall_env=FALL_ENV, **more):
    """A: n envs under the rescale, per_link mass and kp. B: the same envs, env e under variant e + 1 = ScaledVariant under A's reported factors (one env more than
    A: a table may hold num_envs variants, and variant 0 is the batch's own model). Both start from Reset and run `warm` frames, then the three frames the
    issue asks for, which hold a fall and a redraw of A (TERRAIN_SEED). After every frame poses and velocities of all envs are equal, bit for bit; the scalars
    of the two records are equal whenever they are (re)loaded. An env of A that fell has drawn new scales in front of its reset: B's variant is loaded again
    from the newly reported factors, and A's env goes into B's slot as it stands (B's own reset ran under the old model and left that model's centre of mass
    in prev_com, the one field reset_env derives from the masses), so the frames behind the fall compare the new episode under the two records."""
    a = rescaled(om, arg, n, mode, terrain_seed=terrain_seed, **more)
    b = V.batch(arg, n + 1, terrain_seed=terrain_seed, rand_seed=3, **mode, **more)
    pol = V.policy_for(om, arg)
    b.SetPolicy(pol[1], *pol[2:])
    b.SetExplore(*V.EXPLORE)
    b.CreateVariants(n + 1)
    info = check_factors(a, ("mass", "kp"), what="A after Reset")
    for e in range(n):
        load_scaled(b, e + 1, info["factors"][e], arg)
    b.AssignVariants(range(n), [e + 1 for e in range(n)])
    b.Reset()
    for e in range(n):
        assert_scalars_equal(a, e, b, e, "env %d, first episode" % e)
    V.assert_envs_equal(a, b, range(n), "after Reset")
    redrawn, after_redraw = 0, 0
    episodes = info["episodes"].copy()
    for f in range(warm + frames):
        a.Update(); b.Update()
        (qa, qda), (qb, qdb) = a.PoseVel(), b.PoseVel(list(range(n)))
        assert same_bits(qa, qb) and same_bits(qda, qdb), "frame %d: poses or velocities differ" % f
        info = check_factors(a, ("mass", "kp"), what="frame %d" % f)
        moved = [e for e in range(n) if info["episodes"][e] != episodes[e]]
        after_redraw += redrawn > 0 and f >= warm
        V.assert_envs_equal(a, b, [e for e in range(n) if e not in moved], "frame %d" % f)
        for e in moved:
            assert f >= warm, "env %d fell in warm-up frame %d: choose another terrain seed" % (e, f)
            load_scaled(b, e + 1, info["factors"][e], arg)
            assert_scalars_equal(a, e, b, e, "env %d, episode %d" % (e, info["episodes"][e]))
            transplant(a, e, b)
            redrawn += 1
        episodes = info["episodes"].copy()
    print(dict(redrawn=redrawn, frames_behind_a_redraw=int(after_redraw), episodes=list(map(int, episodes))))
    assert redrawn >= 1 and after_redraw >= 1 and (fall_env is None or episodes[fall_env] == 2), (redrawn, after_redraw, episodes)


@pytest.mark.parametrize("mode", T.MODES, ids=T.MODE_IDS)
def test_records_equal_the_loader(da, om, mode):
    run_records_equal_the_loader(om, DOG, mode)


def test_records_equal_the_loader_f32(da, om):
    """The fp32 library writes the `real` bits its own loader loads: scalars only (a handful of envs, first episode and one Reset)."""
    mode = dict(physics_precision="f32")
    n = 5
    a = rescaled(om, DOG, n, mode)
    b = V.batch(DOG, n + 1, terrain_seed=TERRAIN_SEED, rand_seed=3, **mode)
    b.CreateVariants(n + 1)
    for rnd in range(2):
        info = check_factors(a, ("mass", "kp"))
        for e in range(n):
            load_scaled(b, e + 1, info["factors"][e], DOG)
        b.AssignVariants(range(n), [e + 1 for e in range(n)])
        for e in range(n):
            assert_scalars_equal(a, e, b, e, "fp32, env %d, round %d" % (e, rnd))
            m = a.VariantScalars(e)[0]["mass"]
            assert same_bits(m, m.astype(np.float32).astype(np.float64))        # `real` is float here
        a.Reset()


# ---- 3. envs outside the rescale ----
@pytest.mark.parametrize("mode", T.MODES, ids=T.MODE_IDS)
def test_envs_outside_the_rescale_are_untouched(da, om, tmp_path, mode, n=7, frames=25):
    """Envs 0, 1 under the rescale (base 0), envs 2 .. 4 under ordinary variants 1 / 2 inside a redraw 1 .. 2, envs 5, 6 under variant 0. Against the same batch
    without the rescale, envs 2 .. 6 run bitwise the same -- through falls and a Reset that names envs of all three kinds -- and the redraw draws the same;
    against the same batch without the redraw, the rescale's envs do."""
    paths = V.write_variants(tmp_path, DOG)
    assign = [0, 0, 1, 2, 1, 0, 0]

    def make(rescale, redraw):
        b = V.with_variants(om, DOG, n, paths, assign, dict(terrain_seed=TERRAIN_SEED, rand_seed=3, **mode))
        if redraw:
            b.VariantRedraw(1, 2, seed=5)
        if rescale:
            b.VariantRescale(0, env_ids=[0, 1], seed=RESCALE_SEED, per_link=("mass",), **RANGES)
        b.Reset()
        return b
    both, only_redraw, only_rescale = make(True, True), make(False, True), make(True, False)
    assert list(both.GetVariants())[:2] == [3, 4]                                  # V + e
    assert all(1 <= v <= 2 for v in both.GetVariants()[2:5]) and list(both.GetVariants()[5:]) == [0, 0]
    r0 = resets(both)
    for f in range(frames):
        for b in (both, only_redraw, only_rescale):
            b.Update()
            if f == frames // 2:
                b.Reset([1, 3, 6])
        V.assert_envs_equal(both, only_redraw, range(2, n), "frame %d, against the batch without the rescale" % f)
        V.assert_envs_equal(both, only_rescale, range(2), "frame %d, against the batch without the redraw" % f)
    ia, ib = both.VariantRedrawInfo(), only_redraw.VariantRedrawInfo()
    assert list(ia["variant"][2:]) == list(ib["variant"][2:]) and list(ia["draws"]) == list(ib["draws"]) and list(ia["draws"][:2]) == [0, 0], (ia, ib)
    assert ia["draws"].sum() >= 4 and list(ia["variant"][:2]) == [3, 4]
    ra, rb = check_factors(both, ("mass",)), check_factors(only_rescale, ("mass",))
    assert list(ra["episodes"]) == list(rb["episodes"]) and list(ra["episodes"][2:]) == [0] * (n - 2) and ra["episodes"][1] >= 2, (ra, rb)
    assert (resets(both) - r0)[[1, 3, 6]].min() >= 1
    assert [both.VariantStats(v)["n_envs"] for v in range(3)] == [list(ia["variant"]).count(v) for v in range(3)]   # (keeps its range: private keys count nowhere)
    V.refused(da, lambda: both.VariantStats(3), "out of range")
    # the user cannot assign a private key; assigning an ordinary variant takes the env out
    V.refused(da, lambda: both.AssignVariants([0], [3]), "variant 3", "out of range")
    both.AssignVariants([0], [1])
    assert list(both.GetVariants())[:2] == [1, 4]
    ep0 = both.VariantRescaleInfo()["episodes"][0]
    both.VariantRedraw(1, 0)
    both.Reset([0, 1])
    info = check_factors(both, ("mass",))
    assert info["episodes"][0] == ep0 and info["episodes"][1] == ra["episodes"][1] + 1 and info["key"][0] == 1
    ref = V.with_variants(om, DOG, n, paths, [1] * n, dict(terrain_seed=TERRAIN_SEED, rand_seed=3, **mode))
    for k, row in both.VariantScalars(0)[0].items():
        assert same_bits(row, ref.VariantScalars(0)[0][k]), k
    com, _, _ = both.LinkStates([1])                                               # (ModelOf: a private key reads the base's geometry)
    assert np.isfinite(com).all()


# ---- 4. refusals ----
def test_refusals(da, om, tmp_path, n=4):
    """Every refusal is DTRL_ERR_ARG, names its argument and changes nothing."""
    pol = V.policy_for(om, DOG)
    b = V.batch(DOG, n, terrain_seed=11)
    b.SetPolicy(pol[1], *pol[2:])
    V.refused(da, lambda: b.VariantRescale(0), "no model variants")
    V.refused(da, lambda: b.VariantRescaleInfo(), "no model variants")
    assert same_bits(b.VariantScalars(0)[0]["mass"], [x["Mass"] for x in V.nominal_doc(DOG)["BodyDefs"]])   # (any env, variants or not)
    V.refused(da, lambda: b.VariantScalars(n), "env id", "out of range")
    b.CreateVariants(3)
    b.LoadVariant(1, V.write_variants(tmp_path, DOG)[1])
    V.refused(da, lambda: b.VariantRescaleInfo(), "no variant rescale")
    V.refused(da, lambda: b.VariantRescale(3), "base 3", "out of range")
    V.refused(da, lambda: b.VariantRescale(-1), "base -1", "out of range")
    V.refused(da, lambda: b.VariantRescale(2), "base", "variant 2", "is empty")
    nan, inf = float("nan"), float("inf")
    V.refused(da, lambda: b.VariantRescale(0, mass=(0.0, 1.0)), "mass", "greater than 0")
    V.refused(da, lambda: b.VariantRescale(0, kp=(-1.0, 1.0)), "kp", "greater than 0")
    V.refused(da, lambda: b.VariantRescale(0, kd=(1.2, 1.1)), "kd", "exceeds")
    V.refused(da, lambda: b.VariantRescale(0, torque_lim=(nan, 1.0)), "torque_lim", "finite")
    V.refused(da, lambda: b.VariantRescale(0, mass=(1.0, inf)), "mass", "finite")
    V.refused(da, lambda: b.VariantRescale(0, env_ids=[0, n]), "env id %d" % n, "out of range")
    V.refused(da, lambda: b.VariantRescale(0, env_ids=[-1]), "env id", "out of range")
    with pytest.raises(da.DtrlError):
        b.VariantRescale(0, per_link=("size",))
    V.refused(da, lambda: b.VariantRescaleInfo(), "no variant rescale")          # none of the refused calls turned it on
    assert list(b.GetVariants()) == [0] * n
    b.UpdateBegin()
    V.refused(da, lambda: b.VariantRescale(0), "frame is in flight")
    V.refused(da, lambda: b.VariantScalars(0), "frame is in flight")
    b.UpdateEnd()
    b.VariantRescale(1, env_ids=[0, 2], seed=3, mass=(0.8, 1.2))
    assert list(b.GetVariants()) == [3, 0, 5, 0]
    V.refused(da, lambda: b.LoadVariant(1, V.write_variants(tmp_path, DOG)[2]), "variant 1", "base of the variant rescale")
    V.refused(da, lambda: b.VariantRescale(0, env_ids=[], mass=(0.8, 1.2)), "base 0", "differs")
    V.refused(da, lambda: b.VariantRescale(1, mass=(2.0, 1.0)), "mass", "exceeds")   # a refused replacement leaves the rescale in place
    info = b.VariantRescaleInfo([2, 3])
    assert info["base"] == 1 and info["ranges"]["mass"] == (0.8, 1.2) and list(info["key"]) == [5, 0] and list(info["episodes"]) == [0, 0]
    V.refused(da, lambda: b.VariantRescaleInfo([n]), "out of range")
    b.VariantRescale(1, env_ids=[], seed=3, mass=(0.9, 1.1))                        # n = 0: the settings only
    assert b.VariantRescaleInfo()["ranges"]["mass"] == (0.9, 1.1) and list(b.GetVariants()) == [3, 0, 5, 0]
    b.UpdateBegin()
    V.refused(da, lambda: b.VariantRescaleInfo(), "frame is in flight")
    b.UpdateEnd()
    b.LoadVariant(2, V.write_variants(tmp_path, DOG)[2])                            # (any other variant may be loaded)


# ---- 5. state handling ----
def all_scalars(b):
    return [b.VariantScalars(e) for e in range(b.num_envs)]


def same_scalars(x, y):
    return all(same_bits(sa[k], sb[k]) for (sa, ta), (sb, tb) in zip(x, y) for k in sa) and all(same_bits(a[1], b[1]) for a, b in zip(x, y))


@pytest.mark.parametrize("mode", T.MODES, ids=T.MODE_IDS)
def test_batch_state_and_removal(da, om, mode, n=6, frames=20):
    a = rescaled(om, DOG, n, mode)
    snap = a.SaveState()
    for _ in range(frames):
        a.Update()
    info, rec = check_factors(a, ("mass", "kp")), all_scalars(a)
    assert info["episodes"].max() >= 2
    a.RestoreState(snap); snap.free()
    a.CloneEnvs([0, 1], [2, 3])
    after = check_factors(a, ("mass", "kp"), what="after RestoreState and CloneEnvs")
    assert list(after["episodes"]) == list(info["episodes"]) and list(after["key"]) == list(info["key"]) and same_bits(after["factors"], info["factors"])
    assert same_scalars(all_scalars(a), rec) and after["ranges"] == info["ranges"]
    # removal: the envs go back to the base, the counters stay
    a.VariantRescale(None)
    assert list(a.GetVariants()) == [0] * n
    V.refused(da, lambda: a.VariantRescaleInfo(), "no variant rescale")
    plain = V.batch(DOG, n, terrain_seed=TERRAIN_SEED, rand_seed=3, **mode)
    assert same_scalars(all_scalars(a), all_scalars(plain))
    b = rescaled(om, DOG, n, mode, reset=False)
    b.VariantRescale(None)
    V.hand_over(a, [b])
    for f in range(5):
        a.Update(); b.Update()
        V.assert_envs_equal(a, b, range(n), "after removal, frame %d" % f)
    a.VariantRescale(0, env_ids=[1, 4], seed=RESCALE_SEED, per_link=("mass", "kp"), **RANGES)   # back on: the counters were kept
    back = a.VariantRescaleInfo()
    assert list(back["episodes"]) == list(info["episodes"]) and list(back["key"]) == [0, 2, 0, 0, 5, 0]
    a.Reset([1])
    assert check_factors(a, ("mass", "kp"))["episodes"][1] == info["episodes"][1] + 1


# ---- 6. launches ----
def test_launch_counts(da, om, tmp_path, n=6, frames=20):
    """A batch without a rescale -- plain, or with variants -- advances the backend's launch counter exactly as before: per frame the group's one frame launch plus, on
    the check build (whose counter sees the 0-step launches too), one compact reset launch in a frame that ended with a fall; with K variants the per-key default
    makes that one launch per key in use. The counter counts FRAME-KERNEL launches only: the rule's own launch (one per group and frame, like the redraw's and the
    push schedule's) never passes it, on either backend, and a host wait cannot be seen through it at all. What it does show under a rescale is that the rule adds
    no frame-kernel launch of its own: the check build's count is the per-key default's -- one launch per private key, n a frame, plus one per env that fell."""
    emul = Scenario is EmulScenario
    extra = dict(terrain_seed=TERRAIN_SEED, rand_seed=3)
    b = V.plain(om, DOG, n, None, extra)
    bv = V.with_variants(om, DOG, n, V.write_variants(tmp_path, DOG), [0] * n, extra)
    a = rescaled(om, DOG, n, {})
    for x in (b, bv, a):
        x.KernelTimeMs()
    rb, ra = resets(b), resets(a)
    for f in range(frames):
        b.Update(); bv.Update(); a.Update()
        r1, r2 = resets(b), resets(a)
        want = 1 + (1 if (emul and (r1 != rb).any()) else 0)
        assert b.KernelTimeMs()[1] == want and bv.KernelTimeMs()[1] == want, "frame %d" % f
        assert a.KernelTimeMs()[1] == ((n + int((r2 != ra).sum())) if emul else 1), "frame %d" % f
        rb, ra = r1, r2
    assert (resets(a) > 0).any()


# ---- 7. the training loop ----
def run_train_loop_with_rescale(max_iters, max_frames, **more):
    """train_loop.train(..., rescale=...) on a tiny run: it creates the one-record table, puts every env but the held-out ones under the rescale and trains;
    greedy envs are refused. (Settings of tests/test_variant_redraw.py's loop test.)"""
    from deepterrainrl_amd import train_loop
    extra = {"terrain_seed": 3, "trainer_num_init_samples": 10, "trainer_replay_mem_size": 512, "trainer_freeze_target_iters": 4,
             "init_exp_rate": 0.3, "init_exp_base_rate": 0.1, "trainer_init_input_offset_scale": "false"}
    n = 32
    kw = dict(num_envs=n, seed=1, scenario_cls=Scenario, trainer="hip", extra_args=extra, **more)
    spec = dict(mass=(0.8, 1.2), torque_lim=(0.6, 1.2), kp=(0.9, 1.1), per_link=("mass",), seed=3, hold_out=[0, n - 1])
    out = train_loop.train(V.TRAIN, REFDATA, max_iters=max_iters, max_frames=max_frames, rescale=spec, **kw)
    info = out["rescale"]
    print(dict(frames=out["frames"], iters=out["iters"], episodes=int(info["episodes"].sum())))
    assert info["hold_out"] == [0, n - 1] and list(info["key"][[0, n - 1]]) == [0, 0] and list(info["key"][1:n - 1]) == [1 + e for e in range(1, n - 1)], info
    assert list(info["episodes"][[0, n - 1]]) == [0, 0] and info["episodes"][1:n - 1].min() >= 1 and info["episodes"].sum() >= n - 2 + 3, info   # episodes ended, the next ones drew afresh
    f = info["factors"][1:n - 1]
    assert np.all(f[:, 0] >= 0.8) and np.all(f[:, 0] <= 1.2) and np.all(f[:, 3] >= 0.6) and np.all(f[:, 3] <= 1.2) and np.all(f[:, 2] == 1.0)
    assert np.all(np.isfinite(out["weights"]))
    with pytest.raises(ValueError, match="greedy_envs"):
        train_loop.train(V.TRAIN, REFDATA, max_iters=10, rescale=spec, greedy_envs=8, **kw)
    with pytest.raises(ValueError, match="unknown keys"):
        train_loop.train(V.TRAIN, REFDATA, max_iters=10, rescale=dict(size=(0.9, 1.1)), **kw)
    return out


def test_train_loop_with_rescale(da, om):
    """(32 dogs and 75 frames: the loop, the set-up and the returned record are what is checked here, and the check build's trainer step is slow)"""
    out = run_train_loop_with_rescale(None, 75, trainer_device="cpu", trainer_lib=os.path.join(os.path.dirname(__file__), "emul", "libdtrl_trainer_emul.so"))
    assert out["frames"] >= 75 and out["iters"] >= 1, (out["frames"], out["iters"])
