"""Model variants (include/dtrl.h dtrl_variants_create ...): several character models in one batch, one per env. The yardstick is always the single-model path:
env e of a K-variant batch, sitting in variant v, must equal -- bit for bit, every field of its EnvState record, its policy state, its ground window and build
count -- env e of a plain batch of the same size, arguments and seeds that was created with variant v's character file and continues from the same state.
Runs on the lane-loop check build of the kernel source (tests/emul: the per-key default of Backend::LaunchKeyed); tests/test_gpu_model_variants.py points
`Scenario` at the product library (one launch of the variant kernels). The variant character files are written at run time from the committed nominal ones."""
import copy
import json
import os

import numpy as np
import pytest

import test_external_policy as X          # env_states / same_record / ground_key / observe: helpers that take a batch
import test_host_and_emul as H
from conftest import REFDATA, EmulScenario, dog_policy, emul_f32_scenario

Scenario = EmulScenario   # the GPU twin points this at the product class

DOG, RAPTOR, TRAIN = "args/dog_slopes_mixed_args.txt", "args/raptor_narrow_gaps_args.txt", "args/opt_args_train_mace.txt"
EXPLORE = (1, 0.5, 0.25, 0.1)


def batch(arg, n, **extra):
    if extra.get("physics_precision") == "f32" and Scenario is EmulScenario:
        return emul_f32_scenario(arg, n, data_root=REFDATA, extra_args=extra)
    return Scenario(arg, n, data_root=REFDATA, extra_args=extra)


def policy_for(om, arg):
    return H.raptor_policy(om) if "raptor" in arg else dog_policy(om)


def nominal_doc(arg):
    with open(os.path.join(REFDATA, "data/characters", "raptor.txt" if "raptor" in arg else "dog.txt")) as f:
        return json.load(f)


def scale(doc, mass=None, param0=None, param1=None, kp=1.0, kd=1.0, torque_lim=1.0):
    """A copy of a character description with body masses / box sizes scaled by name and every PD controller's gains and torque limit scaled."""
    d = copy.deepcopy(doc)
    for b in d["BodyDefs"]:
        b["Mass"] = b["Mass"] * (mass or {}).get(b["Name"], 1.0)
        b["Param0"] = b["Param0"] * (param0 or {}).get(b["Name"], 1.0)
        b["Param1"] = b["Param1"] * (param1 or {}).get(b["Name"], 1.0)
    for pd in d["PDControllers"]:
        pd["Kp"] = pd["Kp"] * kp; pd["Kd"] = pd["Kd"] * kd; pd["TorqueLim"] = pd["TorqueLim"] * torque_lim
    return d


def variant_docs(arg):
    """[v1, v2] of the scene's character. Dog v2 changes box sizes too, so that contact points, margins, breaking thresholds and pair boxes differ."""
    doc = nominal_doc(arg)
    names = [b["Name"] for b in doc["BodyDefs"]]
    if "raptor" in arg:
        return [scale(doc, mass={names[0]: 1.25}, torque_lim=0.8, kp=0.9),
                scale(doc, mass={names[-2]: 1.5, names[-1]: 1.5}, kp=0.7, kd=1.2)]
    return [scale(doc, mass={"torso": 1.3, "head": 1.2}, torque_lim=0.8),
            scale(doc, mass={"toe": 2.0, "finger": 2.0, "foot": 1.5, "hand": 1.5}, kp=0.7, kd=1.2, param0={"toe": 1.2, "finger": 1.2}, param1={"torso": 1.15})]


def write_doc(tmp_path, name, doc):
    p = tmp_path / name
    p.write_text(json.dumps(doc))
    return str(p)


def write_variants(tmp_path, arg):
    """[None (the nominal model), path of v1, path of v2]"""
    return [None] + [write_doc(tmp_path, "v%d.txt" % (k + 1), d) for k, d in enumerate(variant_docs(arg))]


def plain(om, arg, n, path, extra):
    """A single-model batch created with the variant's file as -character_file= (None: the nominal one)."""
    x = dict(extra)
    if path is not None:
        x["character_file"] = path
    b = batch(arg, n, **x)
    pol = policy_for(om, arg)
    b.SetPolicy(pol[1], *pol[2:])
    b.SetExplore(*EXPLORE)
    return b


def with_variants(om, arg, n, paths, assign, extra):
    b = batch(arg, n, **extra)
    pol = policy_for(om, arg)
    b.SetPolicy(pol[1], *pol[2:])
    b.SetExplore(*EXPLORE)
    b.CreateVariants(len(paths))
    assert b.num_variants == len(paths) and list(b.GetVariants()) == [0] * n
    for v in range(1, len(paths)):
        b.LoadVariant(v, paths[v])
    b.AssignVariants(None, assign)
    assert list(b.GetVariants()) == list(assign)
    return b


def hand_over(src, dsts):
    """Every env of `src` as it stands, into every batch of `dsts` (a blob: its header does not depend on the model)."""
    snap = src.SaveState()
    blob = snap.export(); snap.free()
    for d in dsts:
        s = d.ImportState(blob); d.RestoreState(s); s.free()


def assert_envs_equal(bs, ref, envs, what):
    """Envs `envs` of batch bs against the same envs of batch ref."""
    envs = list(envs)
    if not envs:
        return
    oa, ob = X.observe(bs, envs), X.observe(ref, envs)
    for e in envs:
        (sa, pa, ga), (sb, pb, gb) = oa[e], ob[e]
        bad = X.same_record(sa, sb)
        assert bad is None, "%s: env %d: EnvState.%s differs from the single-model run" % (what, e, bad)
        assert pa.tobytes() == pb.tobytes(), "%s: env %d: policy state differs" % (what, e)
        assert ga == gb, "%s: env %d: ground window / build count differs" % (what, e)


EQUAL_CASES = [(DOG, dict(terrain_seed=11)), (RAPTOR, dict(terrain_seed=5)), (DOG, dict(terrain_seed=11, terrain_gen="device")), (RAPTOR, dict(terrain_seed=5, terrain_gen="device"))]
EQUAL_IDS = ["dog", "raptor", "dog_device_terrain", "raptor_device_terrain"]


def run_equals_single_model(om, tmp_path, arg, extra, n=12, frames=45, reassign_at=12):
    """Tests 1 and 2 in one walk. A: 12 envs round-robin over (nominal, v1, v2); after 3 frames its state goes into three plain batches P0 / P1 / P2, one per
    model; for 45 frames every env of A equals the same env of its variant's plain batch. At frame 12 half of variant 0's envs move to v1: their records do not
    change by the call, and from there on they equal a fourth plain batch of v1 that took A's state at that moment."""
    paths = write_variants(tmp_path, arg)
    assign = [e % 3 for e in range(n)]
    a = with_variants(om, arg, n, paths, assign, extra)
    for _ in range(3):
        a.Update()
    refs = [plain(om, arg, n, paths[v], extra) for v in range(3)]
    hand_over(a, refs)
    for v in range(3):
        assert_envs_equal(a, refs[v], range(n), "after the hand-over, P%d" % v)
    c0 = X.env_states(a)["num_cycles"].copy()
    moved, late, c_at = [e for e in range(n) if assign[e] == 0][::2], None, None
    for f in range(frames):
        if f == reassign_at:
            before = X.observe(a, moved)
            a.AssignVariants(moved, [1] * len(moved))
            assert list(a.GetVariants(moved)) == [1] * len(moved)
            after = X.observe(a, moved)
            for e in moved:
                assert X.same_record(before[e][0], after[e][0]) is None and before[e][1].tobytes() == after[e][1].tobytes() and before[e][2] == after[e][2], "env %d changed by the reassignment" % e
            late = plain(om, arg, n, paths[1], extra)
            hand_over(a, [late])
            c_at = X.env_states(a)["num_cycles"].copy()
        a.Update()
        for r in refs:
            r.Update()
        if late is not None:
            late.Update()
            assert_envs_equal(a, late, moved, "frame %d, moved envs" % f)
        for v in range(3):
            assert_envs_equal(a, refs[v], [e for e in range(n) if assign[e] == v and (late is None or e not in moved)], "frame %d variant %d" % (f, v))
    st = X.env_states(a)
    for v in range(3):   # otherwise the comparison shows nothing
        assert any(st["num_cycles"][e] > c0[e] for e in range(n) if assign[e] == v and e not in moved), "no env of variant %d made a decision" % v
    assert any(st["num_cycles"][e] > c_at[e] for e in moved), "no moved env made a decision under its new model"
    assert st["num_resets"].sum() >= 1, "the run saw no reset"
    q0 = X.env_states(refs[0])["q"]
    for e in range(n):
        if assign[e] != 0 or e in moved:
            assert st["q"][e].tobytes() != q0[e].tobytes(), "env %d (variant %d) ends where the nominal model ends: the variant changed nothing" % (e, a.GetVariants([e])[0])
    return a


@pytest.mark.parametrize("arg,extra", EQUAL_CASES, ids=EQUAL_IDS)
def test_equals_single_model_runs(da, om, tmp_path, arg, extra):
    """1, 2. 12 envs round-robin over 3 models, 45 frames, a reassignment at frame 12: every frame, every env equals its single-model run."""
    run_equals_single_model(om, tmp_path, arg, extra)


def drain_into(b, tuples):
    rows, fl, ids = b.DrainTuples()
    for r, x, e in zip(rows, fl, ids):
        tuples[int(e)].append((r.tobytes(), int(x)))


def test_exp_scenario_tuples(da, om, tmp_path, n=12, frames=45):
    """3. The MACE training scene (cScenarioExp), 2 variants: per env, the drained rows and flag words are the single-model run's, in order."""
    extra = dict(terrain_seed=74, rand_seed=2)
    paths = write_variants(tmp_path, TRAIN)[:2]
    assign = [e % 2 for e in range(n)]
    a = with_variants(om, TRAIN, n, paths, assign, extra)
    for _ in range(3):
        a.Update()
    refs = [plain(om, TRAIN, n, paths[v], extra) for v in range(2)]
    for b in [a] + refs:
        b.DrainTuples()
    hand_over(a, refs)
    ts = {e: [] for e in range(n)}
    tr = [{e: [] for e in range(n)} for _ in range(2)]
    for f in range(frames):
        a.Update(); drain_into(a, ts)
        for v in range(2):
            refs[v].Update(); drain_into(refs[v], tr[v])
    total = 0
    for e in range(n):
        assert ts[e] == tr[assign[e]][e], "env %d (variant %d): tuples differ (%d / %d rows)" % (e, assign[e], len(ts[e]), len(tr[assign[e]][e]))
        total += len(ts[e])
    assert total >= n, total
    for v in range(2):
        assert_envs_equal(a, refs[v], [e for e in range(n) if assign[e] == v], "end, variant %d" % v)
        assert sum(len(ts[e]) for e in range(n) if assign[e] == v) > 0, "variant %d wrote no tuple" % v
    assert any(ts[e] != tr[0][e] for e in range(n) if assign[e] == 1), "variant 1's envs wrote the nominal model's tuples"


def check_variant_stats(b, n_variants):
    st = X.env_states(b)
    var = b.GetVariants()
    ev = b.EvalStats()
    tot = dict(n_envs=0, episodes=0, cycles=0, resets=0); dist = 0.0
    for v in range(n_variants):
        got = b.VariantStats(v)
        again = b.VariantStats(v)
        assert got == again and np.float64(got["avg_dist"]).tobytes() == np.float64(again["avg_dist"]).tobytes(), "variant %d: two calls differ" % v
        m = var == v
        ep = int(st["num_episodes"][m].sum())
        assert (got["n_envs"], got["episodes"], got["cycles"], got["resets"]) == (int(m.sum()), ep, int(st["num_cycles"][m].sum()), int(st["num_resets"][m].sum())), (v, got)
        want = float((st["avg_dist"][m].astype(np.float64) * st["num_episodes"][m]).sum() / ep) if ep else 0.0
        assert abs(got["avg_dist"] - want) <= 1e-12 * abs(want), (v, got["avg_dist"], want)    # (another summation order)
        for k in tot:
            tot[k] += got[k]
        dist += got["avg_dist"] * got["episodes"]
    assert (tot["n_envs"], tot["episodes"], tot["cycles"], tot["resets"]) == (b.num_envs, ev["episodes"], ev["cycles"], ev["resets"])
    got = dist / tot["episodes"] if tot["episodes"] else 0.0
    assert abs(got - ev["avg_dist"]) <= 1e-12 * abs(ev["avg_dist"]), (got, ev["avg_dist"])
    return tot


def test_variant_stats(da, om, tmp_path, n=12, frames=45):
    """4. dtrl_variant_stats equals a host-side reduction over the EnvState records split by GetVariants(), is the same over two calls, and summed over the
    variants it is dtrl_eval_stats."""
    paths = write_variants(tmp_path, DOG)
    b = with_variants(om, DOG, n, paths, [e % 3 for e in range(n)], dict(terrain_seed=11))
    for f in range(frames):
        b.Update()
    tot = check_variant_stats(b, 3)
    assert tot["cycles"] > 0 and tot["episodes"] > 0, tot


def test_variant_stats_more_variants_than_one_window(da, om, n=70, frames=3):
    """One model per env, 70 envs: the reduction takes the table in windows of 32 variants; variant v holds exactly env v."""
    b = batch(DOG, n, terrain_seed=11)
    pol = policy_for(om, DOG)
    b.SetPolicy(pol[1], *pol[2:])
    b.CreateVariants(n)
    rng = np.random.RandomState(5)
    for v in range(1, n):
        b.ScaledVariant(v, mass=float(rng.uniform(0.8, 1.2)), torque_lim=float(rng.uniform(0.8, 1.2)))
    b.AssignVariants(None, list(range(n)))
    for f in range(frames):
        b.Update()
    tot = check_variant_stats(b, n)
    assert tot["n_envs"] == n


def geometry_doc():
    """A dog whose attach points and root body angle differ: what the host-side readers of per-env geometry (dtrl_get_link_states, dtrl_add_perturb) read."""
    d = copy.deepcopy(nominal_doc(DOG))
    for b in d["BodyDefs"]:
        if b["Name"] == "root":
            b["Theta"] = b["Theta"] + 0.05
        if b["Name"] == "torso":
            b["AttachX"] = b["AttachX"] * 1.2
    for j in d["Skeleton"]["Joints"]:
        if j["Name"] == "spine0":
            j["AttachX"] = j["AttachX"] * 1.1
    return d


def test_batch_state_and_host_readers(da, om, tmp_path, n=8, frames=6):
    """5. The assignment is batch state: snapshot / restore / clone / Reset leave it as it was set. dtrl_get_link_states and dtrl_add_perturb read the env's
    own model: on an env of v2, and of a variant with other attach points and another root body angle, they agree with the plain batch of that model."""
    extra = dict(terrain_seed=11)
    paths = write_variants(tmp_path, DOG) + [write_doc(tmp_path, "geom.txt", geometry_doc())]
    assign = [e % 4 for e in range(n)]
    a = with_variants(om, DOG, n, paths, assign, extra)
    for f in range(3):
        a.Update()
    refs = [plain(om, DOG, n, paths[v], extra) for v in range(4)]
    hand_over(a, refs)
    link = np.zeros(n, np.int32); force = np.tile([40.0, 15.0], (n, 1)); dur = np.full(n, 0.2); lp = np.tile([0.05, 0.02], (n, 1))
    for b in [a] + refs:
        b.AddPerturb(link, force, dur, local_pos=lp)
    sa = X.env_states(a)
    for v in (2, 3):
        envs = [e for e in range(n) if assign[e] == v]
        assert_envs_equal(a, refs[v], envs, "after AddPerturb, variant %d" % v)
    e3 = assign.index(3)
    assert sa["pert_lp"][e3].tobytes() != X.env_states(refs[0])["pert_lp"][e3].tobytes(), "the perturbation offset did not see the variant's body angle"
    for f in range(frames):
        a.Update()
        for r in refs:
            r.Update()
    la = a.LinkStates()
    for v in range(4):
        lr = refs[v].LinkStates()
        for e in range(n):
            if assign[e] == v:
                assert all(x[e].tobytes() == y[e].tobytes() for x, y in zip(la, lr)), "LinkStates of env %d (variant %d) differ from the plain batch's" % (e, v)
    # (same state, other model: the nominal reader would have answered otherwise)
    q, qd = a.PoseVel([e3])
    refs[0].SetPoseVel(q, qd, env_ids=[e3])
    assert any(x[e3].tobytes() != y[e3].tobytes() for x, y in zip(la, refs[0].LinkStates())), "LinkStates did not see the variant's attach points"
    one = a.LinkStates([e3])
    assert all(x[0].tobytes() == y[e3].tobytes() for x, y in zip(one, la))
    # snapshots, clones and resets
    before = a.SaveState()
    a.AssignVariants([0, 5], [2, 0])
    want = list(assign); want[0] = 2; want[5] = 0
    a.RestoreState(before); before.free()
    assert list(a.GetVariants()) == want
    a.CloneEnvs([1], [2])
    assert list(a.GetVariants()) == want
    a.Reset([2, 3])
    assert list(a.GetVariants()) == want
    a.Update()


def test_scaled_variant_equals_the_file(da, om, tmp_path, n=4, frames=8):
    """BatchScenario.ScaledVariant(mass={...}, torque_lim=) builds dog v1 in memory: the same bits as the file."""
    extra = dict(terrain_seed=11)
    paths = write_variants(tmp_path, DOG)[:2]
    a = with_variants(om, DOG, n, paths, [1] * n, extra)
    b = batch(DOG, n, **extra)
    pol = policy_for(om, DOG)
    b.SetPolicy(pol[1], *pol[2:]); b.SetExplore(*EXPLORE)
    assert os.path.samefile(b.CharacterFile(), os.path.join(REFDATA, "data/characters/dog.txt"))
    b.CreateVariants(2)
    text = b.ScaledVariant(1, mass={"torso": 1.3, "head": 1.2}, torque_lim=0.8)
    assert json.loads(text) == variant_docs(DOG)[0]
    b.AssignVariants(None, [1] * n)
    for f in range(frames):
        a.Update(); b.Update()
    assert_envs_equal(a, b, range(n), "ScaledVariant against LoadVariant")
    with pytest.raises(da.DtrlError):
        b.ScaledVariant(1, mass={"no_such_body": 2.0})


def refused(da, fn, *words, code="(1)"):
    with pytest.raises(da.DtrlError) as ei:
        fn()
    msg = str(ei.value)
    assert code in msg, msg                                        # DTRL_ERR_ARG unless stated
    for w in words:
        assert w in msg, (w, msg)


def test_refusals(da, om, tmp_path, n=4):
    """6. Every refusal is DTRL_ERR_ARG with the reason in the message."""
    paths = write_variants(tmp_path, DOG)
    pol = policy_for(om, DOG)
    b = batch(DOG, n, policy_mode="external")
    refused(da, lambda: b.CreateVariants(2), "external")
    b = batch(DOG, n, terrain_seed=11)
    b.SetPolicy(pol[1], *pol[2:])
    b.CreateSlots(2)
    refused(da, lambda: b.CreateVariants(2), "policy slots")
    b = batch(DOG, n, terrain_seed=11)
    b.SetPolicy(pol[1], *pol[2:])
    refused(da, lambda: b.AssignVariants(None, [0] * n), "dtrl_variants_create")   # no variants yet
    refused(da, lambda: b.LoadVariant(1, paths[1]), "dtrl_variants_create")
    refused(da, lambda: b.GetVariants(), "dtrl_variants_create")
    refused(da, lambda: b.VariantStats(0), "dtrl_variants_create")
    refused(da, lambda: b.CreateVariants(0), "n_variants")
    refused(da, lambda: b.CreateVariants(n + 1), "n_variants")
    b.UpdateBegin()
    refused(da, lambda: b.CreateVariants(3), "dtrl_step_begin", "dtrl_step_end")
    b.UpdateEnd()
    b.CreateVariants(3)
    refused(da, lambda: b.CreateVariants(3), "already", "once")
    refused(da, lambda: b.CreateSlots(2), "model variants")
    refused(da, lambda: b.LoadVariant(3, paths[1]), "variant 3", "out of range")
    refused(da, lambda: b.LoadVariant(-1, paths[1]), "out of range")
    refused(da, lambda: b.LoadVariant(0, paths[1]), "variant 0", "own model")
    refused(da, lambda: b.VariantStats(3), "out of range")
    refused(da, lambda: b.AssignVariants(None, [0, 3, 0, 0]), "variant 3", "out of range")
    refused(da, lambda: b.AssignVariants(None, [0, 1, 0, 0]), "variant 1", "empty")
    assert list(b.GetVariants()) == [0] * n                                         # all or nothing
    refused(da, lambda: b.LoadVariant(1, str(tmp_path / "missing.txt")), "cannot open", code="(2)")   # DTRL_ERR_IO
    refused(da, lambda: b.LoadVariantJson(1, "{ not json"), code="(2)")
    doc = nominal_doc(DOG)
    short = copy.deepcopy(doc)                                                      # another joint count
    for key in ("BodyDefs", "PDControllers"):
        short[key] = short[key][:-1]
    short["Skeleton"]["Joints"] = short["Skeleton"]["Joints"][:-1]
    refused(da, lambda: b.LoadVariant(1, write_doc(tmp_path, "short.txt", short)), "does not fit", "L differs", "20")
    perm = copy.deepcopy(doc)                                                       # the same joints, another tree: tail0 hangs on spine0 instead of the root
    assert perm["Skeleton"]["Joints"][9]["Name"] == "tail0" and perm["Skeleton"]["Joints"][9]["Parent"] == 0
    perm["Skeleton"]["Joints"][9]["Parent"] = 1
    refused(da, lambda: b.LoadVariant(1, write_doc(tmp_path, "perm.txt", perm)), "does not fit", "parent")
    acts = copy.deepcopy(doc)
    acts["Controllers"]["Actions"][1]["Blend"] = 0.5
    refused(da, lambda: b.LoadVariantJson(1, json.dumps(acts)), "does not fit", "act_blend")
    acts = copy.deepcopy(doc)
    acts["Controllers"]["Actions"] = acts["Controllers"]["Actions"][:-1]
    refused(da, lambda: b.LoadVariantJson(1, json.dumps(acts)), "does not fit", "n_actions")
    refused(da, lambda: b.AssignVariants(None, [0, 1, 0, 0]), "variant 1", "empty")    # a refused load leaves the variant empty
    b.LoadVariant(1, paths[1]); b.LoadVariantJson(2, json.dumps(variant_docs(DOG)[1]))
    b.UpdateBegin()
    refused(da, lambda: b.AssignVariants(None, [0] * n), "dtrl_step_begin")
    refused(da, lambda: b.LoadVariant(1, paths[1]), "dtrl_step_begin")
    refused(da, lambda: b.LoadVariantJson(1, json.dumps(doc)), "dtrl_step_begin")
    refused(da, lambda: b.VariantStats(1), "dtrl_step_begin")
    assert list(b.GetVariants()) == [0] * n                                         # (valid at any time)
    b.UpdateEnd()
    refused(da, lambda: b.AssignVariants([0, n], [1, 1]), "env id", "out of range")
    refused(da, lambda: b.AssignVariants([-1], [1]), "env id", "out of range")
    refused(da, lambda: b.GetVariants([n]), "out of range")
    b.AssignVariants([1, 3], [1, 2])
    assert list(b.GetVariants()) == [0, 1, 0, 2]
    b.Update()


def test_batch_without_variants_launches_as_before(da, om, tmp_path, n=6, frames=30):
    """7. A batch that never calls CreateVariants does not enter the variant path: per frame the backend's launch counter advances by the group's one frame launch,
    plus -- on the check build, whose counter sees the 0-step launches too -- one compact reset launch in a frame that ended with a fall. The same batch with
    three variants shows what the counter would have seen on the per-variant path."""
    emul = Scenario is EmulScenario
    extra = dict(terrain_seed=11)
    b = plain(om, DOG, n, None, extra)
    bv = with_variants(om, DOG, n, write_variants(tmp_path, DOG), [e % 3 for e in range(n)], extra)
    b.KernelTimeMs(); bv.KernelTimeMs()
    r0 = X.env_states(b)["num_resets"].sum()
    var_launches = 0
    for f in range(frames):
        b.Update(); bv.Update()
        r1 = X.env_states(b)["num_resets"].sum()
        assert b.KernelTimeMs()[1] == 1 + (1 if (emul and r1 != r0) else 0), "frame %d" % f
        r0 = r1
        var_launches += bv.KernelTimeMs()[1]
    assert var_launches >= (3 * frames if emul else frames)
