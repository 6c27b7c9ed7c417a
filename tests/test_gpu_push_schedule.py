"""Push schedule on the product library (libdtrl.so / libdtrl_f32.so on cuda:0): the twins of tests/test_push_schedule.py -- there the host defaults of
Backend::PushSchedule and Backend::PerturbScatter, here ONE launch of dtrl_push_schedule per env group and frame in both terrain modes and ONE launch of
dtrl_perturb_scatter per dtrl_add_perturb -- and what only exists on HIP: the kernels against their host fallbacks (DTRL_PUSH_FALLBACK=1, DTRL_PERTURB_FALLBACK=1)
at 70 envs / rows (two 64-thread blocks, the second partial) with one and two env groups in both libraries, frames queued without a host wait (RunFrames) against
frame-by-frame Update, run-to-run determinism, the fast kernel against the reference kernel under a schedule, every frame-boundary rule (ladder, redraw, schedule) in ONE batch
against all the host fallbacks at once, and the new symbols in both libraries."""
import pytest

import test_external_policy as X
import test_host_and_emul as H
import test_model_variants as V
import test_policy_slots as P
import test_push_schedule as R
import test_terrain_ladder as LD
import test_terrain_sets as T
from product import assert_same_end, end_state, product_batch, set_knobs, symbols_test
# ---- twins: the CPU tests themselves, collected here under the module's gpu mark and fixture ----
from test_push_schedule import (test_add_perturb_equals_row_by_row, test_apply_rand_force_goes_through_the_launch, test_batch_state_resets_and_removal,  # noqa: F401
                                test_held_out_envs_equal_a_batch_without_schedule, test_push_robustness_tool, test_refusals, test_replay_through_add_perturb,
                                test_scale_multiplies_the_force_and_nothing_else, test_scheduled_push_vs_oracle, test_shard_invariance,
                                test_with_model_variants_and_redraw, test_with_policy_slots, test_with_terrain_ladder)

pytestmark = pytest.mark.gpu
hip_batch = product_batch(R, T, V, X, P, LD, H)
NOT_TWINNED = {}


# ---- twins with cases or a body of their own ----
@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("mode", T.MODES, ids=T.MODE_IDS)
def test_records_equal_the_rule(da, om, mode, precision):
    """(both libraries: the rule is doubles and integers in either, so the fp32 library's records equal the same Python rule, given its own falls)"""
    R.test_records_equal_the_rule(da, om, mode, **(dict(physics_precision="f32") if precision == "f32" else {}))


def test_train_loop_with_pushes(da, om):
    """A few hundred iterations of the native trainer on the product libraries under a schedule."""
    out, _ = R.run_train_loop_with_pushes(200, 4000, trainer_device="cuda")
    assert out["iters"] >= 200, (out["frames"], out["iters"])


# ---- GPU only: 70 envs (two blocks of 64 threads, the second partial), bit for bit ----
N, FRAMES = 70, 30


def push_end(b):
    info = b.PushInfo()
    return end_state(b, info, push_records={k: v.tobytes() for k, v in info.items()})


def push_run(om, monkeypatch, env, mode, extra, run_frames=False):
    set_knobs(monkeypatch, env)
    scale = [0.0 if e % 7 == 3 else 1.0 + 0.25 * (e % 3) for e in range(N)]     # held-out envs and a magnitude sweep in both blocks
    b = R.push_batch(om, N, mode, scale=scale, **extra)
    if run_frames:
        b.RunFrames(FRAMES)
    else:
        for _ in range(FRAMES):
            b.Update()
    out = push_end(b)
    pushes = out["info"]["pushes"]
    assert pushes[[e for e in range(N) if e % 7 != 3]].min() >= 3 and not pushes[3::7].any() and out["env_states"]["num_resets"][64:].sum() >= 1, pushes
    return out


@pytest.mark.parametrize("groups", ["1", "2"], ids=["one_group", "two_groups"])
@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("mode", T.MODES, ids=T.MODE_IDS)
def test_push_kernel_equals_host_fallback(da, om, monkeypatch, mode, precision, groups):
    """One launch of dtrl_push_schedule per group and frame against the rule run on the host, env by env (DTRL_PUSH_FALLBACK=1); two groups: the second starts at a
    non-zero e0."""
    extra = dict(physics_precision="f32") if precision == "f32" else {}
    base = push_run(om, monkeypatch, {"DTRL_GROUPS": groups}, mode, extra)
    assert_same_end(base, push_run(om, monkeypatch, {"DTRL_GROUPS": groups, "DTRL_PUSH_FALLBACK": "1"}, mode, extra), "host fallback")


@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_perturb_scatter_equals_host_fallback(da, om, tmp_path, monkeypatch, precision, n=70, rows=70):
    """dtrl_perturb_scatter against the per-env copy loop the call ran before (DTRL_PERTURB_FALLBACK=1): 70 rows over 70 envs of four variants, offsets, an env
    named three times."""
    env, link, force, lp, dur = R.perturb_rows(n, rows)
    paths = V.write_variants(tmp_path, R.DOG) + [V.write_doc(tmp_path, "geom.txt", V.geometry_doc())]
    extra = dict(terrain_seed=11, **(dict(physics_precision="f32") if precision == "f32" else {}))

    def run(fallback):
        set_knobs(monkeypatch, {"DTRL_PERTURB_FALLBACK": "1"} if fallback else {})
        b = V.with_variants(om, R.DOG, n, paths, [e % 4 for e in range(n)], extra)
        b.Update()
        b.AddPerturb(link, force, dur, local_pos=lp, env_ids=env)
        b.ApplyRandForce(5, env_ids=[1, 2, 66])
        written = X.env_states(b)
        for _ in range(3):
            b.Update()
        return written, X.env_states(b)
    (wa, sa), (wb, sb) = run(False), run(True)
    for what, x, y in (("after the calls", wa, wb), ("three frames on", sa, sb)):
        for e in range(n):
            bad = X.same_record(x[e], y[e])
            assert bad is None, "%s: env %d: EnvState.%s differs from the host fallback" % (what, e, bad)
    named = set(env.tolist()) | {1, 2, 66}
    assert [e for e in range(n) if wa["pert_link"][e] >= 0] == sorted(named) and len(named) >= 40     # every named env's slot was written, no other


@pytest.mark.parametrize("mode", T.MODES, ids=T.MODE_IDS)
def test_queued_frames_equal_frame_by_frame_and_repeat(da, om, monkeypatch, mode):
    """RunFrames -- with device terrain every frame, boundary, push and reset launch queued, the host never waits between them -- equals frame-by-frame Update(); a
    second run gives the same bits."""
    base = push_run(om, monkeypatch, {}, mode, {})
    assert_same_end(base, push_run(om, monkeypatch, {}, mode, {}, run_frames=True), "RunFrames")
    assert_same_end(base, push_run(om, monkeypatch, {}, mode, {}), "run after run")


def test_fast_kernel_equals_reference_kernel_under_a_schedule(da, om, monkeypatch):
    mode = dict(terrain_gen="device")
    base = push_run(om, monkeypatch, {}, mode, {})
    assert_same_end(base, push_run(om, monkeypatch, {"DTRL_KERNEL": "ref"}, mode, {}), "DTRL_KERNEL=ref")


# ---- GPU only: every frame-boundary rule in one batch ----
RESET_IDS = [69, 3, 64, 17, 66, 0, 40, 65]     # out of order, in both 64-thread blocks: the env-list form of every rule


def all_rules_run(om, tmp_path, monkeypatch, env, n=N, frames=FRAMES):
    """Terrain sets under a ladder, model variants under a redraw and a push schedule on device terrain; a reset of RESET_IDS halfway."""
    set_knobs(monkeypatch, env)
    paths = V.write_variants(tmp_path, R.DOG)
    b = V.with_variants(om, R.DOG, n, paths, [e % 3 for e in range(n)], dict(terrain_seed=31, rand_seed=3, terrain_gen="device"))
    T.fill(b, T.four_walkable_files(T.DOG))
    b.AssignTerrains(None, [(e // 3) % 3 for e in range(n)], restart=True)
    b.TerrainLadder(0, 2, up_dist=2.0, down_dist=1.5)
    b.VariantRedraw(0, 2, seed=5)
    b.PushSchedule(R.WAIT, seed=R.SEED, force=R.FORCE, duration=R.DUR)
    for f in range(frames):
        if f == frames // 2:
            b.Reset(RESET_IDS)
        b.Update()
    terrains, again = list(b.GetTerrains()), list(b.GetTerrains())      # no frame between: the second call finds the host keys current and copies nothing
    assert terrains == again
    ladder, redraw = b.LadderInfo(), b.VariantRedrawInfo()
    keys = {"terrain": terrains, "variant": list(b.GetVariants())}
    keys.update(("ladder " + k, v.tobytes()) for k, v in ladder.items())
    keys.update(("redraw " + k, v.tobytes() if hasattr(v, "tobytes") else v) for k, v in redraw.items())
    assert keys["variant"] == list(redraw["variant"])
    moved = int(ladder["ups"].sum() + ladder["downs"].sum())
    return push_end(b), keys, (moved, int(redraw["draws"].sum()), int(redraw["draws"][64:].sum()))


@pytest.mark.parametrize("groups", ["1", "2"], ids=["one_group", "two_groups"])
def test_all_rules_in_one_batch_equal_the_host_fallbacks(da, om, tmp_path, monkeypatch, groups):
    """70 envs (two 64-thread blocks, the second partial) under a terrain ladder, a variant redraw and a push schedule at once, 30 frames with a dtrl_reset of a
    listed subset halfway: the boundary, redraw and push kernels against the host defaults of all three (DTRL_TERRAINS_FALLBACK, DTRL_VARIANTS_FALLBACK,
    DTRL_PUSH_FALLBACK) -- env states, windows, terrain and variant keys, ladder records, redraw counters and push records bit for bit. Two calls of
    dtrl_get_terrains with no frame between return the same levels (the second refreshes nothing)."""
    base, keys, (moved, draws, draws_hi) = all_rules_run(om, tmp_path, monkeypatch, {"DTRL_GROUPS": groups})
    assert moved >= 1 and draws >= len(RESET_IDS) + 1 and draws_hi >= 1 and base["info"]["pushes"].min() >= 1, (moved, draws, draws_hi, base["info"]["pushes"])
    fb = {"DTRL_GROUPS": groups, "DTRL_TERRAINS_FALLBACK": "1", "DTRL_VARIANTS_FALLBACK": "1", "DTRL_PUSH_FALLBACK": "1"}
    other, other_keys, _ = all_rules_run(om, tmp_path, monkeypatch, fb)
    assert_same_end(base, other, "host fallbacks")
    for k in keys:
        assert keys[k] == other_keys[k], "%s differs from the host fallbacks" % k


test_new_symbols_resolve = symbols_test(("dtrl_push_schedule", "dtrl_push_scale", "dtrl_push_info"))
