"""Episode limits on the product libraries (libdtrl.so / libdtrl_f32.so on cuda:0): the twins of tests/test_episode_limit.py -- there the host default of
Backend::EpisodeLimit, here ONE launch of dtrl_episode_limit per env group and frame in both terrain modes -- and what only exists on HIP: the kernel against its
host fallback (DTRL_EPISODE_FALLBACK=1) at 70 envs (two 64-thread blocks, the second partial) with one and two env groups in both libraries and both terrain
modes, with falls among the endings; frames queued without a host wait (RunFrames) against frame-by-frame Update; run-to-run determinism; the fast kernel against
the reference kernel under limits; every frame-boundary rule in ONE batch against all the host fallbacks at once, per frame and in the listed episode starts (dtrl_reset, a terrain restart, an
env coming into the limit); and the new symbols in both libraries."""
import pytest

import test_episode_limit as E
import test_external_policy as X
import test_host_and_emul as H
import test_model_variants as V
import test_policy_slots as P
import test_push_schedule as R
import test_terrain_ladder as LD
import test_terrain_sets as T
from product import assert_same_end, end_state, product_batch, set_knobs, symbols_test
# ---- twins: the CPU tests themselves, collected here under the module's gpu mark and fixture (both libraries: the rule is doubles and integers in either, so
# the fp32 library's records equal the same Python rule, given its own falls) ----
from test_episode_limit import (test_a_truncation_is_a_reset, test_batch_state_and_lifecycle, test_distance_limit_and_poli_eval, test_every_rule_at_once,  # noqa: F401
                                test_fsm_dog_resets_at_exactly_its_drawn_limits, test_held_out_envs_equal_a_batch_without_limit, test_listed_starts_under_every_rule,
                                test_records_equal_the_rule_under_the_net, test_records_equal_the_rule_with_falls, test_refusals,
                                test_setup_episode_limit_holds_the_greedy_envs_out, test_shard_invariance)

pytestmark = pytest.mark.gpu
hip_batch = product_batch(R, T, V, X, P, LD, H)
NOT_TWINNED = {}

# ---- GPU only: 70 envs (two blocks of 64 threads, the second partial), bit for bit ----
N, FRAMES = E.N, 30
HELD = [e for e in range(N) if e % 7 == 3]      # held-out envs in both blocks


def limit_run(om, monkeypatch, env, mode, extra, run_frames=False, pushes=None):
    set_knobs(monkeypatch, env)
    if pushes is not None:
        extra = dict(extra, min_perturb=pushes[0], max_perturb=pushes[1], min_pertrub_duration=0.1, max_perturb_duration=0.25)
    b = E.limit_batch(om, N, mode, limit=False, **extra)
    b.EpisodeLimitEnvs(0, env_ids=HELD)
    b.EpisodeLimit(E.LIMITS, seed=E.SEED)
    if run_frames:
        b.RunFrames(FRAMES)
    else:
        for f in range(FRAMES):
            if pushes is not None and f % 2 == 0:
                b.ApplyRandForce(f)
            b.Update()
    info = b.EpisodeInfo()
    inn = [e for e in range(N) if e not in HELD]
    # (no episode outlasts the largest limit, whichever way it ends)
    assert (info["by_limit"] + info["by_fall"])[inn].min() >= FRAMES // E.LIMITS[1] and not any(v[HELD].any() for v in info.values()) and info["by_limit"][64:].sum() >= 1, info
    if pushes is not None:
        assert info["by_fall"].sum() >= 10, info["by_fall"]
    return end_state(b, info, **{"episode " + k: v.tobytes() for k, v in info.items()})


@pytest.mark.parametrize("groups", ["1", "2"], ids=["one_group", "two_groups"])
@pytest.mark.parametrize("prec", E.PRECISIONS, ids=E.PRECISION_IDS)
@pytest.mark.parametrize("mode", T.MODES, ids=T.MODE_IDS)
def test_limit_kernel_equals_host_fallback(da, om, monkeypatch, mode, prec, groups):
    """One launch of dtrl_episode_limit per group and frame against the rule run on the host, env by env (DTRL_EPISODE_FALLBACK=1), under hard pushes so that
    episodes end by falls too; two groups: the second starts at a non-zero e0."""
    base = limit_run(om, monkeypatch, {"DTRL_GROUPS": groups}, mode, prec, pushes=E.HARD)
    assert_same_end(base, limit_run(om, monkeypatch, {"DTRL_GROUPS": groups, "DTRL_EPISODE_FALLBACK": "1"}, mode, prec, pushes=E.HARD), "host fallback")


@pytest.mark.parametrize("mode", T.MODES, ids=T.MODE_IDS)
def test_queued_frames_equal_frame_by_frame_and_repeat(da, om, monkeypatch, mode):
    """RunFrames -- with device terrain every frame, limit, boundary and reset launch queued, the host never waits between them: equal bits show that the rule
    needs no host wait -- equals frame-by-frame Update(); a second run gives the same bits."""
    base = limit_run(om, monkeypatch, {}, mode, {})
    assert_same_end(base, limit_run(om, monkeypatch, {}, mode, {}, run_frames=True), "RunFrames")
    assert_same_end(base, limit_run(om, monkeypatch, {}, mode, {}), "run after run")


def test_fast_kernel_equals_reference_kernel_under_limits(da, om, monkeypatch):
    mode = dict(terrain_gen="device")
    base = limit_run(om, monkeypatch, {}, mode, {})
    assert_same_end(base, limit_run(om, monkeypatch, {"DTRL_KERNEL": "ref"}, mode, {}), "DTRL_KERNEL=ref")


FALLBACKS = dict.fromkeys(("DTRL_TERRAINS_FALLBACK", "DTRL_VARIANTS_FALLBACK", "DTRL_PUSH_FALLBACK", "DTRL_PERTURB_FALLBACK", "DTRL_EPISODE_FALLBACK"), "1")


@pytest.mark.parametrize("groups", ["1", "2"], ids=["one_group", "two_groups"])
@pytest.mark.parametrize("mode", T.MODES, ids=T.MODE_IDS)
def test_every_rule_at_once_equals_the_host_fallbacks(da, om, tmp_path, monkeypatch, mode, groups):
    """Ladder, redraw, rescale, push schedule and episode limit in one batch: the one-launch paths against every DTRL_*_FALLBACK knob at once, in states, windows
    and every rule's records."""
    set_knobs(monkeypatch, {"DTRL_GROUPS": groups})
    base = E.run_all_rules(om, tmp_path, mode)
    set_knobs(monkeypatch, dict(FALLBACKS, DTRL_GROUPS=groups))
    E.assert_same_run(base, E.run_all_rules(om, tmp_path, mode), "host fallbacks")


@pytest.mark.parametrize("groups", ["1", "2"], ids=["one_group", "two_groups"])
@pytest.mark.parametrize("mode", T.MODES, ids=T.MODE_IDS)
def test_listed_starts_equal_the_host_fallbacks(da, om, tmp_path, monkeypatch, mode, groups):
    """dtrl_reset, a terrain restart and an env coming into the limit between frames under all five rules: the listed launches against every DTRL_*_FALLBACK
    knob at once, in states, windows and every rule's records."""
    set_knobs(monkeypatch, {"DTRL_GROUPS": groups})
    base = E.run_listed_starts(om, tmp_path, mode)
    set_knobs(monkeypatch, dict(FALLBACKS, DTRL_GROUPS=groups))
    E.assert_same_run(base, E.run_listed_starts(om, tmp_path, mode), "host fallbacks")


test_new_symbols_resolve = symbols_test(("dtrl_episode_limit", "dtrl_episode_limit_envs", "dtrl_episode_info"))
