"""Episode log on the product libraries (libdtrl.so / libdtrl_f32.so on cuda:0): the twins of tests/test_episode_log.py -- there the host default of
Backend::EpisodeLog, here ONE launch of dtrl_episode_log (one workgroup of 1024 threads) per env group and frame -- and what only exists on HIP: the kernel
against its host fallback (DTRL_EPISODE_LOG_FALLBACK=1) byte for byte in the drained rows, EpisodeLogInfo and every env's EnvState, at 70 envs (two waves of thread
ranges, the second ragged) with one and two env groups, both terrain modes and both libraries, with rings of 4096 rows and of 4 (the slot-collision case: 70 rows in
one boundary); at 1100 envs in one group (two envs per thread with a ragged tail, rows from every wave through the scan's second level); frames queued without a
host wait (RunFrames) against frame-by-frame Update, run after run; and the new symbols in both libraries."""
import pytest

import test_episode_limit as E
import test_episode_log as L
import test_external_policy as X
import test_host_and_emul as H
import test_model_variants as V
import test_policy_slots as P
import test_push_schedule as R
import test_terrain_ladder as LD
import test_terrain_sets as T
import test_variant_rescale as VR
from product import product_batch, set_knobs, symbols_test
# ---- twins: the CPU tests themselves, collected here under the module's gpu mark and fixture ----
from test_episode_log import (test_a_parked_env_counts_no_frame, test_drain_while_a_frame_is_in_flight, test_episode_outcomes_tool, test_external_log_equals_internal,  # noqa: F401
                              test_keys_and_draws_are_the_episodes_own, test_listed_starts_and_lifecycle, test_ring_keeps_the_last_rows_of_a_boundary,
                              test_rows_carry_the_slot, test_rows_equal_frame_by_frame_polling, test_rows_equal_frame_by_frame_polling_fp32,
                              test_two_env_groups_merge_in_boundary_env_order)

pytestmark = pytest.mark.gpu
hip_batch = product_batch(R, T, V, X, P, LD, H, VR)
NOT_TWINNED = {}


@pytest.mark.parametrize("overlap", [False, True], ids=["sequential", "overlapped"])
def test_train_loop_logs_episodes(da, om, monkeypatch, overlap):
    monkeypatch.setattr(L, "LOOP_TRAINER", {})         # the native trainer on the device, not the check build's trainer library
    L.test_train_loop_logs_episodes(da, om, overlap)


# ---- GPU only: the kernel against its host fallback, byte for byte ----
N, FRAMES = L.N, 30


def logged_run(om, monkeypatch, env, mode, extra, capacity, run_frames=False, n=N, frames=FRAMES, limits=E.LIMITS, pushes=True):
    set_knobs(monkeypatch, env)
    if pushes:
        extra = dict(extra, min_perturb=E.HARD[0], max_perturb=E.HARD[1], min_pertrub_duration=0.1, max_perturb_duration=0.25)   # hard pushes: falls among the rows
    b = E.limit_batch(om, n, mode, frames=limits, **extra)
    if pushes:
        b.PushSchedule((3, 6), seed=R.SEED)             # (on the device: RunFrames queues it)
    b.EpisodeLog(capacity)
    if run_frames:
        b.RunFrames(frames)
    else:
        for _ in range(frames):
            b.Update()
    info = b.EpisodeLogInfo()
    rows = b.EpisodeLogDrain()
    assert L.in_order(rows) and rows["lost"] == info["lost"] and len(rows["env"]) + info["lost"] == info["written"]
    return rows, info, X.env_states(b)


def assert_same_log(x, y, what, n=N):
    assert L.rows_of(x[0]) == L.rows_of(y[0]), "%s: the drained rows differ" % what
    assert x[1] == y[1], "%s: EpisodeLogInfo differs (%r, %r)" % (what, x[1], y[1])
    for e in range(n):
        bad = X.same_record(x[2][e], y[2][e])
        assert bad is None, "%s: env %d: EnvState.%s differs" % (what, e, bad)


CASES = {"ring_4096": (4096, E.LIMITS), "ring_4_all_end_together": (4, (3, 3))}


@pytest.mark.parametrize("case", list(CASES), ids=list(CASES))
@pytest.mark.parametrize("groups", ["1", "2"], ids=["one_group", "two_groups"])
@pytest.mark.parametrize("mode", T.MODES, ids=T.MODE_IDS)
def test_kernel_equals_host_fallback(da, om, monkeypatch, mode, groups, case):
    capacity, limits = CASES[case]
    kw = dict(limits=limits, pushes=capacity != 4)     # (ring of 4: no pushes, so that all 70 episodes end in one boundary, every third)
    base = logged_run(om, monkeypatch, {"DTRL_GROUPS": groups}, mode, {}, capacity, **kw)
    if capacity == 4:                                  # 70 rows in one boundary, four slots a ring
        G = int(groups)
        assert base[1]["written"] == N * (FRAMES // 3) and base[1]["lost"] == base[1]["written"] - 4 * G
        assert sorted(base[0]["env"]) == sorted(e for g in range(G) for e in range(N * (g + 1) // G - 4, N * (g + 1) // G)) and (base[0]["boundary"] == FRAMES - 1).all()
    else:
        cause = base[0]["cause"]
        assert base[1]["lost"] == 0 and (cause == 1).sum() >= 10 and (cause == 2).sum() >= 10, "the run is meant to hold falls and limits"
    assert_same_log(base, logged_run(om, monkeypatch, {"DTRL_GROUPS": groups, "DTRL_EPISODE_LOG_FALLBACK": "1"}, mode, {}, capacity, **kw), "host fallback")


def test_kernel_equals_host_fallback_fp32(da, om, monkeypatch):
    mode, prec = dict(terrain_gen="device"), dict(physics_precision="f32")
    base = logged_run(om, monkeypatch, {"DTRL_GROUPS": "2"}, mode, prec, 4096)
    assert_same_log(base, logged_run(om, monkeypatch, {"DTRL_GROUPS": "2", "DTRL_EPISODE_LOG_FALLBACK": "1"}, mode, prec, 4096), "host fallback, fp32")


def test_more_than_one_env_per_thread(da, om, monkeypatch, n=1100, frames=12):
    """1100 envs in one group: chunk = 2, threads 0 .. 549 own two envs each and the rest none. Limits of at most 4 frames over 12 frames end at least two
    episodes of every env: at least 2200 rows without any fall, from every wave that owns envs."""
    mode = dict(terrain_gen="device")
    kw = dict(n=n, frames=frames, limits=(2, 4), pushes=False)
    base = logged_run(om, monkeypatch, {"DTRL_GROUPS": "1"}, mode, {}, 8192, **kw)
    assert base[1]["n_groups"] == 1 and base[1]["lost"] == 0 and len(base[0]["env"]) >= 1024
    per_env = [int((base[0]["env"] == e).sum()) for e in range(n)]
    assert min(per_env) >= 2, "every env is meant to end at least two episodes"
    assert_same_log(base, logged_run(om, monkeypatch, {"DTRL_GROUPS": "1", "DTRL_EPISODE_LOG_FALLBACK": "1"}, mode, {}, 8192, **kw), "host fallback, 1100 envs", n=n)


@pytest.mark.parametrize("mode", T.MODES, ids=T.MODE_IDS)
def test_queued_frames_equal_frame_by_frame_and_repeat(da, om, monkeypatch, mode):
    """RunFrames(30) -- with device terrain every frame, rule and reset launch queued, the host never waits between them -- equals 30 Update()s in rows and
    states: the rule needs no host wait. A second run gives the same bytes."""
    base = logged_run(om, monkeypatch, {}, mode, {}, 4096)
    assert len(base[0]["env"]) >= 20
    assert_same_log(base, logged_run(om, monkeypatch, {}, mode, {}, 4096, run_frames=True), "RunFrames")
    assert_same_log(base, logged_run(om, monkeypatch, {}, mode, {}, 4096), "run after run")


test_new_symbols_resolve = symbols_test(("dtrl_episode_log", "dtrl_episode_log_info", "dtrl_episode_log_drain", "dtrl_variant_rescale_factors"))
