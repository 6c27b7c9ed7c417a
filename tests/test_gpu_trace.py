"""Frame trace on the product libraries (libdtrl.so / libdtrl_f32.so on cuda:0): the twins of tests/test_trace.py -- there the host defaults of
Backend::TraceRecord / TraceGather, here ONE launch of dtrl_trace_record per env group and frame over the group's own list of traced envs and ONE launch of
dtrl_trace_gather per read -- and what only exists on HIP: the kernels against their host fallback (DTRL_TRACE_FALLBACK=1) at 70 envs with 1, 3 and all envs
traced, the ids unsorted, with one and two env groups (with three envs traced all of them sit in the first group: the second queues nothing), both terrain modes
and both libraries, with falls among the rows; frames queued without a host wait (RunFrames) against frame-by-frame Update; the read into device memory against the
read into host memory; run-to-run determinism; and the new symbols in both libraries."""
import pytest

import test_episode_limit as E
import test_external_policy as X
import test_host_and_emul as H
import test_model_variants as V
import test_policy_slots as P
import test_push_schedule as R
import test_terrain_ladder as LD
import test_terrain_sets as T
import test_trace as TR
from product import product_batch, set_knobs, symbols_test
# ---- twins: the CPU tests themselves, collected here under the module's gpu mark and fixture ----
from test_trace import (test_a_fallen_envs_row_is_its_last_pose, test_a_parked_env_writes_no_row, test_export_motion_files, test_external_trace_equals_internal,  # noqa: F401
                        test_lifecycle_and_refusals, test_ring_and_untouched_batch, test_row_carries_the_keys_the_frame_ran_under,
                        test_row_carries_the_limits_need_reset, test_rows_equal_getters_dog_with_variants_and_terrains, test_rows_equal_getters_fp32,
                        test_rows_equal_getters_raptor_with_slots)

pytestmark = pytest.mark.gpu
hip_batch = product_batch(R, T, V, X, P, LD, H)
NOT_TWINNED = {}

# ---- GPU only: 70 envs, bit for bit ----
N, FRAMES, RING = E.N, 30, 20         # (the ring is shorter than the run: the reads unroll a ring that has wrapped)
LISTS = {"one": [66], "three": [30, 2, 17], "all": None}    # "three": unsorted, and with two env groups all in the first (envs 0 .. 34): the second has no traced env


def traced_run(om, monkeypatch, env, mode, extra, traced, run_frames=False, device_read=False):
    set_knobs(monkeypatch, env)
    extra = dict(extra, min_perturb=E.HARD[0], max_perturb=E.HARD[1], min_pertrub_duration=0.1, max_perturb_duration=0.25)   # hard pushes: falls among the rows
    b = E.limit_batch(om, N, mode, limit=False, **extra)
    b.PushSchedule((3, 6), seed=R.SEED)
    ids = list(range(N - 1, -1, -1)) if traced is None else traced   # all envs: listed in descending order
    b.Trace(ids, frames=RING)
    if run_frames:
        b.RunFrames(FRAMES)
    else:
        for _ in range(FRAMES):
            b.Update()
    tr = b.TraceRead()
    assert list(tr["env_ids"]) == ids and list(tr["count"]) == [RING] * len(ids) and [list(r) for r in tr["row"]] == [list(range(FRAMES - RING, FRAMES))] * len(ids)
    if device_read:
        vals, ints, count = b.TraceReadDevice()
        assert vals.is_cuda and TR.same(vals.cpu().numpy(), tr["vals"]) and TR.same(ints.cpu().numpy(), tr["ints"]) and list(count) == list(tr["count"])
        v2, i2, c2 = b.TraceReadDevice(env_ids=ids[-1:], max_rows=RING + 5)      # a subset, more rows than the ring holds: rows beyond count are not written
        assert list(c2) == [RING] and TR.same(v2.cpu().numpy()[0, :RING], tr["vals"][-1]) and TR.same(i2.cpu().numpy()[0, :RING], tr["ints"][-1])
        assert not v2.cpu().numpy()[0, RING:].any() and not i2.cpu().numpy()[0, RING:].any()
    return tr, X.env_states(b), int((tr["need_reset"] & 1).sum())


def assert_same_trace(x, y, what):
    for k in ("vals", "ints", "count", "env_ids"):
        assert TR.same(x[0][k], y[0][k]), "%s: %s of the trace differs" % (what, k)
    for e in range(N):
        bad = X.same_record(x[1][e], y[1][e])
        assert bad is None, "%s: env %d: EnvState.%s differs" % (what, e, bad)


@pytest.mark.parametrize("traced", list(LISTS), ids=list(LISTS))
@pytest.mark.parametrize("groups", ["1", "2"], ids=["one_group", "two_groups"])
@pytest.mark.parametrize("mode", T.MODES, ids=T.MODE_IDS)
def test_trace_kernels_equal_host_fallback(da, om, monkeypatch, mode, groups, traced):
    base = traced_run(om, monkeypatch, {"DTRL_GROUPS": groups}, mode, {}, LISTS[traced], device_read=True)
    if traced == "all":
        assert base[2] >= 10, "the run is meant to have falls among the rows"
    assert_same_trace(base, traced_run(om, monkeypatch, {"DTRL_GROUPS": groups, "DTRL_TRACE_FALLBACK": "1"}, mode, {}, LISTS[traced], device_read=True), "host fallback")


def test_trace_kernels_equal_host_fallback_fp32(da, om, monkeypatch):
    mode, prec = dict(terrain_gen="device"), dict(physics_precision="f32")
    base = traced_run(om, monkeypatch, {"DTRL_GROUPS": "2"}, mode, prec, None, device_read=True)
    assert_same_trace(base, traced_run(om, monkeypatch, {"DTRL_GROUPS": "2", "DTRL_TRACE_FALLBACK": "1"}, mode, prec, None), "host fallback, fp32")


@pytest.mark.parametrize("mode", T.MODES, ids=T.MODE_IDS)
def test_queued_frames_equal_frame_by_frame_and_repeat(da, om, monkeypatch, mode):
    """RunFrames -- with device terrain every frame, trace, boundary and reset launch queued, the host never waits between them: equal bits show that the rule needs
    no host wait -- equals frame-by-frame Update(); a second run gives the same bits."""
    base = traced_run(om, monkeypatch, {}, mode, {}, None)
    assert_same_trace(base, traced_run(om, monkeypatch, {}, mode, {}, None, run_frames=True), "RunFrames")
    assert_same_trace(base, traced_run(om, monkeypatch, {}, mode, {}, None), "run after run")


def test_run_frames_12_equals_twelve_updates(da, om):
    a, b = (T.with_policy(om, T.DOG, 16, dict(terrain_seed=31, rand_seed=3, terrain_gen="device")) for _ in range(2))
    a.Trace([9, 3], 12); b.Trace([9, 3], 12)
    a.RunFrames(12)
    for _ in range(12):
        b.Update()
    ta, tb = a.TraceRead(), b.TraceRead()
    assert list(ta["count"]) == [12, 12] and TR.same(ta["vals"], tb["vals"]) and TR.same(ta["ints"], tb["ints"])


test_new_symbols_resolve = symbols_test(("dtrl_trace", "dtrl_trace_info", "dtrl_trace_read", "dtrl_trace_read_device"))
