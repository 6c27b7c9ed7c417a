"""Policy slots on the product library (libdtrl.so / libdtrl_f32.so on cuda:0): the twins of tests/test_policy_slots.py -- there the per-slot default, here ONE
launch of the slot kernels (dtrl_backend_hip_slots.hip) against the shipped single-policy kernels -- and the cross-checks between the slot fast kernels, the slot
reference kernel, the per-slot fallback, two env groups and device terrain, the deferred hand-over into slot 0 and its alias, and dtrl_slot_stats at full width."""
import numpy as np
import pytest

import test_external_policy as X
import test_policy_slots as T
from precision import assert_library, both_precisions, extra_for
from product import assert_same_end, end_state, product_batch, set_knobs
# ---- twins: the CPU tests themselves, collected here under the module's gpu mark and fixture ----
from test_policy_slots import (test_alias_follows_slot0, test_batch_without_slots_launches_as_before, test_exp_scenario_tuples, test_reassignment_mid_run,  # noqa: F401
                               test_refusals, test_slot_stats, test_slot_stats_waits_for_a_frame_in_flight, test_snapshots_and_clones_keep_the_assignment)

pytestmark = pytest.mark.gpu
hip_batch = product_batch(T)
NOT_TWINNED = {"test_train_loop_greedy_envs": "the loop's host logic, on a recording subclass of the lane-loop scenario: lane-loop build only"}


# ---- the twin with cases of its own: both libraries ----
F32_CASES = [(T.DOG, dict(terrain_seed=11, physics_precision="f32")), (T.RAPTOR, dict(terrain_seed=5, physics_precision="f32"))]


@pytest.mark.parametrize("arg,extra", T.EQUAL_CASES + F32_CASES, ids=T.EQUAL_IDS + ["dog_f32", "raptor_f32"])
def test_equals_single_policy_runs(da, om, arg, extra):
    T.run_equals_single_policy(om, arg, extra)


# ---- cross-checks: 192 envs, 3 slots, 90 frames, bit for bit ----
def slot_run(om, monkeypatch, arg, env, extra, n=192, frames=90):
    set_knobs(monkeypatch, env)
    b = T.slotted(arg, n, T.policies(om, arg), T.EXPLORE, [e % 3 for e in range(n)], dict(terrain_seed=77, rand_seed=4, **extra))
    assert_library(b, extra.get("physics_precision", "f64"))
    for _ in range(frames):
        b.Update()
    ev, slots = b.EvalStats(), [b.SlotStats(s) for s in range(b.num_slots)]
    assert ev["cycles"] > n and ev["resets"] > 0 and all(s["cycles"] > 0 for s in slots)
    return end_state(b, statistics=(ev, slots))


@pytest.mark.parametrize("arg,prec", both_precisions([T.DOG, T.RAPTOR], ids=["dog", "raptor"]))
def test_slot_fast_kernel_equals_slot_reference_kernel_and_per_slot_fallback(da, om, monkeypatch, arg, prec):
    """One launch of the register-resident slot kernel against one launch of the LDS-phase slot kernel (DTRL_KERNEL=ref) and against the per-slot launches of the
    SHIPPED single-policy kernels (DTRL_SLOTS_FALLBACK=1). In libdtrl.so and in libdtrl_f32.so."""
    extra = extra_for(prec)
    base = slot_run(om, monkeypatch, arg, {}, extra)
    assert_same_end(base, slot_run(om, monkeypatch, arg, {"DTRL_KERNEL": "ref"}, extra), "slot reference kernel")
    assert_same_end(base, slot_run(om, monkeypatch, arg, {"DTRL_SLOTS_FALLBACK": "1"}, extra), "per-slot fallback")


def test_two_env_groups(da, om, monkeypatch):
    """DTRL_GROUPS=2: two streams, two launch lists, the same bits."""
    assert_same_end(slot_run(om, monkeypatch, T.DOG, {}, {}), slot_run(om, monkeypatch, T.DOG, {"DTRL_GROUPS": "2"}, {}), "two env groups")


def test_device_terrain_one_launch_equals_fallback(da, om, monkeypatch):
    """-terrain_gen= device (no host wait between frames, launch order computed on the device): one launch of the slot kernel against the per-slot fallback."""
    extra = dict(terrain_gen="device")
    assert_same_end(slot_run(om, monkeypatch, T.RAPTOR, {}, extra), slot_run(om, monkeypatch, T.RAPTOR, {"DTRL_SLOTS_FALLBACK": "1"}, extra), "device terrain")


def test_deferred_handover_reaches_slot0_and_its_alias(da, om, n=256, frames=30, at=10):
    """A SetPolicyDevice on slot 0 issued between step_begin and step_end (gathered into the second weight buffer, switched in with the next launch) reaches slot 0
    and its alias at the same frame as in a single-policy batch making the same call."""
    import torch
    extra = dict(terrain_seed=11)
    p0, p1 = T.policies(om, T.DOG)[:2]
    w1 = torch.tensor(np.ascontiguousarray(p1[1], np.float32), device=torch.device("cuda", 0))
    torch.cuda.synchronize()
    bs = T.batch(T.DOG, n, **extra)
    bs.CreateSlots(2)
    bs.SetPolicy(p0[1], *p0[2:]); bs.SetExplore(*T.EXPLORE[0])
    bs.SlotAlias(1, 0); bs.SlotSetExplore(1, *T.EXPLORE[1])
    assign = [e % 2 for e in range(n)]
    bs.AssignSlots(None, assign)
    refs = [T.single(T.DOG, n, p0, T.EXPLORE[0], extra), T.single(T.DOG, n, p0, T.EXPLORE[1], extra)]
    c_at = None
    for f in range(frames):
        for b in [bs] + refs:
            b.UpdateBegin()
            if f == at:
                b.SetPolicyDevice(w1.data_ptr(), w1.numel())
            b.UpdateEnd()
        if f == at:
            c_at = X.env_states(bs)["num_cycles"].copy()
        if f % 3 == 2 or f in (at, at + 1):
            for s in range(2):
                T.assert_envs_equal(bs, refs[s], [e for e in range(n) if assign[e] == s], "frame %d slot %d" % (f, s))
    st = X.env_states(bs)
    for s in range(2):
        assert sum(1 for e in range(n) if assign[e] == s and st["num_cycles"][e] > c_at[e]) > n // 4, "slot %d: too few decisions under the new weights" % s
    # the new weights did arrive: a batch that never got them ends elsewhere
    old = T.single(T.DOG, n, p0, T.EXPLORE[1], extra)
    for f in range(frames):
        old.Update()
    assert X.same_record(X.env_states(old), X.env_states(refs[1])) is not None


def test_slot_stats_full_width(da, om, n=8192, frames=30):
    """dtrl_slot_stats at 8192 envs and 8 slots (32 workgroups of partial rows) against the records."""
    p0 = T.policies(om, T.DOG)[0]
    b = T.batch(T.DOG, n, terrain_seed=11)
    b.CreateSlots(8)
    b.SetPolicy(p0[1], *p0[2:]); b.SetExplore(*T.EXPLORE[0])
    for s in range(1, 8):
        b.SlotAlias(s, 0); b.SlotSetExplore(s, 1, 0.1 * s, 0.5, 0.05 * s)
    rng = np.random.RandomState(3)
    b.AssignSlots(None, rng.randint(0, 8, n))                  # uneven, unordered
    b.RunFrames(frames)
    tot = T.check_slot_stats(b, 8)
    assert tot["cycles"] > n and tot["episodes"] > 0, tot
