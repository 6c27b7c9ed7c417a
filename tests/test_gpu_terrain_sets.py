"""Terrain sets on the product library (libdtrl.so / libdtrl_f32.so on cuda:0): the twins of tests/test_terrain_sets.py -- there the host default of
Backend::TerrainBoundary, here ONE launch of dtrl_terrain_boundary_keyed per env group and frame -- and what only exists on HIP: the keyed kernel against the
host fallback (DTRL_TERRAINS_FALLBACK=1) with one and two env groups, in both libraries and under the reference frame kernel, determinism and shard invariance of
mixed device terrain, and the new symbols in both libraries."""
import pytest

import test_external_policy as X
import test_model_variants as V
import test_policy_slots as P
import test_terrain_sets as T
from product import assert_same_end, end_state, product_batch, set_knobs, symbols_test
# ---- twins: the CPU tests themselves, collected here under the module's gpu mark and fixture ----
from test_terrain_sets import (test_batch_state, test_batch_without_terrains_launches_as_before, test_envs_are_independent, test_no_restart_equals_curriculum_step,  # noqa: F401
                               test_queued_behind_unfinished_frames, test_refusals, test_restart_after_frames_equals_creation, test_restart_equals_creation,
                               test_terrain_zero_follows_the_curriculum, test_terrains_with_external_policy, test_terrains_with_model_variants,
                               test_terrains_with_policy_slots, test_two_shards_equal_one_process)

pytestmark = pytest.mark.gpu
hip_batch = product_batch(T, V, P, X)
NOT_TWINNED = {"test_terrain_sweep_tool": "a tool test (tools/terrain_sweep.py); had no twin before this change"}


# ---- 7a / 7b. the keyed kernel against the host fallback: 192 envs, 4 terrains (cliffs_rugged among them), 90 frames, bit for bit ----
def mixed_run(om, monkeypatch, env, extra, n=192, frames=90):
    set_knobs(monkeypatch, env)
    b = T.mixed_batch(om, T.DOG, n, T.four_files(T.DOG), [e % 4 for e in range(n)], dict(terrain_seed=77, rand_seed=4, terrain_gen="device", **extra), trained=True)
    for _ in range(frames):
        b.Update()
    dist, ids = b.GetDistLog()
    out = end_state(b, statistics=(b.EvalStats(), [b.TerrainStats(t) for t in range(b.num_terrains)]), distance_logs=[dist[ids == e].tobytes() for e in range(n)])
    assert out["statistics"][0]["resets"] > 0 and all(s["cycles"] > 0 for s in out["statistics"][1])
    assert sum(1 for e in range(n) if out["ground"][e][1] % 2 == 1) > 0, "no window slid"      # (a fall builds two segments, a slide one)
    return out


@pytest.mark.parametrize("groups", ["1", "2"], ids=["one_group", "two_groups"])
@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_keyed_kernel_equals_host_fallback(da, om, monkeypatch, precision, groups):
    """7a. One launch of dtrl_terrain_boundary_keyed per group and frame against tg_env_boundary run on the host, env by env (DTRL_TERRAINS_FALLBACK=1)."""
    extra = dict(physics_precision="f32") if precision == "f32" else {}
    base = mixed_run(om, monkeypatch, {"DTRL_GROUPS": groups}, extra)
    assert_same_end(base, mixed_run(om, monkeypatch, {"DTRL_GROUPS": groups, "DTRL_TERRAINS_FALLBACK": "1"}, extra), "host fallback")


def test_keyed_kernel_equals_host_fallback_under_the_reference_kernel(da, om, monkeypatch):
    """7b. The same run under DTRL_KERNEL=ref."""
    base = mixed_run(om, monkeypatch, {"DTRL_KERNEL": "ref"}, {})
    assert_same_end(base, mixed_run(om, monkeypatch, {"DTRL_KERNEL": "ref", "DTRL_TERRAINS_FALLBACK": "1"}, {}), "host fallback, reference kernel")


# ---- 7c. determinism and shard invariance of mixed device terrain (the pattern of test_device_terrain_determinism_and_shard_invariance) ----
def test_mixed_device_terrain_determinism_and_shard_invariance(da, om, frames=60):
    """Same global env ids -> same windows and trajectories, whether an env runs in a batch of 12 at offset 0 or of 5 at offset 4, run after run, and through
    RunFrames (everything queued, no host wait between frames)."""
    files = T.four_files(T.DOG)
    extra = dict(terrain_seed=9, rand_seed=3, terrain_gen="device")
    deal = lambda g0, n: [(g0 + k) % 4 for k in range(n)]
    a = T.mixed_batch(om, T.DOG, 12, files, deal(0, 12), extra)
    a2 = T.mixed_batch(om, T.DOG, 12, files, deal(0, 12), extra)
    c = T.mixed_batch(om, T.DOG, 5, files, deal(4, 5), dict(extra, global_env_offset=4))
    r = T.mixed_batch(om, T.DOG, 12, files, deal(0, 12), extra)
    for _ in range(frames):
        a.Update(); a2.Update(); c.Update()
    r.RunFrames(frames)
    T.assert_envs_equal(a, a2, range(12), "run after run")
    T.assert_envs_equal(a, r, range(12), "RunFrames")
    oa, oc = X.observe(a, range(4, 9)), X.observe(c, range(5))
    for k in range(5):
        (sa, pa, ga), (sb, pb, gb) = oa[4 + k], oc[k]
        bad = X.same_record(sa, sb)
        assert bad is None, "global env %d: EnvState.%s differs between the shard and the whole batch" % (4 + k, bad)
        assert pa.tobytes() == pb.tobytes() and ga == gb, 4 + k
    assert a.EvalStats()["resets"] >= 1 and a.EvalStats() == r.EvalStats()


# ---- 7d. ABI ----
test_new_symbols_resolve = symbols_test(("dtrl_terrains_create", "dtrl_terrain_set_file", "dtrl_terrain_set_params", "dtrl_terrain_info", "dtrl_assign_terrains", "dtrl_get_terrains",
                                         "dtrl_terrain_stats"))
