"""Terrain ladder on the product library (libdtrl.so / libdtrl_f32.so on cuda:0): the twins of tests/test_terrain_ladder.py -- there the host default of
Backend::TerrainBoundary, here ONE launch of dtrl_terrain_boundary_ladder per env group and frame -- and what only exists on HIP: the kernel against the host
fallback (DTRL_TERRAINS_FALLBACK=1) at 70 envs (two 64-thread blocks, the second partial) with one and two env groups in both libraries, frames queued without a
host wait (RunFrames) against frame-by-frame Update, run-to-run determinism, and the new symbols in both libraries."""
import pytest

import test_external_policy as X
import test_model_variants as V
import test_policy_slots as P
import test_terrain_ladder as L
import test_terrain_sets as T
from product import assert_same_end, end_state, product_batch, set_knobs, symbols_test
# ---- twins: the CPU tests themselves, collected here under the module's gpu mark and fixture ----
from test_terrain_ladder import (test_at_top_draws, test_envs_off_the_ladder_are_untouched, test_key_ownership, test_ladder_equals_hand_driven,  # noqa: F401
                                 test_ladder_with_external_policy, test_ladder_with_model_variants, test_ladder_with_policy_slots, test_refusals,
                                 test_resets_and_restart, test_terrain_ladder_tool)

pytestmark = pytest.mark.gpu
hip_batch = product_batch(L, T, V, P, X)
NOT_TWINNED = {}

# ---- 8. GPU only: 70 envs (two blocks of 64 threads, the second partial), 4 terrains, 40 frames, bit for bit ----
N, FRAMES = 70, 40


def ladder_run(om, monkeypatch, env, extra, run_frames=False, at_top=False):
    set_knobs(monkeypatch, env)
    b = L.plain_batch(om, N, dict(terrain_gen="device"), seed=77, deal=[e % 4 for e in range(N)], **extra)
    b.TerrainLadder(0, 3, 0.3, 0.5, at_top=at_top)
    if run_frames:
        b.RunFrames(FRAMES)
    else:
        for _ in range(FRAMES):
            b.Update()
    info = b.LadderInfo()
    assert info["ups"].sum() >= 5 and info["downs"].sum() >= 5, (info["ups"], info["downs"])
    assert info["ups"][64:].sum() + info["downs"][64:].sum() > 0, "no env of the second block moved"
    return end_state(b, info, levels=list(b.GetTerrains()), ladder_records=(info["mark_x"].tobytes(), info["ups"].tobytes(), info["downs"].tobytes()),
                     terrain_statistics=[b.TerrainStats(t) for t in range(b.num_terrains)])


@pytest.mark.parametrize("groups", ["1", "2"], ids=["one_group", "two_groups"])
@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_ladder_kernel_equals_host_fallback(da, om, monkeypatch, precision, groups):
    """One launch of dtrl_terrain_boundary_ladder per group and frame against the rule and tg_env_boundary run on the host, env by env (DTRL_TERRAINS_FALLBACK=1);
    two groups: the second starts at a non-zero e0."""
    extra = dict(physics_precision="f32") if precision == "f32" else {}
    base = ladder_run(om, monkeypatch, {"DTRL_GROUPS": groups}, extra)
    assert_same_end(base, ladder_run(om, monkeypatch, {"DTRL_GROUPS": groups, "DTRL_TERRAINS_FALLBACK": "1"}, extra), "host fallback")


@pytest.mark.parametrize("at_top", [False, True], ids=["stay_at_top", "draw_at_top"])
def test_queued_frames_equal_frame_by_frame_and_repeat(da, om, monkeypatch, at_top):
    """RunFrames(40) -- every frame and boundary queued, the host never waits between them -- equals 40 x Update(); a second run gives the same bits."""
    base = ladder_run(om, monkeypatch, {}, {}, at_top=at_top)
    assert_same_end(base, ladder_run(om, monkeypatch, {}, {}, run_frames=True, at_top=at_top), "RunFrames")
    assert_same_end(base, ladder_run(om, monkeypatch, {}, {}, at_top=at_top), "run after run")


test_new_symbols_resolve = symbols_test(("dtrl_terrain_ladder", "dtrl_ladder_info"))
