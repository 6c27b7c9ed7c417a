"""Terrain ladder on the product library (libdtrl.so / libdtrl_f32.so on cuda:0): the twins of tests/test_terrain_ladder.py -- there the host default of
Backend::TerrainBoundary, here ONE launch of dtrl_terrain_boundary_ladder per env group and frame -- and what only exists on HIP: the kernel against the host
fallback (DTRL_TERRAINS_FALLBACK=1) at 70 envs (two 64-thread blocks, the second partial) with one and two env groups in both libraries, frames queued without a
host wait (RunFrames) against frame-by-frame Update, run-to-run determinism, and the new symbols in both libraries."""
import ctypes
import os

import pytest

import test_external_policy as X
import test_model_variants as V
import test_policy_slots as P
import test_terrain_ladder as L
import test_terrain_sets as T
from conftest import HIP_LIB

pytestmark = pytest.mark.gpu

KNOBS = ("DTRL_KERNEL", "DTRL_TERRAINS_FALLBACK", "DTRL_SLOTS_FALLBACK", "DTRL_VARIANTS_FALLBACK", "DTRL_GROUPS")


@pytest.fixture(autouse=True)
def hip_batch(monkeypatch):
    import deepterrainrl_amd
    for mod in (L, T, V, P, X):
        monkeypatch.setattr(mod, "Scenario", deepterrainrl_amd.BatchScenario)   # product path: batch() now loads libdtrl.so (libdtrl_f32.so for physics_precision=f32)
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


# ---- twins ----
@pytest.mark.parametrize("mode", T.MODES, ids=T.MODE_IDS)
def test_ladder_equals_hand_driven(da, om, mode):
    L.test_ladder_equals_hand_driven(da, om, mode)


@pytest.mark.parametrize("mode", T.MODES, ids=T.MODE_IDS)
def test_envs_off_the_ladder_are_untouched(da, om, mode):
    L.test_envs_off_the_ladder_are_untouched(da, om, mode)


@pytest.mark.parametrize("mode", T.MODES, ids=T.MODE_IDS)
def test_resets_and_restart(da, om, mode):
    L.test_resets_and_restart(da, om, mode)


@pytest.mark.parametrize("mode", T.MODES, ids=T.MODE_IDS)
def test_at_top_draws(da, om, mode):
    L.test_at_top_draws(da, om, mode)


@pytest.mark.parametrize("mode", T.MODES, ids=T.MODE_IDS)
def test_key_ownership(da, om, mode):
    L.test_key_ownership(da, om, mode)


@pytest.mark.parametrize("mode", T.MODES, ids=T.MODE_IDS)
def test_ladder_with_policy_slots(da, om, mode):
    L.run_with_slots(om, mode)


@pytest.mark.parametrize("mode", T.MODES, ids=T.MODE_IDS)
def test_ladder_with_model_variants(da, om, tmp_path, mode):
    L.run_with_variants(om, tmp_path, mode)


@pytest.mark.parametrize("mode", T.MODES, ids=T.MODE_IDS)
def test_ladder_with_external_policy(da, om, mode):
    L.run_with_external_policy(da, om, mode)


def test_refusals(da, om, tmp_path):
    L.test_refusals(da, om, tmp_path)


def test_terrain_ladder_tool(da, om):
    L.test_terrain_ladder_tool(da, om)


# ---- 8. GPU only: 70 envs (two blocks of 64 threads, the second partial), 4 terrains, 40 frames, bit for bit ----
N, FRAMES = 70, 40


def end_state(b):
    info = b.LadderInfo()
    return (X.env_states(b), b.RecordPoliState(), [X.ground_key(b, e) for e in range(b.num_envs)], list(b.GetTerrains()),
            (info["mark_x"].tobytes(), info["ups"].tobytes(), info["downs"].tobytes()), [b.TerrainStats(t) for t in range(b.num_terrains)], info)


def assert_same_end(x, y, what):
    bad = X.same_record(x[0], y[0])
    assert bad is None, "%s: EnvState.%s differs" % (what, bad)
    assert x[1].tobytes() == y[1].tobytes(), "%s: policy states differ" % what
    assert x[2] == y[2], "%s: ground windows / build counts differ" % what
    assert x[3] == y[3], "%s: levels differ" % what
    assert x[4] == y[4], "%s: ladder records differ" % what
    assert x[5] == y[5], "%s: terrain statistics differ" % what


def ladder_run(om, monkeypatch, env, extra, run_frames=False, at_top=False):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    b = L.plain_batch(om, N, dict(terrain_gen="device"), seed=77, deal=[e % 4 for e in range(N)], **extra)
    b.TerrainLadder(0, 3, 0.3, 0.5, at_top=at_top)
    if run_frames:
        b.RunFrames(FRAMES)
    else:
        for _ in range(FRAMES):
            b.Update()
    out = end_state(b)
    info = out[6]
    assert info["ups"].sum() >= 5 and info["downs"].sum() >= 5, (info["ups"], info["downs"])
    assert info["ups"][64:].sum() + info["downs"][64:].sum() > 0, "no env of the second block moved"
    return out


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


SYMBOLS = ("dtrl_terrain_ladder", "dtrl_ladder_info")


@pytest.mark.parametrize("lib", ["libdtrl.so", "libdtrl_f32.so"])
def test_new_symbols_resolve(lib):
    lib_ = ctypes.CDLL(os.path.join(os.path.dirname(HIP_LIB), lib))
    for name in SYMBOLS:
        assert getattr(lib_, name) is not None, name
