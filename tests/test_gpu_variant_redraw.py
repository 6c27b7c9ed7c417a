"""Variant redraw on the product library (libdtrl.so / libdtrl_f32.so on cuda:0): the twins of tests/test_variant_redraw.py -- there the host default of
Backend::VariantRedraw, here ONE launch of dtrl_variant_redraw per env group and frame with -terrain_gen= device -- and what only exists on HIP: the kernel against
the host fallback (DTRL_VARIANTS_FALLBACK=1) at 70 envs (two 64-thread blocks, the second partial) with one and two env groups in both libraries, frames queued
without a host wait (RunFrames) against frame-by-frame Update, run-to-run determinism, the variant fast kernel against the reference kernel under redraw, and the
new symbols in both libraries."""
import ctypes
import os

import pytest

import test_external_policy as X
import test_model_variants as V
import test_terrain_sets as T
import test_variant_redraw as R
from conftest import HIP_LIB

pytestmark = pytest.mark.gpu

KNOBS = ("DTRL_KERNEL", "DTRL_TERRAINS_FALLBACK", "DTRL_SLOTS_FALLBACK", "DTRL_VARIANTS_FALLBACK", "DTRL_GROUPS")


@pytest.fixture(autouse=True)
def hip_batch(monkeypatch):
    import deepterrainrl_amd
    for mod in (R, T, V, X):
        monkeypatch.setattr(mod, "Scenario", deepterrainrl_amd.BatchScenario)   # product path: batch() now loads libdtrl.so (libdtrl_f32.so for physics_precision=f32)
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


# ---- twins ----
@pytest.mark.parametrize("weights", R.WEIGHT_CASES, ids=R.WEIGHT_IDS)
@pytest.mark.parametrize("mode", T.MODES, ids=T.MODE_IDS)
def test_keys_and_counters_equal_the_rule(da, om, tmp_path, mode, weights):
    R.test_keys_and_counters_equal_the_rule(da, om, tmp_path, mode, weights)


@pytest.mark.parametrize("mode", T.MODES, ids=T.MODE_IDS)
def test_every_episode_equals_its_single_model_run(da, om, tmp_path, mode):
    R.test_every_episode_equals_its_single_model_run(da, om, tmp_path, mode)


@pytest.mark.parametrize("mode", T.MODES, ids=T.MODE_IDS)
def test_the_reset_runs_under_the_new_model(da, om, tmp_path, mode):
    R.test_the_reset_runs_under_the_new_model(da, om, tmp_path, mode)


@pytest.mark.parametrize("mode", T.MODES, ids=T.MODE_IDS)
def test_envs_outside_the_range_are_untouched(da, om, tmp_path, mode):
    R.test_envs_outside_the_range_are_untouched(da, om, tmp_path, mode)


@pytest.mark.parametrize("mode", T.MODES, ids=T.MODE_IDS)
def test_removal(da, om, tmp_path, mode):
    R.test_removal(da, om, tmp_path, mode)


@pytest.mark.parametrize("mode", T.MODES, ids=T.MODE_IDS)
def test_batch_state_resets_and_restart(da, om, tmp_path, mode):
    R.test_batch_state_resets_and_restart(da, om, tmp_path, mode)


@pytest.mark.parametrize("mode", T.MODES, ids=T.MODE_IDS)
def test_key_ownership(da, om, tmp_path, mode):
    R.test_key_ownership(da, om, tmp_path, mode)


@pytest.mark.parametrize("mode", T.MODES, ids=T.MODE_IDS)
def test_shard_invariance(da, om, tmp_path, mode):
    R.test_shard_invariance(da, om, tmp_path, mode)


def test_refusals(da, om, tmp_path):
    R.test_refusals(da, om, tmp_path)


@pytest.mark.parametrize("mode", T.MODES, ids=T.MODE_IDS)
def test_overlapped_loop_equals_frame_by_frame(da, om, tmp_path, mode):
    R.test_overlapped_loop_equals_frame_by_frame(da, om, tmp_path, mode)


def test_train_loop_with_variants(da, om):
    """A few hundred iterations of the native trainer on the product libraries under a redraw."""
    out = R.run_train_loop_with_variants(300, 6000, trainer_device="cuda")
    assert out["iters"] >= 300, (out["frames"], out["iters"])


# ---- GPU only: 70 envs (two blocks of 64 threads, the second partial), device terrain, 3 variants, bit for bit ----
# (terrain seed 41: on the check build it gives 22 draws in fp64 and 24 in fp32 inside the issue's 40 frames, two of them in the second block)
N, FRAMES, TERRAIN_SEED = 70, 40, 41


def end_state(b):
    info = b.VariantRedrawInfo()
    return (X.env_states(b), b.RecordPoliState(), [X.ground_key(b, e) for e in range(b.num_envs)], list(b.GetVariants()), info["draws"].tobytes(),
            [b.VariantStats(v) for v in range(b.num_variants)], info)


def assert_same_end(x, y, what):
    bad = X.same_record(x[0], y[0])
    assert bad is None, "%s: EnvState.%s differs" % (what, bad)
    assert x[1].tobytes() == y[1].tobytes(), "%s: policy states differ" % what
    assert x[2] == y[2], "%s: ground windows / build counts differ" % what
    assert x[3] == y[3], "%s: variants differ" % what
    assert x[4] == y[4], "%s: draw counters differ" % what
    assert x[5] == y[5], "%s: variant statistics differ" % what


def redraw_run(om, tmp_path, monkeypatch, env, extra, run_frames=False):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    b = R.redraw_batch(om, tmp_path, N, dict(terrain_gen="device"), seed=9, weights=(1, 2, 1), terrain_seed=TERRAIN_SEED, **extra)
    if run_frames:
        b.RunFrames(FRAMES)
    else:
        for _ in range(FRAMES):
            b.Update()
    out = end_state(b)
    draws = out[6]["draws"]
    assert draws.sum() >= 5 and draws[64:].sum() >= 1, draws
    return out


@pytest.mark.parametrize("groups", ["1", "2"], ids=["one_group", "two_groups"])
@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_redraw_kernel_equals_host_fallback(da, om, tmp_path, monkeypatch, precision, groups):
    """One launch of dtrl_variant_redraw per group and frame against the rule run on the host, env by env, and the per-key launches that read the keys back from the
    device (DTRL_VARIANTS_FALLBACK=1); two groups: the second starts at a non-zero e0."""
    extra = dict(physics_precision="f32") if precision == "f32" else {}
    base = redraw_run(om, tmp_path, monkeypatch, {"DTRL_GROUPS": groups}, extra)
    assert_same_end(base, redraw_run(om, tmp_path, monkeypatch, {"DTRL_GROUPS": groups, "DTRL_VARIANTS_FALLBACK": "1"}, extra), "host fallback")


def test_queued_frames_equal_frame_by_frame_and_repeat(da, om, tmp_path, monkeypatch):
    """RunFrames -- every frame, boundary, redraw and reset launch queued, the host never waits between them -- equals frame-by-frame Update(); a second run gives the
    same bits."""
    base = redraw_run(om, tmp_path, monkeypatch, {}, {})
    assert_same_end(base, redraw_run(om, tmp_path, monkeypatch, {}, {}, run_frames=True), "RunFrames")
    assert_same_end(base, redraw_run(om, tmp_path, monkeypatch, {}, {}), "run after run")


def test_fast_kernel_equals_reference_kernel_under_redraw(da, om, tmp_path, monkeypatch):
    base = redraw_run(om, tmp_path, monkeypatch, {}, {})
    assert_same_end(base, redraw_run(om, tmp_path, monkeypatch, {"DTRL_KERNEL": "ref"}, {}), "DTRL_KERNEL=ref")


SYMBOLS = ("dtrl_variant_redraw", "dtrl_variant_redraw_info")


@pytest.mark.parametrize("lib", ["libdtrl.so", "libdtrl_f32.so"])
def test_new_symbols_resolve(lib):
    lib_ = ctypes.CDLL(os.path.join(os.path.dirname(HIP_LIB), lib))
    for name in SYMBOLS:
        assert getattr(lib_, name) is not None, name
