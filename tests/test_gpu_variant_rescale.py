"""Variant rescale on the product library (libdtrl.so / libdtrl_f32.so on cuda:0): the twins of tests/test_variant_rescale.py -- there the host default of
Backend::VariantRescale, here ONE launch of dtrl_variant_rescale per env group and frame -- and what only exists on HIP: the kernel against the host fallback
(DTRL_VARIANTS_FALLBACK=1) at 67 envs (not a multiple of 64) in two env groups, dog and raptor, both terrain modes, uniform and per-link factors, in the frames
and under Reset with a list (the listed form); the kernel against the ScaledVariant path in both libraries; frames queued without a host wait, run after run;
two shards against the whole batch; and the new symbols in both libraries."""
import ctypes
import os

import numpy as np
import pytest

import test_external_policy as X
import test_model_variants as V
import test_terrain_sets as T
import test_variant_rescale as R
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
@pytest.mark.parametrize("mode", T.MODES, ids=T.MODE_IDS)
def test_factors_equal_the_restatement(da, om, mode):
    R.test_factors_equal_the_restatement(da, om, mode, frames=30)


@pytest.mark.parametrize("mode", T.MODES, ids=T.MODE_IDS)
def test_envs_outside_the_rescale_are_untouched(da, om, tmp_path, mode):
    R.test_envs_outside_the_rescale_are_untouched(da, om, tmp_path, mode)


def test_refusals(da, om, tmp_path):
    R.test_refusals(da, om, tmp_path)


@pytest.mark.parametrize("mode", T.MODES, ids=T.MODE_IDS)
def test_batch_state_and_removal(da, om, mode):
    R.test_batch_state_and_removal(da, om, mode, frames=30)


def test_launch_counts(da, om, tmp_path):
    R.test_launch_counts(da, om, tmp_path)


# ---- HIP against the ScaledVariant path, in the fp64 library and in libdtrl_f32.so ----
@pytest.mark.parametrize("mode", T.MODES, ids=T.MODE_IDS)
def test_records_equal_the_loader(da, om, mode):
    """(no warm-up and no named env here: which env falls first is the check build's finding; 30 frames hold falls, redraws and frames behind them)"""
    R.run_records_equal_the_loader(om, R.DOG, mode, warm=0, frames=30, fall_env=None)


def test_records_equal_the_loader_f32(da, om):
    R.test_records_equal_the_loader_f32(da, om)


def test_records_equal_the_loader_f32_trajectories(da, om):
    R.run_records_equal_the_loader(om, R.DOG, dict(terrain_gen="device"), warm=0, frames=30, fall_env=None, physics_precision="f32")


# ---- the kernel against the host fallback: 67 envs, two groups ----
N, FRAMES = 67, 30
PER_LINK = [(), ("mass", "kp", "kd", "torque_lim")]
PER_LINK_IDS = ["uniform", "per_link"]


def end_state(b):
    info = b.VariantRescaleInfo()
    return (X.env_states(b), b.RecordPoliState(), [X.ground_key(b, e) for e in range(b.num_envs)], list(b.GetVariants()), info["episodes"].tobytes(),
            [b.VariantScalars(e) for e in range(b.num_envs)], info)


def assert_same_end(x, y, what):
    bad = X.same_record(x[0], y[0])
    assert bad is None, "%s: EnvState.%s differs" % (what, bad)
    assert x[1].tobytes() == y[1].tobytes(), "%s: policy states differ" % what
    assert x[2] == y[2], "%s: ground windows / build counts differ" % what
    assert x[3] == y[3] and x[4] == y[4], "%s: keys or episode counters differ" % what
    assert R.same_scalars(x[5], y[5]), "%s: the scalars of a model record differ" % what
    assert R.same_bits(x[6]["factors"], y[6]["factors"]), "%s: factors differ" % what


def rescale_run(om, monkeypatch, env, arg, mode, per_link, n=N, run_frames=False, min_starts=8, **more):
    """n envs under the rescale for FRAMES frames; the state at the end, and again after Reset with a list (the rule's listed form, envs of both groups)"""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    b = R.rescaled(om, arg, n, mode, per_link=per_link, **more)
    if run_frames:
        b.RunFrames(FRAMES)
    else:
        for _ in range(FRAMES):
            b.Update()
    out = end_state(b)
    R.check_factors(b, per_link, base=more.get("global_env_offset", 0))
    starts = out[6]["episodes"] - 1                     # (every env started one episode in Reset)
    print(dict(episode_starts_in_frames=int(starts.sum()), second_group=int(starts[n // 2:].sum())))
    assert starts.sum() >= min_starts, starts          # the comparison cannot pass without draws
    listed = [0, 5, n // 2, n - 1]
    b.Reset(listed + [5])
    again = end_state(b)
    assert list(again[6]["episodes"] - out[6]["episodes"]) == [1 if e in listed else 0 for e in range(n)]
    return out, again


@pytest.mark.parametrize("per_link", PER_LINK, ids=PER_LINK_IDS)
@pytest.mark.parametrize("mode", T.MODES, ids=T.MODE_IDS)
@pytest.mark.parametrize("arg", [R.DOG, R.RAPTOR], ids=["dog", "raptor"])
def test_rescale_kernel_equals_host_fallback(da, om, monkeypatch, arg, mode, per_link):
    """One launch of dtrl_variant_rescale per group and frame against the rule run on the host, env by env, with per-key frame launches (DTRL_VARIANTS_FALLBACK=1):
    the scalars of every env's record, poses and everything else of the envs, bit for bit; two groups: the second starts at a non-zero e0 and is partial."""
    hip = rescale_run(om, monkeypatch, {"DTRL_GROUPS": "2"}, arg, mode, per_link)
    host = rescale_run(om, monkeypatch, {"DTRL_GROUPS": "2", "DTRL_VARIANTS_FALLBACK": "1"}, arg, mode, per_link)
    assert_same_end(hip[0], host[0], "host fallback, after %d frames" % FRAMES)
    assert_same_end(hip[1], host[1], "host fallback, after Reset with a list")


def test_queued_frames_repeat(da, om, monkeypatch):
    """RunFrames -- every frame, boundary, rescale and reset launch queued, the host never waits between them -- twice: the same bits; and equal to Update()."""
    mode, pl = dict(terrain_gen="device"), PER_LINK[1]
    first = rescale_run(om, monkeypatch, {"DTRL_GROUPS": "2"}, R.DOG, mode, pl, run_frames=True)
    second = rescale_run(om, monkeypatch, {"DTRL_GROUPS": "2"}, R.DOG, mode, pl, run_frames=True)
    assert_same_end(first[0], second[0], "RunFrames, run after run")
    assert_same_end(first[1], second[1], "RunFrames, run after run, after Reset with a list")
    assert_same_end(first[0], rescale_run(om, monkeypatch, {"DTRL_GROUPS": "2"}, R.DOG, mode, pl)[0], "RunFrames against Update")


def test_shards_equal_the_whole_batch(da, om, monkeypatch):
    """Shards of 34 + 33 envs (the second created with the global-id offset) against 67 envs in one batch."""
    mode, pl = dict(terrain_gen="device"), PER_LINK[1]
    whole = rescale_run(om, monkeypatch, {"DTRL_GROUPS": "2"}, R.DOG, mode, pl)[0]
    lo = rescale_run(om, monkeypatch, {}, R.DOG, mode, pl, n=34, min_starts=1)[0]
    hi = rescale_run(om, monkeypatch, {}, R.DOG, mode, pl, n=33, min_starts=1, global_env_offset=34)[0]
    for g in range(N):
        s, e = (lo, g) if g < 34 else (hi, g - 34)
        bad = X.same_record(whole[0][g], s[0][e])
        assert bad is None, "global env %d: EnvState.%s differs between the shard and the whole batch" % (g, bad)
        assert whole[1][g].tobytes() == s[1][e].tobytes() and whole[2][g] == s[2][e], g
        assert R.same_scalars([whole[5][g]], [s[5][e]]) and R.same_bits(whole[6]["factors"][g], s[6]["factors"][e]), g
    assert whole[4] == lo[4] + hi[4]


SYMBOLS = ("dtrl_variant_rescale", "dtrl_variant_rescale_info", "dtrl_variant_scalars")


@pytest.mark.parametrize("lib", ["libdtrl.so", "libdtrl_f32.so"])
def test_new_symbols_resolve(lib):
    lib_ = ctypes.CDLL(os.path.join(os.path.dirname(HIP_LIB), lib))
    for name in SYMBOLS:
        assert getattr(lib_, name) is not None, name
