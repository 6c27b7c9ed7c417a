"""Variant rescale on the product library (libdtrl.so / libdtrl_f32.so on cuda:0): the twins of tests/test_variant_rescale.py -- there the host default of
Backend::VariantRescale, here ONE launch of dtrl_variant_rescale per env group and frame -- and what only exists on HIP: the kernel against the host fallback
(DTRL_VARIANTS_FALLBACK=1) at 67 envs (not a multiple of 64) in two env groups, dog and raptor, both terrain modes, uniform and per-link factors, in the frames
and under Reset with a list (the listed form); the kernel against the ScaledVariant path in both libraries; frames queued without a host wait, run after run;
two shards against the whole batch; and the new symbols in both libraries."""
import pytest

import test_external_policy as X
import test_model_variants as V
import test_terrain_sets as T
import test_variant_rescale as R
from product import assert_same_end, end_state, product_batch, set_knobs, symbols_test
# ---- twins: the CPU tests themselves, collected here under the module's gpu mark and fixture ----
from test_variant_rescale import test_envs_outside_the_rescale_are_untouched, test_launch_counts, test_records_equal_the_loader_f32, test_refusals  # noqa: F401

pytestmark = pytest.mark.gpu
hip_batch = product_batch(R, T, V, X)
NOT_TWINNED = {"test_shard_invariance": "runs here as test_shards_equal_the_whole_batch: 34 + 33 envs against 67 in two env groups",
               "test_train_loop_with_rescale": "drives the check build's trainer library; had no twin before this change"}


# ---- twins under other parameters (30 frames) ----
@pytest.mark.parametrize("mode", T.MODES, ids=T.MODE_IDS)
def test_factors_equal_the_restatement(da, om, mode):
    R.test_factors_equal_the_restatement(da, om, mode, frames=30)


@pytest.mark.parametrize("mode", T.MODES, ids=T.MODE_IDS)
def test_batch_state_and_removal(da, om, mode):
    R.test_batch_state_and_removal(da, om, mode, frames=30)


# ---- HIP against the ScaledVariant path, in the fp64 library and in libdtrl_f32.so ----
@pytest.mark.parametrize("mode", T.MODES, ids=T.MODE_IDS)
def test_records_equal_the_loader(da, om, mode):
    """(no warm-up and no named env here: which env falls first is the check build's finding; 30 frames hold falls, redraws and frames behind them)"""
    R.run_records_equal_the_loader(om, R.DOG, mode, warm=0, frames=30, fall_env=None)


def test_records_equal_the_loader_f32_trajectories(da, om):
    R.run_records_equal_the_loader(om, R.DOG, dict(terrain_gen="device"), warm=0, frames=30, fall_env=None, physics_precision="f32")


# ---- the kernel against the host fallback: 67 envs, two groups ----
N, FRAMES = 67, 30
PER_LINK = [(), ("mass", "kp", "kd", "torque_lim")]
PER_LINK_IDS = ["uniform", "per_link"]


def rescale_end(b):
    info = b.VariantRescaleInfo()
    return end_state(b, info, keys=list(b.GetVariants()), episode_counters=info["episodes"].tobytes(), scalars=[b.VariantScalars(e) for e in range(b.num_envs)],
                     factors=info["factors"])


SAME = dict(scalars=R.same_scalars, factors=R.same_bits)      # how assert_same_end compares the extras that do not compare with ==


def rescale_run(om, monkeypatch, env, arg, mode, per_link, n=N, run_frames=False, min_starts=8, **more):
    """n envs under the rescale for FRAMES frames; the state at the end, and again after Reset with a list (the rule's listed form, envs of both groups)"""
    set_knobs(monkeypatch, env)
    b = R.rescaled(om, arg, n, mode, per_link=per_link, **more)
    if run_frames:
        b.RunFrames(FRAMES)
    else:
        for _ in range(FRAMES):
            b.Update()
    out = rescale_end(b)
    R.check_factors(b, per_link, base=more.get("global_env_offset", 0))
    starts = out["info"]["episodes"] - 1                     # (every env started one episode in Reset)
    print(dict(episode_starts_in_frames=int(starts.sum()), second_group=int(starts[n // 2:].sum())))
    assert starts.sum() >= min_starts, starts          # the comparison cannot pass without draws
    listed = [0, 5, n // 2, n - 1]
    b.Reset(listed + [5])
    again = rescale_end(b)
    assert list(again["info"]["episodes"] - out["info"]["episodes"]) == [1 if e in listed else 0 for e in range(n)]
    return out, again


@pytest.mark.parametrize("per_link", PER_LINK, ids=PER_LINK_IDS)
@pytest.mark.parametrize("mode", T.MODES, ids=T.MODE_IDS)
@pytest.mark.parametrize("arg", [R.DOG, R.RAPTOR], ids=["dog", "raptor"])
def test_rescale_kernel_equals_host_fallback(da, om, monkeypatch, arg, mode, per_link):
    """One launch of dtrl_variant_rescale per group and frame against the rule run on the host, env by env, with per-key frame launches (DTRL_VARIANTS_FALLBACK=1):
    the scalars of every env's record, poses and everything else of the envs, bit for bit; two groups: the second starts at a non-zero e0 and is partial."""
    hip = rescale_run(om, monkeypatch, {"DTRL_GROUPS": "2"}, arg, mode, per_link)
    host = rescale_run(om, monkeypatch, {"DTRL_GROUPS": "2", "DTRL_VARIANTS_FALLBACK": "1"}, arg, mode, per_link)
    assert_same_end(hip[0], host[0], "host fallback, after %d frames" % FRAMES, **SAME)
    assert_same_end(hip[1], host[1], "host fallback, after Reset with a list", **SAME)


def test_queued_frames_repeat(da, om, monkeypatch):
    """RunFrames -- every frame, boundary, rescale and reset launch queued, the host never waits between them -- twice: the same bits; and equal to Update()."""
    mode, pl = dict(terrain_gen="device"), PER_LINK[1]
    first = rescale_run(om, monkeypatch, {"DTRL_GROUPS": "2"}, R.DOG, mode, pl, run_frames=True)
    second = rescale_run(om, monkeypatch, {"DTRL_GROUPS": "2"}, R.DOG, mode, pl, run_frames=True)
    assert_same_end(first[0], second[0], "RunFrames, run after run", **SAME)
    assert_same_end(first[1], second[1], "RunFrames, run after run, after Reset with a list", **SAME)
    assert_same_end(first[0], rescale_run(om, monkeypatch, {"DTRL_GROUPS": "2"}, R.DOG, mode, pl)[0], "RunFrames against Update", **SAME)


def test_shards_equal_the_whole_batch(da, om, monkeypatch):
    """Shards of 34 + 33 envs (the second created with the global-id offset) against 67 envs in one batch."""
    mode, pl = dict(terrain_gen="device"), PER_LINK[1]
    whole = rescale_run(om, monkeypatch, {"DTRL_GROUPS": "2"}, R.DOG, mode, pl)[0]
    lo = rescale_run(om, monkeypatch, {}, R.DOG, mode, pl, n=34, min_starts=1)[0]
    hi = rescale_run(om, monkeypatch, {}, R.DOG, mode, pl, n=33, min_starts=1, global_env_offset=34)[0]
    for g in range(N):
        s, e = (lo, g) if g < 34 else (hi, g - 34)
        bad = X.same_record(whole["env_states"][g], s["env_states"][e])
        assert bad is None, "global env %d: EnvState.%s differs between the shard and the whole batch" % (g, bad)
        assert whole["poli_state"][g].tobytes() == s["poli_state"][e].tobytes() and whole["ground"][g] == s["ground"][e], g
        assert R.same_scalars([whole["scalars"][g]], [s["scalars"][e]]) and R.same_bits(whole["factors"][g], s["factors"][e]), g
    assert whole["episode_counters"] == lo["episode_counters"] + hi["episode_counters"]


test_new_symbols_resolve = symbols_test(("dtrl_variant_rescale", "dtrl_variant_rescale_info", "dtrl_variant_scalars"))
