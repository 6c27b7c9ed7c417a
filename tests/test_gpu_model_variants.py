"""Model variants on the product library (libdtrl.so / libdtrl_f32.so on cuda:0): the twins of tests/test_model_variants.py -- there the per-variant default,
here ONE launch of the variant kernels (dtrl_backend_hip_variants.hip) against the shipped single-model kernels -- and what only exists on HIP: the variant fast
kernels against the variant reference kernel and the per-variant fallback, two env groups, device terrain, and free-running variants against the CPU oracle."""
import numpy as np
import pytest

import test_model_variants as T
from conftest import REFDATA
from precision import assert_library, both_precisions, extra_for
from product import assert_same_end, end_state, product_batch, set_knobs
# ---- twins: the CPU tests themselves, collected here under the module's gpu mark and fixture ----
from test_model_variants import (test_batch_state_and_host_readers, test_batch_without_variants_launches_as_before, test_exp_scenario_tuples, test_refusals,  # noqa: F401
                                 test_scaled_variant_equals_the_file, test_variant_stats, test_variant_stats_more_variants_than_one_window)

pytestmark = pytest.mark.gpu
hip_batch = product_batch(T)
NOT_TWINNED = {}


# ---- the twin with cases of its own: both libraries ----
F32_CASES = [(T.DOG, dict(terrain_seed=11, physics_precision="f32")), (T.RAPTOR, dict(terrain_seed=5, physics_precision="f32"))]


@pytest.mark.parametrize("arg,extra", T.EQUAL_CASES + F32_CASES, ids=T.EQUAL_IDS + ["dog_f32", "raptor_f32"])
def test_equals_single_model_runs(da, om, tmp_path, arg, extra):
    T.run_equals_single_model(om, tmp_path, arg, extra)


# ---- cross-checks: 192 envs, 3 variants, 90 frames, bit for bit ----
def variant_run(om, monkeypatch, tmp_path, arg, env, extra, n=192, frames=90):
    set_knobs(monkeypatch, env)
    b = T.with_variants(om, arg, n, T.write_variants(tmp_path, arg), [e % 3 for e in range(n)], dict(terrain_seed=77, rand_seed=4, **extra))
    assert_library(b, extra.get("physics_precision", "f64"))
    for _ in range(frames):
        b.Update()
    ev, variants = b.EvalStats(), [b.VariantStats(v) for v in range(b.num_variants)]
    assert ev["cycles"] > n and ev["resets"] > 0 and all(s["cycles"] > 0 for s in variants)
    return end_state(b, statistics=(ev, variants))


@pytest.mark.parametrize("arg,prec", both_precisions([T.DOG, T.RAPTOR], ids=["dog", "raptor"]))
def test_variant_fast_kernel_equals_variant_reference_kernel_and_per_variant_fallback(da, om, monkeypatch, tmp_path, arg, prec):
    """One launch of the register-resident variant kernel against one launch of the LDS-phase variant kernel (DTRL_KERNEL=ref) and against the per-variant launches
    of the SHIPPED single-model kernels (DTRL_VARIANTS_FALLBACK=1). In libdtrl.so and in libdtrl_f32.so."""
    extra = extra_for(prec)
    base = variant_run(om, monkeypatch, tmp_path, arg, {}, extra)
    assert_same_end(base, variant_run(om, monkeypatch, tmp_path, arg, {"DTRL_KERNEL": "ref"}, extra), "variant reference kernel")
    assert_same_end(base, variant_run(om, monkeypatch, tmp_path, arg, {"DTRL_VARIANTS_FALLBACK": "1"}, extra), "per-variant fallback")


def test_two_env_groups(da, om, monkeypatch, tmp_path):
    """DTRL_GROUPS=2: two streams, two launch lists, the same bits."""
    assert_same_end(variant_run(om, monkeypatch, tmp_path, T.DOG, {}, {}), variant_run(om, monkeypatch, tmp_path, T.DOG, {"DTRL_GROUPS": "2"}, {}), "two env groups")


def test_device_terrain_one_launch_equals_fallback(da, om, monkeypatch, tmp_path):
    """-terrain_gen= device (no host wait between frames, launch order computed on the device): one launch of the variant kernel against the per-variant fallback."""
    extra = dict(terrain_gen="device")
    assert_same_end(variant_run(om, monkeypatch, tmp_path, T.RAPTOR, {}, extra), variant_run(om, monkeypatch, tmp_path, T.RAPTOR, {"DTRL_VARIANTS_FALLBACK": "1"}, extra), "device terrain")


# ---- against the oracle ----
@pytest.mark.parametrize("arg,seed", [(T.DOG, 1000), (T.RAPTOR, 5000)], ids=["dog", "raptor"])
def test_variants_track_the_oracle_1200_substeps(da, om, tmp_path, arg, seed, n=16, frames=12):
    """16 envs, 8 in v1 and 8 in v2, xavier policy, 12 frames = 1200 substeps free-running; every env is held against an OracleEnv built from its variant's
    character file. Per frame |dq| and |dqd| < 1e-6, the bound test_config1_slopes_mixed_1200_substeps_64_envs holds the nominal model to (the oracle against
    itself nudged by 1e-13 stays within 5e-10 over this horizon for every one of these variants: the bound is far above the chaos floor). No env is excused.
    The envs start as a batch of their own model starts them: the creation-time initialisation ran under the nominal model (it records a centre of mass), so each
    half takes the initial state of a plain batch created with its variant's file."""
    paths = T.write_variants(tmp_path, arg)
    pol = T.policy_for(om, arg)
    assign = [1] * (n // 2) + [2] * (n - n // 2)
    b = T.batch(arg, n, terrain_seed=seed)
    b.SetPolicy(pol[1], *pol[2:])
    b.CreateVariants(3)
    for v in (1, 2):
        b.LoadVariant(v, paths[v])
        fresh = T.batch(arg, n, terrain_seed=seed, character_file=paths[v])
        envs = [e for e in range(n) if assign[e] == v]
        snap = fresh.SaveState(envs)
        blob = snap.export(); snap.free()
        s = b.ImportState(blob); b.RestoreState(s); s.free()
    b.AssignVariants(None, assign)
    models = {v: om.build_model(arg, REFDATA, overrides={"character_file": paths[v]})[0] for v in (1, 2)}
    es = [om.OracleEnv(models[assign[i]], terrain_seed=seed + i, rng_seed=0, env_id=i, policy=pol) for i in range(n)]
    worst = 0.0
    for f in range(frames):
        b.Update()
        for e in es:
            e.update()
        q, qd = b.PoseVel()
        for i, e in enumerate(es):
            qo, qdo = e.pose_vel()
            dq, dqd = np.abs(q[i] - qo).max(), np.abs(qd[i] - qdo).max()
            worst = max(worst, dq, dqd)
            assert dq < 1e-6 and dqd < 1e-6, "frame %d env %d (variant %d): |dq| %.3e |dqd| %.3e" % (f, i, assign[i], dq, dqd)
    print("%s, %d envs in v1 / v2 x 1200 substeps: max |dq|, |dqd| = %.3e" % (arg, n, worst))
