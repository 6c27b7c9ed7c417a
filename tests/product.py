"""What the GPU test modules (tests/test_gpu_*.py) share: the library's per-call A/B switches and how a test clears and sets them, the autouse fixture that points
the CPU test modules at the product library, the end-of-run state two runs are compared in, the symbol test, and the fast-against-reference run of the frame-kernel
tests. A plain module beside precision.py; tests/test_product_helpers.py checks it without a GPU."""
import ctypes
import os

import numpy as np
import pytest

import test_external_policy as X
from conftest import HIP_LIB

# every switch the library reads per call (deepterrainrl_amd/csrc: test_product_helpers.py holds this tuple to the sources)
ALL_KNOBS = ("DTRL_KERNEL", "DTRL_GROUPS") + tuple("DTRL_%s_FALLBACK" % k for k in (
    "SNAPSHOT", "SLOTS", "VARIANTS", "TERRAINS", "PUSH", "PERTURB", "EPISODE", "TRACE", "EPISODE_LOG"))


def set_knobs(monkeypatch, env):
    """Exactly `env` of the switches is set: none comes from the environment the tests were started in or from an earlier call."""
    for k in ALL_KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def product_batch(*modules):
    """hip_batch = product_batch(R, T, ...) at module level: the autouse fixture under which batch() of the named CPU test modules loads libdtrl.so (libdtrl_f32.so
    for physics_precision=f32) and no switch is set."""
    @pytest.fixture(autouse=True)
    def hip_batch(monkeypatch):
        import deepterrainrl_amd
        for mod in modules:
            monkeypatch.setattr(mod, "Scenario", deepterrainrl_amd.BatchScenario)
        set_knobs(monkeypatch, {})
    return hip_batch


def end_state(b, info=None, **extras):
    """What two runs are compared in: every env's EnvState record, the policy states, every env's ground window and build count, and the module's own named
    `extras` (bytes, lists, dicts: whatever compares with ==, or with the predicate the module hands assert_same_end). `info` travels along uncompared, for the
    run's own coverage assertions."""
    out = {"env_states": X.env_states(b), "poli_state": b.RecordPoliState(), "ground": [X.ground_key(b, e) for e in range(b.num_envs)], "info": info}
    assert not set(extras) & set(out), extras.keys()
    out.update(extras)
    return out


def assert_same_end(x, y, what, **same):
    """same: extra name -> predicate, for the extras that do not compare with =="""
    for e in range(len(x["env_states"])):
        bad = X.same_record(x["env_states"][e], y["env_states"][e])
        assert bad is None, "%s: env %d: EnvState.%s differs" % (what, e, bad)
    assert x["poli_state"].tobytes() == y["poli_state"].tobytes(), "%s: policy states differ" % what
    assert x["ground"] == y["ground"], "%s: ground windows / build counts differ" % what
    assert x.keys() == y.keys() and set(same) <= set(x), "%s: %s on one side only" % (what, sorted(set(x) ^ set(y) | set(same) - set(x)))
    for k in x:
        if k not in ("env_states", "poli_state", "ground", "info"):
            assert same[k](x[k], y[k]) if k in same else x[k] == y[k], "%s: %s differ" % (what, k)


def symbols_test(names):
    """test_new_symbols_resolve = symbols_test((...)): the names resolve in both product libraries"""
    @pytest.mark.parametrize("lib", ["libdtrl.so", "libdtrl_f32.so"])
    def test_new_symbols_resolve(lib):
        lib_ = ctypes.CDLL(os.path.join(os.path.dirname(HIP_LIB), lib))
        for name in names:
            assert getattr(lib_, name) is not None, name
    return test_new_symbols_resolve


def fast_and_reference(monkeypatch, run, names):
    """run() -> (per-frame records, ...) under the fast kernel (DTRL_KERNEL unset), then under the reference kernel (DTRL_KERNEL=ref): every field of every frame's
    record is the same array, `names` naming them. Returns both results for what the test asserts beyond the frames."""
    set_knobs(monkeypatch, {})
    fast = run()
    set_knobs(monkeypatch, {"DTRL_KERNEL": "ref"})
    ref = run()
    assert len(fast[0]) == len(ref[0]) > 0
    for f, (a, b_) in enumerate(zip(fast[0], ref[0])):
        assert len(a) == len(b_) == len(names), (len(a), len(b_), names)
        for name, x, y in zip(names, a, b_):
            assert np.array_equal(x, y), "frame %d: %s differ" % (f, name)
    return fast, ref
