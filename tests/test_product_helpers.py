"""tests/product.py, without a GPU and without a library: the knob list against the sources, every GPU module's twin list against its CPU module, and the two
helpers that decide what a cross-check compares."""
import glob
import importlib
import os
import re

import numpy as np
import pytest

import product
from conftest import REPO

TESTS = os.path.dirname(os.path.abspath(__file__))
# tests/test_gpu_<feature>.py pairs with tests/test_<feature>.py wherever both exist: a new feature's pair is held to the rule below without being listed here
PAIRS = sorted((os.path.basename(g)[:-3], "test_" + os.path.basename(g)[9:-3]) for g in glob.glob(os.path.join(TESTS, "test_gpu_*.py"))
               if os.path.exists(os.path.join(TESTS, "test_" + os.path.basename(g)[9:])))


def test_all_knobs_are_the_switches_the_sources_read():
    found = {"DTRL_KERNEL", "DTRL_GROUPS"}
    for ext in ("h", "hip", "cpp"):
        for path in glob.glob(os.path.join(REPO, "deepterrainrl_amd", "csrc", "*." + ext)):
            found.update(re.findall(r'"(DTRL_\w+_FALLBACK)"', open(path).read()))
    assert len(found) > 2, "no fallback switch found: the sources moved"
    assert set(product.ALL_KNOBS) == found and len(set(product.ALL_KNOBS)) == len(product.ALL_KNOBS), sorted(found ^ set(product.ALL_KNOBS))


def test_the_pairs_are_found():
    assert len(PAIRS) >= 11 and ("test_gpu_variant_redraw", "test_variant_redraw") in PAIRS, PAIRS


@pytest.mark.parametrize("gpu,cpu", PAIRS, ids=[p[1][5:] for p in PAIRS])
def test_every_cpu_test_is_twinned_or_has_a_reason(gpu, cpu):
    g, c = importlib.import_module(gpu), importlib.import_module(cpu)
    cpu_tests = {k for k, v in vars(c).items() if k.startswith("test_") and callable(v) and getattr(v, "__module__", None) == cpu}
    assert cpu_tests, cpu
    twinned = {k for k in cpu_tests if callable(getattr(g, k, None))}
    left_out = g.NOT_TWINNED
    assert cpu_tests - twinned - set(left_out) == set(), "%s: neither twinned in %s nor in its NOT_TWINNED" % (sorted(cpu_tests - twinned - set(left_out)), gpu)
    assert set(left_out) & twinned == set(), "%s: twinned and in NOT_TWINNED" % sorted(set(left_out) & twinned)
    assert set(left_out) <= cpu_tests, "%s: NOT_TWINNED names no test of %s" % (sorted(set(left_out) - cpu_tests), cpu)
    assert all(isinstance(r, str) and r.strip() for r in left_out.values()), left_out


class Env(dict):
    """monkeypatch's delenv / setenv on a dict"""
    def delenv(self, k, raising=True):
        self.pop(k, None)

    def setenv(self, k, v):
        self[k] = v


def test_set_knobs_leaves_nothing_of_an_earlier_call_or_of_the_environment():
    env = Env(DTRL_SNAPSHOT_FALLBACK="1", DTRL_GROUPS="2", HOME="/somewhere")
    product.set_knobs(env, {"DTRL_KERNEL": "ref", "DTRL_TRACE_FALLBACK": "1"})
    assert env == {"HOME": "/somewhere", "DTRL_KERNEL": "ref", "DTRL_TRACE_FALLBACK": "1"}
    product.set_knobs(env, {"DTRL_GROUPS": "1"})
    assert env == {"HOME": "/somewhere", "DTRL_GROUPS": "1"}
    product.set_knobs(env, {})
    assert env == {"HOME": "/somewhere"}


def synthetic_end(**extras):
    """what product.end_state() returns, made by hand: 3 envs"""
    st = np.zeros(3, dtype=[("q", np.float64, 4), ("num_resets", np.int32)])
    st["q"] = np.arange(12.0).reshape(3, 4)
    out = {"env_states": st, "poli_state": np.arange(6.0).reshape(3, 2), "ground": [([(0.0, 1.0, b"ab")], e) for e in range(3)], "info": {"not": "compared"}}
    out.update(extras)
    return out


def same_bits(a, b):
    return np.asarray(a).tobytes() == np.asarray(b).tobytes()


def test_assert_same_end_passes_on_equal_states_and_names_what_differs():
    mk = lambda: synthetic_end(levels=[0, 1, 2], counters=np.arange(3).tobytes(), factors=np.array([1.0, np.nan, 3.0]))
    x, y = mk(), mk()
    y["info"] = {"never": "looked at"}
    product.assert_same_end(x, y, "equal", factors=same_bits)        # (a NaN equals itself under the module's predicate)

    def fails(change, needle, **same):
        y = mk()
        change(y)
        with pytest.raises(AssertionError) as err:
            product.assert_same_end(x, y, "run B", factors=same_bits, **same)
        assert "run B" in str(err.value) and needle in str(err.value), str(err.value)

    fails(lambda y: y.update(levels=[0, 1, 3]), "levels")
    fails(lambda y: y.update(counters=np.array([0, 1, 3]).tobytes()), "counters")
    fails(lambda y: y.update(factors=np.array([1.0, np.nan, 3.5])), "factors")
    fails(lambda y: y["env_states"]["q"].__setitem__((2, 1), -0.0 if x["env_states"]["q"][2, 1] == 0 else 99.0), "env 2: EnvState.q")
    fails(lambda y: y["env_states"]["num_resets"].__setitem__(1, 5), "env 1: EnvState.num_resets")
    fails(lambda y: y["poli_state"].__setitem__((0, 0), 7.0), "policy states")
    fails(lambda y: y["ground"].__setitem__(1, ([(0.0, 1.0, b"ab")], 9)), "ground windows")
    fails(lambda y: y.pop("levels"), "levels")                        # an extra taken on one side only
    fails(lambda y: None, "levels", levels=lambda a, b: False)       # the module's predicate decides, not ==
