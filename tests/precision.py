"""The precision parameter of the fast-kernel = reference-kernel tests: every case runs on the fp64 library (libdtrl.so) and on the fp32 library
(libdtrl_f32.so, `-physics_precision= f32`), which holds its own fast and reference kernels, compiled from the same source with `real` = float.

The fp64 case of a parametrised test keeps the id it had before the parameter existed (its inputs are unchanged and so is its name); the fp32 case carries the
same id with "-f32" behind it."""
import pytest

from conftest import EmulScenario, emul_f32_scenario

PRECISIONS = ("f64", "f32")


def both_precisions(cases, ids=None):
    """cases: the value tuples of a parametrize call, ids: its ids (None: pytest's own, the values joined by "-"). Returns the pytest.param list with the precision
    behind the values of every case."""
    out = []
    for k, case in enumerate(cases):
        case = case if isinstance(case, tuple) else (case,)
        name = ids[k] if ids is not None else "-".join(str(v) for v in case)
        out.append(pytest.param(*case, "f64", id=name))
        out.append(pytest.param(*case, "f32", id=name + "-f32"))
    return out


def extra_for(prec, **extra):
    """extra_args of a batch of this precision; the fp64 case passes exactly what it passed before"""
    if prec == "f32":
        extra["physics_precision"] = "f32"
    return extra


def check_build(prec):
    """the lane-loop build of this precision (conftest.EmulScenario / emul_f32_scenario)"""
    return emul_f32_scenario if prec == "f32" else EmulScenario


def assert_library(b, prec):
    """a case must not silently run the other library"""
    assert ("fp32" in b._lib.dtrl_version().decode()) == (prec == "f32"), (prec, b._lib.dtrl_version())
