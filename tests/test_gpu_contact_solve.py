"""Contact solve of the fast kernel with a solving substep's row data kept on its lanes and the Gauss-Seidel passes in slot order (dtrl_kernel_fast.h: the row count
travels as a wave-uniform argument, warm_match_fast() takes the cached ids from the lanes, the residual's velocity term comes from a per-lane descriptor batch, the
Delassus tail hands the row residual to pgs_solve_fast() in a register, and each pass of a sweep walks its own rows only; the velocity update is the loop it was,
docs/EXPERIMENTS.md 38): bit for bit the reference kernel (DTRL_KERNEL=ref: warm_match() / build_delassus() / pgs_solve() /
finish_substep() of dtrl_kernel.h), after every frame, for the three skeleton instances and both libraries.

The rollout is the one of test_gpu_fsub_rhs.py (192 envs, 30 frames, terrain seed 77; envs on their backs, with a folded leg, on their noses in the ground, pushed).
What it is made to reach is asserted on the REFERENCE kernel's run, per env-frame, from ContactCache() after the frame (the rows of the last solved substep):
  (a) 1 <= count <= 15: the one-tile MFMA form of the Delassus product
  (b) count >= 17: the general Delassus path and, on the raptor (16 register rows), the plain Gauss-Seidel loop
  (c) count == 1
  (d) count == 0 in a frame after one with count > 0: the cache is cleared
  (e) a ground row (id < 512) with a non-zero cached impulse: the next substep's warm start
  (f) a ground normal row (even id) with impulse exactly 0 followed by its tangent (id + 1): a held friction row
  (g) the same with impulse > 0: a loaded friction row
  (h) the five conditions of test_gpu_fsub_rhs.py: limit row, link--link pair, the 24-row cap, airborne, pushed with rows.
Env-frames that reached (a) .. (g) on the fp64 lane-loop build: dog 4081 / 276 / 203 / 636 / 3090 / 1306 / 2897, raptor 3770 / 592 / 516 / 406 / 3151 / 1144 / 2900,
goat 4413 / 693 / 467 / 399 / 3440 / 2076 / 3114 (the fp32 one: within 6 % of these, every case reached)."""
import numpy as np
import pytest

import test_gpu_fsub_rhs as F
from conftest import REFDATA
from precision import both_precisions, check_build, extra_for
from product import fast_and_reference

GROUND_IDS = F.FIRST_PAIR_ROW_ID      # ground contact rows: 2 x sample point + (0 normal, 1 tangent)


def solve_cases(frames):
    """env-frames of a rollout (F.rollout()'s per-frame records) that reached (a) .. (g)"""
    got = dict.fromkeys("abcdefg", 0)
    prev = None
    for rec in frames:
        cnt, rid, lam = (np.asarray(x) for x in rec[:3])
        rid = rid.astype(np.int64)
        live = np.arange(rid.shape[1])[None, :] < cnt[:, None]
        ground = live & (rid < GROUND_IDS)
        got["a"] += int(((cnt >= 1) & (cnt <= 15)).sum())
        got["b"] += int((cnt >= 17).sum())
        got["c"] += int((cnt == 1).sum())
        if prev is not None:
            got["d"] += int(((cnt == 0) & (prev > 0)).sum())
        got["e"] += int((ground & (lam != 0)).any(axis=1).sum())
        pair = ground[:, :-1] & (rid[:, :-1] % 2 == 0) & live[:, 1:] & (rid[:, 1:] == rid[:, :-1] + 1)   # a normal row and its tangent behind it
        got["f"] += int((pair & (lam[:, :-1] == 0)).any(axis=1).sum())
        got["g"] += int((pair & (lam[:, :-1] > 0)).any(axis=1).sum())
        prev = cnt.copy()
    return got


def check_solve_cases(got):
    print("env-frames that reached (a) .. (g): %s" % got)
    for what, count in got.items():
        assert count >= 1, (what, got)


@pytest.mark.gpu
@pytest.mark.parametrize("arg,skel,prec", both_precisions(F.CASES))
def test_contact_solve_fast_equals_reference_bitwise(da, om, monkeypatch, arg, skel, prec):
    pol = F.policy_of(om, skel)
    (ff, rf), (fr, rr) = fast_and_reference(monkeypatch, lambda: F.rollout(F.product(da, arg, F.N_ENVS, prec, terrain_seed=F.TERRAIN_SEED), pol, skel), F.NAMES)
    check_solve_cases(solve_cases(fr))
    F.check_reached(rr)
    assert len(ff) == len(fr) == F.FRAMES
    assert rf == rr


@pytest.mark.parametrize("arg,skel,prec", both_precisions(F.CASES))
def test_contact_solve_rollout_reaches_every_case_on_the_lane_loop_build(om, arg, skel, prec):
    """The CPU twin: the same rollout through the lane-loop build of dtrl_kernel.h (of either precision) reaches (a) .. (h). It does not run the fast code, which
    exists on the device only."""
    pol = F.policy_of(om, skel)
    frames, reached = F.rollout(lambda: check_build(prec)(arg, F.N_ENVS, data_root=REFDATA, extra_args=extra_for(prec, terrain_seed=F.TERRAIN_SEED)), pol, skel)
    check_solve_cases(solve_cases(frames))
    F.check_reached(reached)
