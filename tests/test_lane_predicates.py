"""Lane predicates of the fast kernel (dtrl_kernel_fast.h): the transposed copy of U in factorize_regs() stores whole columns without a lane mask and reads them
back under EXEC windows, and the unrolled row sequences of pgs_solve_fast() test their loop-invariant row masks per sweep (both contact models: the two-pass sweep
and the generic sweep of -warm_start= 0). Neither changes an operation, so the fast kernel stays bit for bit on the reference kernel: pose, velocity, torques, the
contact cache of every frame and EvalStats, for the three skeleton instances, with every third env lying on its back (the many-row substeps), in the fp64 library
and in the fp32 library (whose EXEC-window helpers are spelled v_fma_f32 / v_mov_b32 and whose generic sweep keeps R visible).

The env and frame counts are the smallest for which the reference kernel alone (lane-loop build, then DTRL_KERNEL=ref) fills the coverage bins asserted below:
96 envs x 12 frames for the dog and the goat; the raptor needs 30 frames to reach R > 16 (its plain loop behind the 16 register rows): 0 such frames after 12,
0 (default) / 1 (-warm_start= 0) after 20, 3 / 3 after 30.

Row counts R = 0 / 1-6 / 7-12 / 13+ (raptor: and R > 16) in the fp32 library, default | -warm_start= 0, lane-loop check build and reference kernel on the device:
  dog     check build 512 / 466 / 140 / 34 | 517 / 461 / 140 / 34, device 511 / 467 / 140 / 34 | 517 / 461 / 140 / 34
  raptor  check build 650 / 1099 / 1109 / 22 (4) | 743 / 877 / 1222 / 38 (3), device 662 / 1093 / 1097 / 28 (4) | 742 / 870 / 1224 / 44 (3)
  goat    check build 293 / 548 / 88 / 223 | 291 / 548 / 90 / 223, device 292 / 549 / 88 / 223 | 291 / 548 / 90 / 223
(fp64 on the device: raptor R > 16 in 1 | 3 frames.)"""
import numpy as np
import pytest

import test_host_and_emul as T
from conftest import REFDATA, dog_policy
from precision import both_precisions, check_build, extra_for
from product import fast_and_reference
from test_gpu_fsub_rhs import NAMES, product

CELLS = [("args/dog_slopes_mixed_args.txt", "dog", 12), ("args/raptor_narrow_gaps_args.txt", "raptor", 30), ("args/goat_cliffs_args.txt", "goat", 12)]
N_ENVS = 96


def rollout(make, pol, frames, n=N_ENVS):
    """make() -> BatchScenario. Returns the contact cache of every frame, the end state and EvalStats."""
    b = make()
    b.SetPolicy(pol[1], *pol[2:])
    b.RunFrames(2)
    # every third env is turned on its back and dropped: a character lying on the ground carries 13-24 constraint rows per substep
    q, qd = b.PoseVel()
    ids = np.arange(0, n, 3, dtype=np.int32)
    ql = q[ids].copy()
    ql[:, 2] += np.pi
    b.SetPoseVel(ql, np.zeros_like(qd[ids]), ids)
    trace = []
    for _ in range(frames):
        b.RunFrames(1)
        cnt, rid, lam = b.ContactCache()
        trace.append((cnt.copy(), rid.copy(), lam.copy()))
    qf, qdf = b.PoseVel()
    return trace, qf, qdf, b.Torques(), b.EvalStats()


def check_reached(trace, skel):
    """the inputs: the bins (airborne, few rows, R >= 7: rows behind the sixth of the unrolled sequences, many rows) are filled"""
    hist = np.bincount(np.concatenate([t[0] for t in trace]), minlength=25)
    print("row-count histogram: R = 0 / 1-6 / 7-12 / 13+ = %d / %d / %d / %d, R > 16: %d" % (hist[0], hist[1:7].sum(), hist[7:13].sum(), hist[13:].sum(), hist[17:].sum()))
    assert hist[0] > 0 and hist[1:7].sum() > 0 and hist[7:13].sum() > 0 and hist[13:].sum() > 0, hist.tolist()
    if skel == "raptor":
        assert hist[17:].sum() > 0, hist.tolist()   # more rows than the raptor instance's 16 register rows: the plain loop


def extra_of(prec, warm_start):
    extra = {"terrain_seed": 77}
    if warm_start is not None:
        extra["warm_start"] = warm_start
    return extra_for(prec, **extra)


@pytest.mark.gpu
@pytest.mark.parametrize("warm_start", [None, 0], ids=["default", "warm_start0"])
@pytest.mark.parametrize("arg,skel,frames,prec", both_precisions(CELLS, ids=[c[1] for c in CELLS]))
def test_lane_predicates_fast_equals_reference_bitwise(da, om, monkeypatch, arg, skel, frames, prec, warm_start):
    pol = T.raptor_policy(om) if skel == "raptor" else dog_policy(om)
    # (the per-frame records are the contact cache: the first three of NAMES)
    (tf, qf, qdf, (tcf, taf), sf), (tr, qr, qdr, (tcr, tar), sr) = fast_and_reference(
        monkeypatch, lambda: rollout(product(da, arg, N_ENVS, prec, **extra_of(None, warm_start)), pol, frames), NAMES[:3])
    check_reached(tr, skel)                                    # the inputs: the reference kernel alone fills the bins
    assert np.array_equal(qf, qr) and np.array_equal(qdf, qdr)
    assert np.array_equal(tcf, tcr) and np.array_equal(taf, tar)
    assert sf == sr


@pytest.mark.parametrize("warm_start", [None, 0], ids=["default", "warm_start0"])
@pytest.mark.parametrize("arg,skel,frames,prec", both_precisions(CELLS, ids=[c[1] for c in CELLS]))
def test_lane_predicates_rollout_fills_the_bins_on_the_lane_loop_build(om, arg, skel, frames, prec, warm_start):
    """The CPU twin: the same rollout through the lane-loop build of dtrl_kernel.h (of either precision) fills the bins."""
    pol = T.raptor_policy(om) if skel == "raptor" else dog_policy(om)
    trace = rollout(lambda: check_build(prec)(arg, N_ENVS, data_root=REFDATA, extra_args=extra_of(prec, warm_start)), pol, frames)[0]
    check_reached(trace, skel)
