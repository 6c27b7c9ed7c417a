"""Row-per-lane first substitution of the fast kernel (dtrl_kernel_fast.h: usolve_rows for substeps with constraint rows, the register chain for
substeps without): bit for bit the reference kernel's forward_subst_rows(), on both sides of the cutover and on the many-row substeps of characters
lying on the ground, for the three skeleton instances, in the fp64 library and in the fp32 library (whose bcast() and wave_shr1() move one register
where the fp64 ones move a lo/hi pair).

Row counts R = 0 / 1-6 / 7-12 / 13+, asserted on the reference kernel's run; in the fp32 library, lane-loop check build | reference kernel on the device:
  dog 1695 / 3329 / 674 / 62 | 1698 / 3368 / 629 / 65, raptor 1306 / 2181 / 2227 / 46 | 1326 / 2187 / 2193 / 54, goat 759 / 2755 / 1573 / 673 | 763 / 2745 / 1584 / 668."""
import numpy as np
import pytest

import test_host_and_emul as T
from conftest import REFDATA, dog_policy
from precision import both_precisions, check_build, extra_for
from product import fast_and_reference
from test_gpu_fsub_rhs import NAMES, product

CASES = [("args/dog_slopes_mixed_args.txt", "dog"), ("args/raptor_narrow_gaps_args.txt", "raptor"), ("args/goat_cliffs_args.txt", "goat")]
N_ENVS, FRAMES = 192, 30


def rollout(make, pol, n=N_ENVS, frames=FRAMES):
    """make() -> BatchScenario. Returns the contact cache of every frame, the row counts of all frames, the end state and EvalStats."""
    b = make()
    b.SetPolicy(pol[1], *pol[2:])
    b.RunFrames(2)
    # every third env is turned on its back and dropped: a character lying on the ground carries 13-24 constraint rows per substep
    q, qd = b.PoseVel()
    ids = np.arange(0, n, 3, dtype=np.int32)
    ql = q[ids].copy()
    ql[:, 2] += np.pi
    b.SetPoseVel(ql, np.zeros_like(qd[ids]), ids)
    counts, trace = [], []
    for _ in range(frames):
        b.RunFrames(1)
        cnt, rid, lam = b.ContactCache()
        counts.append(cnt.copy())
        trace.append((cnt, rid, lam))
    qf, qdf = b.PoseVel()
    return trace, np.concatenate(counts), qf, qdf, b.Torques(), b.EvalStats()


def check_reached(counts):
    """the run covered airborne substeps (R = 0: register chain), the row form's few-row and many-row substeps"""
    hist = np.bincount(counts, minlength=25)
    print("row-count histogram: R = 0 / 1-6 / 7-12 / 13+ = %d / %d / %d / %d" % (hist[0], hist[1:7].sum(), hist[7:13].sum(), hist[13:].sum()))
    assert hist[0] > 0 and hist[1:7].sum() > 0 and hist[7:13].sum() > 0 and hist[13:].sum() > 0, hist.tolist()


@pytest.mark.gpu
@pytest.mark.parametrize("arg,skel,prec", both_precisions(CASES))
def test_fsub_rows_fast_equals_reference_bitwise(da, om, monkeypatch, arg, skel, prec):
    pol = T.raptor_policy(om) if skel == "raptor" else dog_policy(om)
    # (the per-frame records are the contact cache: the first three of NAMES)
    (tf, cf, qf, qdf, (tcf, taf), sf), (tr, cr, qr, qdr, (tcr, tar), sr) = fast_and_reference(
        monkeypatch, lambda: rollout(product(da, arg, N_ENVS, prec, terrain_seed=77), pol), NAMES[:3])
    check_reached(cr)                                          # on the reference kernel's run: the condition does not depend on the code under test
    assert np.array_equal(qf, qr) and np.array_equal(qdf, qdr) and np.array_equal(tcf, tcr) and np.array_equal(taf, tar)
    assert sf == sr
    assert np.array_equal(cf, cr)


@pytest.mark.parametrize("arg,skel,prec", both_precisions(CASES))
def test_fsub_rows_rollout_fills_the_bins_on_the_lane_loop_build(om, arg, skel, prec):
    """The CPU twin: the same rollout through the lane-loop build of dtrl_kernel.h (of either precision) fills the bins."""
    pol = T.raptor_policy(om) if skel == "raptor" else dog_policy(om)
    counts = rollout(lambda: check_build(prec)(arg, N_ENVS, data_root=REFDATA, extra_args=extra_for(prec, terrain_seed=77)), pol)[1]
    check_reached(counts)
