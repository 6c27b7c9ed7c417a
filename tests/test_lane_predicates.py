"""Lane predicates of the fast kernel (dtrl_kernel_fast.h): the transposed copy of U in factorize_regs() stores whole columns without a lane mask and reads them
back under EXEC windows, and the unrolled row sequences of pgs_solve_fast() test their loop-invariant row masks per sweep (both contact models: the two-pass sweep
and the generic sweep of -warm_start= 0). Neither changes an operation, so the fast kernel stays bit for bit on the reference kernel: pose, velocity, torques, the
contact cache of every frame and EvalStats, for the three skeleton instances, with every third env lying on its back (the many-row substeps).

The env and frame counts are the smallest for which the reference kernel alone (lane-loop build, then DTRL_KERNEL=ref) fills the coverage bins asserted below:
96 envs x 12 frames for the dog and the goat; the raptor needs 30 frames to reach R > 16 (its plain loop behind the 16 register rows): 0 such frames after 12,
0 (default) / 1 (-warm_start= 0) after 20, 3 / 3 after 30."""
import numpy as np
import pytest

import test_host_and_emul as T
from conftest import REFDATA, dog_policy

pytestmark = pytest.mark.gpu

CELLS = [("args/dog_slopes_mixed_args.txt", "dog", 12), ("args/raptor_narrow_gaps_args.txt", "raptor", 30), ("args/goat_cliffs_args.txt", "goat", 12)]


@pytest.mark.parametrize("warm_start", [None, 0], ids=["default", "warm_start0"])
@pytest.mark.parametrize("arg,skel,frames", CELLS, ids=[c[1] for c in CELLS])
def test_lane_predicates_fast_equals_reference_bitwise(da, om, monkeypatch, arg, skel, frames, warm_start):
    n = 96
    pol = T.raptor_policy(om) if skel == "raptor" else dog_policy(om)
    extra = {"terrain_seed": 77}
    if warm_start is not None:
        extra["warm_start"] = warm_start

    def run(kernel):
        if kernel:
            monkeypatch.setenv("DTRL_KERNEL", kernel)
        else:
            monkeypatch.delenv("DTRL_KERNEL", raising=False)
        b = da.BatchScenario(arg, n, data_root=REFDATA, extra_args=extra)   # product path: libdtrl.so
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

    tr, qr, qdr, (tcr, tar), sr = run("ref")
    # the inputs first: the reference kernel alone fills the bins (airborne, few rows, R >= 7: rows behind the sixth of the unrolled sequences, many rows)
    hist = np.bincount(np.concatenate([t[0] for t in tr]), minlength=25)
    assert hist[0] > 0 and hist[1:7].sum() > 0 and hist[7:13].sum() > 0 and hist[13:].sum() > 0, hist.tolist()
    if skel == "raptor":
        assert hist[17:].sum() > 0, hist.tolist()   # more rows than the raptor instance's 16 register rows: the plain loop
    tf, qf, qdf, (tcf, taf), sf = run(None)
    for f, (a, b_) in enumerate(zip(tf, tr)):
        assert all(np.array_equal(x, y) for x, y in zip(a, b_)), "contact cache differs in frame %d" % f
    assert np.array_equal(qf, qr) and np.array_equal(qdf, qdr)
    assert np.array_equal(tcf, tcr) and np.array_equal(taf, tar)
    assert sf == sr
