"""Row-per-lane first substitution of the fast kernel (dtrl_kernel_fast.h: usolve_rows for substeps with constraint rows, the register chain for
substeps without): bit for bit the reference kernel's forward_subst_rows(), on both sides of the cutover and on the many-row substeps of characters
lying on the ground, for the three skeleton instances."""
import numpy as np
import pytest

import test_host_and_emul as T
from conftest import REFDATA, dog_policy

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("arg,skel", [("args/dog_slopes_mixed_args.txt", "dog"), ("args/raptor_narrow_gaps_args.txt", "raptor"),
                                      ("args/goat_cliffs_args.txt", "goat")])
def test_fsub_rows_fast_equals_reference_bitwise(da, om, monkeypatch, arg, skel):
    n, frames = 192, 30
    pol = T.raptor_policy(om) if skel == "raptor" else dog_policy(om)

    def run(kernel):
        if kernel:
            monkeypatch.setenv("DTRL_KERNEL", kernel)
        else:
            monkeypatch.delenv("DTRL_KERNEL", raising=False)
        b = da.BatchScenario(arg, n, data_root=REFDATA, extra_args={"terrain_seed": 77})   # product path: libdtrl.so
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
        return np.concatenate(counts), trace, qf, qdf, b.Torques(), b.EvalStats()

    cf, tf, qf, qdf, (tcf, taf), sf = run(None)
    cr, tr, qr, qdr, (tcr, tar), sr = run("ref")
    for (a, b_) in zip(tf, tr):
        assert all(np.array_equal(x, y) for x, y in zip(a, b_))
    assert np.array_equal(qf, qr) and np.array_equal(qdf, qdr) and np.array_equal(tcf, tcr) and np.array_equal(taf, tar)
    assert sf == sr
    hist = np.bincount(cf, minlength=25)
    # the run covered airborne substeps (R = 0: register chain), the row form's few-row and many-row substeps
    assert hist[0] > 0 and hist[1:7].sum() > 0 and hist[7:13].sum() > 0 and hist[13:].sum() > 0, hist.tolist()
