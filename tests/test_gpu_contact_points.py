"""Ground contact sampling of the fast kernel (dtrl_kernel_fast.h eval_points: all of a lane's sample points in one interleaved, branch-free pass, the ground
header loaded once, the point count per lane a compile-time constant of the skeleton) and the batched PD set-up of controller_update(): bit for bit the
reference kernel (DTRL_KERNEL=ref: contact_point_eval() one point at a time), after every frame, for the three skeleton instances.

What the run is made to reach, asserted on the REFERENCE kernel's run (so the conditions do not depend on the code under test; the seeds were chosen
with the lane-loop CPU build, which satisfies them through the same calls -- rollout() takes the scenario class):
  (a) a sixth of the envs (env % 6 == 1) are put with their root ON the seam between the two segments of their ground window (GroundWindow: max_x of the
      first segment), at the height above ground they had: links on either side of the seam, i.e. sample points of ONE env and ONE pass in both segments
      (the per-point segment select against the header that is loaded once). Asserted: at least one env-frame has link centres in both segments.
  (b) every third env (env % 3 == 0) is turned on its back and dropped, as in test_fsub_rows.py: the row-count histogram is non-empty at 0, 1-6, 7-12 and
      13+ (link cap and row cap paths, which consume the sample points).
  (c) by construction: the dog / goat (126 points) and the raptor (114) leave lanes 62 / 50 ... 63 without a second point (they evaluate a clamped index and
      are deselected), and every skeleton has links that do not collide with the ground (col = 0: evaluated like the others, deselected).

Both libraries: the fp32 cases (-physics_precision= f32: libdtrl_f32.so) run the same rollout and compare the same fields. Env-frames with links in both segments and
row counts 0 / 1-6 / 7-12 / 13+ in fp32, lane-loop check build | reference kernel on the device:
  dog 187, 1699 / 3169 / 673 / 219 | 188, 1696 / 3198 / 647 / 219, raptor 490, 1152 / 2383 / 2173 / 52 | 485, 1169 / 2368 / 2170 / 53,
  goat 71, 772 / 2792 / 1586 / 610 | 71, 775 / 2782 / 1599 / 604."""
import numpy as np
import pytest

import test_host_and_emul as T
from conftest import REFDATA, dog_policy
from precision import both_precisions, check_build, extra_for
from product import fast_and_reference
from test_gpu_fsub_rhs import NAMES, product

CASES = [("args/dog_slopes_mixed_args.txt", "dog"), ("args/raptor_narrow_gaps_args.txt", "raptor"), ("args/goat_cliffs_args.txt", "goat")]
N_ENVS, FRAMES, TERRAIN_SEED = 192, 30, 77


def rollout(make, pol, n=N_ENVS, frames=FRAMES):
    """make() -> BatchScenario. Returns the per-frame records, the row counts of all frames and the number of env-frames whose links lie in both ground segments."""
    b = make()
    b.SetPolicy(pol[1], *pol[2:])
    b.RunFrames(2)
    q, qd = b.PoseVel()
    back = np.arange(0, n, 3, dtype=np.int32)
    ql = q[back].copy()
    ql[:, 2] += np.pi
    b.SetPoseVel(ql, np.zeros_like(qd[back]), back)
    seam = np.arange(1, n, 6, dtype=np.int32)
    qs, qds = q[seam].copy(), qd[seam].copy()
    for k, e in enumerate(seam):
        win, _ = b.GroundWindow(int(e))
        sx = win[0][1]                                    # the first segment ends and the second begins here
        h = b.SampleGround(int(e), [qs[k, 0], sx])[0]
        qs[k, 0] = sx
        qs[k, 1] += h[1] - h[0]                           # the same height above the ground
    b.SetPoseVel(qs, qds, seam)
    frames_out, counts, both = [], [], 0
    for _ in range(frames):
        b.RunFrames(1)
        cnt, rid, lam = b.ContactCache()
        q1, qd1 = b.PoseVel()
        tc, ta = b.Torques()
        st = b.EvalStats()
        frames_out.append((cnt, rid, lam, b.Contacts(), q1, qd1, tc, ta, np.array([st["avg_dist"], st["episodes"], st["cycles"], st["resets"]])))
        counts.append(cnt.copy())
        cx = b.LinkStates(seam)[0][:, :, 0]
        for k, e in enumerate(seam):
            seg = b.SampleGround(int(e), cx[k])[1]
            both += int(seg.min() == 0 and seg.max() == 1)
    return frames_out, np.concatenate(counts), both


def check_reached(counts, both):
    hist = np.bincount(counts, minlength=25)
    print("env-frames with links in both ground segments: %d; row-count histogram: %s" % (both, hist.tolist()))
    assert both >= 1, both
    assert hist[0] > 0 and hist[1:7].sum() > 0 and hist[7:13].sum() > 0 and hist[13:].sum() > 0, hist.tolist()


def policy_of(om, skel):
    return T.raptor_policy(om) if skel == "raptor" else dog_policy(om)


@pytest.mark.gpu
@pytest.mark.parametrize("arg,skel,prec", both_precisions(CASES))
def test_contact_points_fast_equals_reference_bitwise(da, om, monkeypatch, arg, skel, prec):
    pol = policy_of(om, skel)
    (_, cf, bf), (_, cr, br) = fast_and_reference(monkeypatch, lambda: rollout(product(da, arg, N_ENVS, prec, terrain_seed=TERRAIN_SEED), pol),
                                                      NAMES[:8] + NAMES[-1:])    # (this rollout's records hold no cycle and reset counters)
    check_reached(cr, br)
    assert bf == br and np.array_equal(cf, cr)


@pytest.mark.parametrize("arg,skel,prec", both_precisions(CASES))
def test_contact_points_rollout_reaches_every_case_on_the_lane_loop_build(om, arg, skel, prec):
    """The CPU twin: the same rollout through the lane-loop build of dtrl_kernel.h (of either precision) reaches (a) and (b)."""
    pol = policy_of(om, skel)
    _, counts, both = rollout(lambda: check_build(prec)(arg, N_ENVS, data_root=REFDATA, extra_args=extra_for(prec, terrain_seed=TERRAIN_SEED)), pol)
    check_reached(counts, both)
