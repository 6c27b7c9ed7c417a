"""First substitution of the fast kernel with the constraint rows' descriptors loaded in one batch (dtrl_kernel_fast.h FastPath::substep: lane r loads its own
row's kind, links, direction and point once, the loop over the rows broadcasts row r's from lane r instead of reading it through LDS in three to four dependent
trips; the free right-hand side goes into Z[R] behind the loop): bit for bit the reference kernel (DTRL_KERNEL=ref: row_jac() / forward_subst_rows() of
dtrl_kernel.h), after every frame, for the three skeleton instances.

What the run is made to reach, asserted on the REFERENCE kernel's run, so that the conditions do not depend on the code under test (seed, frame count and the
poses below were chosen with the lane-loop CPU build, which goes through the same rollout() in the CPU twin at the end of this file):
  (a) joint-limit rows (kind 0: dx alone at DoF link + 2, the other descriptor fields of the row's lane hold whatever an earlier substep left): kNoRowId among the cached row ids of an env-frame
  (b) link--link rows (link2 >= 0: the second subtree bit, zero at the root translations): cached ids from kFirstPairRowId up. Every sixth env (env % 6 == 4)
      starts in mid-air with one leg folded onto itself (test_link_link_contacts_vs_oracle's pose for the dog and the goat)
  (c) the 24-row cap (every lane index below 24 carries a row, the free right-hand side is row 24): every third env (env % 3 == 0) is turned on its back and dropped, as in test_fsub_rows.py, and
      every sixth (env % 6 == 2) is stood on its nose with the root SINK metres lower, a dozen and more sample points in the ground
  (d) a perturbation active while the env has rows (the free right-hand side carries perturb_gen_force): every fourth env (env % 4 == 1) is pushed for longer than
      the run lasts; an env-frame counts when the env has not been reset since the push (a reset clears the slot) and its last substep had rows
  (e) airborne substeps (R = 0: the register chain, untouched).

Both libraries: the fp32 cases (-physics_precision= f32: libdtrl_f32.so, whose bcast() moves one register where the fp64 one moves a lo/hi pair) run the same rollout
and compare the same fields. Env-frames that reached (a) / (b) / (c) / (e) / (d) in fp32, lane-loop check build | reference kernel on the device:
  dog 2703 / 2408 / 129 / 1348 / 748 | 2711 / 2413 / 132 / 1337 / 754, raptor 2632 / 2678 / 25 / 1379 / 747 | 2659 / 2676 / 25 / 1369 / 740,
  goat 4075 / 2793 / 178 / 649 / 755 | 4076 / 2792 / 177 / 645 / 762."""
import numpy as np
import pytest

import test_host_and_emul as T
from conftest import REFDATA, dog_policy
from precision import assert_library, both_precisions, check_build, extra_for
from product import fast_and_reference

CASES = [("args/dog_slopes_mixed_args.txt", "dog"), ("args/raptor_narrow_gaps_args.txt", "raptor"), ("args/goat_cliffs_args.txt", "goat")]
N_ENVS, FRAMES, TERRAIN_SEED = 192, 30, 77
NO_ROW_ID, FIRST_PAIR_ROW_ID, MAX_ROWS = 0xffff, 512, 24      # dtrl_kernel.h kNoRowId, kFirstPairRowId; dtrl_types.h kMaxRows
FOLD = {"dog": ((14, 2.95), (15, 0.3)), "goat": ((14, 2.95), (15, 0.3)), "raptor": ((12, 2.6), (13, -2.6))}   # (link, hinge angle): a leg folded until two of its boxes overlap
PUSH_FRAME = 3
SINK = 0.25
# the fields of a frame's record, in rollout()'s order: the one tuple of names of the fast-against-reference tests
NAMES = ("cache count", "cache ids", "cache impulses", "contact flags", "pose", "velocity", "control torques", "applied torques", "cycle counters", "reset counters", "eval stats")


def rollout(make, pol, skel, n=N_ENVS, frames=FRAMES):
    """make() -> BatchScenario. Returns the per-frame records and what check_reached() looks at."""
    b = make()
    b.SetPolicy(pol[1], *pol[2:])
    b.RunFrames(2)
    q, qd = b.PoseVel()
    back = np.arange(0, n, 3, dtype=np.int32)
    ql = q[back].copy()
    ql[:, 2] += np.pi
    b.SetPoseVel(ql, np.zeros_like(qd[back]), back)
    fold = np.arange(4, n, 6, dtype=np.int32)
    qf = q[fold].copy()
    qf[:, 1] += 1.0
    for link, ang in FOLD[skel]:
        qf[:, 2 + link] = ang
    b.SetPoseVel(qf, np.zeros_like(qd[fold]), fold)
    sunk = np.arange(2, n, 6, dtype=np.int32)
    qs = q[sunk].copy()
    qs[:, 2] -= np.pi / 2
    qs[:, 1] -= SINK
    b.SetPoseVel(qs, np.zeros_like(qd[sunk]), sunk)
    pushed = np.arange(1, n, 4, dtype=np.int32)
    frames_out = []
    reached = {"limit": 0, "pair": 0, "cap": 0, "airborne": 0, "pushed_with_rows": 0}
    resets_at_push = None
    for f in range(frames):
        if f == PUSH_FRAME:
            b.AddPerturb(5, (60.0, 45.0), 10.0, local_pos=(0.1, -0.05), env_ids=pushed)
            resets_at_push = b.CycleInfo(pushed)[1].copy()
        b.RunFrames(1)
        cnt, rid, lam = b.ContactCache()
        q1, qd1 = b.PoseVel()
        tc, ta = b.Torques()
        nc, nr = b.CycleInfo()[:2]
        st = b.EvalStats()
        frames_out.append((cnt, rid, lam, b.Contacts(), q1, qd1, tc, ta, nc, nr, np.array([st["avg_dist"], st["episodes"], st["cycles"], st["resets"]])))
        live = np.arange(rid.shape[1])[None, :] < cnt[:, None]
        reached["limit"] += int((live & (rid == NO_ROW_ID)).any(axis=1).sum())
        reached["pair"] += int((live & (rid >= FIRST_PAIR_ROW_ID) & (rid != NO_ROW_ID)).any(axis=1).sum())
        reached["cap"] += int((cnt == MAX_ROWS).sum())
        reached["airborne"] += int((cnt == 0).sum())
        if resets_at_push is not None:
            reached["pushed_with_rows"] += int(((nr[pushed] == resets_at_push) & (cnt[pushed] > 0)).sum())
    return frames_out, reached


def check_reached(reached):
    print("env-frames that reached: %s" % reached)
    for what, count in reached.items():
        assert count >= 1, (what, reached)


def policy_of(om, skel):
    return T.raptor_policy(om) if skel == "raptor" else dog_policy(om)


def product(da, arg, n, prec, **extra):
    """make() of the product path: libdtrl.so, libdtrl_f32.so for prec = "f32" (asserted: a case cannot silently run the other library)"""
    def make():
        b = da.BatchScenario(arg, n, data_root=REFDATA, extra_args=extra_for(prec, **extra))
        assert_library(b, prec)
        return b
    return make


@pytest.mark.gpu
@pytest.mark.parametrize("arg,skel,prec", both_precisions(CASES))
def test_fsub_rhs_fast_equals_reference_bitwise(da, om, monkeypatch, arg, skel, prec):
    pol = policy_of(om, skel)
    (_, rf), (_, rr) = fast_and_reference(monkeypatch, lambda: rollout(product(da, arg, N_ENVS, prec, terrain_seed=TERRAIN_SEED), pol, skel), NAMES)
    check_reached(rr)
    assert rf == rr


@pytest.mark.parametrize("arg,skel,prec", both_precisions(CASES))
def test_fsub_rhs_rollout_reaches_every_case_on_the_lane_loop_build(om, arg, skel, prec):
    """The CPU twin: the same rollout through the lane-loop build of dtrl_kernel.h (of either precision) reaches (a) .. (e)."""
    pol = policy_of(om, skel)
    _, reached = rollout(lambda: check_build(prec)(arg, N_ENVS, data_root=REFDATA, extra_args=extra_for(prec, terrain_seed=TERRAIN_SEED)), pol, skel)
    check_reached(reached)
