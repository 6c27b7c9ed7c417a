"""Kinematics of the fast kernel per skeleton (dtrl_kernel_fast.h kin_dyn_terms_fast<Topo>: substeps 2 to 5 and the post-step evaluation of every env-step; operands
in batches, the lane's own values in registers, path loops of the skeleton's depth): bit for bit the reference kernel (DTRL_KERNEL=ref: kin_dyn_terms() of
dtrl_kernel.h), after every frame, for the three skeleton instances.

What is compared: the link states (COM, velocity, angle -- the C API rebuilds them from the pose on the host, so they follow the pose), pose and velocity, control and
applied torques, contact flags, the contact cache, cycle and reset counters. Everything the kinematics writes is read by the contact pass, the mass rows, the bias and the
controller within the same env-step, so a wrong bit in any of its arrays is in the pose one substep later.

What the run is made to reach, asserted on the REFERENCE kernel's run, so that the conditions do not depend on the code under test (seed, frame count and the poses
below were chosen with the lane-loop CPU build, which goes through the same rollout() in the CPU twin at the end of this file):
  (a) envs without rows (airborne) and envs with rows at the end of a frame
  (b) envs turned by pi and dropped (env % 3 == 0, as in test_gpu_fsub_rhs.py): one of them lies on rows before it is reset
  (c) a root angle several turns out (env % 6 == 2: + TURNS x 2 pi -- the argument reduction of sincos): |q[2]| > 4 pi in a compared frame, the env not reset since
  (d) an env spinning at >= 20 rad/s at the end of a compared frame (env % 6 == 4: lifted by a metre, the whole body turning at SPIN rad/s: the centripetal terms)
  (e) the hinge velocity of every link at the end of a longest path (the last iteration of the path loops) non-zero in a compared frame
  (f) a reset in a frame that is not the last one (the cold generic evaluation of the reset, then fast ones on top of it).

Both libraries: the fp32 cases (-physics_precision= f32: libdtrl_f32.so; the raptor instance at three waves per SIMD with scratch reloads in its substep loop) run the
same rollout and compare the same fields. Env-frames that reached airborne / rows / turned_on_rows / turns_out / spinning / reset_before_last in fp32 (deepest_moving
holds in all), lane-loop check build | reference kernel on the device:
  dog 1694 / 4066 / 175 / 958 / 170 / 98 | 1701 / 4059 / 175 / 960 / 176 / 96, raptor 1312 / 4448 / 128 / 789 / 33 / 207 | 1317 / 4443 / 128 / 754 / 33 / 212,
  goat 768 / 4992 / 255 / 903 / 3 / 142 | 791 / 4969 / 255 / 893 / 4 / 146 (the thinnest bin: the goat's spinning env-frames, 3 | 4; fp64: 3 | 3)."""
import numpy as np
import pytest

from conftest import REFDATA
from precision import both_precisions, check_build, extra_for
from product import fast_and_reference
from test_gpu_fsub_rhs import CASES, policy_of, product

N_ENVS, FRAMES, TERRAIN_SEED = 192, 30, 77
# this rollout's records: the link states in front, no eval stats (not test_gpu_fsub_rhs.NAMES)
NAMES = ("link COM", "link velocity", "link angle", "pose", "velocity", "control torques", "applied torques", "contact flags", "cache count", "cache ids", "cache impulses",
         "cycle counters", "reset counters")
TURNS, SPIN, LIFT = 7, 25.0, 1.0
PARENT = {   # dtrl_topo.h
    "dog": (-1, 0, 1, 2, 3, 4, 5, 6, 7, 0, 9, 10, 11, 5, 13, 14, 15, 0, 17, 18, 19),
    "raptor": (-1, 0, 1, 2, 3, 4, 0, 6, 7, 8, 9, 0, 11, 12, 13, 0, 15, 16, 17),
}
PARENT["goat"] = PARENT["dog"]


def deepest_links(skel):
    par = PARENT[skel]
    n = []
    for l in range(len(par)):
        k, a = 0, l
        while a >= 0:
            k, a = k + 1, par[a]
        n.append(k)
    return [l for l in range(len(par)) if n[l] == max(n)]


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
    far = np.arange(2, n, 6, dtype=np.int32)
    qt = q[far].copy()
    qt[:, 2] += TURNS * 2 * np.pi
    b.SetPoseVel(qt, qd[far], far)
    spun = np.arange(4, n, 6, dtype=np.int32)
    qs = q[spun].copy()
    qs[:, 1] += LIFT
    qds = np.zeros_like(qd[spun])
    qds[:, 2] = SPIN
    b.SetPoseVel(qs, qds, spun)
    resets0 = b.CycleInfo()[1].copy()
    deep = deepest_links(skel)
    moved = np.zeros(len(deep), bool)
    frames_out = []
    reached = {"airborne": 0, "rows": 0, "turned_on_rows": 0, "turns_out": 0, "spinning": 0, "deepest_moving": 0, "reset_before_last": 0}
    for f in range(frames):
        b.RunFrames(1)
        cnt, rid, lam = b.ContactCache()
        q1, qd1 = b.PoseVel()
        tc, ta = b.Torques()
        nc, nr = b.CycleInfo()[:2]
        com, vel, ang = b.LinkStates()
        frames_out.append((com, vel, ang, q1, qd1, tc, ta, b.Contacts(), cnt, rid, lam, nc, nr))
        fresh = nr == resets0
        reached["airborne"] += int((cnt == 0).sum())
        reached["rows"] += int((cnt > 0).sum())
        reached["turned_on_rows"] += int((fresh[back] & (cnt[back] > 0)).sum())
        reached["turns_out"] += int((fresh[far] & (np.abs(q1[far, 2]) > 4 * np.pi)).sum())
        reached["spinning"] += int((np.abs(qd1[:, 2]) >= 20.0).sum())
        moved |= (qd1[:, [2 + l for l in deep]] != 0.0).any(axis=0)
        if f < frames - 1:
            reached["reset_before_last"] += int((nr != (frames_out[-2][12] if f else resets0)).sum())
    reached["deepest_moving"] = int(moved.all())
    return frames_out, reached


def check_reached(reached):
    print("env-frames that reached: %s" % reached)
    for what, count in reached.items():
        assert count >= 1, (what, reached)


@pytest.mark.gpu
@pytest.mark.parametrize("arg,skel,prec", both_precisions(CASES))
def test_fast_kinematics_equals_reference_bitwise(da, om, monkeypatch, arg, skel, prec):
    pol = policy_of(om, skel)
    (_, rf), (_, rr) = fast_and_reference(monkeypatch, lambda: rollout(product(da, arg, N_ENVS, prec, terrain_seed=TERRAIN_SEED), pol, skel), NAMES)
    check_reached(rr)
    assert rf == rr


@pytest.mark.parametrize("arg,skel,prec", both_precisions(CASES))
def test_fast_kinematics_rollout_reaches_every_case_on_the_lane_loop_build(om, arg, skel, prec):
    """The CPU twin: the same rollout through the lane-loop build of dtrl_kernel.h (of either precision) reaches (a) .. (f)."""
    pol = policy_of(om, skel)
    _, reached = rollout(lambda: check_build(prec)(arg, N_ENVS, data_root=REFDATA, extra_args=extra_for(prec, terrain_seed=TERRAIN_SEED)), pol, skel)
    check_reached(reached)
