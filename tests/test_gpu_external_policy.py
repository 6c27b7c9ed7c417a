"""External policy mode on the product library (libdtrl.so / libdtrl_f32.so on cuda:0): the twins of tests/test_external_policy.py, the cross-checks between the
external fast kernels, the external reference kernel and the lane-loop build, the device calls, and a full-width torch loop."""
import numpy as np
import pytest

import test_external_policy as T
from conftest import REFDATA, EmulScenario
from precision import assert_library, both_precisions, extra_for
from product import product_batch, set_knobs
# ---- twins: the CPU tests themselves, collected here under the module's gpu mark and fixture ----
from test_external_policy import (test_exp_scenario_tuples_equal, test_first_decision_against_oracle_forward, test_liveness_and_accounting, test_refusals,  # noqa: F401
                                  test_replay_internal_run_bit_for_bit, test_run_external_host_callable, test_snapshots_carry_park_state_and_delivered_actions)

pytestmark = pytest.mark.gpu
hip_batch = product_batch(T)
NOT_TWINNED = {"test_hand_over_at_width": "runs at the same width in tests/test_gpu_handover_width.py, on torch tensors, with the other hand-over kernels' second paths"}


# ---- cross-checks ----
def drive(b, frames, tuples=False, by_env=False):
    """Ticks under the scripted policy (a function of the handed-out state alone; by_env: and of the env's id) until every env has completed `frames` frames; returns
    the end state (with the number of ticks that took) and the drained tuples sorted by env, then order."""
    policy = T.scripted(b, by_env)
    rows_all, flags_all, ids_all = [], [], []
    frames_done = np.zeros(b.num_envs, int); ticks = 0
    while frames_done.min() < frames:
        assert ticks < 4 * frames, ("envs do not get through their frames", frames_done.min())
        b.Update(); ticks += 1
        frames_done += b.ExtEnvInfo()[0] == 0                   # after a tick an env is parked or has completed a frame
        ids, states = b.PendingActions()
        if len(ids):
            b.SupplyActions(ids, *policy(ids, states))
        if tuples:
            r, f, i = b.DrainTuples()
            rows_all.append(r); flags_all.append(f); ids_all.append(i)
    out = T.full_state(b) + (ticks,)
    if tuples:
        r, f, i = np.concatenate(rows_all), np.concatenate(flags_all), np.concatenate(ids_all)
        o = np.lexsort((np.arange(len(i)), i))
        return out, (r[o], f[o], i[o])
    return out, None


@pytest.mark.parametrize("arg,n,tuples,prec", both_precisions([(T.DOG, 256, False), (T.RAPTOR, 192, False), (T.TRAIN, 128, True)]))
def test_external_fast_kernel_equals_external_reference_kernel_bitwise(da, om, monkeypatch, arg, n, tuples, prec, frames=90):
    """The external instantiations of the register-resident kernels and of the LDS-phase reference kernel (DTRL_KERNEL=ref) park, resume and compute alike: as many
    ticks as every env needs for 90 frames (the same number on both), with falls, resets, decisions and tuples -- every EnvState record, policy state, ground window,
    park state and tuple row equal. In libdtrl.so and in libdtrl_f32.so (whose external raptor instance has scratch reloads of its own).

    The fp32 raptor case runs under scripted(by_env=True). The 192 raptors start alike on the level run-up of narrow_gaps, so under the plain scripted policy they
    take the same rows until the ground ahead of them differs: on the device the whole batch walks ONE trajectory (fp64: every env falls at the same two ticks,
    resets = 2 x 192, x = 1.757 in all of them at the end; fp32: the eight rows every env takes -- 3 first, then 0, 5 twice, 6, 7 three times -- hold all of them at x = 0.21 for the 90 frames, 8 cycles each
    and no reset, while the fp32 check build, whose states differ in the last bits and so pick other rows, reaches the gaps: 60 distinct x, 29 resets). `resets > 0` on
    the reference kernel's run is the coverage condition, so the fp32 case's input is widened, not the condition: with the env's id in the label the envs part at
    the first decision. Reached under by_env, lane-loop check build | reference kernel on the device: 101 ticks,
    1629 cycles, 76 resets, 108 distinct x | 101 ticks, 1626 cycles, 91 resets, 102 distinct x."""
    def run(kernel):
        set_knobs(monkeypatch, {"DTRL_KERNEL": kernel} if kernel else {})
        b = T.batch(da, arg, n, **extra_for(prec, policy_mode="external", terrain_seed=77, rand_seed=4))
        assert_library(b, prec)
        out = drive(b, frames, tuples, by_env=(prec == "f32" and arg == T.RAPTOR))
        s = b.ExtStats()
        assert s["env_frames_total"] >= frames * n and out[0][4] > frames     # (decisions cost ticks)
        return out + (b.EvalStats(),)
    sf, tf, ef = run(None)
    sr, tr, er = run("ref")
    print("reference kernel's run: %d ticks, %d cycles, %d resets, %d distinct x" % (sr[4], er["cycles"], er["resets"], len(np.unique(sr[0]["q"][:, 0]))))
    T.assert_same_full(sf, sr)
    assert sf[4] == sr[4], "the same number of ticks"
    assert ef == er and ef["cycles"] > n and ef["resets"] > 0
    if tuples:
        assert all(np.array_equal(a, b) for a, b in zip(tf, tr)) and len(tf[0]) > n // 2


@pytest.mark.parametrize("arg", [T.DOG, T.RAPTOR])
def test_external_kernels_against_lane_loop_build(da, om, monkeypatch, arg, n=32):
    """Against the same source run by the host compiler (tests/emul). hipcc and g++ agree on the integer side -- which envs park and when -- and differ in the last
    bits of the floating-point side (hardware reciprocals on the device), so the comparison is the one smoke() and the GPU twins of the oracle tests hold the
    product to: poses within 1e-6 after two frames from a common start. Both kernels; both sides get the rows computed from the check build's states."""
    def make(cls, **kw):
        return cls(arg, n, data_root=REFDATA, extra_args=dict(policy_mode="external", terrain_seed=77, rand_seed=4, **kw))
    for kernel in (None, "ref"):
        set_knobs(monkeypatch, {"DTRL_KERNEL": kernel} if kernel else {})
        g = make(da.BatchScenario); c = make(EmulScenario)
        policy = T.scripted(c)
        for _ in range(3):                                     # first env-step (every env parks), then two whole frames
            g.Update(); c.Update()
            pg, lg = g.ExtEnvInfo(); pc, lc = c.ExtEnvInfo()
            assert np.array_equal(pg, pc) and np.array_equal(lg, lc)
            ig, sg = g.PendingActions(); ic, sc = c.PendingActions()
            assert np.array_equal(ig, ic)
            if len(ic):
                assert np.abs(sg - sc).max() < 1e-6
                rows = policy(ic, sc)
                g.SupplyActions(ig, *rows); c.SupplyActions(ic, *rows)
        (qg, qdg), (qc, qdc) = g.PoseVel(), c.PoseVel()
        err = max(np.abs(qg - qc).max(), np.abs(qdg - qdc).max())
        print("external %s kernel vs lane-loop build after 2 frames: max |dq|, |dqd| = %.3e" % (kernel or "fast", err))
        assert err < 1e-6, (kernel, err)
        assert g.ExtStats() == c.ExtStats()


# ---- device calls ----
def test_device_calls(da, om, n=256):
    """dtrl_pending_actions_device hands out the host call's ids and float32(its states); a run driven through dtrl_supply_actions_device equals a run driven through
    dtrl_supply_actions with the same float-rounded rows, bit for bit; a row for an env that is not awaiting is counted in `rejected` and changes nothing."""
    import torch
    dev = torch.device("cuda", 0)
    mk = lambda: T.batch(da, T.DOG, n, policy_mode="external", terrain_seed=9, rand_seed=1)
    bd, bh = mk(), mk()
    table = torch.tensor(bd.ActionTable(), dtype=torch.float32, device=dev)
    ids_t = torch.zeros(n, dtype=torch.int32, device=dev); st_t = torch.zeros((n, bd.S), dtype=torch.float32, device=dev)
    lab_t = torch.zeros(n, dtype=torch.int32, device=dev); prm_t = torch.zeros((n, bd.n_opt), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    decisions = 0
    for t in range(60):
        bd.Update(); bh.Update()
        ih, sh = bh.PendingActions()
        m = bd.PendingActionsDevice(ids_t.data_ptr(), st_t.data_ptr(), n)
        assert m == len(ih)
        if m == 0:
            continue
        assert np.array_equal(ids_t[:m].cpu().numpy(), ih)
        assert np.array_equal(st_t[:m].cpu().numpy(), sh.astype(np.float32))
        lab = (st_t[:m, 200:].abs().sum(dim=1) * 1000).to(torch.int64) % table.shape[0]
        lab_t[:m] = lab.to(torch.int32)
        prm_t[:m] = table[lab] * (1.0 + 0.01 * torch.sin(st_t[:m, 200:201]))          # not a table row: exercises the float -> real conversion
        torch.cuda.synchronize()
        if t == 20:
            # rows for envs that are not awaiting (and one id out of range): counted, nothing changes
            before = T.full_state(bd)
            others = np.setdiff1d(np.arange(n), ih)[:5].astype(np.int32)
            bad = torch.tensor(np.concatenate([others, [n + 3]]).astype(np.int32), device=dev)
            torch.cuda.synchronize()
            rej = bd.SupplyActionsDevice(bad.data_ptr(), len(bad), lab_t.data_ptr(), prm_t.data_ptr(), 0)
            assert rej == len(bad)
            T.assert_same_full(before, T.full_state(bd))
        rej = bd.SupplyActionsDevice(ids_t.data_ptr(), m, lab_t.data_ptr(), prm_t.data_ptr(), 0)
        assert rej == 0
        bh.SupplyActions(ih, lab_t[:m].cpu().numpy(), prm_t[:m].cpu().numpy().astype(np.float64))
        decisions += m
        if t == 30:
            rej = bd.SupplyActionsDevice(ids_t.data_ptr(), m, lab_t.data_ptr(), prm_t.data_ptr(), 0)   # the same rows again: every env already has its action
            assert rej == m
    assert decisions > 2 * n
    T.assert_same_full(T.full_state(bd), T.full_state(bh))
    assert bd.ExtLaunchMs(0) > 0 and bd.ExtLaunchMs(1) > 0


def test_full_width_torch_loop(da, om, n=4096, ticks=120):
    """run_external with a torch MLP (283-256-256-n_opt) on 4096 dogs: 120 ticks through the device calls; finite outputs, every env took an external decision,
    and the accounting of test_liveness_and_accounting holds at the end."""
    import torch
    from deepterrainrl_amd.external import run_external
    dev = torch.device("cuda", 0)
    b = T.batch(da, T.DOG, n, policy_mode="external", terrain_seed=11, rand_seed=0)
    base = torch.tensor(b.ActionTable()[0], dtype=torch.float32, device=dev)

    class Mlp(torch.nn.Module):
        def __init__(self):
            super().__init__()
            torch.manual_seed(0)
            self.net = torch.nn.Sequential(torch.nn.Linear(b.S, 256), torch.nn.ReLU(), torch.nn.Linear(256, 256), torch.nn.ReLU(), torch.nn.Linear(256, b.n_opt))

        def forward(self, s):
            return base + 0.05 * torch.tanh(self.net(s))       # a perturbation of the first base action

    r = run_external(b, Mlp().to(dev), ticks)
    q, qd = b.PoseVel()
    assert np.isfinite(q).all() and np.isfinite(qd).all()
    assert r["rejected"] == 0 and r["decisions"] >= n
    nc, nr, _, _, _ = b.CycleInfo()
    assert (nc >= 1).all(), "every env took at least one external decision"
    steps = b.num_update_steps

    def accounted(s):
        # every env has completed env_frames whole frames plus the finished part of the frame it is parked in (awaiting, or holding a delivered action)
        park, left = b.ExtEnvInfo()
        assert s["awaiting"] == int((park == 1).sum()) and s["ready"] == int((park == 2).sum()) and s["awaiting"] + s["ready"] <= n
        print("ticks %d: awaiting %d, ready %d, env_steps %d, env_frames %d" % (ticks, s["awaiting"], s["ready"], s["env_steps_total"], s["env_frames_total"]))
        assert s["env_steps_total"] == s["env_frames_total"] * steps + int(np.where(park != 0, steps - left, 0).sum())

    # the loop ends behind its last supply: the envs answered in the last tick hold their rows, nobody else is waiting
    assert r["awaiting"] == 0
    accounted(r)
    b.Update()
    s = b.ExtStats()
    assert s["ready"] == 0, "%d delivered actions were not consumed by the next tick" % s["ready"]
    accounted(s)
    assert s["env_frames_total"] > 0.8 * n * ticks
