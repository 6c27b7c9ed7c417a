"""The hand-over kernels of dtrl_backend_hip.hip at the smallest widths that take their second code path, bit for bit against plain references:
dtrl_tuple_order / _pack / _finish above 1024 envs, 2048 pending rows and 1024 carried rows, and with a full ring; dtrl_ext_collect above 1024 envs with a `cap`
that cuts inside one thread's chunk; dtrl_order_by_cost above 1024 envs in one group; dtrl_slot_partials in two passes. The helpers live beside their
small-width siblings (tests/test_boundary.py, test_external_policy.py, test_device_terrain.py); on the lane-loop check build the host defaults stand in for
these kernels, so only the hand-over above 1024 envs has a CPU twin there (the others take minutes on it: their reference logic and floors were proved on it once)."""
import time

import numpy as np
import pytest

import test_boundary as B
import test_device_terrain as D
import test_external_policy as X
import test_policy_slots as P
from product import product_batch

pytestmark = pytest.mark.gpu
hip_batch = product_batch(B, X, P)


@pytest.fixture(autouse=True)
def wall_time(request):
    t0 = time.time()
    yield
    print("%s: %.1f s" % (request.node.name, time.time() - t0))


TO_PTR = dict(to_ptr=lambda t: t.data_ptr(), read=lambda t: t.cpu().numpy())

# 1100 envs: a chunk of two envs per thread of dtrl_tuple_order's scan, threads 550 .. 1023 without an env, no multiple of 64. Drained every 52 frames, three
# times; the check build (17 minutes there): 9530 rows in three drains, the first 2587 and the largest 3619, up to 1060 envs with two or more rows in one
# drain, carries of 1887 after the first drain and 7430 after the third behind the 700-row block (floors: 2048, 256, 1024 -- each exceeded by more than a
# quarter). The rings hold 10240 rows: `c` has 8130 pending before its third drain.
WIDE_DRAIN = dict(n_envs=1100, cap=10240, small=700, frames=156, every=52, ring_cap=10240, min_drain=2048, min_multi_envs=256, min_carry=1024)


@pytest.mark.parametrize("extra_b", [None, {"tuple_ring": "host"}], ids=["device_ring", "host_ring"])
def test_packed_drain_many_rows_long_carry(om, extra_b):
    """Packed drains of more than 2048 pending rows at 1100 envs against the plain drain's rows (stable argsort by env id), and a 700-row block whose carry of
    more than 1024 rows goes through the staging rows and the scan again: the same rows per env in the same order. Also with the rings in page-locked memory."""
    B.run_packed_drain_equals_plain_drain(B.Scenario, om, extra_b=extra_b, **TO_PTR, **WIDE_DRAIN)


def test_packed_drain_of_a_full_ring(om):
    """1100 envs, a ring of 1500 rows left undrained for 46 frames (the check build: 1967 rows in the twin, 467 lost, 1485 from frames that ended before the
    ring was full; the helper's floor is 256 lost), a block of 1200: header [1200, lost, 300], the counters, and the rows held to the properties of run_packed_drain_of_a_full_ring."""
    lost = B.run_packed_drain_of_a_full_ring(B.Scenario, om, frames=46, **TO_PTR)
    assert lost > 0


class TorchArrays:
    """test_external_policy.HostArrays on cuda:0 (torch's stream is drained before a pointer goes to the library, which works on streams of its own)"""
    @staticmethod
    def full(shape, value, dtype):
        import torch
        return torch.full(shape if isinstance(shape, tuple) else (shape,), value, dtype={np.int32: torch.int32, np.float32: torch.float32}[dtype], device="cuda")

    @staticmethod
    def ptr(t):
        import torch
        torch.cuda.synchronize()
        return t.data_ptr()

    @staticmethod
    def read(t):
        return t.cpu().numpy()

    @staticmethod
    def write(t, values):
        import torch
        t[:len(values)] = torch.from_numpy(np.ascontiguousarray(values)).to(t.device)


def test_hand_over_above_1024_envs_with_a_cutting_cap(da, om):
    """2304 dogs (three envs per thread of dtrl_ext_collect): ids and states of every tick against ExtEnvInfo / RecordPoliState, caps of 1, 1000 and
    awaiting - 1 with sentinels behind them, device calls on torch tensors against host calls, equal batches at the end."""
    lo, hi = X.run_hand_over_at_width(da, om, arrays=TorchArrays)
    assert 0 < lo < 1024 < hi


def test_launch_order_of_a_wide_group(om):
    """2304 envs in ONE group (both loops of dtrl_order_by_cost run three times) against three batches of 768 with the same global env ids: 40 frames, 20 of
    them queued, at least 20 resets (the check build: 306)."""
    import deepterrainrl_amd
    D.run_wide_group_equals_its_shards(deepterrainrl_amd.BatchScenario, om)


def test_slot_stats_two_passes(da, om, n=16684, frames=30):
    """dtrl_slot_stats at 16 384 + 300 envs: 64 workgroups of partial rows and a second pass of four whole wavefronts and 44 lanes of a fifth in workgroup 0
    and 1 only; 8 slots, one of them left empty, against the records."""
    p0 = P.policies(om, P.DOG)[0]
    b = P.batch(P.DOG, n, terrain_seed=11, terrain_gen="device")
    b.CreateSlots(8)
    b.SetPolicy(p0[1], *p0[2:]); b.SetExplore(*P.EXPLORE[0])
    for s in range(1, 8):
        b.SlotAlias(s, 0); b.SlotSetExplore(s, 1, 0.1 * s, 0.5, 0.05 * s)
    empty = 5
    rng = np.random.RandomState(3)
    assign = rng.choice([s for s in range(8) if s != empty], size=n, p=[0.3, 0.05, 0.2, 0.1, 0.15, 0.12, 0.08])   # uneven, unordered, slot 5 left out
    b.AssignSlots(None, assign)
    b.RunFrames(frames)
    tot = P.check_slot_stats(b, 8)
    assert tot["cycles"] > n and tot["episodes"] > 0, tot
    assert b.SlotStats(empty) == {"n_envs": 0, "avg_dist": 0.0, "episodes": 0, "cycles": 0, "resets": 0}
    assert set(np.unique(b.GetSlots()[16384:])) >= {0, 2, 4}, "the second pass holds envs of several slots"
