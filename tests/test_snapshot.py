"""Full env snapshots (include/dtrl.h: dtrl_snapshot_save / _restore / _export / _import, dtrl_clone_envs): an env put back from a snapshot must repeat its
own future BIT FOR BIT -- pose, FSM, timers, soft-fall filter, exploration draws, pending resets, terrain windows including the segments built after the restore,
the tuple in progress and the tuples that complete later. Every comparison is np.array_equal on what the ordinary getters return; nothing here is a tolerance,
except the one HIP-vs-check-build frame of the cross-build test, which takes the bound test_gpu_parity.test_device_terrain_equals_the_lane_loop_build uses (1e-6).

CPU half: the lane-loop build (conftest.EmulScenario), whose backend has no snapshot code of its own and so runs the Backend defaults built from D2D / D2H / H2D.
GPU half (marked gpu): libdtrl.so, where the HIP backend moves all records of all listed envs in one kernel launch.

The replay windows must be EVENTFUL (a fall or reset, a terrain segment rebuild and a completed tuple inside the compared frames); each test asserts that, so
that a change of seeds or of the engine cannot quietly turn it into a comparison of characters standing still."""
import numpy as np
import pytest

from conftest import REFDATA, EmulScenario, dog_policy, emul_f32_scenario

DOG = ("args/opt_args_train_mace.txt", "data/terrain/slopes_mixed.txt")          # dog + slopes_mixed, exploration scenario (tuples)
RAPTOR = ("args/opt_args_train_raptor_mace.txt", "data/terrain/narrow_gaps.txt")  # raptor + narrow_gaps
EXPLORE = (True, 0.2, 0.025, 0.002)


def raptor_policy(om):
    import os
    desc = om.parse_deploy_prototxt(os.path.join(REFDATA, "data/policies/raptor/nets/raptor_mace3_deploy.prototxt"))
    w = om.xavier_weights(desc, 4321)
    io, isc, oo, osc = om.load_scale_file(os.path.join(REFDATA, "data/policies/raptor/models/raptor_mace3_narrow_gaps_model_scale.txt"))
    return desc, w, io, isc, oo, osc


def make(scn, om, n, which=DOG, device_terrain=False, explore=True, terrain_seed=77, rand_seed=3, **extra):
    args = {"terrain_file": which[1], "terrain_seed": terrain_seed, "rand_seed": rand_seed}
    if device_terrain:
        args["terrain_gen"] = "device"
    args.update(extra)
    b = scn(which[0], n, data_root=REFDATA, extra_args=args)
    pol = dog_policy(om) if which is DOG else raptor_policy(om)
    b.SetPolicy(pol[1], *pol[2:])
    if explore:
        b.SetExplore(*EXPLORE)
    else:
        b.SetExplore(False, 0.0, 0.025, 0.0)
    return b


def window_key(b, e):
    win, nb = b.GroundWindow(e)
    return (win[0][0], win[0][1], win[1][0], win[1][1], nb), np.concatenate([win[0][2], win[1][2]])


def observe(b, win_envs, envs=None):
    """Everything the ordinary getters show of the batch (or of `envs`) at a frame boundary, as a flat list of arrays."""
    q, qd = b.PoseVel(envs)
    out = [q, qd, b.Flags(envs)]
    out += list(b.Ctrl(envs))
    out += list(b.CycleInfo(envs))
    out += list(b.ContactCache(envs))
    out += [b.RecordPoliState(envs), b.PolicyOutput(envs)]
    for e in win_envs:
        key, h = window_key(b, e)
        out += [np.array(key, np.float64), h]
    return out


def run_record(b, frames, win_envs, envs=None, drain=True):
    """`frames` outer frames; per frame the observation and the drained tuples. Also what happened in the window (events)."""
    rec = []
    ev = {"resets": 0, "rebuilds": 0, "tuples": 0}
    resets0 = b.CycleInfo()[1].copy()
    wins0 = [window_key(b, e)[0] for e in win_envs]
    for _ in range(frames):
        b.Update()
        obs = observe(b, win_envs, envs)
        if drain:
            rows, fl, ids = b.DrainTuples()
            order = np.lexsort((np.arange(len(ids)), ids))     # (ring order between envs is scheduling; per env it is time order)
            obs += [rows[order], fl[order], ids[order]]
            ev["tuples"] += len(ids)
        rec.append(obs)
        wins = [window_key(b, e)[0] for e in win_envs]
        ev["rebuilds"] += sum(1 for a, c in zip(wins0, wins) if a != c)
        wins0 = wins
    ev["resets"] = int((b.CycleInfo()[1] - resets0).sum())
    return rec, ev


def assert_same(rec_a, rec_b, what=""):
    assert len(rec_a) == len(rec_b)
    for f, (oa, ob) in enumerate(zip(rec_a, rec_b)):
        assert len(oa) == len(ob)
        for k, (x, y) in enumerate(zip(oa, ob)):
            assert x.shape == y.shape and np.array_equal(x, y), (what, "frame", f, "item", k)


def assert_eventful(ev, what=""):
    print("events in the compared window %s: %s" % (what, ev))
    assert ev["resets"] >= 1 and ev["rebuilds"] >= 1 and ev["tuples"] >= 1, (what, ev)


# ---- test 1 / 2: replay ----
def run_replay(scn, om, n, which=DOG, device_terrain=False, lead_in=50, frames=60, n_win=None):
    b = make(scn, om, n, which, device_terrain)
    win_envs = list(range(n if n_win is None else n_win))
    for _ in range(lead_in):
        b.Update()
    b.DrainTuples()
    snap = b.SaveState()
    assert snap.num_envs == n and snap.bytes_per_env > 8000
    first, ev = run_record(b, frames, win_envs)
    assert_eventful(ev, "(replay, %s, %s terrain)" % (which[0], "device" if device_terrain else "host"))
    b.RestoreState(snap)
    second, ev2 = run_record(b, frames, win_envs)
    assert ev2 == ev
    assert_same(first, second, "replay")
    snap.free()
    b.close()


def test_replay_host_terrain(om):
    run_replay(EmulScenario, om, 16)


def test_replay_device_terrain(om):
    run_replay(EmulScenario, om, 12, device_terrain=True)


# ---- test 3: subset restore ----
def run_subset_restore(scn, om, n, subset, t_save=50, t_restore=70, frames_after=45):
    """Two identical batches; in `b` the subset is saved at frame t_save and restored at frame t_restore. From then on b's subset must repeat what the control's
    subset did from frame t_save on (the control keeps running, so its frames t_save .. are on record), and every other env of b must stay on the control."""
    a = make(scn, om, n)       # control, never touched
    b = make(scn, om, n)
    subset = list(subset)
    others = [e for e in range(n) if e not in subset]
    win_sub = subset[:8]; win_oth = others[:8]
    for _ in range(t_save):
        a.Update(); b.Update()
    snap = b.SaveState(subset)
    assert snap.num_envs == len(subset) and list(snap.env_ids()) == subset
    ctl_sub = []               # the control's subset, frame t_save + k
    resets_sub0 = a.CycleInfo(subset)[1].copy(); wins_sub0 = [window_key(a, e)[0] for e in win_sub]
    for _ in range(t_restore - t_save):
        a.Update(); b.Update()
        ctl_sub.append(observe(a, win_sub, subset))
        for k, (x, y) in enumerate(zip(ctl_sub[-1], observe(b, win_sub, subset))):
            assert np.array_equal(x, y), ("the batches differ before the restore", k)
    b.RestoreState(snap)
    r0 = a.CycleInfo(others)[1].copy(); w0 = [window_key(a, e)[0] for e in win_oth]
    for f in range(frames_after):
        a.Update(); b.Update()
        ctl_sub.append(observe(a, win_sub, subset))
        for k, (x, y) in enumerate(zip(observe(a, win_oth, others), observe(b, win_oth, others))):
            assert np.array_equal(x, y), ("an untouched env left the control's trajectory", f, k)
        for k, (x, y) in enumerate(zip(ctl_sub[f], observe(b, win_sub, subset))):
            assert np.array_equal(x, y), ("a restored env does not repeat its saved continuation", f, k)
    # what the restored envs went through in the frames they repeated (control frames t_save .. t_save + frames_after), and the others meanwhile
    wins_rep = [np.array(o[-2 * len(win_sub)::2]) for o in ctl_sub[:frames_after]]
    ev = {"subset_resets": int((ctl_sub[frames_after - 1][9] - resets_sub0).sum()),
          "subset_rebuilds": sum(int((x != y).any(1).sum()) for x, y in zip([np.array(wins_sub0)] + wins_rep[:-1], wins_rep)),
          "others_resets": int((a.CycleInfo(others)[1] - r0).sum()), "others_rebuilds": sum(1 for x, e in zip(w0, win_oth) if x != window_key(a, e)[0])}
    print("subset restore:", ev)
    assert min(ev.values()) >= 1, ev
    snap.free()
    a.close(); b.close()


def test_subset_restore(om):
    run_subset_restore(EmulScenario, om, 16, [1, 7, 8])


# ---- test 4: clone and transplant ----
def run_clone(scn, om, n, a_env, b_env, lead_in=20, frames=80):
    def start():
        b = make(scn, om, n, explore=False)
        for _ in range(lead_in):
            b.Update()
        return b
    # clone
    b = start()
    b.CloneEnvs([a_env], [b_env])
    same = 0
    r0 = b.CycleInfo([a_env, b_env])[1].copy()
    for f in range(frames):
        b.Update()
        if (b.CycleInfo([a_env, b_env])[1] != r0).any():
            break
        oa = observe(b, [], [a_env]); ob = observe(b, [], [b_env])
        for k, (x, y) in enumerate(zip(oa, ob)):
            assert np.array_equal(x, y), ("clone left its source", f, k)
        # the clone's window is the source's window
        assert window_key(b, a_env)[0][:4] == window_key(b, b_env)[0][:4] and np.array_equal(window_key(b, a_env)[1], window_key(b, b_env)[1])
        same += 1
    print("clone: %d identical frames before the first reset of either env" % same)
    assert same >= 20, same
    clone_final = observe(b, [b_env], [b_env])
    n_clone = same
    b.close()
    # transplant through a snapshot: the same outcome as the clone
    t = start()
    snap = t.SaveState([a_env])
    t.RestoreState(snap, env_ids=[b_env])
    for f in range(n_clone + (1 if n_clone < frames else 0)):
        t.Update()
    tr_final = observe(t, [b_env], [b_env])
    for k, (x, y) in enumerate(zip(clone_final, tr_final)):
        assert np.array_equal(x, y), ("transplant differs from clone", k)
    t.close()


def run_clone_overlap(scn, om, n=4):
    b = make(scn, om, n, explore=False)
    for _ in range(12):
        b.Update()
    before = [observe(b, [e], [e]) for e in range(3)]
    b.CloneEnvs([0, 1], [1, 2])
    after = [observe(b, [e], [e]) for e in range(3)]
    for e_new, e_old in ((0, 0), (1, 0), (2, 1)):      # read all, then write all: env 2 gets the OLD env 1
        for k, (x, y) in enumerate(zip(after[e_new], before[e_old])):
            assert np.array_equal(x, y), (e_new, e_old, k)
    assert not np.array_equal(before[1][0], before[0][0])
    b.Update()                                          # and the batch steps on
    q, _ = b.PoseVel([0, 1])
    assert np.array_equal(q[0], q[1]) and np.isfinite(q).all()
    b.close()


def test_clone_and_transplant(om):
    run_clone(EmulScenario, om, 8, 1, 6)


def test_clone_overlapping_lists(om):
    run_clone_overlap(EmulScenario, om)


# ---- test 5: export / import ----
def run_export_import(scn, om, n, lead_in=50, frames=60, n_win=None, which=DOG, scn_fresh=None):
    a = make(scn, om, n, which)
    win_envs = list(range(n if n_win is None else n_win))
    for _ in range(lead_in):
        a.Update()
    a.DrainTuples()
    snap = a.SaveState()
    blob = snap.export()
    # fields read through env_state() are what the getters report
    st = snap.env_state()
    assert st.dtype.itemsize == snap.sizeof_env_state
    state, phase, aid, _, _ = a.Ctrl()
    assert np.array_equal(st["state"], state) and np.array_equal(st["phase"], phase) and np.array_equal(st["action_id"], aid)
    assert np.array_equal(st["num_cycles"], a.CycleInfo()[0])
    fresh = make(scn_fresh or scn, om, n, which)
    imp = fresh.ImportState(blob)
    assert imp.export() == blob                        # exporting the imported snapshot gives back the same bytes
    fresh.RestoreState(imp)
    ra, ev = run_record(a, frames, win_envs)
    rf, _ = run_record(fresh, frames, win_envs)
    assert_eventful(ev, "(export / import)")
    assert_same(ra, rf, "fresh batch after import")
    # edit one field, import, restore: it shows up in dtrl_get_ctrl
    edit = bytearray(blob)
    ste = snap.env_state(edit)
    ste["phase"][:] = 0.4375
    ste["state"][0] = (int(ste["state"][0]) + 1) % 4
    want_state = ste["state"].copy()
    imp2 = fresh.ImportState(edit)
    fresh.RestoreState(imp2)
    state2, phase2, _, _, _ = fresh.Ctrl()
    assert np.array_equal(phase2, np.full(n, 0.4375)) and np.array_equal(state2, want_state)
    for s in (snap, imp, imp2):
        s.free()
    a.close(); fresh.close()


def test_export_import_fresh_batch(om):
    run_export_import(EmulScenario, om, 16)


def test_env_state_dtype_matches_both_precisions(om, da):
    for scn, real in ((EmulScenario, np.float64), (emul_f32_scenario, np.float32)):
        extra = {"physics_precision": "f32"} if real is np.float32 else {}
        b = make(scn, om, 3, **extra)
        for _ in range(5):
            b.Update()
        snap = b.SaveState()
        assert da.env_state_dtype(real).itemsize == snap.sizeof_env_state
        st = snap.env_state()
        state, phase, aid, _, _ = b.Ctrl()
        assert st.dtype["phase"] == np.dtype(real)
        assert np.array_equal(st["state"], state) and np.array_equal(st["phase"].astype(np.float64), phase) and np.array_equal(st["action_id"], aid)
        assert np.array_equal(st["num_cycles"], b.CycleInfo()[0])
        snap.free(); b.close()


# ---- test 6: refusals ----
def expect_refusal(da, fn, *words):
    with pytest.raises(da.DtrlError) as ei:
        fn()
    msg = str(ei.value)
    assert "(1)" in msg, msg                       # DTRL_ERR_ARG
    for w in words:
        assert w in msg, (w, msg)


def run_refusals(scn, scn_f32, om, da, n=4):
    ctl = make(scn, om, n); b = make(scn, om, n)
    for _ in range(6):
        ctl.Update(); b.Update()
    snap = b.SaveState()
    blob = snap.export()

    def still_good():
        ctl.Update(); b.Update()
        for k, (x, y) in enumerate(zip(observe(ctl, range(n)), observe(b, range(n)))):
            assert np.array_equal(x, y), k

    # a dog blob into a raptor batch
    r = make(scn, om, n, RAPTOR)
    expect_refusal(da, lambda: r.ImportState(blob), "character type")
    r.Update(); assert np.isfinite(r.PoseVel()[0]).all(); r.close()
    # an fp64 blob into the fp32 check build
    if scn_f32 is not None:
        f = make(scn_f32, om, n, physics_precision="f32")
        expect_refusal(da, lambda: f.ImportState(blob), "sizeof(real)")
        f.Update(); assert np.isfinite(f.PoseVel()[0]).all(); f.close()
    # a host-terrain blob into a device-terrain batch
    d = make(scn, om, n, device_terrain=True)
    expect_refusal(da, lambda: d.ImportState(blob), "terrain mode")
    d.Update(); assert np.isfinite(d.PoseVel()[0]).all(); d.close()
    # truncated, wrong magic
    expect_refusal(da, lambda: b.ImportState(blob[:-16]), "truncated"); still_good()
    expect_refusal(da, lambda: b.ImportState(blob[:40]), "truncated"); still_good()
    expect_refusal(da, lambda: b.ImportState(b"\x01" + blob[1:]), "magic"); still_good()
    # an edited blob whose indices would address out of bounds
    bad = bytearray(blob); snap.env_state(bad)["ws_R"][1] = 1000
    expect_refusal(da, lambda: b.ImportState(bad), "ws_R"); still_good()
    # env ids out of range, duplicate destinations
    expect_refusal(da, lambda: b.SaveState([0, n]), "out of range"); still_good()
    expect_refusal(da, lambda: b.RestoreState(snap, env_ids=[-1]), "out of range"); still_good()
    expect_refusal(da, lambda: b.RestoreState(snap, env_ids=[1, 1]), "twice"); still_good()
    expect_refusal(da, lambda: b.CloneEnvs([0, 1], [2, 2]), "twice"); still_good()
    expect_refusal(da, lambda: b.CloneEnvs([0, n], [1, 2]), "out of range"); still_good()
    # a snapshot held by another batch
    expect_refusal(da, lambda: ctl.RestoreState(snap), "another batch"); still_good()
    # every snapshot call between dtrl_step_begin and dtrl_step_end
    b.UpdateBegin()
    for fn in (lambda: b.SaveState(), lambda: b.RestoreState(snap), lambda: b.CloneEnvs([0], [1]), lambda: snap.export(), lambda: b.ImportState(blob)):
        expect_refusal(da, fn, "frame is in flight")
    b.UpdateEnd(); ctl.Update()
    still_good()
    snap.free()
    ctl.close(); b.close()


def test_refusals(om, da):
    run_refusals(EmulScenario, emul_f32_scenario, om, da)


def test_snapshot_outlives_its_batch(om, da):
    b = make(EmulScenario, om, 2)
    snap = b.SaveState()
    b.close()
    assert snap.num_envs == 2
    with pytest.raises(da.DtrlError):
        snap.export()
    snap.free()


# ---- GPU half ----
@pytest.mark.gpu
def test_gpu_native_snapshot_path_is_loaded(da, om):
    b = make(da.BatchScenario, om, 8)
    assert "libdtrl.so" in open("/proc/self/maps").read()
    s = b.SaveState(); assert s.bytes_per_env > 8000; s.free(); b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("which,n", [(DOG, 4096), (RAPTOR, 8192)], ids=["dog_4096", "raptor_8192"])
def test_gpu_replay_host_terrain_full_width(da, om, which, n):
    run_replay(da.BatchScenario, om, n, which, lead_in=50, frames=40, n_win=24)


@pytest.mark.gpu
def test_gpu_replay_device_terrain_full_width(da, om):
    run_replay(da.BatchScenario, om, 4096, DOG, device_terrain=True, lead_in=50, frames=40, n_win=24)


@pytest.mark.gpu
def test_gpu_subset_restore(da, om):
    run_subset_restore(da.BatchScenario, om, 256, range(100, 132))


@pytest.mark.gpu
def test_gpu_clone_and_transplant(da, om):
    run_clone(da.BatchScenario, om, 8, 1, 6)
    run_clone_overlap(da.BatchScenario, om)


@pytest.mark.gpu
def test_gpu_export_import_fresh_batch(da, om):
    run_export_import(da.BatchScenario, om, 256, lead_in=50, frames=40, n_win=16)


@pytest.mark.gpu
def test_gpu_refusals(da, om):
    run_refusals(da.BatchScenario, None, om, da)


@pytest.mark.gpu
def test_gpu_cross_build_blob(da, om):
    """A blob exported by the lane-loop build imports into the HIP batch: pose, velocity, ctrl and ground windows equal bitwise (transport only); one further
    frame stays within 1e-6 of the check build, the bound test_gpu_parity.test_device_terrain_equals_the_lane_loop_build uses for HIP against the lane-loop build."""
    n = 16
    c = make(EmulScenario, om, n)
    for _ in range(25):
        c.Update()
    blob = c.SaveState().export()
    g = make(da.BatchScenario, om, n)
    g.RestoreState(g.ImportState(blob))
    oc = observe(c, range(n)); og = observe(g, range(n))
    for k, (x, y) in enumerate(zip(oc, og)):
        assert np.array_equal(x, y), k
    c.Update(); g.Update()
    qc, _ = c.PoseVel(); qg, _ = g.PoseVel()
    print("one frame after the cross-build import: max |dq| = %.3e" % np.abs(qc - qg).max())
    assert np.abs(qc - qg).max() < 1e-6
    c.close(); g.close()
