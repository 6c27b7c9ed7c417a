"""Caffe's six solver types and learning-rate policies in the native trainer (include/dtrl_trainer.h: dtrl_solver_desc; cNNSolver::BuildSolver,
learning/NNSolver.cpp:9-35). CPU tests run the plain-loop check build (tests/emul/libdtrl_trainer_emul.so: the element-wise functors of dtrl_trainer_core.h), their
-m gpu twins lib/libdtrl.so (the dedicated apply / sum-of-squares kernels of dtrl_trainer.hip). Shapes: cases A (inside the fused plan, 110 534 parameters = 27 633
groups of four + a tail of two, 27 partial sums of squares) and D (layer by layer, 1 319 parameters, tail of three) of tests/test_hip_trainer_shapes.py.

`restate` below is the specification (include/dtrl_trainer.h) written out in numpy fp64.

Tolerances of the rule tests (TOL_RULE), per array, relative to the array's largest entry: 20 x the worst deviation the check build shows against `restate` on the
inputs of test_rule_in_isolation (worst over the six types x three clip settings on case A, the clip that bites on case D, four calls each: w 5.74e-8, h 1.10e-7,
h2 1.59e-7 -- one or two float32 roundings of the array's largest entries), so w 1.15e-6, h 2.2e-6, h2 3.2e-6. A wrong formula shows far above. Broken once each on a
scratch copy of dtrl_trainer_ops.h and run through run_rule on case A (clip off / clip that bites), w deviated by: delta inside the root 2.0e-2 / 1.8e-2 (AdaGrad),
1.6e-1 / 8.2e-2 (RMSProp), 8.5e-3 / 6.6e-3 (Adam) -- carried by the entries T with a tiny gradient and no history --; AdaDelta's e from h2 after its update 6.8e-4 / 3.4e-4;
Adam's correction at t instead of t + 1 2.3e-2 / 4.9e-2 (docs/EXPERIMENTS.md, "Solver types and learning-rate policies")."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import REPO, REFDATA
from test_hip_trainer_shapes import (CASES, EMUL_TRAINER_LIB, RELU_MARGIN, SOLVER, TOL_GRAD, TOL_LOSS, TOL_W, _per_blob, _rows_ptr, blob_slices, make_desc, make_ref_net,
                                     reference, relu_preactivations, write_prototxts)

TYPES = ("sgd", "nesterov", "adagrad", "rmsprop", "adadelta", "adam")
TOL_RULE = dict(w=1.15e-6, h=2.2e-6, h2=3.2e-6)
f32 = lambda a: np.asarray(a, np.float32)


def solver_of(ty, **over):
    """a full solver dict (trainer.parse_solver's keys) of type `ty`: the numbers as float32 holds them, which is what the library computes with"""
    s = dict(type=ty, lr_policy="fixed", base_lr=0.01, momentum=0.0 if ty in ("adagrad", "rmsprop") else 0.9, momentum2=0.999, rms_decay=0.99, delta=1e-8,
             weight_decay=0.0005, gamma=0.1, power=0.75, clip_gradients=-1.0, stepsize=1)
    s.update(over)
    return {k: (v if k in ("type", "lr_policy", "stepsize") else float(np.float32(v))) for k, v in s.items()}


def lr_rate(s, t):
    if s["lr_policy"] == "step":
        return s["base_lr"] * s["gamma"] ** (t // int(s["stepsize"]))
    if s["lr_policy"] == "exp":
        return s["base_lr"] * s["gamma"] ** t
    if s["lr_policy"] == "inv":
        return s["base_lr"] * (1 + s["gamma"] * t) ** (-s["power"])
    return s["base_lr"]


def restate(s, w, h, h2, t, g, rows, batch, lr_mult, decay_mult):
    """one update in fp64 from float32 (or float64) inputs: (w, h, h2, t) after it. g = the gradient buffer (mean over `batch` rows, summed over ranks), rows behind it"""
    w, h, h2, g, lr_mult, decay_mult = [None if a is None else np.asarray(a, np.float64) for a in (w, h, h2, g, lr_mult, decay_mult)]
    if not rows > 0:
        return w, h, h2, t
    g = g * (batch / rows)
    if s["clip_gradients"] >= 0:
        n = np.sqrt((g * g).sum())
        if n > s["clip_gradients"]:
            g = g * (s["clip_gradients"] / n)
    d = g + s["weight_decay"] * decay_mult * w
    local = lr_rate(s, t) * lr_mult
    mom, delta, ty = s["momentum"], s["delta"], s["type"]
    if ty == "sgd":
        h = mom * h + local * d; u = h
    elif ty == "nesterov":
        hp = h; h = mom * h + local * d; u = (1 + mom) * h - mom * hp
    elif ty == "adagrad":
        h = h + d * d; u = local * d / (np.sqrt(h) + delta)
    elif ty == "rmsprop":
        h = s["rms_decay"] * h + (1 - s["rms_decay"]) * d * d; u = local * d / (np.sqrt(h) + delta)
    elif ty == "adadelta":
        h = mom * h + (1 - mom) * d * d
        e = d * np.sqrt((h2 + delta) / (h + delta))
        h2 = mom * h2 + (1 - mom) * e * e
        u = local * e
    else:
        m2 = s["momentum2"]
        h = mom * h + (1 - mom) * d
        h2 = m2 * h2 + (1 - m2) * d * d
        u = local * (np.sqrt(1 - m2 ** (t + 1)) / (1 - mom ** (t + 1))) * h / (np.sqrt(h2) + delta)
    return w - u, h, h2, t + 1


def rel(got, want):
    return float(np.abs(np.asarray(got, np.float64) - want).max() / max(np.abs(want).max(), 1e-300))


# ---- a trainer with a caller's gradient buffer ----
class Rig:
    """NativeTrainer of case `name` with mixed multipliers (biases undecayed) and a bound gradient buffer of num_params + 1 floats the test writes"""

    def __init__(self, name, lib, device, solver=None):
        from deepterrainrl_amd import hip_trainer as ht
        self.c, self.device = CASES[name], device
        self.nt = ht.NativeTrainer(make_desc(self.c), -1 if device == "cpu" else 0, lib)
        self.P, self.B = self.nt.num_params, self.c["batch"]
        self.blobs = blob_slices(make_ref_net(self.c))
        self.lr_mult, self.decay_mult = np.ones(self.P, np.float32), np.ones(self.P, np.float32)
        for i, sl in enumerate(self.blobs):
            if i % 2:
                self.lr_mult[sl], self.decay_mult[sl] = (2.0, 3.0)[(i // 2) % 2], 0.0
            else:
                self.lr_mult[sl], self.decay_mult[sl] = (1.0, 0.5, 1.5, 0.75)[(i // 2) % 4], (1.0, 0.5, 2.0)[(i // 2) % 3]
        self.nt.set_params(3, self.lr_mult); self.nt.set_params(4, self.decay_mult)
        if solver:
            self.nt.set_solver(solver)
        if device == "cpu":
            self.gbuf = np.zeros(self.P + 1, np.float32)
            self.nt.bind_grad(self.gbuf.ctypes.data)
        else:
            import torch
            self.gbuf = torch.zeros(self.P + 1, dtype=torch.float32, device=device)
            self.nt.bind_grad(self.gbuf.data_ptr())

    def put_grad(self, g, rows):
        a = np.concatenate([f32(g), f32([rows])])
        if self.device == "cpu":
            self.gbuf[:] = a
        else:
            import torch
            self.gbuf.copy_(torch.from_numpy(a)); torch.cuda.synchronize()

    def state(self, s):
        return self.nt.get_params(0), self.nt.get_params(2), (self.nt.get_params(5) if s["type"] in ("adadelta", "adam") else None), self.nt.get_solver()[1]

    def close(self):
        self.nt.sync(); self.nt.bind_grad(None); self.nt.close()


def rule_inputs(rig, ty, seed):
    """weights, histories, four gradients and their row counts: exact zeros (gradient, histories, and weight or decay_mult) in Z; gradient entries 1e-6 x the largest on
    zero weights and zero histories in T"""
    rng = np.random.RandomState(seed)
    P = rig.P
    w = f32(rng.normal(0, 0.1, P))
    Z = np.concatenate([np.arange(3), np.arange(rig.blobs[1].start, rig.blobs[1].start + 3), np.arange(P - 2, P)])      # weights (set to 0), biases (not decayed), the tail
    w[:3] = 0.0
    assert not rig.decay_mult[Z[3:]].any()
    T = np.arange(10, 20)
    if ty in ("sgd", "nesterov"):
        h, h2 = f32(rng.normal(0, 1e-3, P)), None
    elif ty in ("adagrad", "rmsprop"):
        h, h2 = f32(rng.uniform(0, 1e-2, P)), None
    elif ty == "adadelta":
        h, h2 = f32(rng.uniform(0, 1e-2, P)), f32(rng.uniform(0, 1e-4, P))
    else:
        h, h2 = f32(rng.normal(0, 0.05, P)), f32(rng.uniform(0, 1e-2, P))
    w[T] = 0.0                      # tiny gradient, no decay term, no history: where delta sits in the rule decides the update
    h[Z] = h[T] = 0.0
    if h2 is not None:
        h2[Z] = h2[T] = 0.0
    grads = []
    for k in range(4):
        g = f32(rng.normal(0, 0.05, P))
        g[T] = 1e-6 * np.abs(g).max() * np.sign(g[T])
        g[Z] = 0.0
        grads.append(g)
    rows = [rig.B, rig.B + 5, 0, 2 * rig.B]
    return w, h, h2, grads, rows, Z, T


CLIPS = ("off", "bites", "idle")


def run_rule(name, ty, clip, lib, device, policy="fixed", t0=3):
    """test 1 (and, with a policy, test 2's arithmetic): four apply_grad calls on chosen gradients, every array against `restate` re-seeded from the trainer's own
    float32 state before the call; returns the worst deviation per array"""
    rig = Rig(name, lib, device)
    w, h, h2, grads, rows, Z, T = rule_inputs(rig, ty, 11 + TYPES.index(ty))
    norms = [float(np.sqrt((g.astype(np.float64) ** 2).sum())) * rig.B / r for g, r in zip(grads, rows) if r]
    cg = {"off": -1.0, "bites": 0.5 * min(norms), "idle": 100.0 * max(norms)}[clip]
    s = solver_of(ty, clip_gradients=cg, lr_policy=policy, gamma=0.5 if policy != "fixed" else 0.1, stepsize=2)
    rig.nt.set_params(0, w)
    rig.nt.set_solver(s)
    got_s, it = rig.nt.get_solver()
    assert it == 0 and all(got_s[k] == s[k] for k in s), (got_s, s)
    assert not rig.nt.get_params(2).any()
    rig.nt.set_params(2, h)
    if h2 is not None:
        rig.nt.set_params(5, h2)
    rig.nt.set_solver_iter(t0)
    worst = dict(w=0.0, h=0.0, h2=0.0)
    for k, (g, r) in enumerate(zip(grads, rows)):
        w0, h0, s0, t = rig.state(s)
        ew, eh, eh2, et = restate(s, w0, h0, s0, t, g, r, rig.B, rig.lr_mult, rig.decay_mult)
        rig.put_grad(g, r)
        rig.nt.apply_grad(2 + k % 2); rig.nt.sync()
        assert rig.nt.loss[2 + k % 2] == r
        w1, h1, s1, t1 = rig.state(s)
        assert t1 == et == (t + (1 if r else 0))
        assert np.isfinite(w1).all() and np.isfinite(h1).all() and (s1 is None or np.isfinite(s1).all())
        if r == 0:
            assert np.array_equal(w1, w0) and np.array_equal(h1, h0) and (s1 is None or np.array_equal(s1, s0))
        else:
            assert np.abs(w1 - w0).max() > 1e-5                       # it moved
        assert np.array_equal(w1[Z], w[Z]) and not h1[Z].any() and (s1 is None or not s1[Z].any())     # d = 0 with zero history: the update is exactly 0
        worst["w"] = max(worst["w"], rel(w1, ew)); worst["h"] = max(worst["h"], rel(h1, eh))
        if s1 is not None:
            worst["h2"] = max(worst["h2"], rel(s1, eh2))
        if r and clip == "bites":      # the clip changed the result by far more than the comparison tolerates
            nw = restate(dict(s, clip_gradients=-1.0), w0, h0, s0, t, g, r, rig.B, rig.lr_mult, rig.decay_mult)[0]
            assert rel(nw, ew) > 100 * TOL_RULE["w"]
    rig.close()
    print("SOLVER-RULE case=%s lib=%s type=%s clip=%s policy=%s w=%.2e h=%.2e h2=%.2e" % (name, "emul" if device == "cpu" else "hip", ty, clip, policy, worst["w"], worst["h"], worst["h2"]))
    for k in worst:
        assert worst[k] <= TOL_RULE[k], (k, worst)
    return worst


RULE_RUNS = [("A", ty, cl) for ty in TYPES for cl in CLIPS] + [("D", ty, "bites") for ty in TYPES]


@pytest.mark.parametrize("name,ty,clip", RULE_RUNS)
def test_rule_in_isolation(name, ty, clip):
    run_rule(name, ty, clip, EMUL_TRAINER_LIB, "cpu")


@pytest.mark.gpu
@pytest.mark.parametrize("name,ty,clip", RULE_RUNS)
def test_gpu_rule_in_isolation(name, ty, clip):
    run_rule(name, ty, clip, None, "cuda")
    assert "libdtrl.so" in open("/proc/self/maps").read()


def test_second_history_is_refused_for_the_types_that_keep_none():
    from deepterrainrl_amd import DtrlError
    rig = Rig("D", EMUL_TRAINER_LIB, "cpu")
    for ty in TYPES:
        rig.nt.set_solver(solver_of(ty))
        if ty in ("adadelta", "adam"):
            assert not rig.nt.get_params(5).any()
        else:
            with pytest.raises(DtrlError):
                rig.nt.get_params(5)
            with pytest.raises(DtrlError):
                rig.nt.set_params(5, np.zeros(rig.P, np.float32))
    rig.close()


# ---- 2. schedules ----
def run_schedule(policy, lib, device):
    rig = Rig("D", lib, device)
    s = solver_of("sgd", lr_policy=policy, gamma=0.5, power=0.75, stepsize=2)
    rng = np.random.RandomState(5)
    w = f32(rng.normal(0, 0.1, rig.P))
    rig.nt.set_params(0, w); rig.nt.set_solver(s)
    grads = [f32(rng.normal(0, 0.05, rig.P)) for _ in range(5)]
    snaps, rates = [], []
    for k, g in enumerate(grads):
        w0, h0, _, t = rig.state(s)
        assert t == k
        ew, eh, _, et = restate(s, w0, h0, None, t, g, rig.B, rig.B, rig.lr_mult, rig.decay_mult)
        rig.put_grad(g, rig.B); rig.nt.apply_grad(2); rig.nt.sync()
        w1, h1, _, t1 = rig.state(s)
        assert t1 == et == k + 1
        assert rel(w1, ew) <= TOL_RULE["w"] and rel(h1, eh) <= TOL_RULE["h"], (policy, k, rel(w1, ew), rel(h1, eh))
        # the rate moved the result: the same update at base_lr is far outside the tolerance once the schedule has left it
        fw = restate(dict(s, lr_policy="fixed"), w0, h0, None, t, g, rig.B, rig.B, rig.lr_mult, rig.decay_mult)[0]
        rates.append(lr_rate(s, k))
        assert (rel(fw, ew) > 100 * TOL_RULE["w"]) == (rates[-1] != s["base_lr"]), (policy, k)
        snaps.append((w1, h1))
    assert {"step": [1, 1, .5, .5, .25], "exp": [1, .5, .25, .125, .0625]}.get(policy, None) in (None, [r / s["base_lr"] for r in rates])
    rig.close()
    # a resumed run: the state after three updates and set_solver_iter(3) continue as the run that got there by itself
    rig = Rig("D", lib, device, s)
    rig.nt.set_params(0, snaps[2][0]); rig.nt.set_params(2, snaps[2][1]); rig.nt.set_solver_iter(3)
    for k in (3, 4):
        rig.put_grad(grads[k], rig.B); rig.nt.apply_grad(2); rig.nt.sync()
        w1, h1, _, t1 = rig.state(s)
        assert t1 == k + 1 and np.array_equal(w1, snaps[k][0]) and np.array_equal(h1, snaps[k][1])
    rig.close()


@pytest.mark.parametrize("policy", ["step", "exp", "inv"])
def test_schedules(policy):
    run_schedule(policy, EMUL_TRAINER_LIB, "cpu")


@pytest.mark.gpu
@pytest.mark.parametrize("policy", ["step", "exp", "inv"])
def test_gpu_schedules(policy):
    run_schedule(policy, None, "cuda")


# ---- 3. step = gradient + apply ----
def replay_rows(c, n, seed):
    """n MACE rows [r | s | a | s'] of case c's shape + flag words"""
    S, A, NF = c["n_terr"] + c["n_char"], 1 + c["frag_size"], c["n_frags"]
    rng = np.random.RandomState(seed)
    rows = f32(rng.normal(0, 1, size=(n, 1 + 2 * S + A)))
    rows[:, 0] = rng.uniform(0, 1, n)
    rows[:, 1 + S] = rng.randint(0, NF, n)
    return rows, (rng.uniform(size=n) < 0.2).astype(np.int64)


def start_trainer(name, lib, device, s, replay=None, stream=None):
    """a trainer from reference(name)'s start under solver s (None: as created); replay = (rows, flags) to bind"""
    from deepterrainrl_amd import hip_trainer as ht
    R = reference(name)
    nt = ht.NativeTrainer(make_desc(R["c"]), -1 if device == "cpu" else 0, lib)
    if stream is not None:
        nt.set_stream(stream)
    if s is not None:
        nt.set_solver(s)
    nt.set_params(0, R["w0"]); nt.set_params(3, R["lr_mult"]); nt.set_params(4, R["decay_mult"])
    nt.set_normalizers(*[a.astype(np.float64) for a in R["norm"]])
    nt.update_target()
    keep = None
    if replay is not None:
        (mp, km), (fp, kf) = _rows_ptr(replay[0], device), _flags_ptr(replay[1], device)
        nt.bind_replay(mp, fp, replay[0].shape[1]); keep = (km, kf)
    return nt, keep


def _flags_ptr(a, device):
    a = np.ascontiguousarray(a, np.int64)
    if device == "cpu":
        return a.ctypes.data, a
    import torch
    t = torch.as_tensor(a).to(device); torch.cuda.synchronize()
    return t.data_ptr(), t


def full_state(nt, s):
    return [nt.get_params(0), nt.get_params(2)] + ([nt.get_params(5)] if s is not None and s["type"] in ("adadelta", "adam") else [])


def run_step_vs_grad_apply(name, ty, lib, device):
    """dtrl_trainer_step (and, case A, critic_step / actor_step on a bound replay memory) against grad_step (critic_grad / actor_grad) + apply_grad on a twin: the same
    launches on the same inputs, so weights and histories are bit-identical after three steps"""
    R = reference(name)
    c, B = R["c"], R["c"]["batch"]
    s = solver_of(ty, lr_policy="inv", gamma=0.5, clip_gradients=1e-3)       # (the random labels' gradient norm is of order 1: this clip bites)
    replay = replay_rows(c, 40, 3) if name == "A" else None
    a, ka = start_trainer(name, lib, device, s, replay)
    b, kb = start_trainer(name, lib, device, s, replay)
    data = [(R["X"][k % 2], R["Y"][k % 2]) for k in range(3)]
    for X, Y in data:
        xp, kx = _rows_ptr(X, device); yp, ky = _rows_ptr(Y, device)
        a.step(xp, yp); a.sync()
        b.grad_step(xp, yp); b.apply_grad(2); b.sync()
    sa, sb = full_state(a, s), full_state(b, s)
    assert all(np.array_equal(x, y) for x, y in zip(sa, sb))
    assert np.abs(sa[0] - R["w0"]).max() > 1e-6 and a.get_solver()[1] == b.get_solver()[1] == 3
    if replay is not None:
        rng = np.random.RandomState(9)
        for k in range(3):
            ids = rng.randint(0, 40, B)
            for nt in (a, b):
                nt.idx[:B] = ids; nt.idx[nt.max_eval:nt.max_eval + B] = ids[::-1]
            a.critic_step(); a.actor_step(); a.sync()
            b.critic_grad(); b.apply_grad(2); b.actor_grad(); b.apply_grad(3); b.sync()
            assert a.loss[0] == b.loss[0] and a.loss[1] == b.loss[1] and np.isfinite(a.loss[:2]).all()
        ta, tb = full_state(a, s), full_state(b, s)
        assert all(np.array_equal(x, y) for x, y in zip(ta, tb))
        assert np.abs(ta[0] - sa[0]).max() > 1e-6 and a.get_solver()[1] == b.get_solver()[1] == 9      # critic and actor steps share the counter
    a.close(); b.close()


@pytest.mark.parametrize("name", ["A", "D"])
@pytest.mark.parametrize("ty", TYPES)
def test_step_equals_grad_plus_apply(name, ty):
    run_step_vs_grad_apply(name, ty, EMUL_TRAINER_LIB, "cpu")


GPU_STEP_RUNS = [(n, ty, m) for n in ("A", "D") for ty in TYPES for m in ((0, 1, 2, 3, 4) if CASES[n]["plan"] else (0, 1))]


@pytest.mark.gpu
@pytest.mark.parametrize("name,ty,mode", GPU_STEP_RUNS)
def test_gpu_step_equals_grad_plus_apply_in_every_fused_mode(monkeypatch, name, ty, mode):
    monkeypatch.setenv("DTRL_TRAINER_FUSED", str(mode))
    run_step_vs_grad_apply(name, ty, None, "cuda")


# ---- 4. Nesterov end to end ----
_NESTEROV = {}


def nesterov_reference(name):
    """two whole steps of oracle/trainer_ref.py's forward / backward with the Nesterov rule on top, from reference(name)'s start; the data seed is the first of range(64)
    for which the fp64 run alone keeps every ReLU pre-activation RELU_MARGIN from zero"""
    if name in _NESTEROV:
        return _NESTEROV[name]
    R = reference(name)
    net, B, S, out = R["net"], R["c"]["batch"], R["S"], R["out"]
    io, isc, oo, osc = [a.astype(np.float64) for a in R["norm"]]
    s = solver_of("nesterov", **SOLVER)
    found = None
    for seed in range(64):
        r = np.random.RandomState(seed)
        X = [f32(r.normal(0, 1, (B, S))) for _ in range(2)]; Y = [f32(r.normal(0, 1, (B, out))) for _ in range(2)]
        w, h, t, steps, margin = R["w0"].astype(np.float64), np.zeros(net.num_params), 0, [], np.inf
        for k in range(2):
            x = (X[k].astype(np.float64) + io) * isc; label = (Y[k].astype(np.float64) + oo) * osc
            o = net.forward(w, x, keep=True)
            margin = min([margin] + [float(np.abs(z).min()) for z in relu_preactivations(net)])
            g = net.backward((o - label) / B)
            w, h, _, t = restate(s, w, h, None, t, g, B, B, R["lr_mult"], R["decay_mult"])
            steps.append(dict(loss=0.5 * ((o - label) ** 2).sum() / B, g=g, w=w, h=h))
        if margin >= RELU_MARGIN:
            found = dict(X=X, Y=Y, steps=steps, seed=seed, s=s)
            break
    assert found, "no data seed in range(64) keeps every ReLU pre-activation of case %s at least %g from zero under the Nesterov run" % (name, RELU_MARGIN)
    _NESTEROV[name] = found
    return found


def run_nesterov(name, lib, device):
    R, N = reference(name), nesterov_reference(name)
    nt, _ = start_trainer(name, lib, device, N["s"])
    P = R["net"].num_params
    for k, st in enumerate(N["steps"]):
        loss = nt.step_host(N["X"][k], N["Y"][k])
        fig = dict(loss=abs(loss - st["loss"]) / max(1.0, st["loss"]), grad=_per_blob(R, nt.debug_get(16, P).astype(np.float64), st["g"]),
                   w=_per_blob(R, nt.get_params(0).astype(np.float64), st["w"]), hist=_per_blob(R, nt.get_params(2).astype(np.float64), st["h"]))
        print("SOLVER-NESTEROV case=%s lib=%s step=%d seed=%d %s" % (name, "emul" if device == "cpu" else "hip", k, N["seed"], fig))
        assert fig["loss"] <= TOL_LOSS and fig["grad"] <= TOL_GRAD and fig["hist"] <= TOL_GRAD and fig["w"] <= TOL_W, fig
    # and the rule is not SGD's: the second step's weights differ from the shapes test's SGD reference by far more than the tolerance
    assert _per_blob(R, N["steps"][1]["w"], R["steps"][1]["w"]) > 100 * TOL_W or N["seed"] != R["seed"]
    assert nt.get_solver()[1] == 2
    nt.close()


@pytest.mark.parametrize("name", ["A", "D"])
def test_nesterov_end_to_end(name):
    run_nesterov(name, EMUL_TRAINER_LIB, "cpu")


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["A", "D"])
def test_gpu_nesterov_end_to_end(name):
    run_nesterov(name, None, "cuda")


# ---- 5. nothing moved for SGD ----
def run_sgd_unchanged(name, lib, device):
    R = reference(name)
    a, _ = start_trainer(name, lib, device, None)
    b, _ = start_trainer(name, lib, device, solver_of("sgd", **SOLVER))
    assert a.get_solver()[0] == b.get_solver()[0] and a.get_solver()[0]["type"] == "sgd" and a.get_solver()[0]["lr_policy"] == "fixed"
    for k in range(3):
        for nt in (a, b):
            nt.step_host(R["X"][k % 2], R["Y"][k % 2])
    assert np.array_equal(a.get_params(0), b.get_params(0)) and np.array_equal(a.get_params(2), b.get_params(2))
    assert np.abs(a.get_params(0) - R["w0"]).max() > 1e-5 and a.get_solver()[1] == b.get_solver()[1] == 3
    a.close(); b.close()


@pytest.mark.parametrize("name", ["A", "D"])
def test_sgd_default_is_unchanged_by_set_solver(name):
    run_sgd_unchanged(name, EMUL_TRAINER_LIB, "cpu")


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["A", "D"])
def test_gpu_sgd_default_is_unchanged_by_set_solver(name):
    run_sgd_unchanged(name, None, "cuda")


# ---- 6. graph replay ----
@pytest.mark.gpu
def test_gpu_recorded_step_replays_with_its_own_iteration():
    """Adam under "step" (stepsize 3) with a clip that bites: a trainer on the legacy stream (plain launches) and one on a stream of its own (critic / actor steps recorded
    once and replayed) stay bit-identical over seven steps, counter included, and step 5 of either differs from a run whose rate never stepped"""
    import torch
    name, B = "A", CASES["A"]["batch"]
    s = solver_of("adam", lr_policy="step", gamma=0.1, stepsize=3, clip_gradients=1e-3, base_lr=0.001)
    replay = replay_rows(CASES[name], 40, 3)
    own = torch.cuda.Stream()
    plain, k0 = start_trainer(name, None, "cuda", s, replay)
    graph, k1 = start_trainer(name, None, "cuda", s, replay, stream=own.cuda_stream)
    flat, k2 = start_trainer(name, None, "cuda", dict(s, lr_policy="fixed"), replay)
    rng = np.random.RandomState(2)
    for k in range(7):
        ids = rng.randint(0, 40, B)
        for nt in (plain, graph, flat):
            nt.idx[:B] = ids; nt.idx[nt.max_eval:nt.max_eval + B] = ids[::-1]
            (nt.critic_step if k % 2 == 0 else nt.actor_step)()       # (each recorded once: steps 0 / 1; replayed from then on)
            nt.sync()
        sp, sg = full_state(plain, s), full_state(graph, s)
        assert all(np.array_equal(x, y) for x, y in zip(sp, sg)), k
        assert plain.get_solver()[1] == graph.get_solver()[1] == k + 1
        if k == 5:
            wf = flat.get_params(0)
            assert np.abs(sp[0] - wf).max() > 1e-5 and np.abs(sg[0] - wf).max() > 1e-5
    for nt in (plain, graph, flat):
        nt.close()
    assert "libdtrl.so" in open("/proc/self/maps").read()


# ---- 7. files and refusals ----
def _files_lib():
    lib = C.CDLL(EMUL_TRAINER_LIB)
    lib.dtrl_trainer_create_from_files.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_float, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
    lib.dtrl_trainer_last_error.restype = C.c_char_p; lib.dtrl_trainer_last_error.argtypes = [C.c_void_p]
    lib.dtrl_trainer_destroy.argtypes = [C.c_void_p]
    return lib


def _from_files(lib, net, solver_txt, tmp_path, tag):
    """(rc, solver dict or error text) of dtrl_trainer_create_from_files on a solver prototxt with the given text"""
    from deepterrainrl_amd import hip_trainer as ht, trainer as tr
    p = tmp_path / ("solver_%s.prototxt" % tag)
    p.write_text(solver_txt)
    h = C.c_void_p()
    rc = lib.dtrl_trainer_create_from_files(net.encode(), str(p).encode(), REFDATA.encode(), 0.9, 0, -1, C.byref(h))
    if rc != 0:
        return rc, lib.dtrl_trainer_last_error(None).decode(), str(p)
    sd, it = ht.SolverDesc(), C.c_int64()
    lib.dtrl_trainer_get_solver.argtypes = [C.c_void_p, C.POINTER(ht.SolverDesc), C.POINTER(C.c_int64)]
    assert lib.dtrl_trainer_get_solver(h, C.byref(sd), C.byref(it)) == 0 and it.value == 0
    d = {k: float(getattr(sd, k)) for k in ht.SOLVER_FLOATS}
    d.update(type=tr.SOLVER_TYPES[sd.type], lr_policy=tr.LR_POLICIES[sd.lr_policy], stepsize=int(sd.stepsize))
    lib.dtrl_trainer_destroy(h)
    return 0, d, str(p)


def test_solver_files_and_refusals(tmp_path):
    from deepterrainrl_amd import trainer as tr, hip_trainer as ht, DtrlError
    lib = _files_lib()
    paths = write_prototxts(tmp_path, CASES["A"])
    net = paths["train"]
    head = 'net: "%s"\nbase_lr: 0.002\nweight_decay: 0.0005\n' % net

    def agree(txt, tag, **want):
        rc, d, p = _from_files(lib, net, head + txt, tmp_path, tag)
        assert rc == 0, d
        ps = tr.parse_solver(p)
        for k in ht.SOLVER_FLOATS + ("type", "lr_policy"):
            assert d[k] == (ps[k] if isinstance(ps[k], str) else float(np.float32(ps[k]))), (tag, k, d[k], ps[k])
        if "stepsize" in txt:
            assert d["stepsize"] == ps["stepsize"]
        for k, v in want.items():
            assert d[k] == (v if isinstance(v, (str, int)) else float(np.float32(v))), (tag, k, d[k], v)
        return d

    # nothing named: SGD / fixed with Caffe's defaults; the existing keys keep their values
    d = agree("momentum: 0.9\n", "plain", type="sgd", lr_policy="fixed", base_lr=0.002, momentum=0.9, weight_decay=0.0005, momentum2=0.999, rms_decay=0.99, delta=1e-8, gamma=0.1,
              power=0.75, clip_gradients=-1.0)
    assert tr.parse_solver(os.path.join(REFDATA, "data/policies/dog/nets/dog_mace3_solver.prototxt"))["type"] == "sgd"
    # both spellings, case-insensitively; every new key
    for k, (enum, later) in enumerate((("SGD", "SGD"), ("NESTEROV", "Nesterov"), ("ADAGRAD", "AdaGrad"), ("RMSPROP", "RMSProp"), ("ADADELTA", "AdaDelta"), ("ADAM", "Adam"))):
        mom = "" if TYPES[k] in ("adagrad", "rmsprop") else "momentum: 0.95\n"
        agree(mom + "solver_type: %s\n" % enum, "enum%d" % k, type=TYPES[k])
        agree(mom + 'type: "%s"\n' % later, "later%d" % k, type=TYPES[k])
        agree(mom + 'type: "%s"\n' % later.upper(), "upper%d" % k, type=TYPES[k])
        agree(mom + "solver_type: %s\n" % enum.lower(), "lower%d" % k, type=TYPES[k])
    agree('momentum: 0.8\nsolver_type: ADAM\nmomentum2: 0.99\nrms_decay: 0.9\ndelta: 1e-6\nlr_policy: "step"\ngamma: 0.5\npower: 0.6\nstepsize: 1000\nclip_gradients: 10\n', "all",
          type="adam", lr_policy="step", momentum=0.8, momentum2=0.99, rms_decay=0.9, delta=1e-6, gamma=0.5, power=0.6, stepsize=1000, clip_gradients=10.0)
    agree('lr_policy: "exp"\ngamma: 0.999\n', "exp", lr_policy="exp", gamma=0.999)
    agree('lr_policy: "inv"\ngamma: 0.0001\npower: 0.75\n', "inv", lr_policy="inv", gamma=0.0001)

    # refusals, by their message: the file and the value, or the field
    def refused(txt, tag, *words):
        rc, msg, p = _from_files(lib, net, head + txt, tmp_path, tag)
        assert rc != 0, (tag, msg)
        for wd in words + (os.path.basename(p),):
            assert wd in msg, (tag, wd, msg)
        return p

    for pol in ("multistep", "poly", "sigmoid"):
        p = refused('lr_policy: "%s"\n' % pol, "pol_" + pol, "lr_policy", '"%s"' % pol)
        with pytest.raises(ValueError, match=pol):
            tr.check_solver(tr.parse_solver(p))
    p = refused('type: "LBFGS"\n', "type", "solver type", '"LBFGS"')
    with pytest.raises(ValueError, match="lbfgs"):
        tr.parse_solver(p)
    refused("solver_type: FTRL\n", "enum", "solver type", '"FTRL"')
    for txt, tag, field in (("momentum: 1.0\n", "mom1", "momentum"), ("momentum: -0.1\n", "momneg", "momentum"), ("solver_type: ADAM\nmomentum2: 1\n", "mom2", "momentum2"),
                            ("solver_type: RMSPROP\nrms_decay: 1.5\n", "rms", "rms_decay"), ("solver_type: ADAGRAD\ndelta: 0\n", "delta0", "delta"),
                            ("solver_type: ADAM\ndelta: -1e-8\n", "deltaneg", "delta"), ("solver_type: ADAGRAD\nmomentum: 0.9\n", "agmom", "momentum"),
                            ("solver_type: RMSPROP\nmomentum: 0.5\n", "rmsmom", "momentum"), ('lr_policy: "step"\nstepsize: 0\n', "step0", "stepsize"),
                            ('lr_policy: "step"\n', "nostep", "stepsize")):
        p = refused(txt, tag, field)
        with pytest.raises(ValueError, match=field):
            ps = tr.parse_solver(p)
            if "stepsize" not in txt:
                ps["stepsize"] = 0
            tr.check_solver(ps)
    agree("delta: 0\n", "sgd_delta0", delta=0.0)       # delta is not read by types 0 and 1
    # the same refusals through dtrl_trainer_set_solver: status 1, the field named, and nothing changed
    rig = Rig("D", EMUL_TRAINER_LIB, "cpu", solver_of("nesterov"))
    for bad, field in ((dict(type=6), "type"), (dict(type=-1), "type"), (dict(lr_policy=4), "lr_policy"), (dict(momentum=1.0), "momentum"), (dict(type="adam", momentum2=1.0), "momentum2"),
                       (dict(type="rmsprop", momentum=0.0, rms_decay=-0.5), "rms_decay"), (dict(type="adadelta", delta=0.0), "delta"), (dict(type="adagrad"), "momentum"),
                       (dict(lr_policy="step", stepsize=0), "stepsize")):
        with pytest.raises(DtrlError, match=field):
            rig.nt.set_solver(dict(solver_of("nesterov"), **bad))
        assert rig.nt.get_solver()[0]["type"] == "nesterov"
    with pytest.raises(DtrlError, match="multistep"):
        rig.nt.set_solver(dict(solver_of("sgd"), lr_policy="multistep"))
    rig.close()


def test_a_trainer_takes_the_solver_of_its_file_and_overrides(tmp_path):
    """HipMACETrainer hands the parsed solver on (it used to refuse every policy but "fixed" and to ignore the type), `solver=` lays overrides over the file"""
    from deepterrainrl_amd import hip_trainer as ht
    c = CASES["A"]
    S, A = c["n_terr"] + c["n_char"], 1 + c["frag_size"]
    p = write_prototxts(tmp_path, c)
    adam = tmp_path / "adam_solver.prototxt"
    adam.write_text('base_lr: 0.001\nmomentum: 0.9\nweight_decay: 0.0005\nsolver_type: ADAM\nlr_policy: "inv"\ngamma: 0.001\npower: 0.5\n')
    t = ht.HipMACETrainer(p["train"], str(adam), S, A, lib_path=EMUL_TRAINER_LIB, mem_size=64, num_init_samples=10, device="cpu", seed=1)
    s, it = t.nt.get_solver()
    assert (s["type"], s["lr_policy"], it) == ("adam", "inv", 0) and s["gamma"] == float(np.float32(0.001)) and s["base_lr"] == float(np.float32(t.solver["base_lr"]))
    t = ht.HipMACETrainer(p["train"], p["solver"], S, A, lib_path=EMUL_TRAINER_LIB, mem_size=64, num_init_samples=10, device="cpu", seed=1,
                          solver=dict(type="RMSProp", momentum=0, base_lr=1e-4, clip_gradients=10))
    s, _ = t.nt.get_solver()
    assert (s["type"], s["clip_gradients"], s["base_lr"]) == ("rmsprop", 10.0, float(np.float32(1e-4)))
    with pytest.raises(ValueError, match="unknown keys"):
        ht.HipMACETrainer(p["train"], p["solver"], S, A, lib_path=EMUL_TRAINER_LIB, mem_size=64, num_init_samples=10, device="cpu", seed=1, solver=dict(beta1=0.9))
    t = ht.HipMACETrainer(p["train"], p["solver"], S, A, lib_path=EMUL_TRAINER_LIB, mem_size=64, num_init_samples=10, device="cpu", seed=1)
    assert t.nt.get_solver()[0]["type"] == "sgd"


def test_init_xavier_clears_both_histories_and_the_counter():
    rig = Rig("D", EMUL_TRAINER_LIB, "cpu", solver_of("adam"))
    rng = np.random.RandomState(0)
    rig.nt.set_params(0, f32(rng.normal(0, 0.1, rig.P)))
    rig.put_grad(f32(rng.normal(0, 0.05, rig.P)), rig.B); rig.nt.apply_grad(2); rig.nt.sync()
    assert rig.nt.get_params(2).any() and rig.nt.get_params(5).any() and rig.nt.get_solver()[1] == 1
    rig.nt.init_xavier(3)
    assert not rig.nt.get_params(2).any() and not rig.nt.get_params(5).any() and rig.nt.get_solver()[1] == 0
    rig.close()


# ---- 8. the torch peer ----
@pytest.mark.parametrize("ty", TYPES)
def test_torch_peer_rules_in_fp64(tmp_path, ty):
    """MACETrainer._solver_step_body under each type against `restate` on the gradient torch computed, two steps under "inv" with a clip that bites, to 1e-12"""
    import torch
    from deepterrainrl_amd import trainer as tr
    c = CASES["D"]
    S, A = c["n_terr"] + c["n_char"], 1 + c["frag_size"]
    p = write_prototxts(tmp_path, c)
    over = dict(type=ty, lr_policy="inv", gamma=0.5, clip_gradients=1e-3, momentum=0.0 if ty in ("adagrad", "rmsprop") else 0.9)
    t = tr.MACETrainer(p["train"], p["solver"], S, A, mem_size=64, num_init_samples=10, device="cpu", dtype=torch.float64, seed=1, use_graphs=False, solver=over)
    assert t.solver["type"] == ty
    rng = np.random.RandomState(4)
    lr_mult, decay_mult = t.rate_mult.numpy().copy(), t.decay_mult.numpy().copy()
    for k in range(2):
        X = torch.as_tensor(rng.normal(0, 1, (t.batch, S))); Y = torch.as_tensor(rng.normal(0, 1, (t.batch, t.out_size)))
        w0, h0 = t.net.flat.detach().numpy().copy(), t.hflat.numpy().copy()
        s0 = t.h2flat.numpy().copy() if getattr(t, "h2flat", None) is not None else np.zeros_like(w0)
        t._solver_step(X, Y)
        g = t.net.gflat.numpy().copy()
        assert np.sqrt((g * g).sum()) > 1e-3
        ew, eh, eh2, et = restate(t.solver, w0, h0, s0, k, g, t.batch, t.batch, lr_mult, decay_mult)
        assert et == t.solver_iter == k + 1
        assert rel(t.net.flat.detach().numpy(), ew) < 1e-12 and rel(t.hflat.numpy(), eh) < 1e-12
        if ty in ("adadelta", "adam"):
            assert rel(t.h2flat.numpy(), eh2) < 1e-12
        assert np.abs(ew - w0).max() > 1e-9


# ---- the training loop ----
@pytest.mark.parametrize("trainer", ["hip", "torch"])
def test_train_loop_lays_solver_overrides_over_the_file(trainer):
    """train_loop.train(solver=...) for both trainers: a tiny run of the dog's MACE loop under Adam with a clip (lane-loop engine, plain-loop trainer build)"""
    from conftest import _emul_scenario_cls
    from deepterrainrl_amd import train_loop
    seen = []
    st = train_loop.train("args/opt_args_train_mace.txt", REFDATA, num_envs=64, seed=1, max_iters=2, max_frames=60, trainer_device="cpu", scenario_cls=_emul_scenario_cls(), trainer=trainer,
                          trainer_lib=EMUL_TRAINER_LIB if trainer == "hip" else None, solver=dict(type="adam", base_lr=1e-4, clip_gradients=10),
                          eval_every=1, eval_fn=lambda it, t, b: seen.append((it, t)),
                          extra_args={"terrain_seed": 3, "trainer_num_init_samples": 30, "trainer_replay_mem_size": 512, "trainer_freeze_target_iters": 4,
                                      "init_exp_rate": 0.3, "init_exp_base_rate": 0.1, "trainer_init_input_offset_scale": "false"})     # (the tiny-run settings of tests/test_variant_redraw.py)
    t = seen[-1][1]
    assert st["iters"] >= 2 and np.isfinite(st["weights"]).all()
    assert (t.solver["type"], t.solver["base_lr"], t.solver["clip_gradients"], t.solver["momentum"]) == ("adam", 1e-4, 10.0, 0.9)
    if trainer == "hip":
        s, it = t.nt.get_solver()
        assert (s["type"], s["clip_gradients"]) == ("adam", 10.0) and it == t.solver_iter >= 2
    else:
        assert t.h2flat is not None and float(t.h2flat.abs().max()) > 0
