#!/usr/bin/env python3
"""What external policy mode costs: env-steps/s of configs[1]'s shape (4096 dogs, slopes_mixed) in one process, one after the other on one GPU:
  (a) internal mode under the xavier weights (dtrl_step per frame -- the call external mode uses -- so that the three figures share their host path);
  (b) external mode with a policy that costs nothing (a constant row): the price of parking plus the round trip through the device calls;
  (c) external mode with a torch MLP 283-256-256-n_opt on the same GPU through the device calls.
Each leg: bench.py's pre-roll (blocks of 20 frames / ticks until the reset rate settles, 60 .. 200), then at least --seconds of timed work. (a) counts 20 env-steps per env
and frame; (b) and (c) take env-steps from dtrl_ext_stats (a tick advances an env by 0 .. 20 env-steps). Also reported: the device time of the collection and scatter
launches per tick. Prints one JSON line; --out appends a readable summary to a file.
  python tools/external_policy_bench.py [--envs 4096] [--seconds 5] [--out profiles/ext_policy.txt]"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import bench as B   # noqa: E402  (configs, synthetic weights, pre-roll constants)


def preroll(b, tick):
    done = 0; rates = []; r_prev = b.EvalStats()["resets"]
    while done < B.PREROLL_MAX:
        for _ in range(B.PREROLL_BLOCK):
            tick()
        done += B.PREROLL_BLOCK
        r = b.EvalStats()["resets"]; rates.append((r - r_prev) / float(B.PREROLL_BLOCK)); r_prev = r
        if done >= B.PREROLL_MIN and len(rates) >= 2 and rates[-1] > 0 and abs(rates[-1] - rates[-2]) <= 0.25 * max(rates[-1], rates[-2]):
            break
    return done


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=B.CONFIGS[1]["envs"])
    ap.add_argument("--seconds", type=float, default=5.0)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import deepterrainrl_amd as da
    da.configure_hw_queues()
    import torch
    dev = torch.device("cuda", 0)
    cfg = B.CONFIGS[1]
    n = a.envs
    res = {"envs": n, "workload": cfg["name"], "min_timed_s": a.seconds}

    # (a) internal
    b = da.BatchScenario(cfg["arg_file"], n, data_root=B.ROOT, device_id=0, extra_args={"terrain_seed": 11})
    b.SetPolicy(B.xavier_weights(b.PolicyNumParams(), cfg["n_char"], cfg["frag"]), *B.load_scale(cfg))
    pre = preroll(b, b.Update)
    torch.cuda.synchronize()
    t0 = time.perf_counter(); frames = 0
    while time.perf_counter() - t0 < a.seconds:
        for _ in range(10):
            b.Update()
        frames += 10
    wall = time.perf_counter() - t0
    res["internal"] = {"env_steps_per_s": frames * B.STEPS_PER_FRAME * n / wall, "frames": frames, "wall_s": wall, "preroll": pre}
    b.close()

    def external(policy_of):
        b = da.BatchScenario(cfg["arg_file"], n, data_root=B.ROOT, device_id=0, extra_args={"terrain_seed": 11, "policy_mode": "external"})
        ids = torch.zeros(n, dtype=torch.int32, device=dev); st = torch.zeros((n, b.S), dtype=torch.float32, device=dev)
        lab = torch.zeros(n, dtype=torch.int32, device=dev); prm = torch.zeros((n, b.n_opt), dtype=torch.float32, device=dev)
        policy = policy_of(b)
        torch.cuda.synchronize()
        box = {"decisions": 0, "rejected": 0}

        def tick():
            b.Update()
            m = b.PendingActionsDevice(ids.data_ptr(), st.data_ptr(), n)
            if m:
                with torch.no_grad():
                    prm[:m] = policy(st[:m])
                torch.cuda.current_stream(dev).synchronize()
                box["rejected"] += b.SupplyActionsDevice(ids.data_ptr(), m, lab.data_ptr(), prm.data_ptr(), 0)
                box["decisions"] += m
        pre = preroll(b, tick)
        b.ExtLaunchMs(0); b.ExtLaunchMs(1)
        s0 = b.ExtStats(); d0 = box["decisions"]
        t0 = time.perf_counter(); ticks = 0
        while time.perf_counter() - t0 < a.seconds:
            for _ in range(10):
                tick()
            ticks += 10
        wall = time.perf_counter() - t0
        s1 = b.ExtStats()
        steps = s1["env_steps_total"] - s0["env_steps_total"]
        out = {"env_steps_per_s": steps / wall, "ticks": ticks, "wall_s": wall, "preroll": pre, "env_steps": steps,
               "env_steps_per_env_tick": steps / float(n * ticks), "decisions_per_env_tick": (box["decisions"] - d0) / float(n * ticks), "rejected": box["rejected"],
               "collect_ms_per_tick": b.ExtLaunchMs(0) / ticks, "scatter_ms_per_tick": b.ExtLaunchMs(1) / ticks}
        b.close()
        return out

    def free_policy(b):
        row = torch.tensor(b.ActionTable()[b.n_labels // 2], dtype=torch.float32, device=dev)
        return lambda s: row.expand(s.shape[0], -1)

    def mlp_policy(b):
        torch.manual_seed(0)
        base = torch.tensor(b.ActionTable()[b.n_labels // 2], dtype=torch.float32, device=dev)
        net = torch.nn.Sequential(torch.nn.Linear(b.S, 256), torch.nn.ReLU(), torch.nn.Linear(256, 256), torch.nn.ReLU(), torch.nn.Linear(256, b.n_opt)).to(dev)
        return lambda s: base + 0.05 * torch.tanh(net(s))

    res["external_free"] = external(free_policy)
    res["external_mlp"] = external(mlp_policy)
    for k in ("external_free", "external_mlp"):
        res[k]["vs_internal"] = res[k]["env_steps_per_s"] / res["internal"]["env_steps_per_s"]
    print(json.dumps(res))
    if a.out:
        with open(a.out, "a") as f:
            f.write("external policy mode, %d dogs on slopes_mixed, one process, >= %.0f s per leg after the pre-roll\n" % (n, a.seconds))
            f.write("  (a) internal, xavier weights, dtrl_step per frame      %8.3f M env-steps/s (%d frames)\n" % (res["internal"]["env_steps_per_s"] / 1e6, res["internal"]["frames"]))
            for k, name in (("external_free", "(b) external, constant row through the device calls "), ("external_mlp", "(c) external, torch MLP 283-256-256-n_opt, device calls")):
                r = res[k]
                f.write("  %s %8.3f M env-steps/s = %.3f of (a); %d ticks, %.2f env-steps and %.4f decisions per env and tick; collection %.3f ms, scatter %.3f ms of device time per tick\n"
                        % (name, r["env_steps_per_s"] / 1e6, r["vs_internal"], r["ticks"], r["env_steps_per_env_tick"], r["decisions_per_env_tick"], r["collect_ms_per_tick"], r["scatter_ms_per_tick"]))


if __name__ == "__main__":
    main()
