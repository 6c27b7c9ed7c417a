"""The tick loop of external policy mode (BatchScenario(..., extra_args={"policy_mode": "external"})): the caller's policy decides, the engine simulates.

    run_external(b, policy, ticks)

`policy` is either
  * a torch.nn.Module on the batch's GPU: states [m][S] float32 -> parameters [m][n_opt], or (parameters, action_ids int[m]). The loop goes through
    dtrl_pending_actions_device / dtrl_supply_actions_device with preallocated tensors: states and actions never leave the device; or
  * a Python callable on numpy arrays: policy(ids int32[m], states float64[m][S]) -> params [m][n_opt] or (action_ids, params) or (action_ids, params, flags);
    the loop goes through the host calls.
Every tick: Update() (each env runs to the end of its frame or to its next decision), collect the parked envs, evaluate, supply."""
import numpy as np


def _is_torch_module(policy):
    try:
        import torch
    except Exception:
        return False
    return isinstance(policy, torch.nn.Module)


def run_external(b, policy, ticks, dt=1.0 / 30.0):
    """Run `ticks` ticks of an external-mode batch under `policy`; returns dict(decisions, rejected, ticks) plus b.ExtStats()."""
    if not getattr(b, "external", False):
        raise ValueError("run_external needs a batch created with extra_args={'policy_mode': 'external'}")
    decisions = rejected = 0
    if _is_torch_module(policy):
        import torch
        dev = next(policy.parameters()).device
        ids = torch.zeros(b.num_envs, dtype=torch.int32, device=dev)
        states = torch.zeros((b.num_envs, b.S), dtype=torch.float32, device=dev)
        act = torch.zeros(b.num_envs, dtype=torch.int32, device=dev)
        params = torch.zeros((b.num_envs, b.n_opt), dtype=torch.float32, device=dev)
        torch.cuda.synchronize(dev)
        with torch.no_grad():
            for _ in range(int(ticks)):
                b.Update(dt)
                m = b.PendingActionsDevice(ids.data_ptr(), states.data_ptr(), b.num_envs)   # (complete on return: the engine synchronised its stream)
                if m == 0:
                    continue
                out = policy(states[:m])
                if isinstance(out, (tuple, list)):
                    params[:m].copy_(out[0]); act[:m].copy_(out[1].to(torch.int32))
                else:
                    params[:m].copy_(out); act[:m].zero_()
                torch.cuda.current_stream(dev).synchronize()                                   # the rows are written before the engine's stream reads them
                rejected += b.SupplyActionsDevice(ids.data_ptr(), m, act.data_ptr(), params.data_ptr(), 0)
                decisions += m
    else:
        for _ in range(int(ticks)):
            b.Update(dt)
            e, s = b.PendingActions()
            if len(e) == 0:
                continue
            out = policy(e, s)
            if isinstance(out, (tuple, list)):
                aid, prm = out[0], out[1]
                fl = out[2] if len(out) > 2 else None
            else:
                aid, prm, fl = None, out, None
            b.SupplyActions(e, aid, np.asarray(prm, np.float64), fl)
            decisions += len(e)
    r = dict(decisions=decisions, rejected=rejected, ticks=int(ticks))
    r.update(b.ExtStats())
    return r
