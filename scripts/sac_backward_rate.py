#!/usr/bin/env python3
"""What the networks' share of SAC's gradient half costs on the device and in torch autograd on the same rows.  One GPU, one
process, same box.

  python scripts/sac_backward_rate.py [--out profiles/sac/backward_rate.json] [--windows 24]

Config 3 (BlueROV2, 16-beam fan, 8 spheres: n_obs 20, n_u 6); ReLU networks 64-64 and 128-128; minibatches of 256 (SB3's batch)
and 65 536 rows read through an int64 index from records of the replay ring's shape ([obs | next_obs | action | reward done
timeout], 262 144 of them).  The forms of one group alternate inside every window (one run of each form per window, each between
two stream events); the figures are minimum, median and maximum over the windows after a warm-up (scripts/sac_rate.py's method).
  q_params   env.q_backward(params=True)                      | torch: autograd.grad of sum(q * grad_q) w.r.t. the critic's parameters
  q_both     env.q_backward(params=True, grad_actions=True)   | torch: ... w.r.t. the parameters and the actions
  q_dx       env.q_backward(params=False, grad_actions=True)  | torch: ... w.r.t. the actions alone
  actor      env.sac_actor_backward                           | torch: autograd.grad of sum(cat(mu, log_std) * grad_out) w.r.t. the actor's
Both sides include their forward (the device kernels recompute the activations; torch runs nn.Sequential twins on the gathered
rows).  A case is "faster" or "slower" when the two ranges do not overlap, else "no gain shown".  q_dx against q_params of the
same run is reported too: the form without parameter gradients does strictly less.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.environ.get("DOCKAUV_PACKAGE_ROOT", ROOT))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

CONFIG, N_ENVS, RING_SLOTS = 3, 256, 262144
BATCHES = [256, 65536]
NETS = [(64, 64), (128, 128)]


def verdict(dev, ref):
    if dev["max_ms"] < ref["min_ms"]:
        return "faster"
    if ref["max_ms"] < dev["min_ms"]:
        return "slower"
    return "no gain shown"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sac", "backward_rate.json"))
    ap.add_argument("--windows", type=int, default=24)
    args = ap.parse_args()
    import torch
    import bench
    from sac_rate import alternating
    from gym_dockauv_amd.envs.torch_env import TorchDocking3d
    nn = torch.nn
    wl = bench.workload(CONFIG, N_ENVS)
    env = TorchDocking3d(wl["cfg"], num_envs=N_ENVS, scenario=wl["scenario"], device_seed=0x5EED0000, vehicles=wl["vehicles"])
    torch.manual_seed(0)
    n_obs, n_u = env.n_obs, env.n_u
    record = 2 * n_obs + n_u + 3
    ring = (torch.rand((RING_SLOTS, record), device="cuda") * 2 - 1).contiguous()
    R_obs, R_act = ring[:, :n_obs], ring[:, 2 * n_obs: 2 * n_obs + n_u]
    result = {"config": CONFIG, "n_obs": n_obs, "n_u": n_u, "ring_slots": RING_SLOTS, "windows": args.windows, "cases": {}}
    for hidden in NETS:
        class Actor(nn.Module):
            def __init__(self):
                super().__init__()
                self.latent_pi = nn.Sequential(nn.Linear(n_obs, hidden[0]), nn.ReLU(), nn.Linear(hidden[0], hidden[1]), nn.ReLU())
                self.mu, self.log_std = nn.Linear(hidden[1], n_u), nn.Linear(hidden[1], n_u)

            def forward(self, obs):
                h = self.latent_pi(obs)
                return torch.cat([self.mu(h), self.log_std(h)], dim=1)

        actor_t = Actor().cuda()
        q_t = nn.Sequential(nn.Linear(n_obs + n_u, hidden[0]), nn.ReLU(), nn.Linear(hidden[0], hidden[1]), nn.ReLU(), nn.Linear(hidden[1], 1)).cuda()
        actor, q = env.make_sac_actor(actor_t, seed=7), env.make_q(q_t)
        q_params, a_params = list(q_t.parameters()), list(actor_t.parameters())
        q_out = [torch.empty_like(p) for p in q_params]
        a_out = [torch.empty_like(p) for p in a_params]
        for B in BATCHES:
            index = torch.randint(0, RING_SLOTS, (B,), device="cuda")
            gq, ga = torch.randn(B, device="cuda"), torch.randn((B, 2 * n_u), device="cuda")

            def torch_q(params, actions):
                a = R_act[index].requires_grad_(actions)
                out = q_t(torch.cat([R_obs[index], a], dim=1))[:, 0]
                return torch.autograd.grad((out * gq).sum(), (q_params if params else []) + ([a] if actions else []))

            forms = {
                "device_q_params": lambda: env.q_backward(q, R_obs, R_act, gq, index, params=True, out=q_out),
                "device_q_both": lambda: env.q_backward(q, R_obs, R_act, gq, index, params=True, grad_actions=True, out=q_out),
                "device_q_dx": lambda: env.q_backward(q, R_obs, R_act, gq, index, params=False, grad_actions=True),
                "device_actor": lambda: env.sac_actor_backward(actor, R_obs, ga, index, out=a_out),
                "torch_q_params": lambda: torch_q(True, False),
                "torch_q_both": lambda: torch_q(True, True),
                "torch_q_dx": lambda: torch_q(False, True),
                "torch_actor": lambda: torch.autograd.grad((actor_t(R_obs[index]) * ga).sum(), a_params),
            }
            r = alternating(forms, args.windows, 3)
            r["notes"] = {k: verdict(r[f"device_{k}"], r[f"torch_{k}"]) for k in ("q_params", "q_both", "q_dx", "actor")}
            r["notes"]["q_dx_vs_q_params"] = ("costs more: a finding" if r["device_q_dx"]["min_ms"] > r["device_q_params"]["max_ms"]
                                              else "does not cost more")
            result["cases"][f"{hidden[0]}-{hidden[1]}_B{B}"] = r
    env.close()
    print(json.dumps(result, indent=1))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
