#!/usr/bin/env python3
"""What SAC's loss head costs on the device and in torch eager doing the same algebra on the same tensors.  One GPU, one process,
same box.

  python scripts/sac_head_rate.py [--out profiles/sac/sac_head_rate.json] [--windows 24]

Config 3 (BlueROV2, 16-beam fan, 8 spheres: n_obs 20, n_u 6); ReLU networks 64-64; dense minibatches of 256 (SB3's batch) and
2 048 rows.  The forms of one group alternate inside every window (one run of each form per window, each between two stream
events); the figures are minimum, median and maximum over the windows after a warm-up (scripts/sac_rate.py's method).
  sample       env.sac_sample              | torch: clamp, exp, randn, tanh, Normal.log_prob and the squashing correction, from heads
  critic_head  env.sac_critic_head         | torch: the two differences, their squares' means, the three means, the two gradients
  actor_head   env.sac_actor_head          | torch: the same closed-form gradient on heads and the four statistics, elementwise
  ent_coef     env.ent_coef_step           | torch: the loss on a scalar leaf, backward, torch.optim.Adam.step
  gradients    env.sac_gradients (20 launches) | torch: SB3 1.5's target, critic loss and actor loss on nn.Module twins, autograd.grad
A case is "faster" or "slower" when the two ranges do not overlap, else "no gain shown".  No threshold is asserted.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.environ.get("DOCKAUV_PACKAGE_ROOT", ROOT))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

CONFIG, N_ENVS = 3, 256
BATCHES = [256, 2048]
HIDDEN = (64, 64)
NAMES = ("sample", "critic_head", "actor_head", "ent_coef", "gradients")


def verdict(dev, ref):
    if dev["max_ms"] < ref["min_ms"]:
        return "faster"
    if ref["max_ms"] < dev["min_ms"]:
        return "slower"
    return "no gain shown"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sac", "sac_head_rate.json"))
    ap.add_argument("--windows", type=int, default=24)
    args = ap.parse_args()
    import torch
    import bench
    from sac_rate import alternating
    from gym_dockauv_amd.envs.torch_env import TorchDocking3d
    from gym_dockauv_amd.replay import ReplaySamples
    nn, F = torch.nn, torch.nn.functional
    wl = bench.workload(CONFIG, N_ENVS)
    env = TorchDocking3d(wl["cfg"], num_envs=N_ENVS, scenario=wl["scenario"], device_seed=0x5EED0000, vehicles=wl["vehicles"])
    torch.manual_seed(0)
    n_obs, n_u = env.n_obs, env.n_u

    class Actor(nn.Module):
        def __init__(self):
            super().__init__()
            self.latent_pi = nn.Sequential(nn.Linear(n_obs, HIDDEN[0]), nn.ReLU(), nn.Linear(HIDDEN[0], HIDDEN[1]), nn.ReLU())
            self.mu, self.log_std = nn.Linear(HIDDEN[1], n_u), nn.Linear(HIDDEN[1], n_u)

        def forward(self, obs):
            h = self.latent_pi(obs)
            return torch.cat([self.mu(h), self.log_std(h)], dim=1)

    def q_net():
        return nn.Sequential(nn.Linear(n_obs + n_u, HIDDEN[0]), nn.ReLU(), nn.Linear(HIDDEN[0], HIDDEN[1]), nn.ReLU(), nn.Linear(HIDDEN[1], 1)).cuda()

    actor_t, qs_t, qts_t = Actor().cuda(), [q_net(), q_net()], [q_net().requires_grad_(False), q_net().requires_grad_(False)]
    actor = env.make_sac_actor(actor_t, seed=7)
    q1, q2, q1t, q2t = (env.make_q(m) for m in qs_t + qts_t)
    a_params, q_params = list(actor_t.parameters()), [p for m in qs_t for p in m.parameters()]
    gamma, alpha, target_entropy = 0.99, 0.2, -float(n_u)

    def sample_t(heads):
        mu, ls = heads[:, :n_u], heads[:, n_u:].clamp(-20.0, 2.0)
        std = ls.exp()
        x = mu + std * torch.randn_like(mu)
        a = torch.tanh(x)
        return a, torch.distributions.Normal(mu, std).log_prob(x).sum(dim=1) - torch.log(1.0 - a ** 2 + 1e-6).sum(dim=1)

    result = {"config": CONFIG, "n_obs": n_obs, "n_u": n_u, "hidden": list(HIDDEN), "windows": args.windows, "cases": {}}
    for B in BATCHES:
        sm = ReplaySamples((torch.rand((B, n_obs), device="cuda") * 2 - 1).contiguous(), (torch.rand((B, n_u), device="cuda") * 2 - 1).contiguous(),
                           (torch.rand((B, n_obs), device="cuda") * 2 - 1).contiguous(), (torch.rand((B, 1), device="cuda") < 0.1).float(),
                           torch.randn((B, 1), device="cuda"))
        heads = env.sac_actor_heads(actor, sm.observations)
        qa, qb, y = torch.randn(B, device="cuda"), torch.randn(B, device="cuda"), torch.randn(B, device="cuda")
        dq1, dq2 = torch.randn((B, n_u), device="cuda"), torch.randn((B, n_u), device="cuda")
        z = torch.randn((B, n_u), device="cuda")
        _, logp = env.sac_sample(actor, heads, 1)
        state = env.ent_coef_state(1.0)
        log_alpha = torch.zeros(1, device="cuda", requires_grad=True)
        adam = torch.optim.Adam([log_alpha], lr=3e-4)
        step = [0]

        def critic_head_t():
            d1, d2 = qa - y, qb - y
            m1, m2 = (d1 * d1).mean(), (d2 * d2).mean()
            return d1 / B, d2 / B, torch.stack([0.5 * (m1 + m2), m1, m2, qa.mean(), qb.mean(), y.mean()])

        def actor_head_t():
            mu, raw = heads[:, :n_u], heads[:, n_u:]
            ls = raw.clamp(-20.0, 2.0)
            std = ls.exp()
            x = mu + std * z
            a = torch.tanh(x)
            s = 1.0 - a * a
            logp_ = (-0.5 * z * z - ls - 0.918938533).sum(dim=1) - torch.log(s + 1e-6).sum(dim=1)
            w = 2.0 * a * s / (s + 1e-6)
            sel = torch.where((qa <= qb)[:, None], dq1, dq2)
            gx = (alpha * w - sel * s) / B
            g_ls = torch.where((raw >= -20.0) & (raw <= 2.0), gx * std * z - alpha / B, torch.zeros_like(gx))
            mq = torch.minimum(qa, qb)
            return torch.cat([gx, g_ls], dim=1), torch.stack([(alpha * logp_ - mq).mean(), logp_.mean(), mq.mean(), torch.tensor(alpha, device="cuda")])

        def ent_coef_d():
            step[0] += 1
            return env.ent_coef_step(state, logp, step[0], 3e-4)

        def ent_coef_t():
            adam.zero_grad()
            (-(log_alpha * (logp + target_entropy).detach()).mean()).backward()
            adam.step()

        def gradients_t():
            with torch.no_grad():
                a2, logp2 = sample_t(actor_t(sm.next_observations))
                xn = torch.cat([sm.next_observations, a2], dim=1)
                nq = torch.min(qts_t[0](xn), qts_t[1](xn)) - alpha * logp2[:, None]
                yy = sm.rewards + (1.0 - sm.dones) * gamma * nq
            xo = torch.cat([sm.observations, sm.actions], dim=1)
            critic_loss = 0.5 * sum(F.mse_loss(q(xo), yy) for q in qs_t)
            gq = torch.autograd.grad(critic_loss, q_params)
            a, lp = sample_t(actor_t(sm.observations))
            xa = torch.cat([sm.observations, a], dim=1)
            actor_loss = (alpha * lp - torch.min(qs_t[0](xa), qs_t[1](xa))[:, 0]).mean()
            return gq, torch.autograd.grad(actor_loss, a_params), lp

        t = [0]

        def gradients_d():
            t[0] += 1
            return env.sac_gradients(actor, q1, q2, q1t, q2t, sm, gamma, t[0], ent_coef=alpha)

        forms = {
            "device_sample": lambda: env.sac_sample(actor, heads, 3),
            "device_critic_head": lambda: env.sac_critic_head(q1, qa, qb, y),
            "device_actor_head": lambda: env.sac_actor_head(actor, heads, 3, qa, qb, dq1, dq2, ent_coef=alpha),
            "device_ent_coef": ent_coef_d,
            "device_gradients": gradients_d,
            "torch_sample": lambda: sample_t(heads),
            "torch_critic_head": critic_head_t,
            "torch_actor_head": actor_head_t,
            "torch_ent_coef": ent_coef_t,
            "torch_gradients": gradients_t,
        }
        r = alternating(forms, args.windows, 3)
        r["notes"] = {k: verdict(r[f"device_{k}"], r[f"torch_{k}"]) for k in NAMES}
        result["cases"][f"B{B}"] = r
    env.close()
    print(json.dumps({c: {k: (v["median_ms"] if isinstance(v, dict) and "median_ms" in v else v) for k, v in r.items()}
                      for c, r in result["cases"].items()}, indent=1))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
