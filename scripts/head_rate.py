#!/usr/bin/env python3
"""One PPO minibatch step up to (not including) opt.step() on the buffers of one collection: the loop body of INTEGRATION.md
section 6 in torch against TorchDocking3d.ppo_minibatch, and the PPO head alone against the same head in torch, on the same box,
in the same process, on the same rows.  Writes profiles/update/head_rate.json.

  python scripts/head_rate.py [--out profiles/update/head_rate.json]

Config 3 (BlueROV2, 16-beam fan, 65 536 envs), a 64-64 tanh actor and a 64-64 tanh critic, the rows of one dockauv_collect of
K = 128 steps; minibatches of 65 536 and of 1 048 576 rows through a random index.  Four paths:
  (a) step_torch:   mlp_apply of the actor and of the critic, the head in torch (Normal, min, clamp, std), loss.backward();
  (b) step_library: ppo_minibatch (weight load, the two forward kernels, dockauv_ppo_head, the two backward kernels);
  head_library:     TorchDocking3d.ppo_head on the outputs of the two forwards;
  head_torch:       the same head in torch with autograd down to mean, v and log_std (mean and v are leaves).
Each path is timed between two stream events per window of `--per-window` passes; recorded are the median, the minimum and the
maximum over 24 windows after a warm-up, in milliseconds per pass.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_ENVS, K = 65536, 128
SIZES = (65536, 1 << 20)
CLIP, VF, ENT = 0.2, 0.5, 0.01


def timed(run, windows, warmup, per_window):
    import torch
    for _ in range(warmup):
        run()
    torch.cuda.synchronize()
    ms = []
    for _ in range(windows):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(per_window):
            run()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1) / per_window)
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "windows": len(ms), "passes_per_window": per_window}


def torch_head(torch, mean, v, log_std, actions, logp_old, adv, ret):
    dist = torch.distributions.Normal(mean, log_std.exp())
    ratio = (dist.log_prob(actions).sum(-1) - logp_old).exp()
    a = (adv - adv.mean()) / (adv.std() + 1e-8)
    return -torch.min(ratio * a, ratio.clamp(1 - CLIP, 1 + CLIP) * a).mean() + VF * ((ret - v) ** 2).mean() \
        - ENT * dist.entropy().sum(-1).mean()


def measure(windows, warmup, per_window):
    import torch
    import bench
    from gym_dockauv_amd.envs.torch_env import TorchDocking3d
    from gym_dockauv_amd.policy import MLPPolicy
    wl = bench.workload(3, N_ENVS)
    env = TorchDocking3d(wl["cfg"], num_envs=N_ENVS, scenario=wl["scenario"], device_seed=0x5EED0000, vehicles=wl["vehicles"])
    res = {"config": 3, "envs": N_ENVS, "steps": K}
    try:
        env.batch._gen = np.random.default_rng(1)
        env.reset()
        torch.manual_seed(0)
        n_obs, n_u = env.n_obs, env.n_u
        net = lambda n_out: torch.nn.Sequential(torch.nn.Linear(n_obs, 64), torch.nn.Tanh(), torch.nn.Linear(64, 64), torch.nn.Tanh(),
                                                torch.nn.Linear(64, n_out)).cuda()
        actor, critic = net(n_u), net(1)
        log_std = torch.full((n_u,), -0.5, device="cuda", requires_grad=True)
        policy = env.make_policy(MLPPolicy.from_torch(actor, log_std=log_std.detach().cpu().numpy()), seed=7)
        value = env.make_value(MLPPolicy.value_from_torch(critic))
        env.load_policy(policy, actor, log_std=log_std)
        c = env.collect(policy, value, K, gamma=0.99, gae_lambda=0.95)
        torch.cuda.synchronize()
        rows = c.obs[:K]
        flat = lambda t: t.reshape(K * N_ENVS, *t.shape[2:])
        actions, logp_old, adv, ret = flat(c.actions), flat(c.log_prob), flat(c.advantages), flat(c.returns)
        # the learner has moved on from the collecting weights, so that ratios spread and some rows are clipped
        with torch.no_grad():
            for p in list(actor.parameters()) + list(critic.parameters()):
                p.add_(0.02 * torch.randn_like(p))
        a_params, c_params = list(actor.parameters()), list(critic.parameters())
        params = a_params + c_params + [log_std]
        res.update(n_obs=n_obs, n_u=n_u, actor=f"{n_obs}-64-64-{n_u} tanh", critic=f"{n_obs}-64-64-1 tanh", rows=K * N_ENVS)
        gen = torch.Generator(device="cuda")
        gen.manual_seed(3)
        perm = torch.randperm(K * N_ENVS, device="cuda", generator=gen)
        for B in SIZES:
            idx = perm[:B].contiguous()

            def step_torch():
                for p in params:
                    p.grad = None
                mean = env.mlp_apply(policy, a_params, rows, idx)
                v = env.mlp_apply(value, c_params, rows, idx)[:, 0]
                loss = torch_head(torch, mean, v, log_std, actions[idx], logp_old[idx], adv[idx], ret[idx])
                loss.backward()
                return loss

            def step_library():
                return env.ppo_minibatch(policy, value, a_params, log_std, c_params, actions, logp_old, adv, ret, rows, idx,
                                         clip_range=CLIP, vf_coef=VF, ent_coef=ENT)

            # the two forms agree (float32, other summation orders)
            loss_t = step_torch()
            grads_t = [p.grad.clone() for p in params]
            stats = step_library()
            torch.cuda.synchronize()
            diff = max(float((p.grad - g).abs().max() / g.abs().max().clamp_min(1e-30)) for p, g in zip(params, grads_t))
            mean = env.mlp_forward(policy, rows, idx)
            v = env.mlp_forward(value, rows, idx).view(-1)

            def head_library():
                return env.ppo_head(policy, mean, v, actions, logp_old, adv, ret, idx, clip_range=CLIP, vf_coef=VF, ent_coef=ENT)

            mean_l, v_l = mean.clone().requires_grad_(), v.clone().requires_grad_()

            def head_torch():
                mean_l.grad = v_l.grad = log_std.grad = None
                loss = torch_head(torch, mean_l, v_l, log_std, actions[idx], logp_old[idx], adv[idx], ret[idx])
                loss.backward()
                return loss

            entry = {"rows": B, "loss_torch": float(loss_t), "loss_library": float(stats[0]), "clip_fraction": float(stats[5]),
                     "max_relative_gradient_difference": diff}
            for name, fn in (("step_torch", step_torch), ("step_library", step_library), ("head_torch", head_torch),
                             ("head_library", head_library)):
                entry[name] = timed(fn, windows, warmup, per_window)
            entry["step_torch_over_library_median"] = entry["step_torch"]["median_ms"] / entry["step_library"]["median_ms"]
            entry["head_torch_over_library_median"] = entry["head_torch"]["median_ms"] / entry["head_library"]["median_ms"]
            print(f"{B} rows: step torch {entry['step_torch']['median_ms']:.3f} ms, library {entry['step_library']['median_ms']:.3f} ms; "
                  f"head torch {entry['head_torch']['median_ms']:.3f} ms, library {entry['head_library']['median_ms']:.3f} ms; gradient "
                  f"difference {diff:.2e}, clip fraction {entry['clip_fraction']:.3f}", file=sys.stderr, flush=True)
            res[f"minibatch_{B}_indexed"] = entry
            for p in params:
                p.grad = None
            del mean, v, mean_l, v_l, grads_t
            torch.cuda.empty_cache()
    finally:
        env.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "update", "head_rate.json"))
    ap.add_argument("--windows", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--per-window", type=int, default=8)
    args = ap.parse_args()
    import torch
    doc = {"what": "one PPO minibatch step without opt.step() on the rows of one dockauv_collect (config 3, K = 128, 64-64 tanh actor "
                   "and critic), milliseconds per pass: the section-6 body in torch (mlp_apply twice, the head in torch, "
                   "loss.backward()) against TorchDocking3d.ppo_minibatch, and the head alone (TorchDocking3d.ppo_head against the "
                   "torch head with autograd to mean, v and log_std); median, min and max over windows between stream events, "
                   "one process",
           "device": torch.cuda.get_device_name(0), "results": [measure(args.windows, args.warmup, args.per_window)]}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(doc, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
