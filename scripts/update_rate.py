#!/usr/bin/env python3
"""One epoch of the PPO update queued by one host call (TorchDocking3d.ppo_train: dockauv_ppo_update) against the Python loop of
the same pieces (TorchDocking3d.ppo_update), on the buffers of one collection, on the same box, in the same process.  Writes
profiles/update/update_rate.json.

  python scripts/update_rate.py [--out profiles/update/update_rate.json]

Config 3 (BlueROV2, 16-beam fan, 65 536 envs), a 64-64 tanh actor and a 64-64 tanh critic, the rows of one dockauv_collect of
K = 128 steps (scripts/optim_rate.py: the same set-up); minibatches of 65 536 and of 1 048 576 rows.
  one_call:  ppo_train(opt, collected, 1, B, lr): the permutation kernel, then per minibatch the two forwards, the head, the two
             backwards and the optimiser with its repack, on the optimiser's own scratch;
  loop:      ppo_update(opt, collected, 1, B, lr): torch.randperm, then per minibatch the same launches issued from Python, with a
             fresh torch tensor for every output.
A window is one epoch over the collection (its permutation inside the window), between two stream events, divided by the number
of minibatches.  The two forms ALTERNATE window by window, so that clock and temperature drift hit both alike.  Recorded are the
median, the minimum and the maximum over 24 windows each after a warm-up epoch each, in milliseconds per minibatch.
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
LR, MAX_NORM = 3e-5, 0.5


def window(run, n_mb):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    run()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / n_mb


def summary(ms, n_mb):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "windows": len(ms), "passes_per_window": n_mb}


def measure(windows):
    import torch
    import bench
    from gym_dockauv_amd.envs.torch_env import TorchDocking3d
    from gym_dockauv_amd.policy import MLPPolicy
    wl = bench.workload(3, N_ENVS)
    env = TorchDocking3d(wl["cfg"], num_envs=N_ENVS, scenario=wl["scenario"], device_seed=0x5EED0000, vehicles=wl["vehicles"])
    res = {"config": 3, "envs": N_ENVS, "steps": K, "lr": LR, "max_grad_norm": MAX_NORM}
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
        M = K * N_ENVS
        with torch.no_grad():
            for p in list(actor.parameters()) + list(critic.parameters()):
                p.add_(0.02 * torch.randn_like(p))
        a_params, c_params = list(actor.parameters()), list(critic.parameters())
        params = a_params + [log_std] + c_params
        start = [p.detach().clone() for p in params]
        res.update(n_obs=n_obs, n_u=n_u, actor=f"{n_obs}-64-64-{n_u} tanh", critic=f"{n_obs}-64-64-1 tanh", rows=M)
        kw = dict(clip_range=CLIP, vf_coef=VF, ent_coef=ENT)
        gen = torch.Generator(device="cuda")
        gen.manual_seed(3)
        opt = env.make_optimizer(policy, value, a_params, log_std, c_params, max_grad_norm=MAX_NORM)
        epoch = [0]

        def one_call(B):
            epoch[0] += 1
            return env.ppo_train(opt, c, 1, B, LR, seed=3, first_epoch=epoch[0], **kw)

        def loop(B):
            return env.ppo_update(opt, c, 1, B, LR, generator=gen, **kw)

        for B in SIZES:
            n_mb = (M + B - 1) // B
            entry = {"rows": B, "minibatches_per_epoch": n_mb}
            with torch.no_grad():
                for p, s in zip(params, start):
                    p.copy_(s)
            first = one_call(B)          # (warm-up, and the first call's allocations)
            loop(B)
            torch.cuda.synchronize()
            entry["first_minibatch"] = {"loss": float(first[0, 0, 0]), "clip_fraction": float(first[0, 0, 5]),
                                        "grad_norm": float(first[0, 0, 8]), "coef": float(first[0, 0, 9])}
            ms = {"one_call": [], "loop": []}
            for _ in range(windows):
                ms["one_call"].append(window(lambda: one_call(B), n_mb))
                ms["loop"].append(window(lambda: loop(B), n_mb))
            entry["one_call"], entry["loop"] = summary(ms["one_call"], n_mb), summary(ms["loop"], n_mb)
            entry["one_call_min_above_loop_max"] = bool(entry["one_call"]["min_ms"] > entry["loop"]["max_ms"])
            entry["loop_min_over_one_call_min"] = entry["loop"]["min_ms"] / entry["one_call"]["min_ms"]
            print(f"{B} rows: one call {entry['one_call']['min_ms']:.4f} .. {entry['one_call']['max_ms']:.4f} ms a minibatch "
                  f"(median {entry['one_call']['median_ms']:.4f}); loop {entry['loop']['min_ms']:.4f} .. {entry['loop']['max_ms']:.4f} "
                  f"(median {entry['loop']['median_ms']:.4f})", file=sys.stderr, flush=True)
            res[f"minibatch_{B}"] = entry
            torch.cuda.empty_cache()
    finally:
        env.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "update", "update_rate.json"))
    ap.add_argument("--windows", type=int, default=24)
    args = ap.parse_args()
    import torch
    doc = {"what": "one epoch of the PPO update on the rows of one dockauv_collect (config 3, K = 128, 64-64 tanh actor and critic), "
                   "milliseconds per minibatch: ppo_train (one dockauv_ppo_update call) against ppo_update (the Python loop of the "
                   "same launches, torch.randperm and a fresh tensor per output); a window is one epoch between two stream events "
                   "divided by its minibatches, the two forms alternate window by window; median, min and max over the windows, "
                   "one process",
           "device": torch.cuda.get_device_name(0), "results": [measure(args.windows)]}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(doc, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
