#!/usr/bin/env python3
"""One PPO iteration's collection: what the value head, the log-probabilities and GAE cost on top of the rollout, on the
device in one host call (dockauv_collect) and rebuilt in torch.  One GPU, one process, same box.

  python scripts/collect_rate.py [--out profiles/collect/collect_rate.json]
  python scripts/collect_rate.py --collect-only --config 3       # form (b) alone: the run to put under a kernel trace
  python scripts/collect_rate.py --merge-kernel-stats <kernel_stats.csv> --config 3 [--out ...]

Config 3 (BlueROV2, 16-beam fan, 8 spheres) at 65 536 envs and config 4 (LAUV, 63 rays, 5 capsules) at 32 768; a 64-64 tanh
actor with a log_std and a 64-64 tanh critic (SB3's MlpPolicy default, train.py:64); K = 128 steps per iteration, stochastic:
  (a) dockauv_rollout alone;
  (b) dockauv_collect: the same launches with the actor's log-prob epilogue, two value launches and one GAE launch;
  (c) dockauv_rollout followed by the same quantities in torch: the critic module on the [K + 1, N] observations,
      Normal.log_prob of the actions under the actor module, and the K-step GAE loop (SB3's compute_returns_and_advantage).
Each form is timed between two stream events per iteration; the figure is the median over the iterations after a warm-up.
Also recorded: the value launch over the K N rows alone.
"""
import argparse
import csv
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = {3: 65536, 4: 32768}
K = 128
GAMMA, GAE_LAMBDA = 0.99, 0.95


def make(config_id, n_envs):
    import torch
    import bench
    from gym_dockauv_amd.envs.batched import BatchedDocking3d
    from gym_dockauv_amd.policy import MLPPolicy
    wl = bench.workload(config_id, n_envs)
    env = BatchedDocking3d(wl["cfg"], num_envs=n_envs, scenario=wl["scenario"], device=0, precision="f32", reset_mode="device",
                           device_seed=0x5EED0000, rng="batched", vehicles=wl["vehicles"])
    env._gen = np.random.default_rng(1)
    env.reset()
    torch.manual_seed(0)
    n_obs, n_u = env.n_observations, env.n_u
    mlp = lambda n_out: torch.nn.Sequential(torch.nn.Linear(n_obs, 64), torch.nn.Tanh(), torch.nn.Linear(64, 64), torch.nn.Tanh(),
                                            torch.nn.Linear(64, n_out)).cuda().requires_grad_(False)
    actor, critic = mlp(n_u), mlp(1)
    log_std = torch.full((n_u,), -0.5, device="cuda")
    pol = env.make_policy(MLPPolicy.from_torch(actor, log_std=log_std.cpu().numpy()), seed=7)
    val = env.make_value(MLPPolicy.value_from_torch(critic))
    return env, actor, critic, log_std, pol, val


def timed(run, iters, warmup):
    """median / min / max milliseconds of `run` over `iters` iterations, each between two stream events"""
    import torch
    for _ in range(warmup):
        run()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "iterations": len(ms)}


def measure(config_id, n_envs, iters, warmup, collect_only=False):
    import torch
    env, actor, critic, log_std, pol, val = make(config_id, n_envs)
    n_obs, n_u, N = env.n_observations, env.n_u, n_envs
    res = {"config": config_id, "envs": N, "n_obs": n_obs, "n_u": n_u, "actor": f"{n_obs}-64-64-{n_u} tanh",
           "critic": f"{n_obs}-64-64-1 tanh", "steps_per_iteration": K, "gamma": GAMMA, "gae_lambda": GAE_LAMBDA}
    try:
        z = lambda *shape: torch.zeros(shape, device="cuda")
        rows = z(K + 1, N, n_obs + 2)          # rows[0]: what the actor reads at step 0
        acts, logp, values, adv, ret = z(K, N, n_u), z(K, N), z(K + 1, N), z(K, N), z(K, N)
        stream = lambda: torch.cuda.current_stream().cuda_stream

        def rollout():
            rows[0].copy_(rows[K])
            env.rollout_device(pol, rows[0].data_ptr(), rows[1].data_ptr(), acts.data_ptr(), K, stochastic=True, stream=stream())

        def collect():
            rows[0].copy_(rows[K])
            env.collect_device(pol, val, rows[0].data_ptr(), rows[1].data_ptr(), acts.data_ptr(), K, gamma=GAMMA, gae_lambda=GAE_LAMBDA,
                               stochastic=True, stream=stream(), log_prob_ptr=logp.data_ptr(), values_ptr=values.data_ptr(),
                               advantages_ptr=adv.data_ptr(), returns_ptr=ret.data_ptr())

        def value_pass():
            env.value_forward_device(val, rows[1].data_ptr(), K * N, values[1].data_ptr(), stream=stream())

        def rollout_then_torch():
            rollout()
            obs = rows[:, :, :n_obs]
            v = critic(obs).squeeze(-1)
            lp = torch.distributions.Normal(actor(obs[:K]), log_std.exp()).log_prob(acts).sum(-1)
            reward, nt = rows[1:, :, n_obs], 1.0 - rows[1:, :, n_obs + 1]
            a, gae = torch.empty_like(reward), torch.zeros_like(reward[0])
            for k in reversed(range(K)):
                delta = reward[k] + GAMMA * v[k + 1] * nt[k] - v[k]
                gae = delta + GAMMA * GAE_LAMBDA * nt[k] * gae
                a[k] = gae
            return lp, a, a + v[:K]

        if collect_only:
            res["b_dockauv_collect"] = timed(collect, iters, warmup)
            return res
        res["a_dockauv_rollout"] = timed(rollout, iters, warmup)
        res["b_dockauv_collect"] = timed(collect, iters, warmup)
        res["value_launch_KN_rows"] = timed(value_pass, iters, warmup)
        res["c_dockauv_rollout_then_torch"] = timed(rollout_then_torch, iters, warmup)
        env.synchronize()
        a, b, c = (res[k]["median_ms"] for k in ("a_dockauv_rollout", "b_dockauv_collect", "c_dockauv_rollout_then_torch"))
        res["collector_extra_ms"] = {"b_minus_a": b - a, "c_minus_a": c - a}
    finally:
        env.close()
    return res


def merge_kernel_stats(doc, path, config_id):
    """calls and durations per kernel from a rocprofv3 kernel_stats.csv of form (b)"""
    entry = next(e for e in doc["results"] if e["config"] == config_id)
    ks = {}
    for r in csv.DictReader(open(path)):
        for key in ("policy_mlp_kernel", "policy_logp_kernel", "gae_kernel", "step_kernel"):
            if key in r["Name"]:
                ks[key] = {"calls": int(r["Calls"]), "average_us": float(r["AverageNs"]) / 1e3, "min_us": float(r["MinNs"]) / 1e3,
                           "max_us": float(r["MaxNs"]) / 1e3}
    entry["kernel_trace"] = dict(ks, source="rocprofv3 --kernel-trace --stats on form (b) alone")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "collect", "collect_rate.json"))
    ap.add_argument("--config", type=int, default=0)
    ap.add_argument("--iterations", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--collect-only", action="store_true")
    ap.add_argument("--merge-kernel-stats", default="")
    args = ap.parse_args()
    if args.merge_kernel_stats:
        doc = json.load(open(args.out))
        merge_kernel_stats(doc, args.merge_kernel_stats, args.config or 3)
        json.dump(doc, open(args.out, "w"), indent=1)
        return
    import torch
    ids = [args.config] if args.config else sorted(CONFIGS)
    results = [measure(c, CONFIGS[c], args.iterations, args.warmup, args.collect_only) for c in ids]
    if args.collect_only:
        print(json.dumps(results))
        return
    doc = {"what": "one PPO iteration's collection, milliseconds per iteration of K = 128 steps: dockauv_rollout (a), dockauv_collect "
                   "(b), dockauv_rollout then critic / Normal.log_prob / GAE loop in torch (c); median of iterations between stream "
                   "events, one process", "device": torch.cuda.get_device_name(0), "results": results}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    json.dump(doc, open(args.out, "w"), indent=1)
    for r in results:
        print(f"config {r['config']} ({r['envs']} envs): a {r['a_dockauv_rollout']['median_ms']:.3f} ms, b "
              f"{r['b_dockauv_collect']['median_ms']:.3f} ms, c {r['c_dockauv_rollout_then_torch']['median_ms']:.3f} ms; value launch over K N rows "
              f"{r['value_launch_KN_rows']['median_ms']:.3f} ms",
              file=sys.stderr)


if __name__ == "__main__":
    main()
