#!/usr/bin/env python3
"""Closed loop with a real actor in it: per-step cost of three ways to run (policy, step) on one GPU, same process, same box.

  python scripts/closed_loop.py [--out profiles/policy/closed_loop.json]
  python scripts/closed_loop.py --rollout-only --config 3        # form (c) alone: the run to put under a kernel trace
  python scripts/closed_loop.py --merge-kernel-stats <kernel_stats.csv> --config 3 [--out ...]

Config 3 (BlueROV2, 16-beam fan, 8 spheres) at 65 536 envs and config 4 (LAUV, 63 rays, 5 capsules) at 32 768, the same
64-64 tanh actor (SB3's MlpPolicy default, train.py:64) everywhere:
  (a) the actor as torch ops + step_device, issued from Python;
  (b) the same 50 steps captured once as a linear HIP graph and replayed (what bench.py: closed_loop_rate does with its
      trivial policy);
  (c) dockauv_rollout: one host call per 50 steps.
Each form runs 50-step windows bracketed by stream events; the figure is the median over the windows after a warm-up.
--merge-kernel-stats adds the average kernel durations of a `rocprofv3 --kernel-trace --stats` run of form (c) (a run of its
own, without counters) to the JSON, the policy kernel's beside its arithmetic floor.
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
K = 50
F32_PEAK_TFLOPS = 157.3   # MI355X exact-f32 matrix / packed-FMA peak


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
    net = torch.nn.Sequential(torch.nn.Linear(n_obs, 64), torch.nn.Tanh(), torch.nn.Linear(64, 64), torch.nn.Tanh(),
                              torch.nn.Linear(64, n_u)).cuda().requires_grad_(False)
    return env, net, env.make_policy(MLPPolicy.from_torch(net))


def windows(run, n_windows, warmup):
    """median / min / max microseconds per step over `n_windows` windows of K steps, each between two stream events"""
    import torch
    for _ in range(warmup):
        run()
    torch.cuda.synchronize()
    us = []
    for _ in range(n_windows):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run()
        e1.record()
        e1.synchronize()
        us.append(e0.elapsed_time(e1) * 1e3 / K)
    return {"median_us_per_step": statistics.median(us), "min_us_per_step": min(us), "max_us_per_step": max(us), "windows": len(us)}


def measure(config_id, n_envs, n_windows, warmup, rollout_only=False):
    import torch
    env, net, pol = make(config_id, n_envs)
    n_obs, n_u, N = env.n_observations, env.n_u, n_envs
    res = {"config": config_id, "envs": N, "n_obs": n_obs, "n_u": n_u, "actor": f"{n_obs}-64-64-{n_u} tanh", "steps_per_window": K}
    try:
        out = torch.zeros((N, n_obs + 2), device="cuda")
        rows = torch.zeros((K, N, n_obs + 2), device="cuda")
        acts = torch.zeros((K, N, n_u), device="cuda")

        def rollout():
            env.rollout_device(pol, rows[K - 1].data_ptr(), rows.data_ptr(), acts.data_ptr(), K,
                               stream=torch.cuda.current_stream().cuda_stream)
        if not rollout_only:
            def loop():
                stream = torch.cuda.current_stream().cuda_stream
                for _ in range(K):
                    a = net(out[:, :n_obs])
                    env.step_device(a.data_ptr(), out.data_ptr(), stream=stream, packed=True)
                return a
            res["a_torch_python_issued"] = windows(loop, n_windows, warmup)
            try:
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    keep = loop()
                res["b_torch_hip_graph"] = windows(g.replay, n_windows, warmup)
                del keep, g
            except Exception as ex:   # (capture is the caller's optimisation; the record says when it was not available)
                res["b_torch_hip_graph"] = {"median_us_per_step": None, "note": f"capture failed: {type(ex).__name__}: {ex}"[:200]}
                torch.cuda.synchronize()
        res["c_dockauv_rollout"] = windows(rollout, n_windows, warmup)
        env.synchronize()
        if not rollout_only:
            c = res["c_dockauv_rollout"]["median_us_per_step"]
            others = [res[k]["median_us_per_step"] for k in ("a_torch_python_issued", "b_torch_hip_graph")]
            res["rollout_faster_than_both"] = all(v is not None and c < v for v in others)
    finally:
        env.close()
    return res


def merge_kernel_stats(doc, path, config_id):
    """average durations of the policy and step kernels from a rocprofv3 kernel_stats.csv of form (c)"""
    entry = next(e for e in doc["results"] if e["config"] == config_id)
    ks = {}
    for r in csv.DictReader(open(path)):
        for key, needle in (("policy_mlp_kernel", "policy_mlp_kernel"), ("step_kernel", "dockauv::step_kernel")):
            if needle in r["Name"]:
                ks[key] = {"calls": int(r["Calls"]), "average_us": float(r["AverageNs"]) / 1e3, "min_us": float(r["MinNs"]) / 1e3,
                           "max_us": float(r["MaxNs"]) / 1e3}
    flop = 2.0 * (entry["n_obs"] * 64 + 64 * 64 + 64 * entry["n_u"]) * entry["envs"]
    floor = flop / (F32_PEAK_TFLOPS * 1e12) * 1e6
    if "policy_mlp_kernel" in ks:
        ks["policy_mlp_kernel"].update(gflop_per_step=flop / 1e9, floor_us_at_157_tflops=floor,
                                       ratio_to_floor=ks["policy_mlp_kernel"]["average_us"] / floor)
    entry["kernel_trace"] = dict(ks, source="rocprofv3 --kernel-trace --stats on form (c) alone")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "policy", "closed_loop.json"))
    ap.add_argument("--config", type=int, default=0)
    ap.add_argument("--windows", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--rollout-only", action="store_true")
    ap.add_argument("--merge-kernel-stats", default="")
    args = ap.parse_args()
    if args.merge_kernel_stats:
        doc = json.load(open(args.out))
        merge_kernel_stats(doc, args.merge_kernel_stats, args.config or 3)
        json.dump(doc, open(args.out, "w"), indent=1)
        return
    import torch
    ids = [args.config] if args.config else sorted(CONFIGS)
    results = [measure(c, CONFIGS[c], args.windows, args.warmup, args.rollout_only) for c in ids]
    if args.rollout_only:
        print(json.dumps(results))
        return
    doc = {"what": "closed loop, microseconds per step: torch actor issued from Python (a), the same as a replayed HIP graph (b), "
                   "dockauv_rollout (c); median of 50-step windows between stream events, one process",
           "device": torch.cuda.get_device_name(0), "results": results}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    json.dump(doc, open(args.out, "w"), indent=1)
    for r in results:
        print(f"config {r['config']} ({r['envs']} envs): " + ", ".join(
            f"{k[0]} {r[k]['median_us_per_step']}" for k in ("a_torch_python_issued", "b_torch_hip_graph", "c_dockauv_rollout")),
            file=sys.stderr)


if __name__ == "__main__":
    main()
