#!/usr/bin/env python3
"""What the replay buffer costs: filling it behind a rollout or a step, and drawing minibatches from it, on the device
(dockauv_replay_push / dockauv_replay_sample) and restated in torch on the same data.  One GPU, one process, same box.

  python scripts/replay_rate.py [--out profiles/replay/replay_rate.json] [--plain-only]

Config 3 (BlueROV2, 16-beam fan, 8 spheres) at 65 536 envs and config 4 (LAUV, 63 rays, 5 capsules) at 32 768; the 64-64 tanh
actor of scripts/collect_rate.py, stochastic; a ring of 128 steps.  The forms of one group alternate inside every window (one
run of each form per window, each between two stream events); the figures are minimum, median and maximum over the windows
after a warm-up.
  rollout:  rollout(K = 128) alone | rb.rollout(K = 128) | the same with a buffer made with
            handle_timeout_termination=False (no outcome scan: what the torch form does) | rollout(K = 128, want_terminal_obs)
            then the torch push
  step:     step alone | step(replay=rb) | the same without the outcome scan | step(want_terminal_obs) then the torch push
  push:     the push launch alone on a rollout's buffers | the torch push alone on the same buffers
  sample:   rb.sample(B, G) | the torch sample, at (B, G) = (256, 1), (8 192, 1), (1 048 576, 1), (8 192, 16)
The torch restatement is SB3's layout -- separate [steps, envs, ..] tensors for observations, next observations, actions,
rewards, dones --: the push is slice assignments with torch.where(done, terminal_obs, obs) for the next observations; the sample
two torch.randint and five advanced-index gathers.  It does not separate time limits from other dones (no outcome scan, no
timeout tensor): it does less than the device form with handle_timeout_termination.
--plain-only: rollout(K = 128) alone, for a run of the same script file against another checkout's package (PYTHONPATH).
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.environ.get("DOCKAUV_PACKAGE_ROOT", ROOT))

CONFIGS = {3: 65536, 4: 32768}
K = 128
SAMPLES = [(256, 1), (8192, 1), (1048576, 1), (8192, 16)]


def make(config_id, n_envs):
    import torch
    import bench
    from gym_dockauv_amd.envs.torch_env import TorchDocking3d
    from gym_dockauv_amd.policy import MLPPolicy
    wl = bench.workload(config_id, n_envs)
    env = TorchDocking3d(wl["cfg"], num_envs=n_envs, scenario=wl["scenario"], device_seed=0x5EED0000, vehicles=wl["vehicles"])
    env.batch._gen = np.random.default_rng(1)
    env.reset()
    torch.manual_seed(0)
    actor = torch.nn.Sequential(torch.nn.Linear(env.n_obs, 64), torch.nn.Tanh(), torch.nn.Linear(64, 64), torch.nn.Tanh(),
                                torch.nn.Linear(64, env.n_u)).cuda().requires_grad_(False)
    pol = env.make_policy(MLPPolicy.from_torch(actor, log_std=np.full(env.n_u, -0.5)), seed=7)
    return env, pol


def alternating(forms, windows, warmup):
    """forms: {name: callable}.  Every window runs each form once, in order, each between two stream events."""
    import torch
    for _ in range(warmup):
        for run in forms.values():
            run()
    torch.cuda.synchronize()
    ms = {name: [] for name in forms}
    for _ in range(windows):
        for name, run in forms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run()
            e1.record()
            e1.synchronize()
            ms[name].append(e0.elapsed_time(e1))
    return {name: {"min_ms": min(v), "median_ms": statistics.median(v), "max_ms": max(v), "windows": len(v)} for name, v in ms.items()}


class TorchReplay:
    """the restatement: SB3's ReplayBuffer layout on the device"""

    def __init__(self, torch, steps, N, n_obs, n_u):
        z = lambda *shape: torch.zeros(shape, device="cuda")
        self.torch, self.steps, self.N = torch, steps, N
        self.obs, self.nxt, self.act = z(steps, N, n_obs), z(steps, N, n_obs), z(steps, N, n_u)
        self.rew, self.done = z(steps, N), z(steps, N)
        self.carry = z(N, n_obs)
        self.pos, self.size = 0, 0

    def push(self, rows, acts, term, n_obs):
        torch, k = self.torch, rows.shape[0]
        assert self.pos + k <= self.steps or k == 1
        s = slice(self.pos, self.pos + k)
        o = rows[:, :, :n_obs]
        self.obs[self.pos] = self.carry
        if k > 1:
            self.obs[self.pos + 1:self.pos + k] = o[:-1]
        done = rows[:, :, n_obs + 1] > 0.5
        self.nxt[s] = torch.where(done[:, :, None], term, o)
        self.act[s], self.rew[s], self.done[s] = acts, rows[:, :, n_obs], done
        self.carry.copy_(o[-1])
        self.pos = (self.pos + k) % self.steps
        self.size = min(self.size + k, self.steps)

    def sample(self, B, G):
        torch = self.torch
        st = torch.randint(0, self.size, (G, B), device="cuda")
        en = torch.randint(0, self.N, (G, B), device="cuda")
        return self.obs[st, en], self.act[st, en], self.nxt[st, en], self.done[st, en].unsqueeze(-1), self.rew[st, en].unsqueeze(-1)


def measure(config_id, n_envs, windows, warmup, plain_only=False):
    import torch
    env, pol = make(config_id, n_envs)
    N, n_obs, n_u = env.num_envs, env.n_obs, env.n_u
    res = {"config": config_id, "envs": N, "n_obs": n_obs, "n_u": n_u, "steps_per_rollout": K, "ring_steps": K}
    try:
        if plain_only:
            res["rollout"] = alternating({"plain": lambda: env.rollout(pol, K, stochastic=True)}, windows, warmup)
            return res
        rb = env.make_replay_buffer(K * N, seed=1)
        tr = TorchReplay(torch, K, N, n_obs, n_u)
        res["record_floats"], res["ring_bytes"] = rb.record_floats, rb.storage.numel() * 4
        a1 = (torch.rand((N, n_u), device="cuda") * 2 - 1).contiguous()

        def rollout_torch():
            env.rollout(pol, K, stochastic=True, want_terminal_obs=True)
            tr.push(env._rollout_bufs[K][0], env._rollout_bufs[K][1], env.rollout_terminal_observation, n_obs)

        def step_torch():
            env.step(a1, want_terminal_obs=True)
            tr.push(env._packed[env._i % len(env._packed)].unsqueeze(0), a1.unsqueeze(0), env.terminal_observation.unsqueeze(0), n_obs)

        raw = env.make_replay_buffer(K * N, seed=1, handle_timeout_termination=False)    # like against like: no outcome scan
        res["rollout"] = alternating({"plain": lambda: env.rollout(pol, K, stochastic=True),
                                      "replay": lambda: rb.rollout(pol, K, stochastic=True),
                                      "replay_raw_dones": lambda: raw.rollout(pol, K, stochastic=True),
                                      "torch": rollout_torch}, windows, warmup)
        res["step"] = alternating({"plain": lambda: env.step(a1), "replay": lambda: env.step(a1, replay=rb),
                                   "replay_raw_dones": lambda: env.step(a1, replay=raw), "torch": step_torch}, windows, warmup)
        env.batch.destroy_replay(raw.handle)
        rb.rollout(pol, K, stochastic=True)       # the ring is full and the rollout's buffers hold K steps
        rows, acts, term = env._rollout_bufs[K]
        ep_out = torch.zeros((K, N), device="cuda", dtype=torch.uint8)
        tr.pos = 0                                            # (the restatement's push does not wrap inside a push)
        res["push"] = alternating({"device": lambda: rb.push(rows, acts, term, ep_outcome=ep_out),
                                   "torch": lambda: tr.push(rows, acts, term, n_obs)}, windows, warmup)
        assert rb.size == K and tr.size == K
        res["sample"] = {}
        for B, G in SAMPLES:
            res["sample"][f"B{B}_G{G}"] = alternating({"device": lambda: rb.sample(B, G), "torch": lambda: tr.sample(B, G)}, windows, warmup)
        torch.cuda.synchronize()
    finally:
        env.close()
    return res


def verdict(a, b):
    """the README's bar: faster only where one form's maximum lies below the other's minimum"""
    if a["max_ms"] < b["min_ms"]:
        return "first faster"
    if b["max_ms"] < a["min_ms"]:
        return "second faster"
    return "no gain shown"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "replay", "replay_rate.json"))
    ap.add_argument("--windows", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--plain-only", action="store_true")
    args = ap.parse_args()
    import torch
    results = [measure(c, CONFIGS[c], args.windows, args.warmup, args.plain_only) for c in sorted(CONFIGS)]
    if not args.plain_only:
        for r in results:
            r["verdicts"] = {"rollout: replay against torch": verdict(r["rollout"]["replay"], r["rollout"]["torch"]),
                             "rollout: replay_raw_dones against torch": verdict(r["rollout"]["replay_raw_dones"], r["rollout"]["torch"]),
                             "step: replay against torch": verdict(r["step"]["replay"], r["step"]["torch"]),
                             "step: replay_raw_dones against torch": verdict(r["step"]["replay_raw_dones"], r["step"]["torch"]),
                             "push: device against torch": verdict(r["push"]["device"], r["push"]["torch"]),
                             **{f"sample {k}: device against torch": verdict(v["device"], v["torch"]) for k, v in r["sample"].items()}}
    doc = {"what": "the replay buffer, milliseconds per call: rollout(K = 128) / step alone, through the buffer (rb.rollout, step(replay=rb)), and with the torch "
                   "restatement of the push behind it; the push alone; sample(B, G) against two torch.randint and five gathers from "
                   "SB3's layout; the forms of a group alternate inside each window between stream events, one process",
           "device": torch.cuda.get_device_name(0), "package": "another checkout (DOCKAUV_PACKAGE_ROOT)" if os.environ.get("DOCKAUV_PACKAGE_ROOT") else "this checkout",
           "results": results}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    json.dump(doc, open(args.out, "w"), indent=1)
    f = lambda d: f"{d['min_ms']:.3f}-{d['max_ms']:.3f}"
    for r in results:
        print(f"config {r['config']} ({r['envs']} envs): " + "; ".join(
            f"{grp} " + ", ".join(f"{n} {f(d)}" for n, d in r[grp].items()) for grp in ("rollout", "step", "push") if grp in r), file=sys.stderr)
        for k, v in r.get("sample", {}).items():
            print(f"  sample {k}: device {f(v['device'])}, torch {f(v['torch'])} ms", file=sys.stderr)


if __name__ == "__main__":
    main()
