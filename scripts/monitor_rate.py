#!/usr/bin/env python3
"""What the episode monitor costs on top of one PPO iteration's collection, and what the same statistics cost rebuilt in torch.
One GPU, one process, same box.

  python scripts/monitor_rate.py [--out profiles/monitor/scan_rate.json]

Config 3 (BlueROV2, 16-beam fan, 8 spheres) at 65 536 envs and config 4 (LAUV, 63 rays, 5 capsules) at 32 768; the 64-64 tanh
actor and critic of scripts/collect_rate.py; K = 128 steps per iteration, stochastic, max_timesteps as configured:
  (a) dockauv_collect as it is queued without a monitor (no terminal observations): the launches of the parent commit;
  (b) dockauv_collect with terminal observations (what a monitor forces);
  (c) (b) followed by dockauv_monitor_scan with values / returns on the same stream: collect(..., monitor=m);
  (d) (b) followed by the same statistics in torch: the segmented scan over [K, N] with a per-env carry, the outcome rule on the
      terminal observations, sums / min / max, and the explained variance;
  scan: dockauv_monitor_scan alone on the collection's buffers (all four launches);  gae: dockauv_gae alone on the same rows.
Each form is timed between two stream events per window; minimum, median and maximum over the windows after a warm-up.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from collect_rate import CONFIGS, GAMMA, GAE_LAMBDA, K, make, timed  # noqa: E402


def torch_statistics(torch, rows, term, values, ret, carry_ret, carry_len, n_obs, max_timesteps):
    """the monitor's statistics from the collection's tensors, in torch: returns (stats [16] float64, new carries)"""
    reward, done = rows[:, :, n_obs], rows[:, :, n_obs + 1] > 0.5
    ep_ret, ep_len = torch.empty_like(reward), torch.empty_like(reward, dtype=torch.int32)
    c_ret, c_len = carry_ret, carry_len
    for k in range(reward.shape[0]):
        r, ln = c_ret + reward[k], c_len + 1
        ep_ret[k], ep_len[k] = r, ln
        c_ret, c_len = torch.where(done[k], 0.0, r), torch.where(done[k], 0, ln)
    t0, t6, t7 = term[:, :, 0], term[:, :, 6].abs(), term[:, :, 7].abs()
    code = torch.where(t0 == 0, 0, torch.where(t0 == 1, 1, torch.where((t6 == 1) | (t7 == 1), 2, torch.where(ep_len > max_timesteps, 3, 4))))
    rets, lens = ep_ret[done].double(), ep_len[done].double()
    stats = torch.zeros(16, device=rows.device, dtype=torch.float64)
    stats[0], stats[1], stats[2], stats[3] = rets.numel(), rets.sum(), (rets * rets).sum(), lens.sum()
    if rets.numel():
        stats[4], stats[5], stats[6], stats[7] = rets.min(), rets.max(), lens.min(), lens.max()
    stats[8:13] = torch.bincount(code[done], minlength=5)[:5]
    stats[13] = rets.numel()
    y, e = ret.double(), (ret - values[:-1]).double()
    stats[14] = 1.0 - e.var(unbiased=False) / y.var(unbiased=False)
    return stats, c_ret, c_len


def measure(config_id, n_envs, iters, warmup):
    import torch
    env, actor, critic, log_std, pol, val = make(config_id, n_envs)
    n_obs, n_u, N = env.n_observations, env.n_u, n_envs
    max_t = int(env.config["max_timesteps"])
    res = {"config": config_id, "envs": N, "n_obs": n_obs, "steps_per_iteration": K, "max_timesteps": max_t}
    try:
        z = lambda *shape: torch.zeros(shape, device="cuda")
        rows, term = z(K + 1, N, n_obs + 2), z(K, N, n_obs)
        acts, logp, values, adv, ret = z(K, N, n_u), z(K, N), z(K + 1, N), z(K, N), z(K, N)
        stats = torch.zeros(16, device="cuda", dtype=torch.float64)
        mon = env.make_monitor()
        stream = lambda: torch.cuda.current_stream().cuda_stream
        carry = [z(N), torch.zeros(N, device="cuda", dtype=torch.int32)]

        def collect(term_ptr=0):
            rows[0].copy_(rows[K])
            env.collect_device(pol, val, rows[0].data_ptr(), rows[1].data_ptr(), acts.data_ptr(), K, gamma=GAMMA, gae_lambda=GAE_LAMBDA,
                               stochastic=True, stream=stream(), terminal_obs_ptr=term_ptr, log_prob_ptr=logp.data_ptr(),
                               values_ptr=values.data_ptr(), advantages_ptr=adv.data_ptr(), returns_ptr=ret.data_ptr())

        def scan():
            env.monitor_scan_device(mon, rows[1].data_ptr(), K, stats.data_ptr(), terminal_obs_ptr=term.data_ptr(),
                                    values_ptr=values.data_ptr(), returns_ptr=ret.data_ptr(), stream=stream())

        def collect_term():
            collect(term.data_ptr())

        def collect_monitor():
            collect(term.data_ptr())
            scan()

        def collect_torch():
            collect(term.data_ptr())
            st, carry[0], carry[1] = torch_statistics(torch, rows[1:], term, values, ret, carry[0], carry[1], n_obs, max_t)
            return st

        def gae():
            env.gae_device(rows[1].data_ptr(), values.data_ptr(), K, GAMMA, GAE_LAMBDA, adv.data_ptr(), ret.data_ptr(), stream=stream())

        res["a_collect"] = timed(collect, iters, warmup)
        res["b_collect_terminal_obs"] = timed(collect_term, iters, warmup)
        env.monitor_sync(mon, stream=stream())
        res["c_collect_monitor"] = timed(collect_monitor, iters, warmup)
        res["scan_alone"] = timed(scan, iters, warmup)
        res["gae_alone"] = timed(gae, iters, warmup)
        res["d_collect_then_torch"] = timed(collect_torch, iters, warmup)
        env.synchronize()
        res["episodes_in_last_scan"] = float(stats[0])
        res["scan_over_gae"] = res["scan_alone"]["median_ms"] / res["gae_alone"]["median_ms"]
    finally:
        env.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "monitor", "scan_rate.json"))
    ap.add_argument("--iterations", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    import torch
    results = [measure(c, CONFIGS[c], args.iterations, args.warmup) for c in sorted(CONFIGS)]
    doc = {"what": "the episode monitor on one PPO iteration's collection, milliseconds per iteration of K = 128 steps: dockauv_collect "
                   "without terminal observations (a: what is queued without a monitor, the parent commit's launches), with them (b), "
                   "with them and dockauv_monitor_scan (c), with them and the same statistics in torch (d); the scan's four launches "
                   "alone and the GAE launch alone; min / median / max over windows between stream events, one process",
           "device": torch.cuda.get_device_name(0), "results": results}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    json.dump(doc, open(args.out, "w"), indent=1)
    for r in results:
        f = lambda k: f"{r[k]['min_ms']:.3f}-{r[k]['max_ms']:.3f}"
        print(f"config {r['config']} ({r['envs']} envs): a {f('a_collect')}, b {f('b_collect_terminal_obs')}, c {f('c_collect_monitor')}, "
              f"d {f('d_collect_then_torch')} ms; scan alone {f('scan_alone')}, gae alone {f('gae_alone')} ms", file=sys.stderr)


if __name__ == "__main__":
    main()
