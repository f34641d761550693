#!/usr/bin/env python3
"""What the truncation bootstrap costs on top of one PPO iteration's collection.  One GPU, one process, same box.

  python scripts/truncation_rate.py [--out profiles/collect/truncation_rate.json]
  python scripts/truncation_rate.py --plain-only --out plain.json     # forms (a) and (b) alone: runs on a commit without the option
  python scripts/truncation_rate.py --merge-plain plain.json [--out ...]

Config 3 (BlueROV2, 16-beam fan, 8 spheres) at 65 536 envs and config 4 (LAUV, 63 rays, 5 capsules) at 32 768; the 64-64 tanh
actor and critic of scripts/collect_rate.py; K = 128 steps per iteration, stochastic, max_timesteps as configured (1000: one slot):
  (a) dockauv_collect without terminal observations: the plain path;
  (b) dockauv_collect with terminal observations (what the option forces);
  (t) dockauv_collect_truncated: (b) with the copy of the step counters in front and the scan, the value launch over the slots and
      the GAE launch with the bootstrap in place of the GAE launch.
The three forms alternate inside every window -- (a), (b), (t), each between two stream events of its own --, so that a drift of
the box meets all of them; minimum, median and maximum over the windows after a warm-up.
For scale, on the buffers of the last collection and likewise alternating: dockauv_gae_truncated (its three launches),
dockauv_truncation_scan alone, dockauv_gae alone, dockauv_monitor_scan (four launches).  These repeat on the same rows, so the
length carries run on as if the rows repeated: the work per launch is the same.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from collect_rate import CONFIGS, GAMMA, GAE_LAMBDA, K, make  # noqa: E402


def timed_alternating(forms, iters, warmup):
    """{name: min / median / max ms} of every form, one event pair per form and window, the forms in order inside a window"""
    import torch
    for _ in range(warmup):
        for run in forms.values():
            run()
    torch.cuda.synchronize()
    ms = {name: [] for name in forms}
    for _ in range(iters):
        for name, run in forms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run()
            e1.record()
            e1.synchronize()
            ms[name].append(e0.elapsed_time(e1))
    return {name: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "windows": len(v)} for name, v in ms.items()}


def measure(config_id, n_envs, iters, warmup, plain_only):
    import torch
    env, actor, critic, log_std, pol, val = make(config_id, n_envs)
    n_obs, n_u, N = env.n_observations, env.n_u, n_envs
    res = {"config": config_id, "envs": N, "n_obs": n_obs, "steps_per_iteration": K, "max_timesteps": int(env.config["max_timesteps"])}
    try:
        z = lambda *shape, dtype=torch.float32: torch.zeros(shape, device="cuda", dtype=dtype)
        rows, term = z(K + 1, N, n_obs + 2), z(K, N, n_obs)
        acts, logp, values, adv, ret = z(K, N, n_u), z(K, N), z(K + 1, N), z(K, N), z(K, N)
        stream = lambda: torch.cuda.current_stream().cuda_stream

        def collect(term_ptr=0):
            rows[0].copy_(rows[K])
            env.collect_device(pol, val, rows[0].data_ptr(), rows[1].data_ptr(), acts.data_ptr(), K, gamma=GAMMA, gae_lambda=GAE_LAMBDA,
                               stochastic=True, stream=stream(), terminal_obs_ptr=term_ptr, log_prob_ptr=logp.data_ptr(),
                               values_ptr=values.data_ptr(), advantages_ptr=adv.data_ptr(), returns_ptr=ret.data_ptr())
        forms = {"a_collect": collect, "b_collect_terminal_obs": lambda: collect(term.data_ptr())}
        if plain_only:
            res.update(timed_alternating(forms, iters, warmup))
            env.synchronize()
            return res
        S = env.truncation_slots(K)
        carry, step, row, vt = z(N, dtype=torch.int32), z(S, N, dtype=torch.int32), z(S, N, dtype=torch.int64), z(S, N)
        res["n_slots"] = S

        def collect_truncated():
            rows[0].copy_(rows[K])
            env.collect_truncated_device(pol, val, rows[0].data_ptr(), rows[1].data_ptr(), acts.data_ptr(), K, S, term.data_ptr(),
                                         values.data_ptr(), adv.data_ptr(), ret.data_ptr(), carry.data_ptr(), step.data_ptr(),
                                         row.data_ptr(), vt.data_ptr(), gamma=GAMMA, gae_lambda=GAE_LAMBDA, stochastic=True,
                                         stream=stream(), log_prob_ptr=logp.data_ptr())
        forms["t_collect_truncated"] = collect_truncated
        res.update(timed_alternating(forms, iters, warmup))
        res["truncated_steps_in_last_collection"] = int((step >= 0).sum())
        mon = env.make_monitor()
        stats = torch.zeros(16, device="cuda", dtype=torch.float64)
        parts = {
            "gae_truncated_three_launches": lambda: env.gae_truncated_device(
                val, rows[1].data_ptr(), term.data_ptr(), values.data_ptr(), K, S, GAMMA, GAE_LAMBDA, carry.data_ptr(), step.data_ptr(),
                row.data_ptr(), vt.data_ptr(), adv.data_ptr(), ret.data_ptr(), stream=stream()),
            "truncation_scan_alone": lambda: env.truncation_scan_device(rows[1].data_ptr(), term.data_ptr(), K, S, carry.data_ptr(),
                                                                        step.data_ptr(), row.data_ptr(), stream=stream()),
            "gae_alone": lambda: env.gae_device(rows[1].data_ptr(), values.data_ptr(), K, GAMMA, GAE_LAMBDA, adv.data_ptr(),
                                                ret.data_ptr(), stream=stream()),
            "monitor_scan_four_launches": lambda: env.monitor_scan_device(mon, rows[1].data_ptr(), K, stats.data_ptr(),
                                                                          terminal_obs_ptr=term.data_ptr(), values_ptr=values.data_ptr(),
                                                                          returns_ptr=ret.data_ptr(), stream=stream()),
        }
        res.update(timed_alternating(parts, iters, warmup))
        env.synchronize()
        res["added_ms_median"] = res["t_collect_truncated"]["median_ms"] - res["b_collect_terminal_obs"]["median_ms"]
        res["added_launches_alone_ms_median"] = res["gae_truncated_three_launches"]["median_ms"] - res["gae_alone"]["median_ms"]
    finally:
        env.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "collect", "truncation_rate.json"))
    ap.add_argument("--iterations", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--merge-plain", default="")
    args = ap.parse_args()
    if args.merge_plain:
        doc = json.load(open(args.out))
        doc["plain_path_on_the_parent_commit"] = json.load(open(args.merge_plain))["results"]
        json.dump(doc, open(args.out, "w"), indent=1)
        return
    import torch
    results = [measure(c, CONFIGS[c], args.iterations, args.warmup, args.plain_only) for c in sorted(CONFIGS)]
    doc = {"what": "the truncation bootstrap on one PPO iteration's collection, milliseconds per iteration of K = 128 steps: "
                   "dockauv_collect without (a) and with (b) terminal observations, dockauv_collect_truncated (t), alternating inside "
                   "every window; dockauv_gae_truncated's three launches, the truncation scan, the GAE launch and the monitor scan alone "
                   "on the last collection's buffers; min / median / max over windows between stream events, one process",
           "device": torch.cuda.get_device_name(0), "results": results}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(doc, open(args.out, "w"), indent=1)
    for r in results:
        f = lambda k: f"{r[k]['min_ms']:.3f}-{r[k]['max_ms']:.3f}"
        line = f"config {r['config']} ({r['envs']} envs): a {f('a_collect')}, b {f('b_collect_terminal_obs')}"
        if not args.plain_only:
            line += (f", t {f('t_collect_truncated')} ms; three launches {f('gae_truncated_three_launches')}, scan {f('truncation_scan_alone')}, "
                     f"gae {f('gae_alone')}, monitor scan {f('monitor_scan_four_launches')}")
        print(line + " ms", file=sys.stderr)


if __name__ == "__main__":
    main()
