#!/usr/bin/env python3
"""What the evaluator costs per chunk of an evaluation, against the episode monitor on the same rows.  One GPU, one process.

  python scripts/eval_rate.py [--out profiles/eval/eval_rate.json]

Config 3 (BlueROV2, 16-beam fan, 8 spheres) at 65 536 envs and config 4 (LAUV, 63 rays, 5 capsules) at 32 768; the 64-64 tanh
actor of scripts/collect_rate.py, deterministic; K = 128 steps per chunk, max_timesteps as configured, target 1 per env (one
slot):
  (r) dockauv_rollout with terminal observations: a chunk without any bookkeeping;
  (m) (r) followed by dockauv_monitor_scan without values / returns (two launches): rollout(..., monitor=m);
  (e) (r) followed by dockauv_eval_scan (two launches): a chunk of TorchDocking3d.evaluate;
  scan_monitor / scan_eval: the two scans alone on the last chunk's rows;  begin_scan_eval: dockauv_eval_begin (two copies and
  a launch) and the scan, so that every window records again (scan_eval alone runs with the quotas already full once every env
  has finished an episode: it walks the rows, stores nothing new and adds up the one slot per env);  begin_eval: the begin alone.
The forms alternate inside every window, each between two stream events of its own; minimum, median and maximum over the
windows after a warm-up.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from collect_rate import CONFIGS, K, make  # noqa: E402
from rewnorm_rate import timed_alternating  # noqa: E402


def measure(config_id, n_envs, iters, warmup):
    import torch
    env, _, _, _, pol, _ = make(config_id, n_envs)
    n_obs, n_u, N = env.n_observations, env.n_u, n_envs
    res = {"config": config_id, "envs": N, "n_obs": n_obs, "steps_per_chunk": K, "max_timesteps": int(env.config["max_timesteps"]),
           "target_per_env": 1, "slots_per_env": 1}
    try:
        z = lambda *shape: torch.zeros(shape, device="cuda")
        rows, term, acts = z(K + 1, N, n_obs + 2), z(K, N, n_obs), z(K, N, n_u)
        st_m, st_e = (torch.zeros(16, device="cuda", dtype=torch.float64) for _ in range(2))
        mon, ev = env.make_monitor(), env.make_evaluator(1)
        stream = lambda: torch.cuda.current_stream().cuda_stream

        def rollout():
            rows[0].copy_(rows[K])
            env.rollout_device(pol, rows[0].data_ptr(), rows[1].data_ptr(), acts.data_ptr(), K, stochastic=False, stream=stream(),
                               terminal_obs_ptr=term.data_ptr())

        def scan_monitor():
            env.monitor_scan_device(mon, rows[1].data_ptr(), K, st_m.data_ptr(), terminal_obs_ptr=term.data_ptr(), stream=stream())

        def scan_eval():
            env.evaluator_scan_device(ev, rows[1].data_ptr(), K, st_e.data_ptr(), terminal_obs_ptr=term.data_ptr(), stream=stream())

        def begin_eval():
            env.evaluator_begin(ev, 0, 1, stream=stream())

        def rollout_monitor():
            rollout()
            scan_monitor()

        def rollout_eval():
            rollout()
            scan_eval()

        def begin_scan_eval():
            begin_eval()
            scan_eval()

        begin_eval()
        env.monitor_sync(mon, stream=stream())
        res.update(timed_alternating({"r_rollout": rollout, "m_rollout_monitor": rollout_monitor, "e_rollout_eval": rollout_eval},
                                     iters, warmup))
        env.synchronize()
        res["episodes_recorded"], res["episodes_missing"] = float(st_e[0]), float(st_e[15])
        res["episodes_in_last_monitor_scan"] = float(st_m[0])
        res.update(timed_alternating({"scan_monitor": scan_monitor, "scan_eval": scan_eval, "begin_scan_eval": begin_scan_eval,
                                      "begin_eval": begin_eval}, iters, warmup))
        env.synchronize()
        res["scan_eval_over_scan_monitor"] = res["scan_eval"]["median_ms"] / res["scan_monitor"]["median_ms"]
        res["begin_scan_eval_over_scan_monitor"] = res["begin_scan_eval"]["median_ms"] / res["scan_monitor"]["median_ms"]
    finally:
        env.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval", "eval_rate.json"))
    ap.add_argument("--iterations", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    import torch
    results = [measure(c, CONFIGS[c], args.iterations, args.warmup) for c in sorted(CONFIGS)]
    doc = {"what": "policy evaluation with an episode quota per env, milliseconds per chunk of K = 128 steps, target 1 per env: "
                   "dockauv_rollout with terminal observations (r), followed by dockauv_monitor_scan (m) or by dockauv_eval_scan (e); "
                   "the two scans alone on the same rows (two launches each), dockauv_eval_begin + scan, the begin alone; the forms "
                   "alternating inside every window, min / median / max over windows between stream events, one process",
           "device": torch.cuda.get_device_name(0), "results": results}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    json.dump(doc, open(args.out, "w"), indent=1)
    for r in results:
        f = lambda k: f"{r[k]['min_ms']:.3f}-{r[k]['max_ms']:.3f}"
        print(f"config {r['config']} ({r['envs']} envs): r {f('r_rollout')}, m {f('m_rollout_monitor')}, e {f('e_rollout_eval')} ms; "
              f"scan_monitor {f('scan_monitor')}, scan_eval {f('scan_eval')}, begin + scan {f('begin_scan_eval')}, begin {f('begin_eval')} ms",
              file=sys.stderr)


if __name__ == "__main__":
    main()
