#!/usr/bin/env python3
"""What reward normalisation costs on top of one PPO iteration's collection.  One GPU, one process, same box.

  python scripts/rewnorm_rate.py [--out profiles/collect/rewnorm_rate.json]
  python scripts/rewnorm_rate.py --plain-only --out plain.json     # form (a) alone: runs on a commit without the option
  python scripts/rewnorm_rate.py --merge-plain plain.json [--merge-plain-here plain_here.json] [--out ...]

Config 3 (BlueROV2, 16-beam fan, 8 spheres) at 65 536 envs and config 4 (LAUV, 63 rays, 5 capsules) at 32 768; the 64-64 tanh
actor and critic of scripts/collect_rate.py; K = 128 steps per iteration, stochastic:
  (a) dockauv_collect: the plain path, which must not change;
  (n) dockauv_collect_normalized: (a) with the normaliser's four launches behind the value launches and the GAE on the column;
  (s) dockauv_rewnorm_scan alone on the last collection's rows (four launches), and frozen (one launch);
  (g) dockauv_gae_normalized and dockauv_gae alone on the same buffers;
  (t) the same normalisation and GAE rebuilt in torch after a plain collection -- the K-step RunningMeanStd loop over the reward
      columns, then the K-step GAE loop: the form a learner has to write without the option.
The forms alternate inside every window, each between two stream events of its own, so that a drift of the box meets all of
them; minimum, median and maximum over the windows after a warm-up.
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

CLIP, EPS = 10.0, 1e-8


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


class TorchNormalizer:
    """SB3's VecNormalize(norm_reward=True) and compute_returns_and_advantage as a learner writes them in torch on device
    tensors: K sequential RunningMeanStd updates (float64 statistics, no host synchronisation), then K GAE steps backwards"""

    def __init__(self, torch, n_envs):
        self.torch = torch
        f64 = dict(device="cuda", dtype=torch.float64)
        self.mean, self.var, self.count = torch.zeros((), **f64), torch.ones((), **f64), torch.full((), 1e-4, **f64)
        self.returns = torch.zeros(n_envs, device="cuda")
        self.n = float(n_envs)

    def normalize(self, reward, done, out):
        torch = self.torch
        for k in range(reward.shape[0]):
            self.returns = self.returns * GAMMA + reward[k]
            x = self.returns.double()
            batch_var, batch_mean = torch.var_mean(x, unbiased=False)
            delta = batch_mean - self.mean
            tot = self.count + self.n
            self.mean = self.mean + delta * self.n / tot
            m2 = self.var * self.count + batch_var * self.n + delta * delta * self.count * self.n / tot
            self.var = m2 / tot
            self.count = tot
            out[k] = torch.clamp(reward[k].double() / torch.sqrt(self.var + EPS), -CLIP, CLIP).float()
            self.returns = torch.where(done[k], torch.zeros_like(self.returns), self.returns)

    def gae(self, reward, done, values, adv, ret):
        torch = self.torch
        gae = torch.zeros_like(reward[0])
        for k in range(reward.shape[0] - 1, -1, -1):
            nt = (~done[k]).float()
            delta = reward[k] + GAMMA * nt * values[k + 1] - values[k]
            gae = delta + GAMMA * GAE_LAMBDA * nt * gae
            adv[k] = gae
        torch.add(adv, values[:-1], out=ret)


def measure(config_id, n_envs, iters, warmup, plain_only):
    import torch
    env, actor, critic, log_std, pol, val = make(config_id, n_envs)
    n_obs, n_u, N = env.n_observations, env.n_u, n_envs
    res = {"config": config_id, "envs": N, "n_obs": n_obs, "steps_per_iteration": K}
    try:
        z = lambda *shape, dtype=torch.float32: torch.zeros(shape, device="cuda", dtype=dtype)
        rows = z(K + 1, N, n_obs + 2)
        acts, logp, values, adv, ret = z(K, N, n_u), z(K, N), z(K + 1, N), z(K, N), z(K, N)
        stream = lambda: torch.cuda.current_stream().cuda_stream

        def collect():
            rows[0].copy_(rows[K])
            env.collect_device(pol, val, rows[0].data_ptr(), rows[1].data_ptr(), acts.data_ptr(), K, gamma=GAMMA, gae_lambda=GAE_LAMBDA,
                               stochastic=True, stream=stream(), log_prob_ptr=logp.data_ptr(), values_ptr=values.data_ptr(),
                               advantages_ptr=adv.data_ptr(), returns_ptr=ret.data_ptr())
        forms = {"a_collect": collect}
        if plain_only:
            res.update(timed_alternating(forms, iters, warmup))
            env.synchronize()
            return res
        rn = env.make_reward_normalizer(GAMMA, CLIP, EPS)
        norm, disc, stats = z(K, N), z(K, N), z(K, 4, dtype=torch.float64)
        tn = TorchNormalizer(torch, N)
        t_norm, t_adv, t_ret = z(K, N), z(K, N), z(K, N)

        def collect_normalized():
            rows[0].copy_(rows[K])
            env.collect_normalized_device(pol, val, rn, rows[0].data_ptr(), rows[1].data_ptr(), acts.data_ptr(), K, norm.data_ptr(),
                                          disc.data_ptr(), stats.data_ptr(), values.data_ptr(), adv.data_ptr(), ret.data_ptr(),
                                          gamma=GAMMA, gae_lambda=GAE_LAMBDA, stochastic=True, stream=stream(),
                                          log_prob_ptr=logp.data_ptr())

        def collect_then_torch():
            collect()
            reward, done = rows[1:, :, n_obs], rows[1:, :, n_obs + 1] > 0.5
            tn.normalize(reward, done, t_norm)
            tn.gae(t_norm, done, values, t_adv, t_ret)
        forms["n_collect_normalized"] = collect_normalized
        forms["t_collect_then_torch_normalize_and_gae"] = collect_then_torch
        res.update(timed_alternating(forms, iters, warmup))
        res["running_var_device"], res["running_var_torch"] = float(stats[K - 1, 2]), float(tn.var)
        scan = lambda training: env.reward_normalizer_scan_device(rn, rows[1].data_ptr(), K, norm.data_ptr(), disc.data_ptr(),
                                                                  stats.data_ptr(), training=training, stream=stream())

        def torch_alone():
            reward, done = rows[1:, :, n_obs], rows[1:, :, n_obs + 1] > 0.5
            tn.normalize(reward, done, t_norm)
            tn.gae(t_norm, done, values, t_adv, t_ret)
        parts = {
            "rewnorm_scan_four_launches": lambda: scan(True),
            "rewnorm_scan_frozen_one_launch": lambda: scan(False),
            "gae_normalized_alone": lambda: env.gae_normalized_device(None, norm.data_ptr(), rows[1].data_ptr(), values.data_ptr(), K,
                                                                      GAMMA, GAE_LAMBDA, adv.data_ptr(), ret.data_ptr(), stream=stream()),
            "gae_alone": lambda: env.gae_device(rows[1].data_ptr(), values.data_ptr(), K, GAMMA, GAE_LAMBDA, adv.data_ptr(),
                                                ret.data_ptr(), stream=stream()),
            "torch_normalize_and_gae_alone": torch_alone,
        }
        res.update(timed_alternating(parts, iters, warmup))
        env.synchronize()
        res["added_ms_median"] = res["n_collect_normalized"]["median_ms"] - res["a_collect"]["median_ms"]
        res["added_by_torch_ms_median"] = res["t_collect_then_torch_normalize_and_gae"]["median_ms"] - res["a_collect"]["median_ms"]
    finally:
        env.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "collect", "rewnorm_rate.json"))
    ap.add_argument("--iterations", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--merge-plain", default="")
    ap.add_argument("--merge-plain-here", default="")
    args = ap.parse_args()
    if args.merge_plain:
        doc = json.load(open(args.out))
        parent = json.load(open(args.merge_plain))["results"]
        doc["plain_path_on_the_parent_commit"] = parent
        # like against like: form (a) alone on this commit's build too (--plain-only), when given; inside the full run it
        # alternates with the torch form, whose several hundred small launches leave the box in another state
        alone = json.load(open(args.merge_plain_here))["results"] if args.merge_plain_here else doc["results"]
        if args.merge_plain_here:
            doc["plain_path_alone_on_this_commit"] = alone
        # the one condition: the plain path within twice the parent's own run-to-run spread (its max - min over the windows)
        doc["plain_path_check"] = []
        for here, there in zip(alone, parent):
            spread = there["a_collect"]["max_ms"] - there["a_collect"]["min_ms"]
            diff = here["a_collect"]["median_ms"] - there["a_collect"]["median_ms"]
            doc["plain_path_check"].append({"config": here["config"], "median_ms": here["a_collect"]["median_ms"],
                                            "parent_median_ms": there["a_collect"]["median_ms"], "difference_ms": diff,
                                            "parent_spread_ms": spread, "within_twice_the_spread": bool(diff <= 2.0 * spread)})
        json.dump(doc, open(args.out, "w"), indent=1)
        return
    import torch
    results = [measure(c, CONFIGS[c], args.iterations, args.warmup, args.plain_only) for c in sorted(CONFIGS)]
    doc = {"what": "reward normalisation on one PPO iteration's collection, milliseconds per iteration of K = 128 steps: dockauv_collect "
                   "(a), dockauv_collect_normalized (n) and a plain collection followed by the K-step RunningMeanStd loop and GAE in "
                   "torch (t), alternating inside every window; dockauv_rewnorm_scan (training: four launches, frozen: one), "
                   "dockauv_gae_normalized, dockauv_gae and the torch loops alone on the last collection's buffers; min / median / max "
                   "over windows between stream events, one process",
           "device": torch.cuda.get_device_name(0), "results": results}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(doc, open(args.out, "w"), indent=1)
    for r in results:
        f = lambda k: f"{r[k]['min_ms']:.3f}-{r[k]['max_ms']:.3f}"
        line = f"config {r['config']} ({r['envs']} envs): a {f('a_collect')}"
        if not args.plain_only:
            line += (f", n {f('n_collect_normalized')}, t {f('t_collect_then_torch_normalize_and_gae')} ms; scan {f('rewnorm_scan_four_launches')}, "
                     f"frozen {f('rewnorm_scan_frozen_one_launch')}, gae on the column {f('gae_normalized_alone')}, gae {f('gae_alone')}, "
                     f"torch alone {f('torch_normalize_and_gae_alone')}")
        print(line + " ms", file=sys.stderr)


if __name__ == "__main__":
    main()
