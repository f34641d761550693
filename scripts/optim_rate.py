#!/usr/bin/env python3
"""The tail of a PPO minibatch step -- gradient-norm clipping, Adam, the weight load -- and the whole step with it, on the
buffers of one collection: the device optimiser (dockauv_optim_step, TorchDocking3d.ppo_update) against torch, on the same box,
in the same process, on the same rows.  Writes profiles/update/optim_rate.json.

  python scripts/optim_rate.py [--out profiles/update/optim_rate.json]

Config 3 (BlueROV2, 16-beam fan, 65 536 envs), a 64-64 tanh actor and a 64-64 tanh critic, the rows of one dockauv_collect of
K = 128 steps; minibatches of 65 536 and of 1 048 576 rows through a random index (scripts/head_rate.py: the same sizes).
  tail_library:      opt.step(lr) of TorchDocking3d.make_optimizer: one launch for the norm, the clipping and Adam, then the
                     repack of both networks;
  tail_torch:        clip_grad_norm_(params, 0.5), torch.optim.Adam(eps=1e-5).step(), load_policy of the actor and of the critic
                     (what the next ppo_minibatch does first); tail_torch_fused: the same with Adam(fused=True);
  step_library:      one minibatch of ppo_update (the two forwards, the head, the two backwards, opt.step);
  step_torch:        the loop body of INTEGRATION.md section 6 before the device optimiser: ppo_minibatch, clip_grad_norm_,
                     Adam.step(); step_torch_fused: with Adam(fused=True).
A tail pass is timed as scripts/head_rate.py times a pass, between two stream events per window, but with `--per-window` = 64
passes a window instead of 8: eight device tails are 0.14 ms, too short a window for the event clock.  A
step is timed over whole epochs, because ppo_update draws its own permutation: a window is one epoch over the collection (one
torch.randperm of all K x N rows and its 128 or 8 minibatches, the permutation inside the window for every form), divided by
the number of minibatches.  Recorded are the median, the minimum and the maximum over 24 windows after a warm-up, in
milliseconds per pass, after the forms' updated weights were compared.
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


def timed(run, windows, warmup, per_window, passes_per_run=1):
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
        ms.append(e0.elapsed_time(e1) / (per_window * passes_per_run))
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "windows": len(ms),
            "passes_per_window": per_window * passes_per_run}


def max_rel_diff(xs, ys):
    return max(float((x - y).abs().max() / y.abs().max().clamp_min(1e-30)) for x, y in zip(xs, ys))


def measure(windows, warmup, per_window):
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
        rows = c.obs[:K]
        flat = lambda t: t.reshape(M, *t.shape[2:])
        actions, logp_old, adv, ret = flat(c.actions), flat(c.log_prob), flat(c.advantages), flat(c.returns)
        # the learner has moved on from the collecting weights, so that ratios spread and some rows are clipped
        with torch.no_grad():
            for p in list(actor.parameters()) + list(critic.parameters()):
                p.add_(0.02 * torch.randn_like(p))
        a_params, c_params = list(actor.parameters()), list(critic.parameters())
        params = a_params + [log_std] + c_params          # the device optimiser's order
        start = [p.detach().clone() for p in params]
        res.update(n_obs=n_obs, n_u=n_u, actor=f"{n_obs}-64-64-{n_u} tanh", critic=f"{n_obs}-64-64-1 tanh", rows=M,
                   parameters=int(sum(p.numel() for p in params)))
        kw = dict(clip_range=CLIP, vf_coef=VF, ent_coef=ENT)
        gen = torch.Generator(device="cuda")

        def restore():
            with torch.no_grad():
                for p, s in zip(params, start):
                    p.copy_(s)

        def torch_tail(adam):
            torch.nn.utils.clip_grad_norm_(params, MAX_NORM)
            adam.step()

        def torch_epoch(adam, B):
            for idx in torch.randperm(M, device="cuda", generator=gen).split(B):
                env.ppo_minibatch(policy, value, a_params, log_std, c_params, actions, logp_old, adv, ret, rows, idx, **kw)
                torch_tail(adam)

        for B in SIZES:
            n_mb = (M + B - 1) // B
            entry = {"rows": B, "minibatches_per_epoch": n_mb}
            # ---- the forms agree: one epoch from the same weights with the same permutation (float32, other summation orders, Adam)
            finals = {}
            for form in ("library", "torch", "torch_fused"):
                restore()
                gen.manual_seed(3)
                if form == "library":
                    opt = env.make_optimizer(policy, value, a_params, log_std, c_params, max_grad_norm=MAX_NORM)
                    stats = env.ppo_update(opt, c, 1, B, LR, generator=gen, **kw)
                    entry["first_minibatch"] = {"loss": float(stats[0, 0, 0]), "clip_fraction": float(stats[0, 0, 5]),
                                                "grad_norm": float(stats[0, 0, 8]), "coef": float(stats[0, 0, 9])}
                else:
                    torch_epoch(torch.optim.Adam(params, lr=LR, eps=1e-5, fused=(form == "torch_fused")), B)
                torch.cuda.synchronize()
                finals[form] = [p.detach().clone() for p in params]
            moved = max_rel_diff(finals["library"], start)
            entry["weights_after_one_epoch"] = {"max_relative_change": moved,
                                                "library_against_torch": max_rel_diff(finals["library"], finals["torch"]),
                                                "library_against_torch_fused": max_rel_diff(finals["library"], finals["torch_fused"])}

            # ---- the tail alone, on the gradients of one minibatch of this size
            restore()
            idx = torch.randperm(M, device="cuda", generator=gen)[:B].contiguous()
            env.ppo_minibatch(policy, value, a_params, log_std, c_params, actions, logp_old, adv, ret, rows, idx, **kw)
            grads = [p.grad.clone() for p in params]
            tails = {}
            opt = env.make_optimizer(policy, value, a_params, log_std, c_params, max_grad_norm=MAX_NORM)
            for g, src in zip(opt.grads, grads):
                g.copy_(src)
            opt.step(LR)
            torch.cuda.synchronize()
            tails["library"] = [p.detach().clone() for p in params]
            adams = {}
            for form, fused in (("torch", False), ("torch_fused", True)):
                restore()
                for p, g in zip(params, grads):
                    p.grad = g.clone()
                adams[form] = torch.optim.Adam(params, lr=LR, eps=1e-5, fused=fused)
                torch_tail(adams[form])
                torch.cuda.synchronize()
                tails[form] = [p.detach().clone() for p in params]
            entry["weights_after_one_tail"] = {"library_against_torch": max_rel_diff(tails["library"], tails["torch"]),
                                               "library_against_torch_fused": max_rel_diff(tails["library"], tails["torch_fused"])}

            def tail_torch(form):
                def run():
                    torch_tail(adams[form])
                    env.load_policy(policy, a_params, log_std=log_std)
                    env.load_policy(value, c_params)
                return run

            entry["tail_library"] = timed(lambda: opt.step(LR), windows, warmup, per_window)
            entry["tail_torch"] = timed(tail_torch("torch"), windows, warmup, per_window)
            entry["tail_torch_fused"] = timed(tail_torch("torch_fused"), windows, warmup, per_window)

            # ---- the whole step: one epoch a window
            restore()
            entry["step_library"] = timed(lambda: env.ppo_update(opt, c, 1, B, LR, generator=gen, **kw), windows, 1, 1, n_mb)
            for form in ("torch", "torch_fused"):
                restore()
                entry[f"step_{form}"] = timed(lambda: torch_epoch(adams[form], B), windows, 1, 1, n_mb)
            for what in ("tail", "step"):
                faster = min(entry[f"{what}_torch"]["min_ms"], entry[f"{what}_torch_fused"]["min_ms"])
                entry[f"{what}_library_min_not_above_faster_torch_min"] = bool(entry[f"{what}_library"]["min_ms"] <= faster)
                entry[f"{what}_faster_torch_min_over_library_min"] = faster / entry[f"{what}_library"]["min_ms"]
            print(f"{B} rows: tail library {entry['tail_library']['median_ms']:.4f} ms, torch {entry['tail_torch']['median_ms']:.4f}, "
                  f"fused {entry['tail_torch_fused']['median_ms']:.4f}; step library {entry['step_library']['median_ms']:.4f} ms, torch "
                  f"{entry['step_torch']['median_ms']:.4f}, fused {entry['step_torch_fused']['median_ms']:.4f}; weights after one epoch "
                  f"library against torch {entry['weights_after_one_epoch']['library_against_torch']:.2e} (moved {moved:.2e})",
                  file=sys.stderr, flush=True)
            res[f"minibatch_{B}_indexed"] = entry
            for p in params:
                p.grad = None
            torch.cuda.empty_cache()
    finally:
        env.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "update", "optim_rate.json"))
    ap.add_argument("--windows", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--per-window", type=int, default=64)
    args = ap.parse_args()
    import torch
    doc = {"what": "the tail of a PPO minibatch step and the whole step on the rows of one dockauv_collect (config 3, K = 128, 64-64 "
                   "tanh actor and critic), milliseconds per pass: opt.step of the device optimiser against clip_grad_norm_ + "
                   "torch.optim.Adam.step (default and fused) + load_policy of both networks, and one ppo_update minibatch against "
                   "ppo_minibatch + clip_grad_norm_ + Adam.step; tails per window of passes between stream events, steps per "
                   "window of one epoch (its torch.randperm included) divided by its minibatches; median, min and max over the "
                   "windows, one process",
           "device": torch.cuda.get_device_name(0), "results": [measure(args.windows, args.warmup, args.per_window)]}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(doc, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
