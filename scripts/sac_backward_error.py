#!/usr/bin/env python3
"""Writes profiles/sac/backward_error.txt: dockauv_sac_actor_backward and dockauv_q_backward against their float64 statements,
measured on one GPU with the helpers of tests/test_gpu_sac_backward.py (the same weights, rows, shapes and row counts as the tests).

  python scripts/sac_backward_error.py [--out profiles/sac/backward_error.txt]
  python scripts/sac_backward_error.py --relu-rows      # CPU only: the relu rows each case drops, for the seeds of the tests

Per case and output tensor: the device's error and the error of the float32 NumPy restatement against float64 (max over the
tensor), and the ratio device / max(e32, floor / 8) that the tests hold against 8 (floor: 4 ulp of max |g64|).
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def cases(T):
    """(kind, n_obs, n_u, hidden, act, rows) of every case the tests hold against float64"""
    big = T.B().ROWS_BEYOND_ONE_PASS
    out = [(kind, 20, 6, h, act, 33) for h in T.ALL_TILES for act in ("tanh", "relu") for kind in ("actor", "Q")]
    out += [("Q", n_obs, n_u, h, act, n) for n_obs, n_u, h, act in T.Q_CASES for n in T.ROW_COUNTS]
    out += [("Q", 20, 6, (64, 64), "relu", big)]
    out += [("actor", 20, 6, (128, 128), "relu", n) for n in T.ROW_COUNTS + (big,)]
    return out


def relu_rows(T):
    for kind, n_obs, n_u, hidden, act, n in cases(T):
        if act != "relu":
            continue
        mlp = T.q_mlp(n_obs, n_u, hidden, act) if kind == "Q" else T.sac_mlp(n_obs, n_u, hidden, act)._both_heads()
        _, dropped, drawn = T.B().draw_rows(mlp, n, T.ROW_SEED)
        print(f"{kind} {n_obs}+{n_u} {'-'.join(map(str, hidden))} rows {n}: {dropped} dropped, {drawn - n} allowed")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sac", "backward_error.txt"))
    ap.add_argument("--relu-rows", action="store_true")
    args = ap.parse_args()
    from tests import test_gpu_sac_backward as T
    if args.relu_rows:
        relu_rows(T)
        return
    import torch  # noqa: F401  (before the library: one HIP runtime serves both, tests/conftest.py)
    lines = ["# dockauv_sac_actor_backward / dockauv_q_backward against float64 (scripts/sac_backward_error.py on the helpers of",
             "# tests/test_gpu_sac_backward.py)",
             "# case tensor device_err numpy_f32_err ratio; ratio = device_err / max(e32, floor / 8), floor = 4 ulp of max |g64|; the",
             "# tests assert ratio <= 8"]
    worst = (0.0, "")
    envs = {}
    try:
        for kind, n_obs, n_u, hidden, act, n in cases(T):
            env = envs.get((n_obs, n_u))
            if env is None:
                env = envs[(n_obs, n_u)] = T.P().fan_env(n_obs, n_u, 64)
            label = f"{kind}_{n_obs}+{n_u}_{'-'.join(map(str, hidden))}_{act}_rows{n}"
            rows = (T.q_case if kind == "Q" else T.actor_case)(env, n_obs, n_u, hidden, act, n, label=label)
            for name, e_dev, e_np, bound in rows:
                ratio = 8.0 * e_dev / bound
                if ratio > worst[0]:
                    worst = (ratio, f"{label} {name}")
                lines.append(f"{label} {name} {e_dev:.3e} {e_np:.3e} {ratio:.2f}")
    finally:
        for env in envs.values():
            env.close()
    lines.append(f"worst_ratio {worst[0]:.2f} {worst[1]}")
    print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
