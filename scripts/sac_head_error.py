#!/usr/bin/env python3
"""Writes profiles/sac/head_error.txt: dockauv_sac_actor_head against its float64 statement on the crafted heads of the tests, and
the whole gradient half (TorchDocking3d.sac_gradients) against the float64 graph, measured on one GPU with the helpers of
tests/test_gpu_sac_head.py (the same weights, rows, shapes and row counts as the tests).

  python scripts/sac_head_error.py [--out profiles/sac/head_error.txt]

Per case and output tensor: the device's error and the error of the float32 restatement against float64 (max over the tensor),
and the ratio device / max(e32, floor / 8) that the tests hold against 8 (floor: 4 ulp of max |g64|).
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sac", "head_error.txt"))
    args = ap.parse_args()
    import torch  # noqa: F401  (before the library: one HIP runtime serves both, tests/conftest.py)
    from tests import test_gpu_sac_head as T
    lines = ["# dockauv_sac_actor_head and TorchDocking3d.sac_gradients against float64 (scripts/sac_head_error.py on the helpers of",
             "# tests/test_gpu_sac_head.py)",
             "# case tensor device_err float32_err ratio; ratio = device_err / max(e32, floor / 8), floor = 4 ulp of max |g64|; the",
             "# tests assert ratio <= 8"]
    worst = (0.0, "")

    def add(label, rows):
        nonlocal worst
        for name, e_dev, e_np, bound in rows:
            ratio = 8.0 * e_dev / bound
            if ratio > worst[0]:
                worst = (ratio, f"{label} {name}")
            lines.append(f"{label} {name.replace(' ', '_')} {e_dev:.3e} {e_np:.3e} {ratio:.2f}")

    for (n_obs, n_u), hidden in T.CASES:
        env = T.S().sac_env(n_obs, n_u, 64)
        try:
            _, _, actor, _ = T.networks(env, hidden)
            for B in T.ROW_COUNTS:
                label = f"actor_head_nu{n_u}_rows{B}"
                add(label, T.actor_head_case(env, actor, B, label=label)[0])
        finally:
            env.close()
    T.test_sac_gradients_end_to_end()
    add("sac_gradients_20+6_64-64_relu_rows129", T.RECORD["sac_gradients_B129"])
    lines.append(f"worst_ratio {worst[0]:.2f} {worst[1]}")
    print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
