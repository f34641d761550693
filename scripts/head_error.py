#!/usr/bin/env python3
"""Writes profiles/update/head_error.txt: dockauv_ppo_head against its float64 statement, measured on one GPU with the helpers of
tests/test_gpu_head.py (the same draws, shapes and row counts as the tests).

  python scripts/head_error.py [--out profiles/update/head_error.txt]

Per action count, row count and output one line: the variant (normalisation, critic, dense or indexed) with the largest ratio
device error / max(e32, floor / 8), which the tests hold against 8 (floor: 4 ulp of max |x64|), with the device's error and the
error of the float32 NumPy restatement against float64 (max over the output) of that variant.  Then the largest ratio per output.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "update", "head_error.txt"))
    args = ap.parse_args()
    import torch  # noqa: F401  (before the library: one HIP runtime per process, tests/conftest.py)
    from tests import test_gpu_head as T
    lines = ["# dockauv_ppo_head against float64 (scripts/head_error.py on the helpers of tests/test_gpu_head.py)",
             "# n_u rows output worst_variant device_err numpy_f32_err ratio; ratio = device_err / max(e32, floor / 8), floor = 4 ulp of",
             "# max |x64|; worst_variant: the one of the case's variants (norm|raw, critic|nocritic, dense|index) with the largest ratio",
             "# (approx_kl: 4 ulp of the largest ratio, tests/test_gpu_head.py: KL_FLOOR_ULPS); the tests assert ratio <= 8"]
    worst, per_case, per_output = (0.0, ""), {}, {}
    cases = [(n_u, n, v) for n_u in (6, 3, 8) for n in T.ROW_COUNTS for v in T.variants(n)]
    cases += [(6, T.ROWS_BEYOND_ONE_PASS, v) for v in ((True, True, True), (True, False, False), (False, True, False))]
    envs = {}
    try:
        for n_u, n, (normalize, critic, indexed) in cases:
            if n_u not in envs:
                envs[n_u] = (T.B_().P().fan_env(T.ENVS[n_u], n_u, 64), {})
            env, actors = envs[n_u]
            variant = f"{'norm' if normalize else 'raw'}_{'critic' if critic else 'nocritic'}_{'index' if indexed else 'dense'}"
            for name, e_dev, e_np, bound, ratio in T.head_case(n_u, n, normalize, critic, indexed, env, actors):
                worst = max(worst, (ratio, f"n_u{n_u} rows{n} {variant} {name}"))
                per_case[(n_u, n, name)] = max(per_case.get((n_u, n, name), (-1.0,)), (ratio, variant, e_dev, e_np))
                per_output[name] = max(per_output.get(name, (-1.0,)), (ratio, f"n_u{n_u} rows{n} {variant}"))
    finally:
        for env, _ in envs.values():
            env.close()
    for (n_u, n, name), (ratio, variant, e_dev, e_np) in per_case.items():
        lines.append(f"n_u{n_u} rows{n} {name} {variant} {e_dev:.3e} {e_np:.3e} {ratio:.2f}")
    for name, (ratio, where) in per_output.items():
        lines.append(f"worst_of_output {name} {ratio:.2f} {where}")
    lines.append(f"worst_ratio {worst[0]:.2f} {worst[1]}")
    print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
