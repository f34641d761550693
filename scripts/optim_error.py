#!/usr/bin/env python3
"""Writes profiles/update/optim_error.txt: dockauv_optim_step against its float64 statement, measured on one GPU with the helpers
of tests/test_gpu_optim.py (the same shapes, gradients and steps as the tests).

  python scripts/optim_error.py [--out profiles/update/optim_error.txt]

Per shape, clipping threshold and step one line per kind of output (norm, coef, parameters, m, v): the array with the largest
ratio device error / max(e32, floor / 8), which the tests hold against 8 (floor: 4 ulp of max |x64|), with the device's error and
the error of the float32 NumPy restatement against float64 (max over that array).  Then the largest ratio overall.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "update", "optim_error.txt"))
    args = ap.parse_args()
    import torch  # noqa: F401  (before the library: one HIP runtime per process, tests/conftest.py)
    from tests import test_gpu_optim as T
    lines = ["# dockauv_optim_step against float64 (scripts/optim_error.py on the helpers of tests/test_gpu_optim.py)",
             "# case_mgn<max_grad_norm>_step<t> kind worst_array device_err numpy_f32_err ratio; ratio = device_err / max(e32, floor / 8),",
             "# floor = 4 ulp of max |x64|; kind: norm, coef, p (parameters), m, v; worst_array: the one of that kind with the largest",
             "# ratio; three consecutive steps of gradient norm 2.0, 0.6, 0.1 and lr 3e-4, 1e-3, 1e-4; the tests assert ratio <= 8"]
    worst, per = (0.0, ""), {}
    for case in T.CASES:
        for max_grad_norm in (0.5, 0.0):
            for label, name, e_dev, e_np, bound, ratio in T.three_steps_case(case, max_grad_norm):
                kind = name.split(".")[0]
                worst = max(worst, (ratio, f"{label} {name}"))
                per[(label, kind)] = max(per.get((label, kind), (-1.0,)), (ratio, name, e_dev, e_np))
    for (label, kind), (ratio, name, e_dev, e_np) in per.items():
        lines.append(f"{label} {kind} {name} {e_dev:.3e} {e_np:.3e} {ratio:.2f}")
    lines.append(f"worst_ratio {worst[0]:.2f} {worst[1]}")
    print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
