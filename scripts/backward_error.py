#!/usr/bin/env python3
"""Writes profiles/update/backward_error.txt: dockauv_policy_backward against its float64 statement, measured on one GPU with the
helpers of tests/test_gpu_backward.py (the same weights, rows, shapes and row counts as the tests).

  python scripts/backward_error.py [--out profiles/update/backward_error.txt]
  python scripts/backward_error.py --relu-rows          # CPU only: the relu rows each case drops, for the seeds of the tests

Per case and gradient tensor: the device's error and the error of the float32 NumPy restatement against float64 (max over the
tensor), once with np.tanh and once with the kernel's own tanh form in the restatement, and the ratio device / max(e32, floor / 8)
that the tests hold against 8 (floor: 4 ulp of max |g64|).
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def relu_rows(T):
    for shape in T.all_cases():
        if shape[3] != "relu":
            continue
        mlp = T.P().make_mlp(shape, seed=1)
        dropped = drawn = 0
        for n in T.ROW_COUNTS:
            _, a, b = T.draw_rows(mlp, n, 2 + n)
            dropped, drawn = dropped + a, drawn + b
        print(f"{T.shape_id(shape)}: {dropped} of {drawn} rows dropped ({100.0 * dropped / drawn:.2f} %)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "update", "backward_error.txt"))
    ap.add_argument("--relu-rows", action="store_true")
    args = ap.parse_args()
    from tests import test_gpu_backward as T
    if args.relu_rows:
        relu_rows(T)
        return
    import torch
    lines = ["# dockauv_policy_backward against float64 (scripts/backward_error.py on the helpers of tests/test_gpu_backward.py)",
             "# case tensor device_err numpy_f32_err(np.tanh) ratio numpy_f32_err(kernel tanh form) ratio; ratio = device_err /",
             "# max(e32, floor / 8), floor = 4 ulp of max |g64|; the tests assert ratio <= 8 with the restatement named by",
             f"# test_gpu_backward.TANH_FORM = {T.TANH_FORM!r}"]
    worst = {"libm": (0.0, ""), "kernel": (0.0, "")}
    big = [((20, (64, 64), 6, "tanh", "none"), T.ROWS_BEYOND_ONE_PASS), ((20, (64, 64), 1, "tanh", "none"), T.ROWS_BEYOND_ONE_PASS)]
    cases = [(s, n) for s in T.all_cases() for n in T.ROW_COUNTS] + big
    for shape, n_rows in cases:
        mlp = T.P().make_mlp(shape, seed=1)
        env = T.P().fan_env(shape[0], 6 if shape[2] == 1 else shape[2], 64)
        try:
            pol = T.device_policy(env, mlp)
            rows, _, _ = T.make_rows(torch, mlp, n_rows, seed=2 + n_rows)
            g = T.make_grad_out(torch, n_rows, shape[2], seed=5 + n_rows)
            got = [t.cpu().numpy() for t in T.run_backward(torch, env, pol, mlp, rows, g)]
            x32, g32 = rows[:, : shape[0]].cpu().numpy(), g.cpu().numpy()
        finally:
            env.close()
        label = f"{T.shape_id(shape)}_rows{n_rows}"
        ref = mlp.backward_reference(x32.astype(np.float64), g32.astype(np.float64))
        f32 = {form: T.backward_float32_numpy(mlp, x32, g32, form) for form in ("libm", "kernel")}
        for i, name in enumerate(T.names_of(mlp)):
            r = ref[i]
            e_dev = float(np.abs(got[i].astype(np.float64) - r).max())
            floor = 4.0 * float(np.spacing(np.float32(np.abs(r).max())))
            parts = []
            for form in ("libm", "kernel"):
                e_np = float(np.abs(f32[form][i].astype(np.float64) - r).max())
                ratio = e_dev / max(e_np, floor / 8.0)
                if ratio > worst[form][0]:
                    worst[form] = (ratio, f"{label} {name}")
                parts.append(f"{e_np:.3e} {ratio:.2f}")
            lines.append(f"{label} {name} {e_dev:.3e} {' '.join(parts)}")
            print(lines[-1], flush=True)
    for form in ("libm", "kernel"):
        lines.append(f"worst_ratio_{form} {worst[form][0]:.2f} {worst[form][1]}")
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
