#!/usr/bin/env python3
"""Writes profiles/sac/logp_error.txt: the error of the squashed-Gaussian actor's log-probability on the device against the
float64 statement fed the device's own normals, next to the error of a float32 NumPy evaluation of the same expressions, on the two
cases of tests/test_gpu_sac.py (default-initialised networks; the log_std head scaled so that some |x| reach about 8).  Needs an
MI355X.  Usage: python scripts/sac_error.py [--out profiles/sac/logp_error.txt]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sac", "logp_error.txt"))
    args = ap.parse_args()
    from tests import test_gpu_sac as T
    lines = ["# squashed-Gaussian actor, 20-64-64-6 ReLU, 4 096 rows, stochastic: max |log_prob - log_prob_f64| with the float64 statement",
             "# (SquashedGaussianMLP.forward_reference) fed the device's own normals; numpy_f32: SquashedGaussianMLP.forward_float32 on the",
             f"# same inputs.  The test asserts device <= 8 x numpy_f32 and device <= {T.LOGP_CAP:g}"]
    for name in ("default", "wide_std"):
        dev, f32, reach = T.logp_errors(name)
        lines += [f"{name}_device_err {dev:.4e}", f"{name}_numpy_f32_err {f32:.4e}", f"{name}_max_abs_x {reach:.3f}"]
        print("\n".join(lines[-3:]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("->", args.out)


if __name__ == "__main__":
    main()
