#!/usr/bin/env python3
"""Writes profiles/policy/forward_error.txt: the policy kernel against its float64 statements, measured on one GPU with the
helpers of tests/test_gpu_policy.py (the same weights, rows, shapes and batch sizes as the tests).

  python scripts/policy_error.py [--out profiles/policy/forward_error.txt]

forward_*: max |a - a_f64| per shape and batch size (MLPPolicy.forward_reference); exploration_max_dev: max |z_dev - z_ref|
against MLPPolicy.normals_reference; scaled_*: the saturated case's device and float32-NumPy errors; closed_loop_*: dockauv_rollout
against the oracle driven by the float64 forward.  tests/test_gpu_policy.py reads exploration_max_dev as the base of its bound (4 x the
value, capped at 1e-4), so the file is to be rewritten only with a kernel whose figures have been looked at.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "policy", "forward_error.txt"))
    args = ap.parse_args()
    import test_gpu_policy as T

    lines = ["# policy kernel against float64 (scripts/policy_error.py on the helpers of tests/test_gpu_policy.py); key value",
             "# forward: max |a - a_f64|, weights U(+-1/sqrt(fan_in)), observations U(-1, 1), reward / done columns NaN; bound "
             f"{T.FORWARD_BOUND:g}"]
    worst = 0.0
    for shape in T.SHAPES + [T.WIDE]:
        for n in (1000, 65536):
            err = T.forward_error(shape, n)
            worst = max(worst, err)
            lines.append(f"forward_{shape[0]}-{'-'.join(map(str, shape[1]))}-{shape[2]}_{shape[3]}_{shape[4]}_N{n} {err:.4e}")
            print(lines[-1], flush=True)
    lines.append(f"forward_max_abs_err {worst:.4e}")
    dev = T.exploration_deviation()
    lines += ["# exploration: max |z_dev - z_ref| over 65 536 x 6 draws, t in {0, 1, 2^32 - 1}, env_id_offset in {0, 1 000 000};",
              f"# z_dev = a_stochastic - a_deterministic with log_std = 0; the test asserts 4 x this value, capped at {T.EXPLORATION_CAP:g}",
              f"exploration_max_dev {dev:.4e}"]
    lines += ["# saturated tanh units: SCALED = 36-128-128-3 tanh actor, every weight and bias x w, observations x x, 1 000 rows; device and",
              "# float32-NumPy error against float64 (max |a - a_f64|) and the largest |a_f64|; the test asserts device <= 8 x NumPy"]
    for w, x in ((4, 10), (16, 100)):
        dev_err, np_err, amax = T.scaled_errors(w, x)
        lines += [f"scaled_x{w}_obs_x{x}_device_err {dev_err:.4e}", f"scaled_x{w}_obs_x{x}_numpy_f32_err {np_err:.4e}",
                  f"scaled_x{w}_obs_x{x}_max_abs_a {amax:.3f}"]
        print("\n".join(lines[-3:]), flush=True)
    obs_dev, rew_dev, done_equal, n_done = T.closed_loop_vs_oracle()
    lines += ["# closed loop: dockauv_rollout of a 36-64-64-6 tanh actor, 48 envs of SimpleCurrentDocking3d x 14 steps, against OracleEnv driven",
              "# by the float64 forward; max |obs - obs_oracle| (bound helpers.TOL f32 obs = 1e-5), max reward deviation relative to max(1, |r|)",
              f"closed_loop_max_obs_dev {obs_dev:.4e}", f"closed_loop_max_reward_dev {rew_dev:.4e}",
              f"closed_loop_done_equal {int(done_equal)}", f"closed_loop_oracle_episodes_ended {n_done}"]
    print("\n".join(lines[-4:]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(f"forward_max_abs_err {worst:.4e}  exploration_max_dev {dev:.4e}  -> {args.out}")


if __name__ == "__main__":
    main()
