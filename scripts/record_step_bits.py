#!/usr/bin/env python3
"""Record what the float32 step kernels compute, bit for bit: tests/golden/step_bits_<case>.npz.

usage: [DOCKAUV_LIB=.../libdockauv_<variant>.so] python scripts/record_step_bits.py [--out DIR] [case ...]

Each case runs STEPS single launches at 66 envs (one full group of 64 and a partial group of two) with a seeded action
ring, in-kernel episode resets (reset_mode="device", fixed device_seed) and max_timesteps = MAX_T, so that every env is
reset inside the window.  Stored as int32 views: the state field and the packed rows after the step that follows the
reset of the envs that ran into max_timesteps (step MAX_T + 1) and after the last step.  The fixtures pin the output of one
toolchain (compiler and flags of gym_dockauv_amd/csrc/build.py): record them with the library of the commit whose results
are to be kept, before a change that must not alter them.  tests/test_gpu_step_bits.py replays them."""
import argparse
import copy
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

N_ENVS, STEPS, MAX_T, RING = 66, 24, 10, 8
# name: (bench.py config id, threads per group)
CASES = {
    "bluerov_fan16_sph8_256": (3, 256), "bluerov_fan16_sph8_64": (3, 64),
    "lauv_rays63_cap5_512": (4, 512), "lauv_rays63_cap5_256": (4, 256), "lauv_rays63_cap5_64": (4, 64),
    "mixed_current_256": (5, 256),
    "bluerov_simple_256": (2, 256), "bluerov_simple_128": (2, 128), "bluerov_simple_64": (2, 64),
}


def golden_path(case: str, folder: str = "") -> str:
    return os.path.join(folder or os.path.join(ROOT, "tests", "golden"), f"step_bits_{case}.npz")


def run_case(case: str) -> dict:
    """The arrays of one case from the library in use (DOCKAUV_LIB or the in-tree build), on cuda:0."""
    import torch
    import bench
    from gym_dockauv_amd.envs.batched import BatchedDocking3d
    config_id, threads = CASES[case]
    wl = bench.workload(config_id, N_ENVS)
    cfg = copy.deepcopy(wl["cfg"])
    cfg["max_timesteps"] = MAX_T
    env = BatchedDocking3d(cfg, num_envs=N_ENVS, scenario=wl["scenario"], precision="f32", reset_mode="device", device_seed=99,
                           rng="batched", vehicles=wl["vehicles"], threads_per_group=threads)
    try:
        assert env.threads_in_use == threads, (case, env.threads_in_use)
        env._gen = np.random.default_rng(3)
        env.reset()
        dev = torch.device("cuda", 0)
        ring = np.random.default_rng(5).uniform(-1.0, 1.0, (RING, N_ENVS, env.n_u)).astype(np.float32)
        acts = torch.from_numpy(ring).to(dev)
        rows = torch.zeros((N_ENVS, env.packed_row_words(True)), device=dev, dtype=torch.float32)
        stream = torch.cuda.current_stream().cuda_stream
        out = {}
        for k in range(STEPS):
            env.step_device(acts[k % RING].data_ptr(), rows.data_ptr(), stream=stream, packed=True)
            if k in (MAX_T, STEPS - 1):
                torch.cuda.synchronize()
                env.synchronize()
                tag = "after_reset" if k == MAX_T else "last"
                out[f"rows_{tag}"] = rows.cpu().numpy().view(np.int32).copy()
                out[f"state_{tag}"] = np.ascontiguousarray(env.state, dtype=np.float32).view(np.int32).copy()
        episodes = env.get_field(9)
        assert int(episodes.min()) >= 1, f"{case}: every env must have been reset inside the window"
        return out
    finally:
        env.close()


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default="", help="folder of the .npz files (default: tests/golden)")
    ap.add_argument("cases", nargs="*", default=[])
    args = ap.parse_args()
    if args.out:
        os.makedirs(args.out, exist_ok=True)
    for case in args.cases or sorted(CASES):
        arrays = run_case(case)
        path = golden_path(case, args.out)
        np.savez_compressed(path, **arrays)
        print(f"{case}: {os.path.getsize(path)} bytes -> {path}", flush=True)


if __name__ == "__main__":
    main()
