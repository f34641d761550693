"""GPU: the kernels that fetch what their roles read behind the integrator from the packed tail part of the parameter block
(gym_dockauv_amd/csrc/dockauv_device.h: TailP; dockauv_step.hip.inc: tail_params_, request_tail_ / pin_tail_) against the full
instantiation of the same shape, which reads EnvP at the uses: 24 single launches with in-kernel resets on 66 envs (one full
group and a partial one) and on 130, packed rows and the state field compared as int32 -- bit for bit.

Every parameter that travels in TailP is off its default, so that a wrong slot cannot go unnoticed: the reward weights and the
five done weights, dist_goal_reached_tol, max_dist_from_goal, max_attitude, max_timesteps = 7 (every env resets several times),
radar max_dist 6 instead of 10.

The full instantiation is selected by asking for the navigation errors (dockauv_step_io.nav), on device pointers like the
product calls; it is also asked for the terminal observations, one buffer per step, and the TERM cases must deliver the same
rows for the envs that finish in a step and leave every other row alone.  Cases: BlueROV2 with the 16-beam fan and 8 spheres at
64 / 256 / 512 threads, the rows with terminal observations (TERM) and with bfloat16 observation columns, and the sensor-free
kernels at 64 / 128 / 256 threads.  Which of them fetch from TailP is a property of the build; the others
run here too and must agree just the same.  No LAUV or mixed kernel fetches from TailP.

The kernels that single launches of a small batch never select have cases of their own, same parameters, same reference (the
riding and the write-back kernel of 256 threads fetch from TailP; the resident kernels do not):
  resident  the 24 steps as one resident step sequence (step_seq_kernel) at 256 and 512 threads;
  ride      the 24 steps as six lag-1 gather sequences of four steps on one rank: the gather of a step rides in the next step's
            launch (step_ride_kernel, 256 threads), and the rows are read where the gathers delivered them;
  the write-back twin of the 256-thread ray kernel serves launches of more than one round of resident groups only
            (select_step: more than 262 144 envs): 262 144 + 66 envs, the smallest such batch with a partial last group, and 8
            launches instead of 24 -- with max_timesteps = 7 every env finishes and resets once in them, and what is compared
            grows with launches x envs."""
import copy
import ctypes as C

import numpy as np
import pytest

K = 24
SIZES = (66, 130)
FAN16, FREE = "SphereDocking3d", "SimpleCurrentDocking3d"
N_WB, K_WB = 262144 + 66, 8


def _config():
    from gym_dockauv_amd.config.env_config import BASE_CONFIG
    cfg = copy.deepcopy(BASE_CONFIG)
    cfg["radar"].update(alpha=30 * np.pi / 180, beta=30 * np.pi / 180, ray_per_deg=10 * np.pi / 180, max_dist=6)
    cfg["max_timesteps"] = 7
    cfg["dist_goal_reached_tol"] = 0.8
    cfg["max_dist_from_goal"] = 17.0
    cfg["max_attitude"] = 50 / 180 * np.pi
    cfg["reward_factors"].update(w_d=1.3, w_delta_psi=0.45, w_delta_theta=0.35, w_phi=0.25, w_theta=0.4, w_Thetadot=0.15,
                                 w_oa=0.3, w_goal=350.0, w_deltad_max=-210.0, w_Theta_max=-190.0, w_t_max=-90.0, w_col=-310.0)
    return cfg


def _run(scenario, n, threads, packed, full, term, how="single", steps=K):
    """`steps` launches on device pointers; returns (rows int32 [steps][n][words], state int32, finished envs, threads in use,
    terminal observations int32 [steps][n][n_obs] -- one buffer per step, zero where the step wrote nothing -- or None)"""
    import torch
    from gym_dockauv_amd import _capi
    from gym_dockauv_amd.envs.batched import BatchedDocking3d
    env = BatchedDocking3d(_config(), num_envs=n, scenario=scenario, precision="f32", reset_mode="device", device_seed=5,
                           rng="batched", threads_per_group=threads)
    try:
        env._gen = np.random.default_rng(4)
        if scenario == FAN16 and n > 1024:
            # (the scenario's sphere shells are drawn env by env on the host, 262 210 of them take 13 s: 1 024 shells, repeated)
            from gym_dockauv_amd import scenarios
            shells = np.stack([scenarios.sphere_shell(np.random.RandomState(10_000 + i), np.zeros(3), env.max_spheres).reshape(-1)
                               for i in range(1024)])
            env._static_spheres = np.resize(shells, (n, shells.shape[1]))
        env.reset()
        dev = torch.device("cuda", env.device)
        words = env.packed_row_words(packed)
        acts = torch.as_tensor(np.random.RandomState(9).uniform(-1, 1, (steps, n, env.n_u)), dtype=torch.float32, device=dev)
        rows = torch.zeros((steps, n, words), dtype=torch.int32, device=dev)
        nav = torch.zeros((n, 4), dtype=torch.float32, device=dev)
        tobs = torch.zeros((steps, n, env.n_observations), dtype=torch.float32, device=dev) if term else None
        stream = torch.cuda.current_stream().cuda_stream
        if how == "single":
            for k in range(steps):
                io = _capi.StepIO()
                io.actions, io.obs = acts[k].data_ptr(), rows[k].data_ptr()
                io.pack_reward_done = env._pack_mode(packed)
                io.nav = nav.data_ptr() if full else None
                io.terminal_obs = tobs[k].data_ptr() if term else None
                rc = env._lib.dockauv_step(env._handle, C.byref(io), C.c_void_p(stream or None))
                _capi.check(env._lib, env._handle, rc, "dockauv_step")
        elif how == "resident":
            assert not full and not term
            env.set_sequence_resident(True)
            ios = env.make_step_sequence([acts[k].data_ptr() for k in range(steps)], [rows[k].data_ptr() for k in range(steps)],
                                         packed=packed)
            env.run_step_sequence(ios, stream=stream)
        else:
            assert how == "ride" and not full and not term and packed is True and steps % 4 == 0
            from gym_dockauv_amd.parallel import P2PShardedStepper
            st = P2PShardedStepper(n, words, lambda a, o: None, dev, world=1, rank=0)
            try:
                for k0 in range(0, steps, 4):
                    seq = st.make_sequence(env, [acts[k0 + i].data_ptr() for i in range(4)])
                    st.run_sequence(env, seq, two_streams=False, ride=True)
                    torch.cuda.synchronize()
                    assert st._ride_ok and st.gather.timed_out() == 0
                    for i in range(4):   # (four gather buffers in turn, from step 0)
                        rows[k0 + i].copy_(st.bufs[i].view(torch.int32))
            finally:
                st.close()
        torch.cuda.synchronize()
        env.synchronize()
        r = rows.cpu().numpy()
        done = r[:, :, -1].view(np.float32) > 0.5
        t = tobs.cpu().numpy().view(np.int32) if term else None
        return r, env.state.astype(np.float32).view(np.int32).copy(), int(done.sum()), env.threads_in_use, t
    finally:
        env.close()


_REFERENCE = {}


def _reference(scenario, n, packed, steps=K, term=True):
    """the full instantiation's run, computed once per (scenario, batch, row format) and left unchanged"""
    key = (scenario, n, packed, steps)
    if key not in _REFERENCE:
        rows, state, n_done, _, tobs = _run(scenario, n, 0, packed, full=True, term=term, steps=steps)
        assert n_done >= (steps // 8) * n, "every env must reset, several times in 24 steps"
        f = rows[:, :, -2].view(np.float32)
        assert np.isfinite(f).all() and np.isfinite(state.view(np.float32)).all()
        if term:   # (a terminal row is written exactly where the step's `done` column is set: sin and cos of the heading
            done = rows[:, :, -1].view(np.float32) > 0.5   # error are two of its columns, never both zero)
            assert np.array_equal((tobs != 0).any(axis=2), done)
            tobs.setflags(write=False)
        rows.setflags(write=False)
        state.setflags(write=False)
        _REFERENCE[key] = (rows, state, tobs)
    return _REFERENCE[key]


def _compare(what, got, ref):
    rows, state, n_done, _, tobs = got
    ref_rows, ref_state, ref_tobs = ref
    assert n_done >= (rows.shape[0] // 8) * rows.shape[1]
    diff = np.argwhere(rows != ref_rows)
    assert diff.size == 0, (f"{what}: {len(diff)} words differ, first at (step, env, word) {tuple(diff[0])}: "
                            f"{rows[tuple(diff[0])]:#x} != {ref_rows[tuple(diff[0])]:#x}")
    assert np.array_equal(state, ref_state), f"{what}: state: {int((state != ref_state).sum())} words differ"
    if tobs is not None:
        diff = np.argwhere(tobs != ref_tobs)
        assert diff.size == 0, (f"{what}: terminal_obs: {len(diff)} words differ, first at (step, env, column) {tuple(diff[0])}: "
                                f"{tobs[tuple(diff[0])]:#x} != {ref_tobs[tuple(diff[0])]:#x}")


CASES = [(FAN16, 64, True, False), (FAN16, 256, True, False), (FAN16, 512, True, False),
         (FAN16, 256, True, True), (FAN16, 512, True, True),
         (FAN16, 256, "bf16", False), (FAN16, 512, "bf16", False),
         (FREE, 64, True, False), (FREE, 128, True, False), (FREE, 256, True, False), (FREE, 256, True, True)]


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("scenario,threads,packed,term", CASES)
def test_product_rows_equal_the_full_instantiation_bit_for_bit(scenario, threads, packed, term, n):
    got = _run(scenario, n, threads, packed, full=False, term=term)
    assert got[3] == threads
    _compare(f"{scenario} threads {threads} packed {packed} term {term} envs {n}", got, _reference(scenario, n, packed))


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("how,threads,packed", [("resident", 256, True), ("resident", 512, True), ("resident", 512, "bf16"),
                                                ("ride", 256, True)])
def test_resident_and_riding_kernels_equal_the_full_instantiation_bit_for_bit(how, threads, packed, n):
    got = _run(FAN16, n, threads, packed, full=False, term=False, how=how)
    assert got[3] == threads
    _compare(f"{how} threads {threads} packed {packed} envs {n}", got, _reference(FAN16, n, packed))


@pytest.mark.gpu
def test_write_back_kernel_equals_the_full_instantiation_bit_for_bit():
    got = _run(FAN16, N_WB, 256, True, full=False, term=False, steps=K_WB)
    assert got[3] == 256
    _compare(f"write-back, {N_WB} envs", got, _reference(FAN16, N_WB, True, steps=K_WB, term=False))
