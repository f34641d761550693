"""GPU: the sphere-only step kernels (gym_dockauv_amd/csrc/dockauv_step.hip.inc: NOCAP; dockauv_device.h: nocap_shape) against the
full instantiation of the same handle state, bit for bit.

Shape: BASELINE config 3's -- BlueROV2, the 16-beam fan against 8 sphere slots, groups of 256 threads -- on 200 envs: three full
groups and a partial one of 8 lanes.  24 steps with in-kernel resets and max_timesteps = 5, so that every env resets four times
inside the run.  The sphere rows are written with set_field so that these cases stand side by side:
  * envs with 0, 3, 4, 5 and 8 open slots, and envs whose slot 2 has rad = 0 while slots 3..7 have rad > 0 (the list ends at
    2) -- in every group, by env index modulo 6;
  * group 1 (envs 64..127): every sphere some 900 m away -- no env of the group is near any sphere in any step;
  * group 2 (envs 128..191): the same, but env 130 stands 1.5 m in front of ONE sphere (slot 6), facing it: in step 0 exactly
    one env of the group is in reach of exactly one sphere and takes an active ray pass;
  * group 0 and the partial group 3 keep the scenario's own sphere shell (3..12 m around the goal: some in reach of a vehicle
    15 m out, some not), and in group 0 env 3 starts within safety + rad of its slot 7 (collision termination in step 0) and
    env 5 INSIDE its slot 4.

The full instantiation is selected by asking for the navigation errors (dockauv_step_io.nav) and also delivers the terminal
observations.  Compared as bits after EVERY step: the packed rows [obs | reward | done] and the fields state (float64 sum of the
float32 row and its low-order word), filtered input, current, goal, step counter, cumulative reward, episode counter and spheres;
for the TERM form the terminal observations as well.  The resident kernel runs the 24 steps as six dockauv_step_sequence calls of
four, the riding kernel as six lag-1 gather sequences of four on one rank; both are compared row by row for every step and on the
fields after every call.

That the sphere-only kernel is what ran is read from dockauv_step_uses_capsules: select_step, which answers the query, is the one
place that picks the kernel of a launch (tests/test_sphere_only_host.py pins its table on a CPU)."""
import copy
import ctypes as C

import numpy as np
import pytest

K = 24
N = 200
FAR = np.array([520.0, 510.0, 530.0])
COLLIDING, INSIDE, FACING = 3, 5, 130
HOWS = ["plain", "term", "resident", "ride"]


def _config():
    from gym_dockauv_amd.config.env_config import BASE_CONFIG
    cfg = copy.deepcopy(BASE_CONFIG)
    cfg["max_timesteps"] = 5
    cfg["vehicle"] = "BlueROV2"
    cfg["radar"].update(alpha=30 * np.pi / 180, beta=30 * np.pi / 180, ray_per_deg=10 * np.pi / 180)
    return cfg


def _open_slots(e):
    """how many slots of env e are open: 8, 0, 3, 4, 5 by index modulo 6; -2: eight radii > 0 but slot 2 has rad = 0"""
    if e in (COLLIDING, FACING):
        return 8
    if e == INSIDE:
        return 5
    return (8, 0, 3, 4, 5, -2)[e % 6]


def _fields(env):
    from gym_dockauv_amd import _capi
    return [_capi.F_STATE, _capi.F_U, _capi.F_CURRENT, _capi.F_GOAL, _capi.F_TSTEPS, _capi.F_CUM_REWARD, _capi.F_EPISODE, _capi.F_SPHERES]


def _snapshot(env):
    return {f: env.get_field(f).view(np.int64).copy() for f in _fields(env)}


def _make():
    from gym_dockauv_amd import _capi
    from gym_dockauv_amd.envs.batched import BatchedDocking3d
    env = BatchedDocking3d(_config(), num_envs=N, scenario="SphereDocking3d", precision="f32", reset_mode="device",
                           device_seed=11, rng="batched", threads_per_group=256)
    env._gen = np.random.default_rng(6)
    env.reset()
    assert env.max_capsules == 0 and env.max_spheres == 8
    sph = env.get_field(_capi.F_SPHERES).reshape(N, 8, 4)
    assert (sph[:, :, 3] > 0).all(), "the scenario's shell fills every slot"
    state = env.get_field(_capi.F_STATE)
    rs = np.random.RandomState(4)
    for e in range(64, 192):   # groups 1 and 2: nothing in reach, ever (resets put a vehicle 15 m from the origin)
        sph[e, :, 0:3] = FAR + rs.uniform(-40, 40, (8, 3))
    for e in range(N):
        k = _open_slots(e)
        if k == -2:
            sph[e, 2, 3] = 0.0
        else:
            sph[e, k:, 3] = -1.0
    # one env 1.5 m in front of one sphere (slot 6), facing it; one within safety + rad of its slot 7; one inside its slot 4
    state[FACING] = 0.0
    state[FACING, 0:3] = (5.0, 0.0, 0.0)
    sph[FACING, 6] = (7.5, 0.0, 0.0, 1.0)   # (1.5 m of water: the sphere fills the fan, so every block maximum sees it)
    state[COLLIDING] = 0.0
    state[COLLIDING, 0:3] = sph[COLLIDING, 7, 0:3] - np.array([sph[COLLIDING, 7, 3] + 0.05, 0.0, 0.0])
    state[INSIDE] = 0.0
    state[INSIDE, 0:3] = sph[INSIDE, 4, 0:3] + np.array([0.2 * sph[INSIDE, 4, 3], 0.0, 0.0])
    env.set_field(_capi.F_SPHERES, sph.reshape(N, 32))
    env.set_field(_capi.F_STATE, state)
    return env


def _run(env, how, steps=K):
    """`steps` steps on device pointers.  how: "full" (navigation errors and terminal observations asked for), "plain", "term",
    "resident", "ride".  Returns (rows int32 [steps][n][words], terminal observations int32 [steps][n][n_obs] or None, the fields
    after every step -- resident and ride: after every call of four steps)."""
    import torch
    from gym_dockauv_amd import _capi
    n = env.num_envs
    dev = torch.device("cuda", env.device)
    words = env.packed_row_words(True)
    acts = torch.as_tensor(np.random.RandomState(21).uniform(-1, 1, (steps, n, env.n_u)), dtype=torch.float32, device=dev)
    rows = torch.zeros((steps, n, words), dtype=torch.int32, device=dev)
    nav = torch.zeros((n, 4), dtype=torch.float32, device=dev)
    term = how in ("full", "term")
    tobs = torch.zeros((steps, n, env.n_observations), dtype=torch.float32, device=dev) if term else None
    stream = torch.cuda.current_stream().cuda_stream
    snaps = []
    if how == "ride":
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
                torch.cuda.synchronize()
                snaps.append(_snapshot(env))
        finally:
            st.close()
    elif how == "resident":
        env.set_sequence_resident(True)
        for k0 in range(0, steps, 4):
            ios = env.make_step_sequence([acts[k0 + i].data_ptr() for i in range(4)], [rows[k0 + i].data_ptr() for i in range(4)], packed=True)
            env.run_step_sequence(ios, stream=stream)
            torch.cuda.synchronize()
            snaps.append(_snapshot(env))
    else:
        for k in range(steps):
            io = _capi.StepIO()
            io.actions, io.obs = acts[k].data_ptr(), rows[k].data_ptr()
            io.pack_reward_done = env._pack_mode(True)
            io.nav = nav.data_ptr() if how == "full" else None
            io.terminal_obs = tobs[k].data_ptr() if term else None
            rc = env._lib.dockauv_step(env._handle, C.byref(io), C.c_void_p(stream or None))
            _capi.check(env._lib, env._handle, rc, "dockauv_step")
            torch.cuda.synchronize()
            snaps.append(_snapshot(env))
    env.synchronize()
    return rows.cpu().numpy(), (tobs.cpu().numpy().view(np.int32) if term else None), snaps


_REFERENCE = []


def _reference():
    """the full instantiation's run, computed once and left unchanged; the cases of the docstring are checked on it"""
    if not _REFERENCE:
        from gym_dockauv_amd import _capi
        env = _make()
        try:
            sph0 = env.get_field(_capi.F_SPHERES).reshape(N, 8, 4)
            rows, tobs, snaps = _run(env, "full")
            n_red = env.n_observations - 16
        finally:
            env.close()
        done = rows[:, :, -1].view(np.float32) > 0.5
        cells = rows[:, :, 16:16 + n_red].view(np.float32)
        assert np.isfinite(rows[:, :, -2].view(np.float32)).all()
        assert (done.sum(axis=0) >= 4).all(), "every env resets four times in 24 steps of max_timesteps = 5"
        # the slot patterns, in every group
        counts = np.array([_open_slots(e) for e in range(N)])
        for g0 in range(0, N, 64):
            assert set(counts[g0:min(g0 + 64, N)]) >= {0, 3, 4, 5, 8, -2}, f"group at env {g0}: a slot pattern is missing"
        special = np.flatnonzero(counts == -2)
        assert (sph0[special, 2, 3] == 0.0).all() and (sph0[special, 5, 3] > 0.0).all()
        # group 1: nothing in reach in any step; group 2: in step 0 env 130 alone, by one sphere alone
        assert (cells[:, 64:128][~done[:, 64:128]] == 1.0).all(), "group 1: a ray hit something"
        hit0 = (cells[0, 128:192] < 1.0).any(axis=1) & ~done[0, 128:192]
        assert hit0.sum() == 1 and hit0[FACING - 128], "group 2: exactly env 130 takes an active pass in step 0"
        d130 = np.linalg.norm(sph0[FACING, :, 0:3] - np.array([5.0, 0.0, 0.0]), axis=1) - sph0[FACING, :, 3]
        assert (d130 <= 10.0).sum() == 1 and d130[6] <= 10.0, "env 130 is in reach of slot 6 alone"
        # group 0: the collision and the env inside a sphere end in step 0
        assert done[0, COLLIDING] and done[0, INSIDE]
        for s in snaps:   # sphere rows are static
            assert (s[_capi.F_SPHERES] == snaps[0][_capi.F_SPHERES]).all()
        rows.setflags(write=False)
        tobs.setflags(write=False)
        _REFERENCE.append((rows, tobs, snaps))
    return _REFERENCE[0]


def _equal_rows(what, rows, ref_rows):
    diff = np.argwhere(rows != ref_rows)
    assert diff.size == 0, (f"{what}: {len(diff)} words differ, first at (step, env, word) {tuple(diff[0])}: "
                            f"{rows[tuple(diff[0])]:#x} != {ref_rows[tuple(diff[0])]:#x}")


def _equal_fields(what, snap, ref_snap):
    assert snap.keys() == ref_snap.keys()
    for f in snap:
        diff = np.argwhere(snap[f] != ref_snap[f])
        assert diff.size == 0, f"{what}: field {f}: {len(diff)} words differ, first at (env, column) {tuple(diff[0])}"


@pytest.mark.gpu
@pytest.mark.parametrize("how", HOWS)
def test_sphere_only_kernels_equal_the_full_instantiation_bit_for_bit(how):
    ref_rows, ref_tobs, ref_snaps = _reference()
    env = _make()
    try:
        assert env.threads_in_use == 256
        assert not env.step_uses_current and not env.step_uses_capsules, "a fresh config 3 handle steps with the sphere-only kernel"
        rows, tobs, snaps = _run(env, how)
        assert not env.step_uses_capsules
    finally:
        env.close()
    what = f"sphere-only {how}"
    _equal_rows(what, rows, ref_rows)
    if how == "term":
        _equal_rows(what + " terminal_obs", tobs, ref_tobs)
    if how in ("resident", "ride"):
        assert len(snaps) == K // 4
        for c, snap in enumerate(snaps):
            _equal_fields(what + f" after step {4 * c + 3}", snap, ref_snaps[4 * c + 3])
    else:
        for k in range(K):
            _equal_fields(what + f" after step {k}", snaps[k], ref_snaps[k])


@pytest.mark.gpu
def test_a_non_zero_current_switches_the_handle_to_the_general_kernel():
    """Three sphere-only steps, then one env gets a current: the query reports the general kernel (with the lean twin the whole
    sphere-only twin is lost) and five further product steps equal the full instantiation with that current, bit for bit."""
    from gym_dockauv_amd import _capi
    envs = [_make(), _make()]
    try:
        out = []
        for env, then in zip(envs, ("plain", "full")):
            if then == "plain":
                assert not env.step_uses_capsules
            head = _run(env, then, steps=3)
            cur = env.get_field(_capi.F_CURRENT, first=7, count=1)
            assert not cur.any()
            cur[0] = (0.3, 0.1, 0.6, 0.2, -0.4)   # V_c, V_min, V_max, alpha, beta
            env.set_field(_capi.F_CURRENT, cur, first=7)
            if then == "plain":
                assert env.step_uses_current and env.step_uses_capsules, "a non-zero current row takes the whole twin away"
            out.append((head, _run(env, then, steps=5)))
            if then == "plain":
                assert env.step_uses_capsules
        (head, tail), (ref_head, ref_tail) = out
        for part, (got, ref) in (("before", (head, ref_head)), ("after", (tail, ref_tail))):
            _equal_rows(f"{part} the write", got[0], ref[0])
            for k, (a, b) in enumerate(zip(got[2], ref[2])):
                _equal_fields(f"{part} the write, step {k}", a, b)
        assert tail[2][0][_capi.F_CURRENT].view(np.float64)[7, 0] != 0.0   # (the current is felt)
    finally:
        for env in envs:
            env.close()


@pytest.mark.gpu
def test_who_never_has_the_sphere_only_kernel():
    from gym_dockauv_amd.envs.batched import BatchedDocking3d

    def make(scenario, threads):
        env = BatchedDocking3d(_config(), num_envs=64, scenario=scenario, precision="f32", reset_mode="device", device_seed=11,
                               rng="batched", threads_per_group=threads)
        env._gen = np.random.default_rng(6)
        env.reset()
        return env
    for scenario, threads, why in (("CapsuleDocking3d", 256, "a handle with a capsule slot"), ("SimpleDocking3d", 256, "a handle without obstacles"),
                                   ("SphereDocking3d", 64, "one-wave groups")):
        env = make(scenario, threads)
        try:
            assert env.step_uses_capsules, why
        finally:
            env.close()
