"""The replay buffer on a real MI355X (include/dockauv.h: dockauv_replay_*; TorchDocking3d.make_replay_buffer, rb.rollout / rb.collect,
step with replay=): synthetic pushes and samples against the NumPy statements bit for bit (gym_dockauv_amd/replay.py:
replay_push_reference, replay_indices_reference), refusals on a live handle, real trajectories through the env whose ring must be
the transitions rebuilt on the host, and a checkpoint.

Shapes: N = 200 envs (no multiple of 64, nor of the 16 records of a group: the last group is partial), the sensor-free scenario
of config 2 and the sphere scenario of config 3 (their record widths are printed), buffer_size = 5 * 200 + 17, i.e. capacity_steps
= 5, so that pushes of K = 3, 3, 1, 5 wrap inside a push and fill the ring in one.  Every env is closed in `finally`."""
import copy
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 200
CAP = 5
BUFFER_SIZE = CAP * N + 17
VARIANTS = ["bluerov2-sensor-free", "sphere-16-beam"]
PUSH_SEED = 20240611


def P():
    from tests import test_gpu_policy
    return test_gpu_policy


def make_env(variant, max_timesteps=4):
    import bench
    from gym_dockauv_amd.envs.torch_env import TorchDocking3d
    cid = {"bluerov2-sensor-free": 2, "sphere-16-beam": 3}[variant]
    wl = bench.workload(cid, N)
    cfg = copy.deepcopy(wl["cfg"])
    cfg["max_timesteps"] = max_timesteps
    env = TorchDocking3d(cfg, num_envs=N, scenario=wl["scenario"], device_seed=9)
    env.batch._gen = np.random.default_rng(5)
    env.reset()
    return env


def u32(x):
    """the bits of a float32 array or tensor, on the host"""
    if not isinstance(x, np.ndarray):
        x = x.detach().cpu().numpy()
    return np.ascontiguousarray(x).view(np.uint32) if x.dtype == np.float32 else x


def synthetic_block(rng, K, n_obs, n_u):
    """random float32 contents with -0.0 sprinkled in, dones with p = 0.3, ep_outcome uniform in 0 .. 4 where done and 255
    elsewhere, terminal observations NaN where not done"""
    rows = rng.standard_normal((K, N, n_obs + 2)).astype(np.float32)
    rows[rng.random(rows.shape) < 0.02] = np.float32(-0.0)
    done = rng.random((K, N)) < 0.3
    rows[:, :, n_obs + 1] = done
    acts = rng.uniform(-1, 1, (K, N, n_u)).astype(np.float32)
    acts[rng.random(acts.shape) < 0.02] = np.float32(-0.0)
    term = np.where(done[:, :, None], rng.standard_normal((K, N, n_obs)), np.nan).astype(np.float32)
    out = np.where(done, rng.integers(0, 5, (K, N)), 255).astype(np.uint8)
    # the properties the test stands on, asserted on its inputs
    assert (done & (out == 3)).any() and (done & (out != 3)).any() and (~done).any()
    assert np.isnan(term[~done]).all() and (out[~done] == 255).all() and np.signbit(rows[rows == 0]).any()
    return rows, acts, term, out


def push_blocks(env, rb, rng, with_outcome=True, ks=(3, 3, 1, 5), check=None):
    """the pushes of test 1 on the device and in NumPy; returns the reference (storage, carry, pos, size) and the last block"""
    import torch
    from gym_dockauv_amd.replay import record_floats, replay_push_reference
    n_obs, n_u = env.n_obs, env.n_u
    ref = (np.zeros((CAP, N, record_floats(n_obs, n_u)), np.float32), np.zeros((N, n_obs), np.float32), 0, 0)
    dev = lambda x: None if x is None else torch.from_numpy(x).cuda()
    for i, K in enumerate(ks):
        rows, acts, term, out = synthetic_block(rng, K, n_obs, n_u)
        rows_in = rng.standard_normal((N, n_obs + 2)).astype(np.float32) if i == 0 else None
        if not with_outcome:
            out = None
        rb.push(dev(rows), dev(acts), dev(term), ep_outcome=dev(out), rows_in=dev(rows_in))
        ref = replay_push_reference(*ref, rows_in, rows, acts, term, out)
        if check is not None:
            check(i, ref)
    return ref


@pytest.mark.parametrize("variant", VARIANTS)
def test_push_is_the_reference_bit_for_bit(variant):
    """K = 3 (explicit rows_in), 3 (a wrap inside the push), 1, 5 (= capacity) through the carry: after every push the ring, the
    carry, pos and size are replay_push_reference's, compared as uint32 -- so no NaN of a terminal observation that was not done,
    and no 255 of an outcome that was not done, reached the ring."""
    import torch
    from gym_dockauv_amd.replay import record_floats
    env = make_env(variant)
    try:
        rb = env.make_replay_buffer(BUFFER_SIZE, seed=1)
        R = record_floats(env.n_obs, env.n_u)
        print(f"{variant}: n_obs {env.n_obs}, n_u {env.n_u}, record_floats {R} ({2 * env.n_obs + env.n_u + 3} used)")
        assert rb.capacity_steps == CAP and rb.record_floats == R and tuple(rb.storage.shape) == (CAP, N, R)
        assert (rb.pos, rb.size, rb.draws) == (0, 0, 0)
        torch.cuda.synchronize()
        assert not u32(rb.storage).any(), "the ring is not zero-filled at create"
        want_pos, want_size = [3, 1, 2, 2], [3, 5, 5, 5]

        def check(i, ref):
            torch.cuda.synchronize()
            assert (rb.pos, rb.size) == (ref[2], ref[3]) == (want_pos[i], want_size[i]), (i, rb.pos, rb.size)
            got = u32(rb.storage)
            bad = np.argwhere(got != u32(ref[0]))
            assert bad.size == 0, f"push {i}: {len(bad)} ring words differ, first at (slot, env, word) {bad[0].tolist()}"
            assert np.array_equal(u32(rb.carry), u32(ref[1])), f"push {i}: the carry differs"
            assert not np.isnan(got.view(np.float32)).any()

        push_blocks(env, rb, np.random.default_rng(PUSH_SEED), check=check)
    finally:
        env.close()


@pytest.mark.parametrize("variant", VARIANTS)
def test_sample_is_the_reference_bit_for_bit(variant):
    """At size = 3 and size = 5, B = 1 and 333, G = 1 and 3: the indices are replay_indices_reference's, every output is the
    field of the reference ring at them, dones = done * (1 - timeout), draws advances by G, two G = 1 calls are one G = 2 call;
    a ring pushed without ep_outcome returns the raw done."""
    import torch
    from gym_dockauv_amd.replay import replay_indices_reference
    seed = 0xC0FFEE_0000_0007
    env = make_env(variant)
    try:
        n_obs, n_u = env.n_obs, env.n_u
        o2, o3 = 2 * n_obs, 2 * n_obs + n_u
        rb = env.make_replay_buffer(BUFFER_SIZE, seed=seed)
        raw = env.make_replay_buffer(BUFFER_SIZE, seed=seed, handle_timeout_termination=False)
        assert rb.monitor is not None and raw.monitor is None

        def check_samples(buf, ref_ring, size, B, G, raw_done):
            d0 = buf.draws
            s = buf.sample(B, G, want_index=True)
            torch.cuda.synchronize()
            assert buf.draws == d0 + G
            idx = buf.index.cpu().numpy().reshape(G, B)
            want = replay_indices_reference(seed, d0, B, G, size, N)
            assert np.array_equal(idx, want), (B, G, size)
            rec = ref_ring.reshape(-1, ref_ring.shape[-1])[want]                    # [G, B, R]
            lead = (G, B) if G > 1 else (B,)
            assert tuple(s.observations.shape) == lead + (n_obs,) and tuple(s.actions.shape) == lead + (n_u,)
            assert tuple(s.dones.shape) == lead + (1,) and tuple(s.rewards.shape) == lead + (1,)
            g = lambda t: u32(t).reshape((G, B) + tuple(t.shape[len(lead):]))
            assert np.array_equal(g(s.observations), u32(rec[..., :n_obs]))
            assert np.array_equal(g(s.next_observations), u32(rec[..., n_obs:o2]))
            assert np.array_equal(g(s.actions), u32(rec[..., o2:o3]))
            assert np.array_equal(g(s.rewards)[..., 0], u32(rec[..., o3]))
            done, timeout = rec[..., o3 + 1], rec[..., o3 + 2]
            want_done = done if raw_done else done * (np.float32(1) - timeout)
            assert np.array_equal(g(s.dones)[..., 0], u32(want_done.astype(np.float32)))
            assert set(np.unique(s.dones.cpu().numpy()).tolist()) <= {0.0, 1.0}
            return done, timeout

        for buf, with_outcome in ((rb, True), (raw, False)):
            seen_timeout = 0
            stage = {}

            def at_stage(i, ref, buf=buf, with_outcome=with_outcome, stage=stage):
                if i not in (0, 3):         # size 3 (partly filled: slots 3, 4 still zero) and size 5
                    return
                size = ref[3]
                assert size == (3, None, None, 5)[i]
                for B in (1, 333):
                    for G in (1, 3):
                        done, timeout = check_samples(buf, ref[0], size, B, G, raw_done=not with_outcome)
                        stage["timeouts"] = stage.get("timeouts", 0) + int((done * timeout).sum())
                # two G = 1 calls are one G = 2 call from the same draws
                pos, size_, d0 = env.batch.replay_counts(buf.handle)
                a = [t.clone() for t in buf.sample(333, 1)]
                b = [t.clone() for t in buf.sample(333, 1)]
                env.batch.replay_set_counts(buf.handle, pos, size_, d0)
                both = [t.clone() for t in buf.sample(333, 2)]
                torch.cuda.synchronize()
                assert buf.draws == d0 + 2
                for x, y, z in zip(a, b, both):
                    assert np.array_equal(u32(x), u32(z[0])) and np.array_equal(u32(y), u32(z[1]))
                assert not np.array_equal(u32(a[0]), u32(b[0]))

            push_blocks(env, buf, np.random.default_rng(PUSH_SEED + 1), with_outcome=with_outcome, check=at_stage)
            seen_timeout = stage.get("timeouts", 0)
            if with_outcome:
                assert seen_timeout > 0, "no sampled transition was a time limit: dones = done * (1 - timeout) went untested"
            else:
                assert seen_timeout == 0
    finally:
        env.close()


def test_refusals_on_a_live_handle():
    """each -1 before any device call, the message naming the field, the ring and the counts unchanged"""
    import torch
    from gym_dockauv_amd import _capi
    env = make_env(VARIANTS[0])
    other = make_env(VARIANTS[0])
    try:
        n_obs, n_u = env.n_obs, env.n_u
        rb = env.make_replay_buffer(BUFFER_SIZE, seed=3, handle_timeout_termination=False)
        lib, h = env.batch._lib, env.batch._handle
        z = lambda *shape: torch.zeros(shape, device="cuda", dtype=torch.float32)

        def refused(call, needle):
            with pytest.raises(_capi.DockAUVError) as ei:
                call()
            assert "(-1)" in str(ei.value) and needle in str(ei.value), str(ei.value)

        def rc_refused(rc, handle, needle):
            msg = lib.dockauv_last_error(handle).decode()
            assert rc == -1 and needle in msg, (rc, msg)

        # sample while empty
        refused(lambda: rb.sample(8), "size")
        assert rb.draws == 0
        rows, acts, term = z(1, N, n_obs + 2), z(1, N, n_u), z(1, N, n_obs)
        rows[:, :, :n_obs] = 0.25
        rb.push(rows, acts, term, rows_in=rows[0])
        torch.cuda.synchronize()
        before = u32(rb.storage).copy()
        counts = env.batch.replay_counts(rb.handle)
        assert counts == (1, 1, 0) and before.any()

        pio = _capi.ReplayPushIO()
        pio.struct_size, pio.n_steps = C.sizeof(pio), 0
        pio.rows_out, pio.actions, pio.terminal_obs = rows.data_ptr(), acts.data_ptr(), term.data_ptr()
        rc_refused(lib.dockauv_replay_push(h, rb.handle.ptr, C.byref(pio), None), h, "n_steps")                  # K = 0
        big = (z(CAP + 1, N, n_obs + 2), z(CAP + 1, N, n_u), z(CAP + 1, N, n_obs))
        refused(lambda: rb.push(*big), "n_steps")                                                                # K = capacity + 1
        pio.n_steps, pio.struct_size = 1, C.sizeof(pio) - 8
        rc_refused(lib.dockauv_replay_push(h, rb.handle.ptr, C.byref(pio), None), h, "struct_size")
        sio = _capi.ReplaySampleIO()
        sio.struct_size, sio.n_batches, sio.batch_size = C.sizeof(sio) + 8, 1, 1
        rc_refused(lib.dockauv_replay_sample(h, rb.handle.ptr, C.byref(sio), None), h, "struct_size")
        refused(lambda: rb.push(rows, acts, None), "terminal_obs")                                               # NULL terminal_obs
        rb_other = other.make_replay_buffer(BUFFER_SIZE, seed=3, handle_timeout_termination=False)
        pio.struct_size = C.sizeof(pio)
        rc_refused(lib.dockauv_replay_push(h, rb_other.handle.ptr, C.byref(pio), None), h, "another handle")
        rc_refused(lib.dockauv_replay_sync(h, rb_other.handle.ptr, C.c_void_p(rows.data_ptr()), None), h, "another handle")
        refused(lambda: env.batch.replay_set_counts(rb.handle, CAP, 1, 0), "pos")
        refused(lambda: env.batch.replay_set_counts(rb.handle, 0, CAP + 1, 0), "size")
        sio.struct_size, sio.batch_size = C.sizeof(sio), 0
        rc_refused(lib.dockauv_replay_sample(h, rb.handle.ptr, C.byref(sio), None), h, "batch_size")
        with pytest.raises(ValueError):
            rb.sample(0)
        with pytest.raises(ValueError):
            rb.rollout(None, CAP + 1)

        torch.cuda.synchronize()
        assert env.batch.replay_counts(rb.handle) == counts and env.batch.replay_counts(rb_other.handle) == (0, 0, 0)
        assert np.array_equal(u32(rb.storage), before) and not u32(rb_other.storage).any()
        # a float64 handle and a handle without auto-reset get no buffer
        import bench
        from gym_dockauv_amd.envs.batched import BatchedDocking3d
        wl = bench.workload(2, 64)
        for kw, needle in ((dict(precision="f64"), "DOCKAUV_F64"), (dict(precision="f32", reset_mode="none"), "RESET_NONE")):
            b = BatchedDocking3d(copy.deepcopy(wl["cfg"]), num_envs=64, scenario=wl["scenario"], device=0, rng="batched", **kw)
            try:
                with pytest.raises(_capi.DockAUVError) as ei:
                    b.make_replay(1000)
                assert "(-1)" in str(ei.value) and needle in str(ei.value), str(ei.value)
            finally:
                b.close()
    finally:
        env.close()
        other.close()


@pytest.mark.parametrize("variant", VARIANTS)
def test_through_the_env(variant):
    """max_timesteps = 4: every env hits the time limit on its fifth step.  rb.rollout(7, stochastic) twice (the second
    through the carry), then three step(replay=rb); after each call the ring is the transitions rebuilt in NumPy from a clone of
    the observation before the call, the returned obs / actions / reward / done, the terminal observations and the monitor
    reference's outcome.  A push takes at most capacity_steps steps, so this buffer has 12 step slots for the 17 steps (the
    second rollout wraps).  The closed-loop call is spelled rb.rollout: tests/test_eval_host.py pins the
    parameter list of TorchDocking3d.rollout, so the env's own method takes no new keyword.  A twin env with the same seeds and no replay buffer returns the same bits."""
    import torch
    from gym_dockauv_amd import _capi
    from gym_dockauv_amd.monitor import episode_scan_reference
    from gym_dockauv_amd.replay import record_floats, replay_push_reference
    cap, K = 12, 7
    env, twin = make_env(variant), make_env(variant)
    try:
        n_obs, n_u = env.n_obs, env.n_u
        mk = lambda e: e.make_policy(P().make_mlp((n_obs, (64, 64), n_u, "tanh", "none"), seed=6, log_std=np.full(n_u, -0.5)), seed=3)
        pol, t_pol = mk(env), mk(twin)
        rb = env.make_replay_buffer(cap * N, seed=5)
        assert rb.capacity_steps == cap
        ref = (np.zeros((cap, N, record_floats(n_obs, n_u)), np.float32), None, 0, 0)
        prev = env._packed[env._i % len(env._packed)][:, :n_obs].clone()      # the reset observation
        gen = torch.Generator(device="cuda")
        gen.manual_seed(17)
        want_pos, want_size = [7, 2, 3, 4, 5], [7, 12, 12, 12, 12]
        for call in range(5):
            c_len = env.batch.get_field(_capi.F_TSTEPS).reshape(-1).astype(np.int32)
            if call < 2:
                obs, acts, reward, done = rb.rollout(pol, K, stochastic=True)
                t_out = twin.rollout(t_pol, K, stochastic=True)
                term = env.rollout_terminal_observation
            else:
                a = (torch.rand((N, n_u), device="cuda", generator=gen) * 2 - 1).contiguous()
                obs, reward, done = (t.unsqueeze(0) for t in env.step(a, replay=rb))
                acts = a.unsqueeze(0)
                t_out = tuple(t.unsqueeze(0) for t in twin.step(a))
                t_out = (t_out[0], acts, t_out[1], t_out[2])
                term = env.terminal_observation.unsqueeze(0)
            torch.cuda.synchronize()
            for name, x, y in zip(("obs", "actions", "reward", "done"), (obs, acts, reward, done), t_out):
                assert np.array_equal(u32(x), u32(y)), f"call {call}: {name} differs from the env without a replay buffer"
            obs_h, rew_h, done_h = obs.cpu().numpy(), reward.cpu().numpy(), done.cpu().numpy()
            term_h = term.cpu().numpy()
            k_steps = obs_h.shape[0]
            rows = np.concatenate([obs_h, rew_h[..., None], done_h[..., None].astype(np.float32)], axis=2)
            scan = episode_scan_reference(rew_h, done_h, np.zeros(N, np.float32), c_len, 4, terminal_obs=term_h)
            ref = replay_push_reference(ref[0], prev.cpu().numpy(), ref[2], ref[3], None, rows, acts.cpu().numpy(), term_h,
                                        scan["ep_outcome"])
            assert (rb.pos, rb.size) == (ref[2], ref[3]) == (want_pos[call], want_size[call])
            bad = np.argwhere(u32(rb.storage) != u32(ref[0]))
            assert bad.size == 0, f"call {call}: {len(bad)} ring words differ, first at (slot, env, word) {bad[0].tolist()}"
            assert np.array_equal(u32(rb.carry), u32(ref[1]))
            assert rb.seen == env._gen and rb.monitor.seen == env._gen
            prev = obs[k_steps - 1].clone()
        o3 = 2 * n_obs + n_u
        ring = rb.storage.cpu().numpy()
        n_timeout, n_done = int(ring[..., o3 + 2].sum()), int(ring[..., o3 + 1].sum())
        print(f"{variant}: {n_done} dones in the ring, {n_timeout} of them time limits")
        assert n_timeout > 0, "no time limit was stored"
    finally:
        env.close()
        twin.close()


def test_checkpoint():
    """state_dict() into a fresh buffer of the same seed, then the same sample calls: identical outputs"""
    import torch
    env = make_env(VARIANTS[1])
    try:
        rb = env.make_replay_buffer(BUFFER_SIZE, seed=77)
        push_blocks(env, rb, np.random.default_rng(PUSH_SEED + 2), ks=(3, 3))
        rb.sample(64)
        sd = rb.state_dict()
        assert (sd["pos"], sd["size"], sd["draws"], sd["seed"]) == (1, 5, 1, 77)
        fresh = env.make_replay_buffer(BUFFER_SIZE, seed=77)
        fresh.load_state_dict(sd)
        assert (fresh.pos, fresh.size, fresh.draws) == (1, 5, 1)
        assert np.array_equal(u32(fresh.storage), u32(rb.storage)) and np.array_equal(u32(fresh.carry), u32(rb.carry))
        for B, G in ((1, 1), (333, 3), (64, 1)):
            a = [t.clone() for t in rb.sample(B, G, want_index=True)] + [rb.index.clone()]
            b = [t.clone() for t in fresh.sample(B, G, want_index=True)] + [fresh.index.clone()]
            torch.cuda.synchronize()
            for x, y in zip(a, b):
                assert np.array_equal(u32(x), u32(y))
        wrong = env.make_replay_buffer(BUFFER_SIZE, seed=78)
        with pytest.raises(ValueError):
            wrong.load_state_dict(sd)
    finally:
        env.close()
