"""The episode monitor on a real MI355X (include/dockauv.h: dockauv_monitor_create / _sync / _scan / _carry;
TorchDocking3d.make_monitor, rollout / collect with monitor=): crafted reward / done / terminal-observation buffers through the C
ABI against the NumPy restatement bit for bit (gym_dockauv_amd/monitor.py: episode_scan_reference), real trajectories whose
carries must be the handle's own cumulative rewards and step counters, the explained variance against float64 NumPy, and
refusals on a live handle.  Shapes: N = 200 (three full 64-lane groups and a partial one), K = 19 (no multiple of the load chunk
of 8) and K = 1.  Every batch is closed in `finally`."""
import copy
import ctypes as C
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_SYN, K_SYN, MAX_T_SYN = 200, 19, 3
SENT_F, SENT_I, SENT_U = -7.0, -7, 99


def P():
    from tests import test_gpu_policy
    return test_gpu_policy


def stream_of(torch):
    return torch.cuda.current_stream().cuda_stream


def carries_of(torch, batch, mon, N):
    """host copies of the monitor's carries (after a synchronisation)"""
    from gym_dockauv_amd.parallel import _DevArray
    r_ptr, l_ptr = batch.monitor_carry(mon)
    torch.cuda.synchronize()
    return (torch.as_tensor(_DevArray(r_ptr, (N,), "<f4"), device="cuda").cpu().numpy().copy(),
            torch.as_tensor(_DevArray(l_ptr, (N,), "<i4"), device="cuda").cpu().numpy().copy())


def crafted(K, N, n_obs, seed, first_last=True):
    """reward U(-1, 1), done with p = 0.15 plus dones at k = 0 (envs 0-3) and k = K - 1 (envs 4-7) and none at all for env 8;
    observation columns NaN (never read).  Terminal rows: NaN except columns 0, 6, 7 where done, which cycle through goal (0),
    out of range (1), obs[6] = +1, -1, obs[7] = +1, -1 and two rows off every threshold (time limit or collision by length)."""
    rng = np.random.default_rng(seed)
    reward = rng.uniform(-1, 1, (K, N)).astype(np.float32)
    done = rng.random((K, N)) < 0.15
    if first_last:
        done[0, 0:4] = True
        done[K - 1, 4:8] = True
    done[:, 8] = False
    rows = np.full((K, N, n_obs + 2), np.nan, dtype=np.float32)
    rows[:, :, n_obs] = reward
    rows[:, :, n_obs + 1] = done
    term = np.full((K, N, n_obs), np.nan, dtype=np.float32)
    ks, es = np.nonzero(done)
    pat = (np.arange(ks.size) + seed) % 8
    t0 = np.where(pat == 0, 0.0, np.where(pat == 1, 1.0, 0.5)).astype(np.float32)
    t6 = np.where(pat == 2, 1.0, np.where(pat == 3, -1.0, 0.3)).astype(np.float32)
    t7 = np.where(pat == 4, 1.0, np.where(pat == 5, -1.0, -0.2)).astype(np.float32)
    term[ks, es, 0], term[ks, es, 6], term[ks, es, 7] = t0, t6, t7
    return rows, reward, done, term


def scan_guarded(torch, batch, mon, rows, term, K, N, values=None, returns=None):
    """dockauv_monitor_scan into sentinel-filled per-row buffers one row ([N]) longer than the outputs; returns host copies
    (stats, ep_return, ep_length, ep_outcome or None), the guard row checked"""
    d_rows = torch.from_numpy(rows).cuda()
    d_term = None if term is None else torch.from_numpy(term).cuda()
    stats = torch.full((16,), float("nan"), device="cuda", dtype=torch.float64)
    ep_ret = torch.full((K + 1, N), SENT_F, device="cuda")
    ep_len = torch.full((K + 1, N), SENT_I, device="cuda", dtype=torch.int32)
    ep_out = torch.full((K + 1, N), SENT_U, device="cuda", dtype=torch.uint8) if term is not None else None
    ptr = lambda t: 0 if t is None else t.data_ptr()
    batch.monitor_scan_device(mon, d_rows.data_ptr(), K, stats.data_ptr(), terminal_obs_ptr=ptr(d_term), values_ptr=ptr(values),
                              returns_ptr=ptr(returns), ep_return_ptr=ep_ret.data_ptr(), ep_length_ptr=ep_len.data_ptr(),
                              ep_outcome_ptr=ptr(ep_out), stream=stream_of(torch))
    torch.cuda.synchronize()
    assert bool((ep_ret[K] == SENT_F).all()) and bool((ep_len[K] == SENT_I).all()), "the kernel wrote behind the last step's row"
    assert ep_out is None or bool((ep_out[K] == SENT_U).all())
    return (stats.cpu().numpy(), ep_ret[:K].cpu().numpy(), ep_len[:K].cpu().numpy(), None if ep_out is None else ep_out[:K].cpu().numpy())


def check_against_restatement(got, ref, done, with_outcome, what):
    """per-row outputs bit for bit where done and untouched elsewhere; counts, length sums and min / max exact; the two float64
    sums within (n - 1) 2^-53 sum |x| of math.fsum (any summation order of n float64 terms stays inside it)"""
    stats, ep_ret, ep_len, ep_out = got
    assert np.array_equal(ep_ret[done].view(np.int32), ref["ep_return"][done].view(np.int32)), what
    assert np.array_equal(ep_len[done], ref["ep_length"][done]), what
    assert (ep_ret[~done] == SENT_F).all() and (ep_len[~done] == SENT_I).all(), f"{what}: a row that is not done was written"
    if with_outcome:
        assert np.array_equal(ep_out[done], ref["ep_outcome"][done]), what
        assert (ep_out[~done] == SENT_U).all(), f"{what}: a row that is not done was written"
    want = ref["stats"]
    n = int(done.sum())
    assert stats[0] == want[0] == n and stats[3] == want[3], (what, stats[:4], want[:4])
    rets = ref["ep_return"][done].astype(np.float64)
    for i, x in ((1, rets), (2, rets * rets)):
        bound = max(n - 1, 0) * 2.0 ** -53 * math.fsum(np.abs(x))
        err = abs(stats[i] - math.fsum(x))
        print(f"{what}: stats[{i}] {stats[i]!r}, fsum {math.fsum(x)!r}, |difference| {err:.3e}, bound {bound:.3e}")
        assert err <= bound, (what, i, err, bound)
    if n:
        assert np.array_equal(stats[4:8], want[4:8]), (what, stats[4:8], want[4:8])
    else:
        assert np.isnan(stats[4:8]).all(), what
    assert np.array_equal(stats[8:14], want[8:14]), (what, stats[8:14], want[8:14])
    assert stats[15] == 0.0


def test_crafted_buffers_through_the_c_abi():
    """Three scans in a row on one monitor -- K = 19, K = 19, K = 1 -- so that episodes span both boundaries; every outcome, both
    signs of obs[6] and obs[7], a goal + time-limit coincidence, dones at k = 0 and k = K - 1, an env with no done.  A second
    monitor of the same handle repeats the first scan (identical stats bits), a third runs it without terminal observations."""
    import torch
    from gym_dockauv_amd.monitor import episode_scan_reference
    N, n_obs = N_SYN, 20
    env = P().env_for(n_obs, 6, N, max_timesteps=MAX_T_SYN)
    try:
        m1, m2, m3 = env.make_monitor(), env.make_monitor(), env.make_monitor()
        c_ret, c_len = carries_of(torch, env, m1, N)
        assert not c_ret.any() and not c_len.any()          # (a fresh handle after reset: the handle's own counters)
        seen_bits, seen_codes, first = set(), set(), None
        for i, K in enumerate((K_SYN, K_SYN, 1)):
            rows, reward, done, term = crafted(K, N, n_obs, seed=40 + i, first_last=K > 1)
            ref = episode_scan_reference(reward, done, c_ret, c_len, MAX_T_SYN, terminal_obs=term)
            got = scan_guarded(torch, env, m1, rows, term, K, N)
            check_against_restatement(got, ref, done, True, f"scan {i} (K = {K})")
            assert np.isnan(got[0][14]) and got[0][13] == done.sum()
            g_ret, g_len = carries_of(torch, env, m1, N)
            assert np.array_equal(g_ret.view(np.int32), ref["carry_return"].view(np.int32)) and np.array_equal(g_len, ref["carry_length"])
            if i == 0:
                first = (rows, reward, done, term, got, ref)
                assert done[0, 0:4].all() and done[K - 1, 4:8].all() and not done[:, 8].any()
                assert g_len[8] == K, "the env without a done carries all K steps"
            seen_bits |= set(ref["ep_bits"][done].tolist())
            seen_codes |= set(ref["ep_outcome"][done].tolist())
            t = term[done]
            if i == 0:
                assert {1.0, -1.0} <= set(t[:, 6].tolist()) and {1.0, -1.0} <= set(t[:, 7].tolist())
            c_ret, c_len = ref["carry_return"], ref["carry_length"]
        assert seen_codes == {0, 1, 2, 3, 4}, seen_codes
        assert 0b1001 in seen_bits, "no goal + time-limit coincidence among the crafted episodes"
        assert c_len.max() > 1, "no episode spans a scan boundary"
        # the same scan on a second monitor of the handle: identical bits
        rows, reward, done, term, got, ref = first
        again = scan_guarded(torch, env, m2, rows, term, K_SYN, N)
        assert np.array_equal(again[0].view(np.int64), got[0].view(np.int64)), "two scans of the same inputs differ in their stats bits"
        # without terminal observations: no outcome, the rest unchanged
        ref_nt = episode_scan_reference(reward, done, np.zeros(N, np.float32), np.zeros(N, np.int32), MAX_T_SYN)
        got_nt = scan_guarded(torch, env, m3, rows, None, K_SYN, N)
        check_against_restatement(got_nt, ref_nt, done, False, "without terminal_obs")
        assert not got_nt[0][8:14].any() and np.array_equal(got_nt[0][:8].view(np.int64), got[0][:8].view(np.int64))
        # nothing finished: NaN min / max
        quiet = np.zeros((2, N, n_obs + 2), dtype=np.float32)
        st = scan_guarded(torch, env, m3, quiet, None, 2, N)[0]
        assert st[0] == 0 and st[1] == 0 and st[3] == 0 and np.isnan(st[4:8]).all()
        # dockauv_monitor_sync: back to the handle's counters
        env.monitor_sync(m1, stream=stream_of(torch))
        z_ret, z_len = carries_of(torch, env, m1, N)
        assert not z_ret.any() and not z_len.any()
    finally:
        env.close()


def ev_numpy(values, returns):
    """SB3's explained_variance in float64 NumPy; the error term is the float32 difference the kernel reads"""
    K = returns.shape[0]
    y = returns.astype(np.float64).ravel()
    e = (returns - values[:K]).astype(np.float64).ravel()
    vy = np.var(y)
    return float("nan") if vy == 0 else 1.0 - np.var(e) / vy


@pytest.mark.parametrize("K", [1, K_SYN, 1501], ids=["K1", "K19", "K1501-every-group-loops"])
def test_explained_variance_against_float64(K):
    """K N = 200, 3 800 (15 groups) and 300 200 (all 256 groups, a lane's second chunk and second pass of the loop), relative
    1e-12; constant returns give NaN."""
    import torch
    N, n_obs = N_SYN, 20
    env = P().env_for(n_obs, 6, N)
    try:
        mon = env.make_monitor()
        rng = np.random.default_rng(K)
        values = rng.normal(0.5, 2.0, (K + 1, N)).astype(np.float32)
        returns = (0.7 * values[:K] + rng.normal(0.2, 1.0, (K, N))).astype(np.float32)
        rows = torch.zeros((K, N, n_obs + 2), device="cuda")
        stats = torch.zeros((16,), device="cuda", dtype=torch.float64)
        for ret in (returns, np.full((K, N), 2.5, dtype=np.float32)):
            d_val, d_ret = torch.from_numpy(values).cuda(), torch.from_numpy(ret).cuda()
            env.monitor_scan_device(mon, rows.data_ptr(), K, stats.data_ptr(), values_ptr=d_val.data_ptr(), returns_ptr=d_ret.data_ptr(),
                                    stream=stream_of(torch))
            torch.cuda.synchronize()
            got, want = float(stats[14]), ev_numpy(values, ret)
            print(f"explained variance K {K}: device {got!r}, float64 NumPy {want!r}")
            if math.isnan(want):
                assert math.isnan(got)
            else:
                assert abs(got - want) <= 1e-12 * abs(want), (got, want)
            assert float(stats[0]) == 0 and float(stats[13]) == 0
    finally:
        env.close()


def make_torch_env(variant, mlp_seed=6):
    import bench
    from gym_dockauv_amd.envs.torch_env import TorchDocking3d
    cid, N = {"bluerov2-sensor-free": (2, 200), "sphere-16-beam": (3, 130)}[variant]
    wl = bench.workload(cid, N)
    cfg = copy.deepcopy(wl["cfg"])
    cfg["max_timesteps"] = 12
    env = TorchDocking3d(cfg, num_envs=N, scenario=wl["scenario"], device_seed=9)
    env.batch._gen = np.random.default_rng(5)
    env.reset()
    actor = P().make_mlp((env.n_obs, (64, 64), env.n_u, "tanh", "none"), seed=mlp_seed, log_std=np.full(env.n_u, -0.5))
    critic = P().make_mlp((env.n_obs, (64, 64), 1, "tanh", "none"), seed=mlp_seed + 1)
    return env, env.make_policy(actor, seed=3), env.make_value(critic)


@pytest.mark.parametrize("variant", ["bluerov2-sensor-free", "sphere-16-beam"])
def test_real_trajectories(variant):
    """Two collect(K = 19, monitor=m) with three plain step() between them (the re-sync), max_timesteps = 12, a random 64-64
    actor; a twin env of the same seed runs the same calls without the keyword and must return the same bits."""
    import torch
    from gym_dockauv_amd import _capi
    from gym_dockauv_amd.monitor import episode_scan_reference
    K, gamma, lam = K_SYN, 0.99, 0.95
    env, pol, val = make_torch_env(variant)
    twin, t_pol, t_val = make_torch_env(variant)
    try:
        N = env.num_envs
        m = env.make_monitor()
        shadow = env.make_monitor()                       # a second monitor for the per-row outputs of the same rows
        gen = torch.Generator(device="cuda")
        n_time_limit = 0
        for it in range(2):
            if it == 1:
                gen.manual_seed(17)
                for _ in range(3):                          # steps the monitor does not see
                    a = (torch.rand((N, env.n_u), device="cuda", generator=gen) * 2 - 1).contiguous()
                    env.step(a)
                    twin.step(a)
            c_ret = env.batch.get_field(_capi.F_CUM_REWARD).reshape(-1).astype(np.float32)
            c_len = env.batch.get_field(_capi.F_TSTEPS).reshape(-1).astype(np.int32)
            if it == 1:
                assert c_len.max() > 0
            shadow.sync()
            c = env.collect(pol, val, K, gamma, lam, monitor=m)
            ct = twin.collect(t_pol, t_val, K, gamma, lam)
            rows = env._collect_bufs[K]["rows"][1:]
            term = env.rollout_terminal_observation
            assert term is not None and m.stats is not None
            st_s, ep_ret, ep_len, ep_out = shadow.scan(rows, terminal_obs=term, values=c.values, returns=c.returns, per_row=True)
            torch.cuda.synchronize()
            for name, x, y in zip(c._fields, c, ct):
                assert torch.equal(x.contiguous().view(torch.int32) if x.dtype == torch.float32 else x,
                                   y.contiguous().view(torch.int32) if y.dtype == torch.float32 else y), f"collect {it}: {name} differs from the env without a monitor"
            stats = m.stats.cpu().numpy()
            assert np.array_equal(stats.view(np.int64), st_s.cpu().numpy().view(np.int64)), "collect's scan and the same scan by hand differ"
            done = c.done.cpu().numpy()
            reward = c.reward.cpu().numpy()
            ref = episode_scan_reference(reward, done, c_ret, c_len, 12, terminal_obs=term.cpu().numpy())
            got = (stats, ep_ret.cpu().numpy(), ep_len.cpu().numpy(), ep_out.cpu().numpy())
            # (per_row buffers are zero-filled, the restatement's rows that are not done are zero as well)
            assert np.array_equal(got[1].view(np.int32), ref["ep_return"].view(np.int32))
            assert np.array_equal(got[2], ref["ep_length"]) and np.array_equal(got[3], ref["ep_outcome"])
            n = int(done.sum())
            assert n > 0 and stats[0] == n == ref["stats"][0] and stats[3] == ref["stats"][3] and stats[13] == n
            assert np.array_equal(stats[4:14], ref["stats"][4:14]), (stats[4:14], ref["stats"][4:14])
            rets = ref["ep_return"][done].astype(np.float64)
            for i, x in ((1, rets), (2, rets * rets)):
                assert abs(stats[i] - math.fsum(x)) <= (n - 1) * 2.0 ** -53 * math.fsum(np.abs(x)), (i, stats[i], math.fsum(x))
            # the carries ARE the handle's cumulative rewards and step counters, for every env
            g_ret, g_len = m.carries()
            torch.cuda.synchronize()
            f_ret = env.batch.get_field(_capi.F_CUM_REWARD).reshape(-1)
            f_len = env.batch.get_field(_capi.F_TSTEPS).reshape(-1)
            assert np.array_equal(g_ret.cpu().numpy().astype(np.float64), f_ret), f"collect {it}: carry_return is not DOCKAUV_F_CUM_REWARD"
            assert np.array_equal(g_len.cpu().numpy().astype(np.float64), f_len), f"collect {it}: carry_length is not DOCKAUV_F_TSTEPS"
            assert np.array_equal(g_ret.cpu().numpy().view(np.int32), ref["carry_return"].view(np.int32))
            tl = ref["ep_outcome"][done] == 3
            assert (ref["ep_length"][done][tl] == 13).all()
            n_time_limit += int(tl.sum())
            # explained variance of collect's own values / returns
            want = ev_numpy(c.values.cpu().numpy(), c.returns.cpu().numpy())
            print(f"{variant} collect {it}: {n} episodes, outcomes {stats[8:13].tolist()}, explained variance {stats[14]!r} (NumPy {want!r})")
            assert abs(stats[14] - want) <= 1e-12 * abs(want), (stats[14], want)
            s = m.summary()
            assert s["n_episodes"] == n and abs(s["rollout/ep_rew_mean"] - rets.mean()) <= 1e-12 * max(1.0, abs(rets.mean()))
            assert abs(s["rollout/ep_len_mean"] - ref["ep_length"][done].mean()) <= 1e-12 * 13
            assert abs(sum(s[k + "_rate"] for k in ("goal", "out_of_range", "attitude", "time_limit", "collision")) - 1.0) < 1e-12
        assert n_time_limit > 0, "no episode ran into max_timesteps"
        # rollout with the monitor continues the same trajectory; after reset() the carries restart from the handle's zeros
        env.rollout(pol, 1, stochastic=True, monitor=m)
        env.reset()
        env.rollout(pol, 1, stochastic=True, monitor=m)
        g_ret, g_len = m.carries()
        torch.cuda.synchronize()
        assert int(g_len.max()) <= 1
        assert np.array_equal(g_len.cpu().numpy().astype(np.float64), env.batch.get_field(_capi.F_TSTEPS).reshape(-1))
    finally:
        env.close()
        twin.close()


def test_refusals_on_a_live_handle():
    import torch
    from gym_dockauv_amd import _capi
    from gym_dockauv_amd.envs.batched import BatchedDocking3d
    import bench
    lib = _capi.load_library()
    p = P()
    ptr = C.c_void_p()
    e64 = p.env_for(20, 6, 64, precision="f64")
    try:
        assert lib.dockauv_monitor_create(e64._handle, C.byref(ptr)) == -1 and not ptr.value
        assert b"float32" in lib.dockauv_last_error(e64._handle)
    finally:
        e64.close()
    wl = bench.workload(2, 64)
    none = BatchedDocking3d(copy.deepcopy(wl["cfg"]), num_envs=64, scenario=wl["scenario"], device=0, precision="f32", reset_mode="none",
                            rng="batched")
    try:
        assert lib.dockauv_monitor_create(none._handle, C.byref(ptr)) == -1 and not ptr.value
        assert b"DOCKAUV_RESET_NONE" in lib.dockauv_last_error(none._handle)
    finally:
        none.close()
    env, other = p.env_for(20, 6, 64), p.env_for(20, 6, 64)
    try:
        K, N = 2, 64
        mon, o_mon = env.make_monitor(), other.make_monitor()
        rows, term = torch.zeros((K, N, 22), device="cuda"), torch.zeros((K, N, 20), device="cuda")
        stats = torch.zeros((16,), device="cuda", dtype=torch.float64)
        out = torch.zeros((K, N), device="cuda", dtype=torch.uint8)
        vals = torch.zeros((K + 1, N), device="cuda")
        err = lambda: lib.dockauv_last_error(env._handle)

        def scan(monitor=mon, **over):
            io = _capi.MonitorIO()
            io.struct_size = C.sizeof(_capi.MonitorIO)
            io.n_steps, io.rows_out, io.terminal_obs, io.stats = K, rows.data_ptr(), term.data_ptr(), stats.data_ptr()
            for k, v in over.items():
                setattr(io, k, v)
            return lib.dockauv_monitor_scan(env._handle, monitor.ptr, C.byref(io), None)

        assert scan() == 0
        assert scan(monitor=o_mon) == -1 and b"another handle" in err()
        assert scan(terminal_obs=None, ep_outcome=out.data_ptr()) == -1 and b"ep_outcome" in err()
        assert scan(values=vals.data_ptr()) == -1 and b"values / returns" in err()
        assert scan(returns=vals.data_ptr()) == -1 and b"values / returns" in err()
        assert scan(struct_size=8) == -1 and b"struct_size" in err()
        assert scan(n_steps=0) == -1 and b"n_steps" in err()
        assert scan(rows_out=None) == -1 and b"rows_out" in err()
        assert scan(stats=None) == -1 and b"stats" in err()
        assert lib.dockauv_monitor_scan(env._handle, None, None, None) == -1 and b"null monitor" in err()
        assert lib.dockauv_monitor_scan(env._handle, mon.ptr, None, None) == -1 and b"io is NULL" in err()
        torch.cuda.synchronize()
    finally:
        env.close()
        other.close()
