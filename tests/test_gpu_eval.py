"""Policy evaluation with an episode quota per env on a real MI355X (include/dockauv.h: dockauv_eval_create / _begin / _scan /
_state; TorchDocking3d.make_evaluator, evaluate): crafted reward / done / terminal-observation buffers through the C ABI against
the NumPy restatement bit for bit (gym_dockauv_amd/evaluate.py: evaluation_scan_reference), chunking, real trajectories whose
slots must be the monitor's per-row outputs cut at the quota and whose carries must be the handle's own counters, ``evaluate``
end to end against a host replay on a twin env, and refusals on a live handle.  Shapes: N = 129 (two full 64-lane groups and one
lane) and N = 1, K = 19 (two load chunks of 8 and a tail of 3), S = 3 slots.  Every batch is closed in `finally`."""
import copy
import ctypes as C
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_SYN, K_SYN, MAX_T_SYN, S_SYN = 129, 19, 3, 3
STATE_KEYS = ("carry_return", "carry_length", "count", "target", "ep_return", "ep_length", "ep_outcome")


def P():
    from tests import test_gpu_policy
    return test_gpu_policy


def H():
    from tests import test_eval_host
    return test_eval_host


def stream_of(torch):
    return torch.cuda.current_stream().cuda_stream


def state_of(torch, batch, ev, N):
    """host copies of the evaluator's arrays (after a synchronisation)"""
    from gym_dockauv_amd.parallel import _DevArray
    S = ev.n_slots
    ptrs = batch.evaluator_state(ev)
    spec = dict(count=((N,), "<i4"), target=((N,), "<i4"), ep_return=((S, N), "<f4"), ep_length=((S, N), "<i4"),
                ep_outcome=((S, N), "|u1"), carry_return=((N,), "<f4"), carry_length=((N,), "<i4"))
    torch.cuda.synchronize()
    return {k: torch.as_tensor(_DevArray(ptrs[k], shape, t), device="cuda").cpu().numpy().copy() for k, (shape, t) in spec.items()}


def scan(torch, batch, ev, rows, term):
    """dockauv_eval_scan of host arrays; returns a host copy of stats"""
    d_rows = torch.from_numpy(np.ascontiguousarray(rows)).cuda()
    d_term = None if term is None else torch.from_numpy(np.ascontiguousarray(term)).cuda()
    stats = torch.full((16,), -7.0, device="cuda", dtype=torch.float64)
    batch.evaluator_scan_device(ev, d_rows.data_ptr(), rows.shape[0], stats.data_ptr(),
                                terminal_obs_ptr=0 if d_term is None else d_term.data_ptr(), stream=stream_of(torch))
    torch.cuda.synchronize()
    return stats.cpu().numpy()


def begin(torch, batch, ev, targets):
    t = torch.from_numpy(np.asarray(targets, dtype=np.int32)).cuda()
    batch.evaluator_begin(ev, t.data_ptr(), 0, stream=stream_of(torch))
    torch.cuda.synchronize()


def check_stats(stats, ref_state, want, what):
    """counts, length sums, min / max and entry 15 exact; the two float64 sums within (n - 1) 2^-53 sum |x| of math.fsum (any
    summation order of n float64 terms stays inside it): the bound tests/test_gpu_monitor.py uses for the same entries"""
    S = ref_state["ep_return"].shape[0]
    rec = np.arange(S)[:, None] < ref_state["count"][None, :]
    rets = ref_state["ep_return"][rec].astype(np.float64)
    n = rets.size
    assert stats[0] == want[0] == n and stats[3] == want[3], (what, stats[:4], want[:4])
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
    assert np.isnan(stats[14]) and stats[15] == want[15] == (ref_state["target"].astype(np.int64) - ref_state["count"]).sum(), (what, stats[15])


@pytest.mark.parametrize("N,n_eval", [(1, 2), (1, 300), (N_SYN, 100), (N_SYN, 300)],
                         ids=["N1-target2", "N1-target300-clamped", "N129-29-envs-at-0", "N129-targets-2-3"])
def test_crafted_buffers_through_the_c_abi(N, n_eval):
    """Three scans of K = 19 after one begin, so that episodes span both boundaries and quotas fill up in different scans: slots,
    counts and carries bit for bit, untouched slots 0 / 0 / 255; then a scan without terminal observations after a second
    begin (outcome 255, nothing classified)."""
    import torch
    from gym_dockauv_amd.evaluate import evaluation_scan_reference, evaluation_state, evaluation_targets
    n_obs = 20
    env = P().env_for(n_obs, 6, N, max_timesteps=MAX_T_SYN)
    try:
        ev = env.make_evaluator(S_SYN)
        fresh = state_of(torch, env, ev, N)
        assert not fresh["target"].any() and not fresh["count"].any() and (fresh["ep_outcome"] == 255).all()   # (create: a begin with 0)
        targets = evaluation_targets(n_eval, N)
        begin(torch, env, ev, targets)
        ref = evaluation_state(targets, S_SYN)          # (a fresh handle after reset: carries 0, the handle's own counters)
        H().same_state(state_of(torch, env, ev, N), ref)
        assert ref["target"].max() <= S_SYN and (n_eval != 100 or (ref["target"][:29] == 0).all())
        codes = set()
        for i in range(3):
            rows, reward, done, term = H().crafted(K_SYN, N, n_obs, seed=60 + i)
            ref, want = evaluation_scan_reference(reward, done, ref, MAX_T_SYN, terminal_obs=term)
            stats = scan(torch, env, ev, rows, term)
            got = state_of(torch, env, ev, N)
            H().same_state(got, ref)
            check_stats(stats, ref, want, f"N {N}, n_eval {n_eval}, scan {i}")
            free = np.arange(S_SYN)[:, None] >= got["count"][None, :]
            assert not got["ep_return"][free].any() and not got["ep_length"][free].any() and (got["ep_outcome"][free] == 255).all()
            codes |= set(got["ep_outcome"][~free].tolist())
        assert ref["carry_length"].max() > 0 or N == 1
        if N > 1:
            assert codes == {0, 1, 2, 3, 4}, codes
            assert (ref["count"] == ref["target"]).all() or n_eval == 300       # (env 8 never finishes: missing with targets >= 2)
            if n_eval == 100:
                assert not ref["count"][:29].any() and stats[0] == 100 and stats[15] == 0
            else:
                assert stats[15] >= 2 and ref["count"][8] == 0
        # a second begin clears everything; without terminal observations nothing is classified
        begin(torch, env, ev, targets)
        ref = evaluation_state(targets, S_SYN)
        H().same_state(state_of(torch, env, ev, N), ref)
        rows, reward, done, term = H().crafted(K_SYN, N, n_obs, seed=70)
        ref, want = evaluation_scan_reference(reward, done, ref, MAX_T_SYN)
        stats = scan(torch, env, ev, rows, None)
        got = state_of(torch, env, ev, N)
        H().same_state(got, ref)
        check_stats(stats, ref, want, f"N {N}, n_eval {n_eval}, without terminal_obs")
        assert (got["ep_outcome"] == 255).all() and not stats[8:14].any()
    finally:
        env.close()


def test_one_scan_of_57_is_three_of_19():
    import torch
    from gym_dockauv_amd.evaluate import evaluation_targets
    N, n_obs = N_SYN, 20
    env = P().env_for(n_obs, 6, N, max_timesteps=MAX_T_SYN)
    try:
        one, three = env.make_evaluator(S_SYN), env.make_evaluator(S_SYN)
        targets = evaluation_targets(300, N)
        begin(torch, env, one, targets)
        begin(torch, env, three, targets)
        rows, _, done, term = H().crafted(57, N, n_obs, seed=11)
        st_one = scan(torch, env, one, rows, term)
        for i in range(3):
            sl = slice(19 * i, 19 * i + 19)
            st_three = scan(torch, env, three, rows[sl], term[sl])
        a, b = state_of(torch, env, one, N), state_of(torch, env, three, N)
        H().same_state(a, b)
        assert np.array_equal(st_one.view(np.int64), st_three.view(np.int64)), (st_one, st_three)
        n_done = done.sum(axis=0)
        assert (n_done > targets).any() and (n_done < targets).any() and st_one[0] == np.minimum(n_done, targets).sum()
    finally:
        env.close()


def make_torch_env(mlp_seed=6):
    """the workload of tests/test_gpu_monitor.py::test_real_trajectories (sphere-16-beam) at N = 129"""
    import bench
    from gym_dockauv_amd.envs.torch_env import TorchDocking3d
    wl = bench.workload(3, N_SYN)
    cfg = copy.deepcopy(wl["cfg"])
    cfg["max_timesteps"] = 12
    env = TorchDocking3d(cfg, num_envs=N_SYN, scenario=wl["scenario"], device_seed=9)
    env.batch._gen = np.random.default_rng(5)
    env.reset()
    actor = P().make_mlp((env.n_obs, (64, 64), env.n_u, "tanh", "none"), seed=mlp_seed, log_std=np.full(env.n_u, -0.5))
    return env, env.make_policy(actor, seed=3)


def test_real_trajectories():
    """Three plain steps the evaluator does not see, a begin mid-trajectory, then three rollouts of K = 19 with a scan each
    (57 steps: every env finishes at least four episodes of at most 13 steps, more than any quota): per env the first ``target``
    entries of the monitor's per-row outputs on the same rows are the slots, and the carries are the handle's own fields."""
    import torch
    from gym_dockauv_amd import _capi
    from gym_dockauv_amd.evaluate import evaluation_targets
    K, N = K_SYN, N_SYN
    env, pol = make_torch_env()
    try:
        ev, shadow = env.make_evaluator(S_SYN), env.make_monitor()
        gen = torch.Generator(device="cuda")
        gen.manual_seed(17)
        for _ in range(3):
            env.step((torch.rand((N, env.n_u), device="cuda", generator=gen) * 2 - 1).contiguous())
        targets = evaluation_targets(300, N)
        ev.begin(targets)
        shadow.sync()
        st0 = {k: v.cpu().numpy() for k, v in ev.state().items()}
        assert st0["carry_length"].max() > 0 and np.array_equal(st0["target"], targets)
        assert np.array_equal(st0["carry_length"].astype(np.float64), env.batch.get_field(_capi.F_TSTEPS).reshape(-1))
        per_row = []
        for it in range(3):
            env.rollout(pol, K, stochastic=False, want_terminal_obs=True)
            rows, term = env._rollout_bufs[K][0], env.rollout_terminal_observation
            stats = ev.scan(rows, terminal_obs=term)
            _, ep_ret, ep_len, ep_out = shadow.scan(rows, terminal_obs=term, per_row=True)
            per_row.append([x.cpu().numpy() for x in (ep_ret, ep_len, ep_out, rows[:, :, env.n_obs + 1] > 0.5)])
            st = {k: v.cpu().numpy() for k, v in ev.state().items()}
            f_ret = env.batch.get_field(_capi.F_CUM_REWARD).reshape(-1)
            f_len = env.batch.get_field(_capi.F_TSTEPS).reshape(-1)
            assert np.array_equal(st["carry_return"].astype(np.float64), f_ret), f"rollout {it}: carry_return is not DOCKAUV_F_CUM_REWARD"
            assert np.array_equal(st["carry_length"].astype(np.float64), f_len), f"rollout {it}: carry_length is not DOCKAUV_F_TSTEPS"
        ep_ret, ep_len, ep_out, done = (np.concatenate([p[i] for p in per_row]) for i in range(4))
        assert (done.sum(axis=0) > targets).all(), "an env finished no more episodes than its quota: nothing was walked past it"
        assert np.array_equal(st["count"], targets) and ev.missing() == 0
        for i in range(N):
            ks = np.flatnonzero(done[:, i])[: targets[i]]
            assert np.array_equal(st["ep_return"][: ks.size, i].view(np.int32), ep_ret[ks, i].view(np.int32)), i
            assert np.array_equal(st["ep_length"][: ks.size, i], ep_len[ks, i]) and np.array_equal(st["ep_outcome"][: ks.size, i], ep_out[ks, i]), i
        free = np.arange(S_SYN)[:, None] >= st["count"][None, :]
        assert free.any() and not st["ep_return"][free].any() and (st["ep_outcome"][free] == 255).all()
        # the read-outs: env-major, then slot order
        r, ln, oc, counts = ev.episodes()
        order = [(j, i) for i in range(N) for j in range(targets[i])]
        assert np.array_equal(counts.cpu().numpy(), targets) and r.shape == (300,)
        assert np.array_equal(r.cpu().numpy().view(np.int32), np.array([st["ep_return"][j, i] for j, i in order], np.float32).view(np.int32))
        assert np.array_equal(ln.cpu().numpy(), [st["ep_length"][j, i] for j, i in order])
        assert np.array_equal(oc.cpu().numpy(), [st["ep_outcome"][j, i] for j, i in order])
        s = ev.summary()
        rets = r.cpu().numpy().astype(np.float64)
        assert s["n_episodes"] == 300 and s["n_missing"] == 0 and abs(s["rollout/ep_rew_mean"] - rets.mean()) <= 1e-12 * max(1.0, abs(rets.mean()))
        assert abs(sum(s[k + "_rate"] for k in ("goal", "out_of_range", "attitude", "time_limit", "collision")) - 1.0) < 1e-12
        assert float(stats[0]) == 300
    finally:
        env.close()


def host_replay(env, pol, targets, K, n_chunks):
    """SB3's evaluate_policy bookkeeping in NumPy on the rows ``rollout`` hands back: float32 running returns, the first
    targets[i] episodes of env i; lists in env-major order"""
    N = env.num_envs
    cur_r, cur_l = np.zeros(N, np.float32), np.zeros(N, np.int64)
    rets, lens = [[] for _ in range(N)], [[] for _ in range(N)]
    for _ in range(n_chunks):
        _, _, reward, done = env.rollout(pol, K, stochastic=False)
        reward, done = reward.cpu().numpy(), done.cpu().numpy()
        for k in range(K):
            cur_r = cur_r + reward[k]
            cur_l += 1
            for i in np.flatnonzero(done[k]):
                if len(rets[i]) < targets[i]:
                    rets[i].append(float(cur_r[i]))
                    lens[i].append(int(cur_l[i]))
                cur_r[i], cur_l[i] = 0.0, 0
    return [x for r in rets for x in r], [x for ln in lens for x in ln]


@pytest.mark.parametrize("n_eval", [200, 100])
def test_evaluate_end_to_end(n_eval):
    from gym_dockauv_amd.evaluate import evaluation_targets
    N = N_SYN
    env, pol = make_torch_env()
    twin, t_pol = make_torch_env()
    try:
        targets = evaluation_targets(n_eval, N)
        ev = env.make_evaluator(int(targets.max()))
        rewards, lengths = env.evaluate(pol, n_eval, seed=5, return_episode_rewards=True, evaluator=ev)
        K, bound = 13, int(targets.max())                   # (K = min(128, max_timesteps + 1); ceil(max(targets) 13 / 13) chunks)
        assert len(rewards) == len(lengths) == n_eval and ev.missing() == 0 and 1 <= ev.n_chunks <= bound
        r, ln, oc, counts = ev.episodes()
        assert np.array_equal(counts.cpu().numpy(), targets) and (oc.cpu().numpy() < 5).all()
        if n_eval == 100:
            st = {k: v.cpu().numpy() for k, v in ev.state().items()}
            assert not st["count"][:29].any() and (st["ep_outcome"][:, :29] == 255).all() and not st["ep_return"][:, :29].any()
        twin.reset(seed=5)
        want_r, want_l = host_replay(twin, t_pol, targets, K, ev.n_chunks)
        assert rewards == want_r and lengths == want_l
        assert max(lengths) <= 13
        s = ev.summary()
        assert s["n_episodes"] == n_eval and s["n_missing"] == 0
        assert abs(sum(s[k + "_rate"] for k in ("goal", "out_of_range", "attitude", "time_limit", "collision")) - 1.0) < 1e-12
        assert abs(s["rollout/ep_rew_mean"] - np.mean(want_r)) <= 1e-12 * max(1.0, abs(np.mean(want_r)))
        # (mean, std) on a fresh pair of envs' worth of the same call: np.mean / np.std of the replayed list
        env2, pol2 = make_torch_env()
        try:
            mean, std = env2.evaluate(pol2, n_eval, seed=5)
            s2 = env2.evaluator.summary()                    # (without evaluator=: the call's own stays at env.evaluator)
            assert s2["n_episodes"] == n_eval and s2["goal_rate"] == s["goal_rate"] and s2["time_limit_rate"] == s["time_limit_rate"]
        finally:
            env2.close()
        assert mean == float(np.mean(np.array(want_r, dtype=np.float64))) and std == float(np.std(np.array(want_r, dtype=np.float64)))
        print(f"n_eval {n_eval}: {ev.n_chunks} chunk(s) of {K}, mean {mean!r}, std {std!r}, goal_rate {s['goal_rate']!r}, "
              f"time_limit_rate {s['time_limit_rate']!r}, collision_rate {s['collision_rate']!r}")
        with pytest.raises(ValueError):
            env.evaluate(pol, 1000, evaluator=ev)            # (needs 8 slots per env)
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
        assert lib.dockauv_eval_create(e64._handle, 2, C.byref(ptr)) == -1 and not ptr.value
        assert b"float32" in lib.dockauv_last_error(e64._handle)
    finally:
        e64.close()
    wl = bench.workload(2, 64)
    none = BatchedDocking3d(copy.deepcopy(wl["cfg"]), num_envs=64, scenario=wl["scenario"], device=0, precision="f32", reset_mode="none",
                            rng="batched")
    try:
        assert lib.dockauv_eval_create(none._handle, 2, C.byref(ptr)) == -1 and not ptr.value
        assert b"DOCKAUV_RESET_NONE" in lib.dockauv_last_error(none._handle)
    finally:
        none.close()
    env, other = p.env_for(20, 6, 64), p.env_for(20, 6, 64)
    try:
        K, N, S = 2, 64, 2
        ev, o_ev = env.make_evaluator(S), other.make_evaluator(S)
        rows, term = torch.zeros((K, N, 22), device="cuda"), torch.zeros((K, N, 20), device="cuda")
        stats = torch.zeros((16,), device="cuda", dtype=torch.float64)
        err = lambda: lib.dockauv_last_error(env._handle)

        def scan_io(evaluator=ev, **over):
            io = _capi.EvalIO()
            io.struct_size = C.sizeof(_capi.EvalIO)
            io.n_steps, io.rows_out, io.terminal_obs, io.stats = K, rows.data_ptr(), term.data_ptr(), stats.data_ptr()
            for k, v in over.items():
                setattr(io, k, v)
            return lib.dockauv_eval_scan(env._handle, None if evaluator is None else evaluator.ptr, C.byref(io), None)

        assert scan_io() == 0
        assert scan_io(evaluator=o_ev) == -1 and b"another handle" in err()
        assert scan_io(evaluator=None) == -1 and b"null evaluator" in err()
        assert scan_io(struct_size=8) == -1 and b"struct_size" in err()
        assert scan_io(n_steps=0) == -1 and b"n_steps" in err()
        assert scan_io(rows_out=None) == -1 and b"rows_out" in err()
        assert scan_io(stats=None) == -1 and b"stats" in err()
        assert lib.dockauv_eval_scan(env._handle, ev.ptr, None, None) == -1 and b"io is NULL" in err()
        for bad in (S + 1, -1):
            assert lib.dockauv_eval_begin(ev.ptr, None, bad, None) == -1 and b"uniform_target" in err() and b"outside [0, 2]" in err()
        assert lib.dockauv_eval_begin(ev.ptr, None, S, None) == 0 and lib.dockauv_eval_begin(ev.ptr, None, 0, None) == 0
        assert lib.dockauv_eval_create(env._handle, 0, C.byref(ptr)) == -1 and b"max_episodes_per_env" in err()
        assert lib.dockauv_eval_create(env._handle, 2 ** 31 // N, C.byref(ptr)) == -1 and b"2^31" in err() and not ptr.value
        torch.cuda.synchronize()
    finally:
        env.close()
        other.close()
