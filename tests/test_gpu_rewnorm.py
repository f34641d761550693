"""Reward normalisation on a real MI355X (include/dockauv.h: dockauv_rewnorm_create / _state / _reset / _scan,
dockauv_gae_normalized, dockauv_collect_normalized; TorchDocking3d.make_reward_normalizer, collect with reward_norm=): crafted
reward / done buffers through the C ABI against the NumPy restatement (gym_dockauv_amd/normalize.py:
reward_normalize_reference) -- the discounted returns and carries bit for bit, the float64 statistics within a bound the test
derives and prints, the normalised rewards within one float32 ulp --, frozen mode, reset and checkpoints, GAE on the column bit
for bit against dockauv_gae / dockauv_gae_truncated on rows that carry the column, and real collections against the by-hand
sequence and against a twin without the option.  Shapes: (K, N) = (19, 200) (three partial chunks of 8 steps, a partly filled
last group), (1, 70), (37, 2500) (a second and a third pass of the 1 024-lane group).  Every batch is closed in `finally`."""
import copy
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SENT = -7.0
U = 2.0 ** -53
GAMMA, EPS = 0.99, 1e-8
CASES = [("K19-19-1-N200", 200, (19, 19, 1), 10.0), ("K1-N70", 70, (1,), 10.0), ("K37-N2500", 2500, (37,), 10.0),
         ("K19-19-1-N200-clip2", 200, (19, 19, 1), 2.0)]


def Cc():
    """the helpers of the collector tests: P (make_mlp, env_for), make_critic, run_gae, bits, stream_of"""
    from tests import test_gpu_collect
    return test_gpu_collect


def Hh():
    from tests import test_rewnorm_host
    return test_rewnorm_host


def state_of(torch, env, rn):
    """host copies of the normaliser's state float64 [4] and carries float32 [N] (after a synchronisation)"""
    from gym_dockauv_amd.parallel import _DevArray
    s_ptr, c_ptr = env.reward_normalizer_state(rn)
    torch.cuda.synchronize()
    return (torch.as_tensor(_DevArray(s_ptr, (4,), "<f8"), device="cuda").cpu().numpy().copy(),
            torch.as_tensor(_DevArray(c_ptr, (env.num_envs,), "<f4"), device="cuda").cpu().numpy().copy())


def scan_guarded(torch, env, rn, rows, K, N, training=True, stats=True):
    """dockauv_rewnorm_scan into sentinel-filled outputs one row longer than needed; returns host copies (reward_norm, discounted,
    step_stats or None), the guard rows checked"""
    d_rows = torch.from_numpy(rows).cuda()
    norm = torch.full((K + 1, N), SENT, device="cuda")
    disc = torch.full((K + 1, N), SENT, device="cuda")
    st = torch.full((K + 1, 4), SENT, device="cuda", dtype=torch.float64) if stats else None
    env.reward_normalizer_scan_device(rn, d_rows.data_ptr(), K, norm.data_ptr(), disc.data_ptr() if training else 0,
                                      st.data_ptr() if stats else 0, training=training, stream=Cc().stream_of(torch))
    torch.cuda.synchronize()
    assert bool((norm[K] == SENT).all()) and bool((disc[K] == SENT).all()), "the kernels wrote behind the last step's row"
    assert st is None or bool((st[K] == SENT).all()), "the kernels wrote behind the last step's statistics"
    assert torch.equal(Cc().bits(d_rows), Cc().bits(torch.from_numpy(rows).cuda())), "the rows changed"
    return norm[:K].cpu().numpy(), disc[:K].cpu().numpy(), None if st is None else st[:K].cpu().numpy()


def ulp_distance(a, b):
    """float32 arrays of one sign pattern: distance in units of the last place"""
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def check_statistics(got_stats, disc, state0, what):
    """batch_mean, batch_var, running var and den of every step against math.fsum-based moments of the (bit-exact) discounted
    column.  The bound, first order in u = 2^-53, n = N envs:
      batch sum: any summation order of n float64 terms stays inside (n - 1) u sum |x| (check_against_restatement of the monitor
        tests); the division by n and fsum's own rounding add 2 u |mean|:           E_m = (n - 1) u sum |x| / n + 2 u |mean|
      batch variance about a mean that is off by E_m: sum (x - m')^2 - sum (x - m)^2 = -2 e sum (x - m) + n e^2, at most
        2 E_m mean |x - m| + E_m^2 per element; every q = x - m is rounded once and squared (3 u relative with the square's own
        rounding, the device's fma saves that one), the n terms are summed in any order ((n - 1) u sum q^2), the division and
        the reference's own roundings take the rest of                               E_v = (n + 8) u var + 2 E_m mad + E_m^2
      merge k (both sides run the same float64 operations, on inputs that differ by the errors so far; a rounding is u relative):
        delta:  e_d   = E_m + e_mean + u |delta|
        mean:   mean' = mean count / tot + batch_mean n / tot in exact arithmetic, a convex combination, so the errors so far
                do not grow:  e_mean' = e_mean count / tot + (E_m + 3 u |delta|) n / tot + u |mean'|
        M2:     e_M2  = e_var count + E_v n + (2 |delta| e_d + e_d^2) count n / tot + 8 u M2      (all terms of M2 are >= 0)
        var:    e_var' = e_M2 / tot + u var'
        den:    e_den = e_var' / (2 den) + 3 u den      (the add, the square root and one ulp for the device's sqrt)
    count takes the same additions on the same values on both sides: exact.  Prints, per statistic, the largest difference with
    the bound at that step and the largest bound of any step; returns the reference's final (mean, var, count) and the bounds on
    the running mean and variance."""
    K, N = disc.shape
    n = float(N)
    mean, var, count = float(state0[0]), float(state0[1]), float(state0[2])
    e_mean = e_var = 0.0
    worst = {name: [-1.0, 0.0, 0.0] for name in ("batch_mean", "batch_var", "var", "den")}

    def look(name, got, want, bound, k):
        err = abs(got - want)
        w = worst[name]
        if err > w[0]:
            w[0], w[1] = err, bound
        w[2] = max(w[2], bound)
        assert err <= bound, (what, name, k, got, want, err, bound)

    for k in range(K):
        x = disc[k].astype(np.float64)
        bm = math.fsum(x) / n
        q = x - bm
        bv = math.fsum(q * q) / n
        E_m = (n - 1) * U * math.fsum(np.abs(x)) / n + 2 * U * abs(bm)
        E_v = (n + 8) * U * bv + 2 * E_m * math.fsum(np.abs(q)) / n + E_m * E_m
        look("batch_mean", got_stats[k, 0], bm, E_m, k)
        look("batch_var", got_stats[k, 1], bv, E_v, k)
        delta = bm - mean
        tot = count + n
        new_mean = mean + (delta * n) / tot
        m2 = (var * count + bv * n) + (((delta * delta) * count) * n) / tot
        new_var = m2 / tot
        e_d = E_m + e_mean + U * abs(delta)
        e_m2 = e_var * count + E_v * n + (2 * abs(delta) * e_d + e_d * e_d) * count * n / tot + 8 * U * m2
        e_mean = e_mean * count / tot + (E_m + 3 * U * abs(delta)) * n / tot + U * abs(new_mean)
        e_var = e_m2 / tot + U * new_var
        mean, var, count = new_mean, new_var, tot
        den = math.sqrt(var + EPS)
        look("var", got_stats[k, 2], var, e_var, k)
        look("den", got_stats[k, 3], den, e_var / (2 * den) + 3 * U * den, k)
    for name, (err, bound, largest) in worst.items():
        print(f"{what}: {name} largest |device - fsum reference| {err:.3e}, the bound there {bound:.3e}, the largest bound {largest:.3e}")
    return mean, var, count, e_mean, e_var


@pytest.mark.parametrize("name,N,Ks,clip", CASES, ids=[c[0] for c in CASES])
def test_scans_against_the_restatement(name, N, Ks, clip):
    """Scans in a row on one normaliser, so that episodes span the boundaries; a second normaliser of the handle repeats the first
    scan from the same state: identical bits in every output."""
    import torch
    from gym_dockauv_amd.normalize import INITIAL_STATE, reward_normalize_reference
    n_obs = 20
    env = Cc().P().env_for(n_obs, 6, N)
    try:
        rn, rn2 = env.make_reward_normalizer(GAMMA, clip, EPS), env.make_reward_normalizer(GAMMA, clip, EPS)
        state, carry = state_of(torch, env, rn)
        assert np.array_equal(state, np.array(INITIAL_STATE)) and not carry.any()
        for i, K in enumerate(Ks):
            rows, reward, done = Hh().crafted(K, N, n_obs, seed=50 + i, first_last=K > 1)
            ref = reward_normalize_reference(reward, done, GAMMA, clip, EPS, state, carry)
            if clip == 2.0:
                # the input choice must clip on both sides, or the case shows nothing (decided on the restatement alone)
                q = reward.astype(np.float64) / ref["step_stats"][:, 3:4]
                hi, lo = float((q > clip).mean()), float((q < -clip).mean())
                print(f"{name} scan {i}: {hi:.3%} of the elements above +{clip}, {lo:.3%} below -{clip}")
                assert 0.01 <= hi <= 0.5 and 0.01 <= lo <= 0.5, (hi, lo)
            norm, disc, stats = scan_guarded(torch, env, rn, rows, K, N)
            what = f"{name} scan {i} (K = {K})"
            assert np.array_equal(disc.view(np.int32), ref["discounted"].view(np.int32)), f"{what}: discounted"
            g_state, g_carry = state_of(torch, env, rn)
            assert np.array_equal(g_carry.view(np.int32), ref["carry"].view(np.int32)), f"{what}: carries"
            assert g_state[2] == ref["state"][2] and round(g_state[2]) == N * sum(Ks[: i + 1]), f"{what}: count"
            mean, var, count, e_mean, e_var = check_statistics(stats, disc, state, what)
            assert abs(g_state[0] - mean) <= e_mean and abs(g_state[1] - var) <= e_var and g_state[3] == 0.0
            assert g_state[1] == stats[K - 1, 2], "the running variance is not the last step's"
            ulps = ulp_distance(norm, ref["reward_norm"])
            print(f"{what}: reward_norm differs from the restatement's in {int((ulps > 0).sum())} of {ulps.size} elements, "
                  f"at most {int(ulps.max())} ulp")
            assert ulps.max() <= 1, what
            if clip == 2.0:
                q = reward.astype(np.float64) / ref["step_stats"][:, 3:4]
                far = np.abs(q) > clip * (1 + 1e-9)
                assert (np.abs(norm[far]) == np.float32(clip)).all() and np.array_equal(np.sign(norm[far]), np.sign(q[far]))
            assert np.abs(norm).max() <= clip
            if i == 0:
                again = scan_guarded(torch, env, rn2, rows, K, N)
                for a, b, dt in zip(again, (norm, disc, stats), (np.int32, np.int32, np.int64)):
                    assert np.array_equal(a.view(dt), b.view(dt)), "two scans of the same inputs from the same state differ"
                s2, c2 = state_of(torch, env, rn2)
                assert np.array_equal(s2.view(np.int64), g_state.view(np.int64)) and np.array_equal(c2.view(np.int32), g_carry.view(np.int32))
                if K > 1:
                    assert done[0, 0:4].all() and done[K - 1, 4:8].all() and not done[:, 8].any()
            state, carry = g_state, g_carry     # (the next scan's restatement continues the device's state: the carries are its own bits)
        assert len(Ks) == 1 or carry.any(), "no episode spans a scan boundary"
    finally:
        env.close()


def test_frozen_mode():
    """training == 0 after one training scan: one divisor for every step, the state and the carries unchanged bit for bit,
    discounted untouched, step_stats optional (rewnorm_apply_kernel<true>, the one launch)"""
    import torch
    from gym_dockauv_amd.normalize import reward_normalize_reference
    N, K, n_obs = 200, 19, 20
    env = Cc().P().env_for(n_obs, 6, N)
    try:
        rn = env.make_reward_normalizer(GAMMA, 10.0, EPS)
        rows, _, _ = Hh().crafted(K, N, n_obs, seed=60)
        scan_guarded(torch, env, rn, rows, K, N)
        state, carry = state_of(torch, env, rn)
        assert state[1] > 100.0 and carry.any()
        for K2 in (K, 1):
            rows2, reward2, done2 = Hh().crafted(K2, N, n_obs, seed=61 + K2, first_last=K2 > 1)
            ref = reward_normalize_reference(reward2, done2, GAMMA, 10.0, EPS, state, carry, training=False)
            norm, disc, stats = scan_guarded(torch, env, rn, rows2, K2, N, training=False)
            assert (disc == SENT).all(), "frozen mode wrote discounted"
            den = stats[:, 3]
            assert (den.view(np.int64) == den.view(np.int64)[0]).all() and abs(den[0] - math.sqrt(state[1] + EPS)) <= 3 * U * den[0]
            assert (stats[:, :3] == SENT).all(), "frozen mode wrote more than den"
            assert ulp_distance(norm, ref["reward_norm"]).max() <= 1
            bare, _, none = scan_guarded(torch, env, rn, rows2, K2, N, training=False, stats=False)
            assert none is None and np.array_equal(bare.view(np.int32), norm.view(np.int32))
            s2, c2 = state_of(torch, env, rn)
            assert np.array_equal(s2.view(np.int64), state.view(np.int64)) and np.array_equal(c2.view(np.int32), carry.view(np.int32))
    finally:
        env.close()


def twin_envs(N, max_timesteps, n=2):
    import bench
    from gym_dockauv_amd.envs.torch_env import TorchDocking3d
    wl = bench.workload(3, N)
    cfg = copy.deepcopy(wl["cfg"])
    cfg["max_timesteps"] = max_timesteps
    envs = []
    for _ in range(n):
        env = TorchDocking3d(cfg, num_envs=N, scenario=wl["scenario"], device_seed=9)
        env.batch._gen = np.random.default_rng(5)
        env.reset()
        envs.append(env)
    return envs


def test_reset_and_checkpoint():
    """``reset`` gives a fresh normaliser's bits; ``state_dict`` / ``load_state_dict`` followed by a further scan give the bits of
    an uninterrupted run"""
    import torch
    from gym_dockauv_amd.normalize import INITIAL_STATE
    N, K = 200, 19
    (env,) = twin_envs(N, 25, n=1)
    try:
        n_obs = env.n_obs
        r1 = torch.from_numpy(Hh().crafted(K, N, n_obs, seed=80)[0]).cuda()
        r2 = torch.from_numpy(Hh().crafted(K, N, n_obs, seed=81)[0]).cuda()
        a, b, fresh = [env.make_reward_normalizer(GAMMA) for _ in range(3)]
        assert (a.mean, a.var, a.count) == INITIAL_STATE[:3] and a.clip_reward == 10.0 and a.epsilon == 1e-8 and a.training
        bits = Cc().bits
        a.scan(r1)
        want = [t.clone() for t in (a.scan(r2), a.discounted, a.step_stats)]
        b.scan(r1)
        sd = b.state_dict()
        assert sd["state"].shape == (4,) and sd["carry"].shape == (N,) and round(sd["state"][2]) == K * N
        b.reset()
        assert (b.mean, b.var, b.count) == INITIAL_STATE[:3] and not bool(b.carries().any())
        got = b.scan(r2)
        first = fresh.scan(r2)
        assert torch.equal(bits(got), bits(first)) and torch.equal(b.step_stats.view(torch.int64), fresh.step_stats.view(torch.int64))
        assert not torch.equal(bits(got), bits(want[0]))
        b.load_state_dict(sd)
        assert b.count == sd["state"][2]
        got = b.scan(r2)
        assert torch.equal(bits(got), bits(want[0])) and torch.equal(bits(b.discounted), bits(want[1]))
        assert torch.equal(b.step_stats.view(torch.int64), want[2].view(torch.int64))
        sa, sb = a.state_dict(), b.state_dict()
        assert np.array_equal(sa["state"].view(np.int64), sb["state"].view(np.int64))
        assert np.array_equal(sa["carry"].view(np.int32), sb["carry"].view(np.int32))
        with pytest.raises(ValueError, match="gamma"):
            env.make_reward_normalizer(0.9).load_state_dict(sd)
    finally:
        env.close()


@pytest.mark.parametrize("K,N", [(19, 200), (37, 2500)])
def test_gae_on_the_column_is_gae_on_rows_that_carry_it(K, N):
    """dockauv_gae_normalized reads the reward from the column and nothing else from the rows' reward word (NaN here): bit for bit
    dockauv_gae, and with a truncation block dockauv_gae_truncated, on a copy of the rows whose reward word is the column"""
    import torch
    from tests import test_gpu_truncation as T
    c = Cc()
    n_obs = 20
    env = T.trunc_env(n_obs, N)
    try:
        val = env.make_value(c.make_critic(n_obs, (64, 64)))
        x = T.inputs(K, N, n_obs, seed=K + N)
        column = np.random.default_rng(K).uniform(-3, 3, (K, N)).astype(np.float32)
        carried = dict(x, reward=column, rows=x["rows"].copy())
        carried["rows"][:, :, n_obs] = column
        blind = x["rows"].copy()
        blind[:, :, n_obs] = np.nan
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        d_rows, d_col, d_val, d_term = dev(blind), dev(column), dev(x["values"]), dev(x["term"])
        S = env.truncation_slots(K)
        for gamma, lam in T.GAMMA_LAMBDA:
            adv, ret = torch.full((K + 1, N), SENT, device="cuda"), torch.full((K + 1, N), SENT, device="cuda")
            env.gae_normalized_device(None, d_col.data_ptr(), d_rows.data_ptr(), d_val.data_ptr(), K, gamma, lam, adv.data_ptr(),
                                      ret.data_ptr(), stream=c.stream_of(torch))
            torch.cuda.synchronize()
            assert bool((adv[K] == SENT).all()) and bool((ret[K] == SENT).all())
            w_adv, w_ret = c.run_gae(torch, env, carried["rows"], x["values"], K, N, gamma, lam)
            assert np.array_equal(adv[:K].cpu().numpy().view(np.int32), w_adv.view(np.int32)), (gamma, lam)
            assert np.array_equal(ret[:K].cpu().numpy().view(np.int32), w_ret.view(np.int32)), (gamma, lam)
            # with the truncation block
            want = T.run(torch, env, val, carried, gamma, lam)
            n_trunc = int((want["step"] >= 0).sum())
            assert n_trunc >= N // 2 and (want["step"][:, 0] >= 0).all(), "the inputs do not truncate"
            carry = dev(x["carry"])
            step, row = torch.full((S, N), -7, device="cuda", dtype=torch.int32), torch.full((S, N), -7, device="cuda", dtype=torch.int64)
            vt = torch.full((S, N), SENT, device="cuda")
            adv.fill_(SENT)
            ret.fill_(SENT)
            trunc = dict(n_slots=S, terminal_obs=d_term.data_ptr(), length_carry=carry.data_ptr(), trunc_step=step.data_ptr(),
                         trunc_row=row.data_ptr(), v_terminal=vt.data_ptr())
            env.gae_normalized_device(val, d_col.data_ptr(), d_rows.data_ptr(), d_val.data_ptr(), K, gamma, lam, adv.data_ptr(),
                                      ret.data_ptr(), stream=c.stream_of(torch), trunc=trunc)
            torch.cuda.synchronize()
            assert bool((adv[K] == SENT).all()) and bool((ret[K] == SENT).all())
            assert np.array_equal(step.cpu().numpy(), want["step"]) and np.array_equal(carry.cpu().numpy(), want["carry"])
            assert np.array_equal(adv[:K].cpu().numpy().view(np.int32), want["adv"].view(np.int32)), (gamma, lam)
            assert np.array_equal(ret[:K].cpu().numpy().view(np.int32), want["ret"].view(np.int32)), (gamma, lam)
            assert not np.array_equal(want["adv"].view(np.int32), w_adv.view(np.int32)), "the bootstrap changed nothing"
    finally:
        env.close()


@pytest.mark.parametrize("bootstrap,monitored", [(False, False), (True, True), (True, False), (False, True)],
                         ids=["plain", "bootstrap-monitor", "bootstrap", "monitor"])
def test_collect_with_the_normaliser(bootstrap, monitored):
    """192 envs, K = 16, max_timesteps 25, three iterations, two envs built alike: what the option leaves alone is bit for bit the
    twin's, what it changes is bit for bit the by-hand sequence on the twin's buffers -- plain collect, dockauv_rewnorm_scan on
    its rows, dockauv_gae_normalized"""
    import torch
    from gym_dockauv_amd import _capi
    from tests import test_gpu_update as Up
    c = Cc()
    N, K, MT, lam = 192, 16, 25, 0.95
    actor_mlp, critic_mlp = Up.mlps()
    ea, eb = twin_envs(N, MT)
    try:
        pa, pb = [e.make_policy(actor_mlp, seed=3) for e in (ea, eb)]
        va, vb = [e.make_value(critic_mlp) for e in (ea, eb)]
        rn, hand = ea.make_reward_normalizer(GAMMA), eb.make_reward_normalizer(GAMMA)
        ma, mb = (ea.make_monitor(), eb.make_monitor()) if monitored else (None, None)
        with pytest.raises(ValueError, match="gamma"):
            ea.collect(pa, va, K, 0.98, lam, reward_norm=rn)
        with pytest.raises(ValueError, match="critic"):
            ea.collect(pa, None, K, GAMMA, lam, reward_norm=rn)
        with pytest.raises(ValueError, match="another env"):
            ea.collect(pa, va, K, GAMMA, lam, reward_norm=hand)
        n_trunc = 0
        for it in range(3):
            carry = eb.batch.get_field(_capi.F_TSTEPS).reshape(-1).astype(np.int32)   # (synchronises: before the collect)
            ca = ea.collect(pa, va, K, GAMMA, lam, monitor=ma, bootstrap_truncated=bootstrap, reward_norm=rn)
            cb = eb.collect(pb, vb, K, GAMMA, lam, monitor=mb, want_terminal_obs=bootstrap)
            torch.cuda.synchronize()
            assert ca._fields == cb._fields
            for name in ("obs", "actions", "reward", "log_prob", "values"):
                assert torch.equal(c.bits(getattr(ca, name)), c.bits(getattr(cb, name))), (it, name)
            assert torch.equal(ca.done, cb.done)
            if monitored:
                assert torch.equal(ma.stats[:14].view(torch.int64), mb.stats[:14].view(torch.int64)), "the monitor saw other rewards"
            # by hand on the twin's buffers
            rows = eb._collect_bufs[K]["rows"]
            norm = hand.scan(rows[1:])
            adv, ret = torch.zeros((K, N), device="cuda"), torch.zeros((K, N), device="cuda")
            trunc = None
            if bootstrap:
                S = eb.batch.truncation_slots(K)
                keep = [torch.from_numpy(carry).cuda(), torch.zeros((S, N), device="cuda", dtype=torch.int32),
                        torch.zeros((S, N), device="cuda", dtype=torch.int64), torch.zeros((S, N), device="cuda")]
                trunc = dict(n_slots=S, terminal_obs=eb.rollout_terminal_observation.data_ptr(), length_carry=keep[0].data_ptr(),
                             trunc_step=keep[1].data_ptr(), trunc_row=keep[2].data_ptr(), v_terminal=keep[3].data_ptr())
            eb.batch.gae_normalized_device(vb, norm.data_ptr(), rows[1].data_ptr(), cb.values.data_ptr(), K, GAMMA, lam,
                                           adv.data_ptr(), ret.data_ptr(), stream=c.stream_of(torch), trunc=trunc)
            torch.cuda.synchronize()
            if bootstrap:
                n_trunc += int((keep[1] >= 0).sum())
            assert torch.equal(c.bits(rn.normalized), c.bits(norm)) and torch.equal(c.bits(rn.discounted), c.bits(hand.discounted)), it
            assert torch.equal(rn.step_stats.view(torch.int64), hand.step_stats.view(torch.int64)), it
            assert torch.equal(c.bits(ca.advantages), c.bits(adv)) and torch.equal(c.bits(ca.returns), c.bits(ret)), it
            assert not torch.equal(c.bits(ca.advantages), c.bits(cb.advantages))
            assert float(rn.normalized.abs().max()) <= 10.0 and rn.count == hand.count and round(rn.count) == (it + 1) * K * N
        assert not bootstrap or n_trunc >= 1, "no episode reached the time limit: the bootstrap was not exercised"
        assert rn.var == hand.var and rn.var != 1.0
        # evaluation: the statistics are applied, not updated
        rn.training = False
        before = rn.state_dict()
        ea.collect(pa, va, K, GAMMA, lam, reward_norm=rn)
        after = rn.state_dict()
        assert np.array_equal(before["state"].view(np.int64), after["state"].view(np.int64))
        assert np.array_equal(before["carry"].view(np.int32), after["carry"].view(np.int32))
        den = rn.step_stats[:, 3].cpu().numpy()
        assert (den == den[0]).all()
        rn.training = True
        # the result feeds the update unchanged
        nets = Up.learner(torch, actor_mlp, critic_mlp)
        opt = Up.optimizer(ea, pa, va, nets)
        stats = ea.ppo_train(opt, ca, 1, 512, 3e-4, seed=1, **Up.KW)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(stats[..., :8]).all()) and opt.steps() == (K * N + 511) // 512
    finally:
        ea.close()
        eb.close()


def test_refusals_on_a_live_handle():
    """a normaliser of another handle and a float64 handle are refused by name, a bad constant on a live handle too"""
    import ctypes as C
    import torch
    from gym_dockauv_amd import _capi
    lib = _capi.load_library()
    p = Cc().P()
    N, K = 64, 4
    e1, e2 = p.env_for(20, 6, N), p.env_for(20, 6, N)
    e64 = p.env_for(20, 6, N, precision="f64")
    try:
        rn2 = e2.make_reward_normalizer(GAMMA)
        z = lambda *shape, dtype=torch.float32: torch.zeros(shape, device="cuda", dtype=dtype)
        rows, norm, disc, st = z(K, N, 22), z(K, N), z(K, N), z(K, 4, dtype=torch.float64)
        with pytest.raises(_capi.DockAUVError, match="created for another handle"):
            e1.reward_normalizer_scan_device(rn2, rows.data_ptr(), K, norm.data_ptr(), disc.data_ptr(), st.data_ptr())
        with pytest.raises(_capi.DockAUVError, match="DOCKAUV_F64"):
            e64.make_reward_normalizer(GAMMA)
        with pytest.raises(_capi.DockAUVError, match="DOCKAUV_F64"):
            e64.gae_normalized_device(None, norm.data_ptr(), rows.data_ptr(), z(K + 1, N).data_ptr(), K, GAMMA, 0.95,
                                      z(K, N).data_ptr(), z(K, N).data_ptr())
        out = C.c_void_p()
        assert lib.dockauv_rewnorm_create(e1._handle, 0.99, -1.0, 1e-8, C.byref(out)) == -1 and not out.value
        assert b"clip_reward" in lib.dockauv_last_error(e1._handle)

        # two defects at once: the first in the order of checks is the one reported (tests/test_collect_precedence_host.py has what
        # is checked before the handle).  The blocks' pointers are fake addresses: every call is refused first.
        c = Cc()
        h = e1._handle
        err = lambda: lib.dockauv_last_error(h)
        rn1 = e1.make_reward_normalizer(GAMMA)
        mlp = c.P().make_mlp((20, (64, 64), 6, "tanh", "none"), seed=1, log_std=np.full(6, -0.5))
        pol, val, o_pol = e1.make_policy(mlp), e1.make_value(c.make_critic(20, (64, 64))), e2.make_policy(mlp)
        ptr = lambda obj: obj.ptr if obj is not None else None

        def blocks(cio=None, tio=None):
            nb, cb, tb = Hh().ios(_capi, K)
            for block, over in ((cb, cio), (tb, tio)):
                for name, value in (over or {}).items():
                    setattr(block, name, value)
            return nb, cb, tb

        def collect(actor=pol, crit=val, rn=rn1, with_tio=False, cio=None, tio=None):
            nb, cb, tb = blocks(cio, tio)
            return lib.dockauv_collect_normalized(h, ptr(actor), ptr(crit), C.byref(cb), C.byref(tb) if with_tio else None, ptr(rn),
                                                  C.byref(nb), None)
        assert collect(rn=None, actor=None) == -1 and b"dockauv_collect_normalized: null normaliser" in err()
        assert collect(rn=rn2, cio=dict(gamma=0.5)) == -1 and b"the normaliser was created for another handle" in err()
        assert collect(cio=dict(gamma=0.5), actor=None) == -1 and b"dockauv_collect_io.gamma: 0.5, the normaliser's is 0.99" in err()
        assert collect(actor=None, crit=None) == -1 and b"dockauv_collect_normalized: null actor" in err()
        assert collect(crit=None, with_tio=True, tio=dict(n_slots=0)) == -1 and b"dockauv_collect_normalized: null critic" in err()
        assert collect(with_tio=True, tio=dict(n_slots=0, rows_out=4096)) == -1 and b"dockauv_truncation_io.n_slots: 0" in err()
        assert collect(with_tio=True, tio=dict(rows_out=4096), actor=o_pol) == -1
        assert b"dockauv_truncation_io.rows_out is not dockauv_collect_io's" in err()
        assert collect(with_tio=True, tio=dict(terminal_obs=4096, values=4096)) == -1
        assert b"dockauv_truncation_io.terminal_obs is not dockauv_collect_io's" in err()
        assert collect(actor=o_pol, crit=pol) == -1 and b"dockauv_collect_normalized: the policy was created for another handle" in err()

        def gae(crit=val, tio=None):      # dockauv_gae_normalized with a truncation block: what the block must share with the call
            _, cb, tb = blocks(tio=tio)
            return lib.dockauv_gae_normalized(h, ptr(crit), C.c_void_p(640), C.byref(tb), C.c_void_p(cb.rows_out), C.c_void_p(cb.values),
                                              K, 0.99, 0.95, C.c_void_p(cb.advantages), C.c_void_p(cb.returns), None)
        whose = b"dockauv_gae_normalized's"
        assert gae(crit=None, tio=dict(n_slots=0)) == -1 and b"dockauv_gae_normalized: null critic" in err()
        assert gae(tio=dict(n_slots=0, n_steps=K + 1)) == -1 and b"dockauv_truncation_io.n_slots: 0" in err()
        assert gae(tio=dict(n_steps=K + 1, rows_out=4096)) == -1 and b"dockauv_truncation_io.n_steps: 5, " + whose + b" is 4" in err()
        assert gae(tio=dict(rows_out=4096, values=4096)) == -1 and b"dockauv_truncation_io.rows_out is not " + whose in err()
        assert gae(tio=dict(values=4096, advantages=4096)) == -1 and b"dockauv_truncation_io.values is not " + whose in err()
        assert gae(tio=dict(advantages=4096, returns=4096)) == -1 and b"dockauv_truncation_io.advantages is not " + whose in err()
        assert gae(tio=dict(returns=4096, gamma=0.5)) == -1 and b"dockauv_truncation_io.returns is not " + whose in err()
        assert gae(tio=dict(gamma=0.5, gae_lambda=0.5)) == -1 and b"dockauv_truncation_io.gamma: 0.5, " + whose + b" is 0.99" in err()
        assert gae(tio=dict(gae_lambda=0.5), crit=pol) == -1 and b"dockauv_truncation_io.gae_lambda: 0.5, " + whose + b" is 0.95" in err()
        assert gae(tio=dict(terminal_obs=4096), crit=pol) == -1 and b"not a critic" in err()   # (the call has no terminal_obs of its own)
        torch.cuda.synchronize()
    finally:
        e1.close()
        e2.close()
        e64.close()
