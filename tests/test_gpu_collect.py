"""The PPO collector on a real MI355X (include/dockauv.h: dockauv_value_create, dockauv_value_forward,
dockauv_policy_forward_logp, dockauv_gae, dockauv_collect; TorchDocking3d.collect): GAE against float64 and its stop at done,
the critic against float64 on 1, 129 and more rows than the device keeps resident and bit for bit independent of where a row
sits, the log-probabilities against the Philox statement, dockauv_collect against its parts bit for bit, the torch wrapper, and
refusals on a live handle.  Every batch is closed in `finally`."""
import copy
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SENTINEL = -7.0
GAMMA_LAMBDA = [(0.99, 0.95), (0.97, 0.90), (1.0, 1.0), (0.99, 0.0)]


def P():
    """the helpers of the policy tests: make_mlp, env_for, fan_env, nan_rows, recorded, FORWARD_BOUND"""
    from tests import test_gpu_policy
    return test_gpu_policy


def stream_of(torch):
    return torch.cuda.current_stream().cuda_stream


def bits(x):
    import torch
    return x.contiguous().view(torch.int32)


def make_critic(n_in, hidden, seed=11):
    return P().make_mlp((n_in, hidden, 1, "tanh", "none"), seed=seed)


# ------------------------------------------------------------------------------------------------------------------ GAE
def gae_inputs(K, N, n_obs, seed, force_first=True, force_last=True):
    """synthetic rows, no stepping: reward U(-1, 1), done with p = 0.05 plus forced dones at k = 0 and k = K - 1, values
    U(-2, 2), observation columns NaN (they must never be read)"""
    rng = np.random.default_rng(seed)
    reward = rng.uniform(-1, 1, (K, N)).astype(np.float32)
    done = rng.random((K, N)) < 0.05
    if force_first:
        done[0] = True
    if force_last:
        done[K - 1] = True
    values = rng.uniform(-2, 2, (K + 1, N)).astype(np.float32)
    rows = np.full((K, N, n_obs + 2), np.nan, dtype=np.float32)
    rows[:, :, n_obs] = reward
    rows[:, :, n_obs + 1] = done
    return rows, reward, done, values


def gae_float32_numpy(reward, done, values, gamma, lam):
    """the recurrence of the header in plain float32 NumPy (no fused multiply-add)"""
    K = reward.shape[0]
    g, l = np.float32(gamma), np.float32(lam)
    nt = (np.float32(1.0) - done.astype(np.float32)).astype(np.float32)
    adv = np.zeros_like(reward)
    gae = np.zeros(reward.shape[1], dtype=np.float32)
    for k in range(K - 1, -1, -1):
        delta = reward[k] + g * nt[k] * values[k + 1] - values[k]
        gae = delta + g * l * nt[k] * gae
        adv[k] = gae
    assert adv.dtype == np.float32
    return adv, adv + values[:K]


def gae_reference_and_bound(reward, done, values, gamma, lam):
    """(float64 advantages, bound on the device's max deviation from them): 8 x the error of the float32 NumPy restatement,
    floor 4 ulp of max |advantage|"""
    from gym_dockauv_amd.policy import MLPPolicy
    ref, _ = MLPPolicy.gae_reference(reward, done, values, gamma, lam)
    f32, _ = gae_float32_numpy(reward, done, values, gamma, lam)
    floor = 4.0 * float(np.spacing(np.float32(np.abs(ref).max())))
    return ref, max(8.0 * float(np.abs(f32.astype(np.float64) - ref).max()), floor)


def run_gae(torch, env, rows, values, K, N, gamma, lam, shift=0):
    """dockauv_gae into sentinel-filled buffers one row ([N] floats) longer than the outputs; the row must stay.  shift = 1:
    the rows start one float behind an allocation's start, so they are 4-byte and not 8-byte aligned"""
    d_rows = torch.empty(rows.size + shift, device="cuda")[shift:].view(rows.shape)
    d_rows.copy_(torch.from_numpy(rows))
    assert d_rows.data_ptr() % 8 == 4 * shift
    d_val = torch.from_numpy(values).cuda()
    adv = torch.full((K + 1, N), SENTINEL, device="cuda")
    ret = torch.full((K + 1, N), SENTINEL, device="cuda")
    env.gae_device(d_rows.data_ptr(), d_val.data_ptr(), K, gamma, lam, adv.data_ptr(), ret.data_ptr(), stream=stream_of(torch))
    torch.cuda.synchronize()
    assert bool((adv[K] == SENTINEL).all()) and bool((ret[K] == SENTINEL).all()), "the kernel wrote behind the last step's row"
    return adv[:K].cpu().numpy(), ret[:K].cpu().numpy()


@pytest.mark.parametrize("N", [1, 63, 257, 1000])
@pytest.mark.parametrize("n_obs", [20, 25], ids=["n_obs20-8byte", "n_obs25-4byte"])
def test_gae_against_float64(n_obs, N):
    """K in {1, 2, 67} (67: no multiple of the chunk of 8, and more than one) x the reference's two (gamma, lambda) pairs, (1, 1)
    and lambda = 0.  Bound: 8 x the error of the same recurrence in plain float32 NumPy against gae_reference (the margin
    test_saturated_tanh_units_against_float32_numpy gives a float32 restatement), floor 4 ulp of max |advantage|."""
    import torch
    from gym_dockauv_amd.policy import MLPPolicy
    env = P().fan_env(n_obs, 6, N)
    try:
        for K in (1, 2, 67):
            rows, reward, done, values = gae_inputs(K, N, n_obs, seed=100 * K + N)
            for gamma, lam in GAMMA_LAMBDA:
                adv, ret = run_gae(torch, env, rows, values, K, N, gamma, lam)
                assert not np.isnan(adv).any() and not np.isnan(ret).any(), "NaN: an observation column or an unwritten lane got in"
                ref_adv, ref_ret = MLPPolicy.gae_reference(reward, done, values, gamma, lam)
                np_adv, np_ret = gae_float32_numpy(reward, done, values, gamma, lam)
                floor = 4.0 * float(np.spacing(np.float32(np.abs(ref_adv).max())))
                for name, dev, f32, ref in (("advantages", adv, np_adv, ref_adv), ("returns", ret, np_ret, ref_ret)):
                    e_np = float(np.abs(f32.astype(np.float64) - ref).max())
                    e_dev = float(np.abs(dev.astype(np.float64) - ref).max())
                    bound = max(8.0 * e_np, floor)
                    print(f"gae n_obs {n_obs} N {N} K {K} gamma {gamma} lambda {lam} {name}: device {e_dev:.3e}, float32 NumPy "
                          f"{e_np:.3e}, bound {bound:.3e}")
                    assert e_dev <= bound, (name, K, gamma, lam, e_dev, bound)
    finally:
        env.close()


@pytest.mark.parametrize("force_first", [True, False], ids=["issue-inputs", "first-done-later"])
@pytest.mark.parametrize("n_obs", [20, 25])
def test_gae_stops_at_done(n_obs, force_first):
    """Changing every reward and value after an env's first done leaves the bits of advantages and returns up to and including
    that step as they were.  With the inputs of the test above every env is done at k = 0; the second variant drops that forced
    done, so that the first done falls anywhere in the window."""
    import torch
    K, N = 67, 257
    env = P().fan_env(n_obs, 6, N)
    try:
        rows, reward, done, values = gae_inputs(K, N, n_obs, seed=100 * K + N, force_first=force_first)
        first = done.argmax(axis=0)                                 # (every env is done at K - 1 at the latest)
        after = np.arange(K)[:, None] > first[None, :]              # steps after the first done
        rng = np.random.default_rng(1)
        rows2, values2 = rows.copy(), values.copy()
        rows2[:, :, n_obs][after] = rng.uniform(-1, 1, int(after.sum())).astype(np.float32)
        after_v = np.arange(K + 1)[:, None] > first[None, :]        # values[first + 1 ..]: masked out by the done
        values2[after_v] = rng.uniform(-2, 2, int(after_v.sum())).astype(np.float32)
        keep = ~after
        assert int(keep.sum()) >= N and (force_first or int(keep.sum()) > 4 * N)
        for gamma, lam in GAMMA_LAMBDA:
            a1, r1 = run_gae(torch, env, rows, values, K, N, gamma, lam)
            a2, r2 = run_gae(torch, env, rows2, values2, K, N, gamma, lam)
            assert np.array_equal(a1.view(np.int32)[keep], a2.view(np.int32)[keep])
            assert np.array_equal(r1.view(np.int32)[keep], r2.view(np.int32)[keep])
            if not force_first:
                assert not np.array_equal(a1.view(np.int32)[after], a2.view(np.int32)[after])
    finally:
        env.close()


@pytest.mark.parametrize("shift", [0, 1], ids=["rows-8byte-aligned", "rows-4byte-aligned"])
@pytest.mark.parametrize("n_obs", [20, 25])
def test_gae_bootstraps_from_the_last_value(n_obs, shift):
    """The inputs of test_gae_against_float64 without the forced dones, so that most envs are not done at k = K - 1 and
    values[K] enters through the bootstrap; K = 5 (a single chunk that reaches below step 0) and 67; same bound.  Another
    values[K] changes the advantages of exactly the envs whose last segment is open.  The rows also one float off an 8-byte
    boundary: the reward / done pair of an even n_obs is then an 8-byte load at a 4-byte aligned address."""
    import torch
    N = 257
    env = P().fan_env(n_obs, 6, N)
    try:
        for K in (5, 67):
            rows, reward, done, values = gae_inputs(K, N, n_obs, seed=7 * K + N, force_first=False, force_last=False)
            open_end = ~done[K - 1]
            assert int(open_end.sum()) > N // 2
            for gamma, lam in GAMMA_LAMBDA:
                adv, ret = run_gae(torch, env, rows, values, K, N, gamma, lam, shift=shift)
                assert not np.isnan(adv).any() and not np.isnan(ret).any()
                ref, bound = gae_reference_and_bound(reward, done, values, gamma, lam)
                err = float(np.abs(adv.astype(np.float64) - ref).max())
                print(f"gae bootstrap n_obs {n_obs} shift {shift} K {K} gamma {gamma} lambda {lam}: device {err:.3e}, bound {bound:.3e}")
                assert err <= bound, (K, gamma, lam, err, bound)
                assert np.array_equal(ret.view(np.int32), (adv + values[:K]).view(np.int32))
                values2 = values.copy()
                values2[K] += 1.0
                adv2, _ = run_gae(torch, env, rows, values2, K, N, gamma, lam, shift=shift)
                changed = adv2[K - 1].view(np.int32) != adv[K - 1].view(np.int32)
                assert np.array_equal(changed, open_end)
    finally:
        env.close()


# --------------------------------------------------------------------------------------------------------------- values
def value_env(n_in):
    p = P()
    return p.env_for(20, 6, 64) if n_in == 20 else (p.env_for(36, 3, 64) if n_in == 36 else p.fan_env(25, 6, 64))


def values_of(torch, env, val, rows):
    """dockauv_value_forward into a guarded buffer"""
    n = rows.shape[0]
    out = torch.full((n + 64,), SENTINEL, device="cuda")
    env.value_forward_device(val, rows.data_ptr(), n, out.data_ptr(), stream=stream_of(torch))
    torch.cuda.synchronize()
    assert bool((out[n:] == SENTINEL).all()), "the kernel wrote behind the last row's value"
    return out[:n]


@pytest.mark.parametrize("shape", [(20, (64, 64)), (36, (128,)), (25, (17, 33))], ids=["20-64-64-1", "36-128-1", "25-17-33-1"])
def test_values_match_float64(shape):
    """1 row, 129 rows (a group plus one lane) and 8 x CUs x 128 + 33 rows: more groups than a device keeps resident (at most 8
    groups of four waves per CU) and a last group with one partial tile, not tied to the batch's 64 envs.  The same 1 000 rows
    alone and at offset 777 of the large call give the same bits."""
    import torch
    p = P()
    n_in, hidden = shape
    critic = make_critic(n_in, hidden)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    env = value_env(n_in)
    try:
        val = env.make_value(critic)
        big_n = cus * 8 * 128 + 33
        big = p.nan_rows(torch, big_n, n_in, seed=3)
        v_big = values_of(torch, env, val, big)
        for n in (1, 129, big_n):
            rows = big if n == big_n else p.nan_rows(torch, n, n_in, seed=2 + n)
            v = (v_big if n == big_n else values_of(torch, env, val, rows)).cpu().numpy()
            assert not np.isnan(v).any() and not (v == SENTINEL).any()
            ref = critic.forward_reference(rows[:, :n_in].cpu().numpy().astype(np.float64))[:, 0]
            err = float(np.abs(v - ref).max())
            print(f"value {n_in}-{'-'.join(map(str, hidden))}-1, {n} rows: max |V - V_f64| = {err:.3e} (bound {p.FORWARD_BOUND:g})")
            assert err <= p.FORWARD_BOUND
        small = big[777:1777].clone()
        v_small = values_of(torch, env, val, small)
        assert torch.equal(bits(v_small), bits(v_big[777:1777]))
    finally:
        env.close()


# ------------------------------------------------------------------------------------------------------------- log-prob
@pytest.mark.parametrize("n_u", [3, 8])
def test_log_prob_is_the_philox_statement(n_u):
    """log_std distinct per action, 3 actions (lane half 0) and 8 (both halves, registers 2 and 3).  Stochastic: against
    log_prob_reference of the statement's normals; a deviation dz of a normal changes its term by |z| dz + dz^2 / 2, dz bounded
    by the recorded exploration bound.  Deterministic: -sum log_std - n_u / 2 log(2 pi).  The actions are those of
    dockauv_policy_forward, bit for bit."""
    import torch
    from gym_dockauv_amd.policy import MLPPolicy
    p = P()
    N, seed, t = 1000, 0xC0FFEE1234, 17
    zb = min(4.0 * p.recorded("exploration_max_dev"), p.EXPLORATION_CAP)
    log_std = np.linspace(-1.5, 0.3, n_u)
    mlp = p.make_mlp((36, (64, 64), n_u, "tanh", "none"), seed=1, log_std=log_std)
    env = p.env_for(36, n_u, N)
    try:
        pol = env.make_policy(mlp, seed=seed)
        rows = p.nan_rows(torch, N, 36, seed=2)
        out = {}
        for sto in (False, True):
            a0 = torch.full((N + 64, n_u), SENTINEL, device="cuda")
            a1 = torch.full((N + 64, n_u), SENTINEL, device="cuda")
            lp = torch.full((N + 64,), SENTINEL, device="cuda")
            env.policy_forward_device(pol, rows.data_ptr(), a0.data_ptr(), t=t, stochastic=sto, stream=stream_of(torch))
            env.policy_forward_logp_device(pol, rows.data_ptr(), a1.data_ptr(), lp.data_ptr(), t=t, stochastic=sto, stream=stream_of(torch))
            torch.cuda.synchronize()
            assert bool((a1[N:] == SENTINEL).all()) and bool((lp[N:] == SENTINEL).all())
            assert torch.equal(bits(a0), bits(a1)) and not torch.isnan(a1).any()
            out[sto] = lp[:N].cpu().numpy().astype(np.float64)
            assert not np.isnan(out[sto]).any() and not (out[sto] == SENTINEL).any()
        # without a log_std, and with a tanh output: refused
        plain = env.make_policy(p.make_mlp((36, (64, 64), n_u, "tanh", "none"), seed=1))
        squashed = env.make_policy(p.make_mlp((36, (64, 64), n_u, "tanh", "tanh"), seed=1, log_std=log_std))
        for bad, needle in ((plain, "log_std"), (squashed, "DOCKAUV_ACT_TANH")):
            with pytest.raises(_capi().DockAUVError, match=needle):
                env.policy_forward_logp_device(bad, rows.data_ptr(), a1.data_ptr(), lp.data_ptr(), t=t, stochastic=True)
    finally:
        env.close()
    z = MLPPolicy.normals_reference(seed, np.arange(N), t, n_u)
    ref = MLPPolicy.log_prob_reference(z, mlp.log_std)
    bound = (np.abs(z) * zb + 0.5 * zb * zb).sum(axis=1) + 1e-5 * (1.0 + np.abs(ref))
    dev = np.abs(out[True] - ref)
    print(f"log_prob n_u {n_u} stochastic: max |lp - lp_ref| = {dev.max():.3e}, smallest bound {bound.min():.3e}, "
          f"worst ratio {(dev / bound).max():.3f}")
    assert np.all(dev <= bound)
    det = -float(mlp.log_std.astype(np.float64).sum()) - 0.5 * n_u * np.log(2.0 * np.pi)
    print(f"log_prob n_u {n_u} deterministic: max |lp - lp_ref| = {np.abs(out[False] - det).max():.3e} (bound 1e-5)")
    assert np.abs(out[False] - det).max() <= 1e-5
    assert np.abs(out[True] - det).max() > 0.1


def _capi():
    from gym_dockauv_amd import _capi
    return _capi


def _logp_tile_pairs():
    """the shapes of test_every_tile_pair_matches_float64 with a raw output (the log-probability of a squashed one is refused)"""
    from tests import test_gpu_policy as p
    return [(s[0], s[1], s[2], s[3], "none") for s in p.TILE_PAIRS + [p.WIDEST]]


@pytest.mark.parametrize("shape", _logp_tile_pairs(), ids=lambda s: f"{s[0]}-{'-'.join(map(str, s[1]))}-{s[2]}-{s[3]}")
def test_every_log_prob_tile_pair(shape):
    """Each of the 20 instantiations of the actor kernel with the log-probability epilogue (and the widest accepted shape) at
    129 envs (a group plus one lane), stochastic: the actions are those of dockauv_policy_forward bit for bit, within 1e-5 of
    float64 given the statement's normals (plus std x the exploration bound), and the log-probability is within the bound of
    test_log_prob_is_the_philox_statement."""
    import torch
    from gym_dockauv_amd.policy import MLPPolicy
    p = P()
    N, seed, t, n_in, n_u = 129, 0xABCDEF, 5, shape[0], shape[2]
    zb = min(4.0 * p.recorded("exploration_max_dev"), p.EXPLORATION_CAP)
    log_std = np.linspace(-1.5, 0.3, n_u)
    mlp = p.make_mlp(shape, seed=1, log_std=log_std)
    env = p.fan_env(n_in, n_u, N)
    try:
        pol = env.make_policy(mlp, seed=seed)
        rows = p.nan_rows(torch, N, n_in, seed=2)
        a0 = torch.full((N + 64, n_u), SENTINEL, device="cuda")
        a1 = torch.full((N + 64, n_u), SENTINEL, device="cuda")
        lp = torch.full((N + 64,), SENTINEL, device="cuda")
        env.policy_forward_device(pol, rows.data_ptr(), a0.data_ptr(), t=t, stochastic=True, stream=stream_of(torch))
        env.policy_forward_logp_device(pol, rows.data_ptr(), a1.data_ptr(), lp.data_ptr(), t=t, stochastic=True, stream=stream_of(torch))
        torch.cuda.synchronize()
        assert bool((a1[N:] == SENTINEL).all()) and bool((lp[N:] == SENTINEL).all())
        assert torch.equal(bits(a0), bits(a1)) and not torch.isnan(a1).any() and not bool((a1[:N] == SENTINEL).any())
        obs = rows[:, :n_in].cpu().numpy().astype(np.float64)
        got_a, got_lp = a1[:N].cpu().numpy().astype(np.float64), lp[:N].cpu().numpy().astype(np.float64)
    finally:
        env.close()
    z = MLPPolicy.normals_reference(seed, np.arange(N), t, n_u)
    assert np.abs(got_a - mlp.forward_reference(obs, z=z)).max() <= p.FORWARD_BOUND + float(np.exp(log_std).max()) * zb
    ref = MLPPolicy.log_prob_reference(z, mlp.log_std)
    assert np.all(np.abs(got_lp - ref) <= (np.abs(z) * zb + 0.5 * zb * zb).sum(axis=1) + 1e-5 * (1.0 + np.abs(ref)))


# -------------------------------------------------------------------------------------------------------------- collect
@pytest.mark.parametrize("case", ["B", "C", "D"])
def test_collect_equals_its_parts_bitwise(case):
    """dockauv_collect on one handle against dockauv_rollout, dockauv_value_forward (rows_in; all of rows_out),
    dockauv_policy_forward_logp per step and dockauv_gae on a twin with the same seed: rows, actions, terminal observations where
    done, values, log-probabilities, advantages and returns as int32 bits; with critic = NULL the rows and actions of
    dockauv_rollout.  max_timesteps = 5 puts in-kernel resets inside the window of K = 12 steps.  B: config 4, C: config 5 at 778
    envs (mixed batch), D: direct thruster control at 1 000 envs (the cases of test_rollout_equals_stepwise_bitwise)."""
    import torch
    p = P()
    n_in, n_out, N = {"B": (36, 3, 2048 + 17), "C": (36, 6, 778), "D": (36, 8, 1000)}[case]
    K, gamma, lam, t0 = 12, 0.99, 0.95, 100
    mlp = p.make_mlp((n_in, (64, 64), n_out, "tanh", "none"), seed=4, log_std=np.full(n_out, -2.0 if case == "D" else -0.5))
    critic = make_critic(n_in, (64, 64))
    envs = [p.env_for(n_in, n_out, N, max_timesteps=5) for _ in range(3)]
    try:
        e1, e2, e3 = envs
        pols = [e.make_policy(mlp, seed=21) for e in envs]
        vals = [e.make_value(critic) for e in envs[:2]]
        s = stream_of(torch)
        mk = lambda *shape: torch.zeros(shape, device="cuda")
        rows0 = mk(N, n_in + 2)

        def buffers():
            return dict(rows=mk(K, N, n_in + 2), acts=mk(K, N, n_out), term=mk(K, N, n_in), logp=mk(K, N), values=mk(K + 1, N),
                        adv=mk(K, N), ret=mk(K, N))
        b1, b2, b3 = buffers(), buffers(), buffers()
        e1.collect_device(pols[0], vals[0], rows0.data_ptr(), b1["rows"].data_ptr(), b1["acts"].data_ptr(), K, gamma=gamma,
                          gae_lambda=lam, t0=t0, stochastic=True, stream=s, terminal_obs_ptr=b1["term"].data_ptr(),
                          log_prob_ptr=b1["logp"].data_ptr(), values_ptr=b1["values"].data_ptr(),
                          advantages_ptr=b1["adv"].data_ptr(), returns_ptr=b1["ret"].data_ptr())
        # the parts
        e2.rollout_device(pols[1], rows0.data_ptr(), b2["rows"].data_ptr(), b2["acts"].data_ptr(), K, t0=t0, stochastic=True,
                          stream=s, terminal_obs_ptr=b2["term"].data_ptr())
        e2.value_forward_device(vals[1], rows0.data_ptr(), N, b2["values"][0].data_ptr(), stream=s)
        e2.value_forward_device(vals[1], b2["rows"].data_ptr(), K * N, b2["values"][1].data_ptr(), stream=s)
        again = mk(K, N, n_out)
        for k in range(K):
            src = rows0 if k == 0 else b2["rows"][k - 1]
            e2.policy_forward_logp_device(pols[1], src.data_ptr(), again[k].data_ptr(), b2["logp"][k].data_ptr(), t=t0 + k,
                                          stochastic=True, stream=s)
        e2.gae_device(b2["rows"].data_ptr(), b2["values"].data_ptr(), K, gamma, lam, b2["adv"].data_ptr(), b2["ret"].data_ptr(), stream=s)
        # critic = NULL
        e3.collect_device(pols[2], None, rows0.data_ptr(), b3["rows"].data_ptr(), b3["acts"].data_ptr(), K, t0=t0, stochastic=True,
                          stream=s, log_prob_ptr=b3["logp"].data_ptr())
        torch.cuda.synchronize()
        for e in envs:
            e.poll_status()
        for name in ("rows", "acts", "values", "logp", "adv", "ret"):
            assert not torch.isnan(b1[name]).any(), name
            assert torch.equal(bits(b1[name]), bits(b2[name])), name
        assert torch.equal(bits(again), bits(b2["acts"]))
        done = b1["rows"][:, :, n_in + 1] > 0.5
        assert int(done.sum()) > N and bool(done[1:K - 1].any()), "no episode ended inside the window"
        assert torch.equal(bits(b1["term"])[done], bits(b2["term"])[done])
        assert torch.equal(bits(b3["rows"]), bits(b2["rows"])) and torch.equal(bits(b3["acts"]), bits(b2["acts"]))
        assert torch.equal(bits(b3["logp"]), bits(b2["logp"]))
        # what was computed is the critic and the recurrence: float64 on the device's rows
        obs = torch.cat([rows0[None], b1["rows"]])[:, :, :n_in].cpu().numpy().astype(np.float64)
        v_ref = critic.forward_reference(obs)[:, :, 0]
        assert np.abs(b1["values"].cpu().numpy() - v_ref).max() <= p.FORWARD_BOUND
        a_ref, bound = gae_reference_and_bound(b1["rows"][:, :, n_in].cpu().numpy(), done.cpu().numpy(), b1["values"].cpu().numpy(), gamma, lam)
        assert float(b1["adv"].abs().max()) > 0 and np.abs(b1["adv"].cpu().numpy() - a_ref).max() <= bound
    finally:
        for e in envs:
            e.close()


def test_torch_env_collect():
    import torch
    import bench
    from gym_dockauv_amd.envs.torch_env import TorchDocking3d
    p = P()
    N, gamma, lam = 1000, 0.99, 0.95
    wl = bench.workload(3, N)
    cfg = copy.deepcopy(wl["cfg"])
    cfg["max_timesteps"] = 6
    mlp = p.make_mlp((20, (64, 64), 6, "tanh", "none"), seed=6, log_std=np.full(6, -0.5))
    critic = make_critic(20, (64, 64))

    def make():
        env = TorchDocking3d(cfg, num_envs=N, scenario=wl["scenario"], device_seed=9)
        env.batch._gen = np.random.default_rng(5)
        env.reset()
        return env
    ea, eb, ec = make(), make(), make()
    try:
        (pa, pb, pc), (va, vb) = [e.make_policy(mlp, seed=3) for e in (ea, eb, ec)], [e.make_value(critic) for e in (ea, eb)]
        c1 = ea.collect(pa, va, 8, gamma, lam)
        assert tuple(c1.obs.shape) == (9, N, 20) and tuple(c1.actions.shape) == (8, N, 6) and tuple(c1.values.shape) == (9, N)
        for x in (c1.reward, c1.done, c1.log_prob, c1.advantages, c1.returns):
            assert tuple(x.shape) == (8, N)
        assert c1.done.dtype == torch.bool and c1.obs.dtype == c1.log_prob.dtype == c1.returns.dtype == torch.float32
        first = [x.clone() for x in c1]                  # (the next collect of the same K reuses the buffers)
        c2 = ea.collect(pa, va, 8, gamma, lam)
        assert c2.obs.data_ptr() == c1.obs.data_ptr()
        c16 = eb.collect(pb, vb, 16, gamma, lam)
        ro, ra, rr, rd = ec.rollout(pc, 16, stochastic=True)
        torch.cuda.synchronize()
        assert torch.equal(bits(first[0][8]), bits(c2.obs[0]))                 # obs[K] of one collect is obs[0] of the next
        assert torch.equal(bits(torch.cat([first[0][:8], c2.obs])), bits(c16.obs))
        assert torch.equal(bits(torch.cat([first[1], c2.actions])), bits(c16.actions))
        assert torch.equal(bits(torch.cat([first[2], c2.reward])), bits(c16.reward))
        assert torch.equal(torch.cat([first[3], c2.done]), c16.done) and bool(c16.done.any())
        assert torch.equal(bits(torch.cat([first[4], c2.log_prob])), bits(c16.log_prob))
        # against rollout: obs[k + 1] is rollout's obs[k]
        assert torch.equal(bits(c16.obs[1:]), bits(ro)) and torch.equal(bits(c16.actions), bits(ra))
        assert torch.equal(bits(c16.reward), bits(rr)) and torch.equal(c16.done, rd)
        assert ea._t == eb._t == ec._t == 16
        for c in (c2, c16):
            K = c.advantages.shape[0]
            assert torch.equal(bits(c.returns), bits(c.advantages + c.values[:K]))
            a_ref, bound = gae_reference_and_bound(c.reward.cpu().numpy(), c.done.cpu().numpy(), c.values.cpu().numpy(), gamma, lam)
            assert np.abs(c.advantages.cpu().numpy() - a_ref).max() <= bound
        # new critic weights from device tensors: the values change and are those of the new weights
        new = make_critic(20, (64, 64), seed=77)
        old_values = c16.values.clone()
        eb.load_policy(vb, [torch.from_numpy(a).cuda() for Wb in new.layers for a in Wb])
        c = eb.collect(pb, vb, 16, gamma, lam)
        torch.cuda.synchronize()
        ref = new.forward_reference(c.obs.cpu().numpy().astype(np.float64))[:, :, 0]
        err = float(np.abs(c.values.cpu().numpy() - ref).max())
        print(f"load_policy of a critic from device tensors: max |V - V_f64(new weights)| = {err:.3e}")
        assert err <= p.FORWARD_BOUND and float((c.values - old_values).abs().max()) > 1e-2
        # mixing with rollout: one trajectory (ea and ec are both 16 steps in); without a critic: rollout and log-prob only
        o_r, a_r, _, _ = ea.rollout(pa, 2, stochastic=True)
        c_n = ec.collect(pc, None, 2, gamma, lam)
        torch.cuda.synchronize()
        assert c_n.values is None and c_n.advantages is None and c_n.returns is None
        assert torch.equal(bits(o_r), bits(c_n.obs[1:])) and torch.equal(bits(a_r), bits(c_n.actions))
        assert torch.equal(bits(c_n.obs[0]), bits(ro[15]))
    finally:
        for e in (ea, eb, ec):
            e.close()


def test_refusals_on_a_live_handle():
    import torch
    capi = _capi()
    lib = capi.load_library()
    p = P()
    mlp = p.make_mlp((20, (64, 64), 6, "tanh", "none"), seed=1, log_std=np.full(6, -0.5))
    critic = make_critic(20, (64, 64))
    e64 = p.env_for(20, 6, 256, precision="f64")
    try:
        d = critic.host_desc()
        ptr = C.c_void_p()
        assert lib.dockauv_value_create(e64._handle, C.byref(d), C.byref(ptr)) == -1 and not ptr.value
        assert b"float32" in lib.dockauv_last_error(e64._handle)
        fake = C.c_void_p(8)
        assert lib.dockauv_gae(e64._handle, fake, fake, 2, 0.99, 0.95, fake, fake, None) == -1
        assert b"float32" in lib.dockauv_last_error(e64._handle)
    finally:
        e64.close()
    env, other = p.env_for(20, 6, 256), p.env_for(20, 6, 256)
    try:
        K, N = 3, 256
        pol, val = env.make_policy(mlp), env.make_value(critic)
        o_pol, o_val = other.make_policy(mlp), other.make_value(critic)
        z = lambda *shape: torch.zeros(shape, device="cuda")
        rows0, rows, acts, logp, values, adv, ret = z(N, 22), z(K, N, 22), z(K, N, 6), z(K, N), z(K + 1, N), z(K, N), z(K, N)
        err = lambda: lib.dockauv_last_error(env._handle)

        def collect(actor, crit, **nulls):
            io = capi.CollectIO()
            io.struct_size = C.sizeof(capi.CollectIO)
            io.n_steps = K
            io.rows_in, io.rows_out, io.actions_out, io.log_prob = rows0.data_ptr(), rows.data_ptr(), acts.data_ptr(), logp.data_ptr()
            io.values, io.advantages, io.returns = values.data_ptr(), adv.data_ptr(), ret.data_ptr()
            io.gamma, io.gae_lambda, io.stochastic = 0.99, 0.95, 1
            for k in nulls:
                setattr(io, k, None)
            return lib.dockauv_collect(env._handle, actor.ptr, crit.ptr if crit is not None else None, C.byref(io), None)
        # an actor in the critic slot, and the reverse
        assert collect(pol, pol) == -1 and b"not a critic" in err()
        assert collect(val, val) == -1 and b"is a critic" in err()
        assert lib.dockauv_value_forward(env._handle, pol.ptr, rows0.data_ptr(), N, values.data_ptr(), None) == -1 and b"not a critic" in err()
        assert lib.dockauv_policy_forward(env._handle, val.ptr, rows0.data_ptr(), acts.data_ptr(), 0, 0, None) == -1 and b"is a critic" in err()
        assert lib.dockauv_policy_forward_logp(env._handle, val.ptr, rows0.data_ptr(), acts.data_ptr(), logp.data_ptr(), 0, 0, None) == -1
        assert b"is a critic" in err()
        assert lib.dockauv_rollout(env._handle, val.ptr, rows0.data_ptr(), rows.data_ptr(), acts.data_ptr(), None, K, 0, 0, None) == -1
        assert b"is a critic" in err()
        # a policy / critic of another handle
        assert collect(o_pol, val) == -1 and b"another handle" in err()
        assert collect(pol, o_val) == -1 and b"another handle" in err()
        assert lib.dockauv_value_forward(env._handle, o_val.ptr, rows0.data_ptr(), N, values.data_ptr(), None) == -1 and b"another handle" in err()
        # values NULL with a critic; critic buffers without one
        assert collect(pol, val, values=None) == -1 and b"with a critic" in err()
        assert collect(pol, None) == -1 and b"without a critic" in err()
        # two defects at once: the first in the order of checks is the one reported (tests/test_collect_precedence_host.py has what
        # is checked before the handle): the block before the actor, the actor before the critic
        assert collect(o_pol, val, values=None) == -1 and b"with a critic" in err()
        assert collect(o_pol, None) == -1 and b"without a critic" in err()
        assert collect(o_pol, o_val) == -1 and b"dockauv_collect: the policy was created for another handle" in err()
        assert collect(o_pol, pol) == -1 and b"dockauv_collect: the policy was created for another handle" in err()
        assert collect(val, pol) == -1 and b"dockauv_collect: the policy is a critic" in err()
        assert collect(val, o_val) == -1 and b"dockauv_collect: the policy is a critic" in err()
        # gamma outside [0, 1]; a critic whose input width is not the handle's; an actor's n_out is still the handle's n_u
        with pytest.raises(capi.DockAUVError, match="gamma"):
            env.gae_device(rows.data_ptr(), values.data_ptr(), K, 1.5, 0.95, adv.data_ptr(), ret.data_ptr())
        with pytest.raises(capi.DockAUVError, match="n_in"):
            env.make_value(make_critic(36, (64, 64)))
        with pytest.raises(capi.DockAUVError, match="n_out"):
            env.make_policy(critic)
        # a reload of the critic must keep the shapes ... and with them it is taken; then everything still runs
        with pytest.raises(capi.DockAUVError, match="differ from the policy"):
            env.load_policy(val, make_critic(20, (64, 32)))
        env.load_policy(val, make_critic(20, (64, 64), seed=5))
        assert collect(pol, val) == 0
        assert collect(pol, None, values=None, advantages=None, returns=None) == 0
        torch.cuda.synchronize()
        env.poll_status()
        assert float(values.abs().max()) > 0 and not torch.isnan(adv).any()
    finally:
        env.close()
        other.close()
