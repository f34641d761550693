"""The gradient-free half of SAC on a real MI355X (include/dockauv.h: dockauv_sac_actor_*, dockauv_q_*, dockauv_sac_target;
TorchDocking3d.make_sac_actor / make_q / q_values / sac_target): the squashed-Gaussian actor against its plain twin bit for bit,
the clamp, Q critics on [obs | action] dense and through an index (an odd n_obs straddles the two sources inside one k step),
the TD target's four launches against the public calls one by one and against ``sac_target_reference``, the ring against the
sampled copies, ``rb.rollout`` with the actor against the same steps issued one by one, the slot-5 normals, refusals on a live
handle, and the float64 comparisons.

Shapes: 1 (one lane), 33 (a tile and a lane) and 129 rows (a group and a lane); hidden (17,), (64, 64) and (128, 128) -- the
launch that asks for more than 64 KiB of LDS -- and, on 33 rows, one shape per (MT1, MT2) so that every instantiation of the three
tile kernels is launched (profiles/coverage/kernels.txt); (n_obs, n_u) = (20, 6), (36, 3), (36, 8), and 25 (odd) for the Q straddle.  Output
buffers carry sentinel rows; the reward and done columns of packed rows are NaN.

Not tested exactly: the Gaussian part of the log-probability on its own.  The kernel returns one sum; taking the correction
off it again is a float32 subtraction that is not exact, so the exact checks are on the actions (which fix mu, std and z) and
the float64 comparison holds the sum.  The rows form of the actor (stream slot 5) has no public call of its own, so its launch
inside dockauv_sac_target is held to float64 and to the Philox statement, not to another call's bits.

Measured figures: profiles/sac/logp_error.txt (scripts/sac_error.py, from the helpers of this file)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SENTINEL = -7.0
FORWARD_BOUND = 1e-5          # tests/test_gpu_policy.py: the project's float32 bar
LOGP_CAP = 1e-3
TANH_ERR = 3e-7               # csrc/dockauv_policy_tile.h: tanh_'s absolute error
HIDDEN = [(17,), (64, 64), (128, 128)]
OBS_ACT = [(20, 6), (36, 3), (36, 8)]
CASES = list(zip(OBS_ACT, HIDDEN))


def P():
    from tests import test_gpu_policy
    return test_gpu_policy


def H():
    from tests import test_sac_host
    return test_sac_host


def u32(x):
    if not isinstance(x, np.ndarray):
        x = x.detach().cpu().numpy()
    return np.ascontiguousarray(x).view(np.uint32) if x.dtype == np.float32 else x


def stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def const_std_actor(n_in, hidden, n_u, c, seed=1):
    """an actor whose log_std head is W_ls = 0, b_ls = c, and its plain twin with log_std = clamp(c)"""
    from gym_dockauv_amd.policy import SquashedGaussianMLP
    base = P().make_mlp((n_in, hidden, n_u, "tanh", "tanh"), seed=seed)
    c = np.asarray(c, dtype=np.float32)
    sac = SquashedGaussianMLP(base.layers[:-1], base.layers[-1], (np.zeros_like(base.layers[-1][0]), c), "tanh")
    return sac, sac.plain_twin("tanh", np.clip(c, -20.0, 2.0))


def fwd(env, pol, rows, t=0, stochastic=False, logp=False):
    """per-env forward into guarded buffers: (actions [n, n_u], log_prob [n] or None)"""
    import torch
    n = rows.shape[0]
    acts = torch.full((n + 64, env.n_u), SENTINEL, device="cuda")
    lp = torch.full((n + 64,), SENTINEL, device="cuda") if logp else None
    if logp:
        env.policy_forward_logp_device(pol, rows.data_ptr(), acts.data_ptr(), lp.data_ptr(), t=t, stochastic=stochastic, stream=stream())
    else:
        env.policy_forward_device(pol, rows.data_ptr(), acts.data_ptr(), t=t, stochastic=stochastic, stream=stream())
    torch.cuda.synchronize()
    assert bool((acts[n:] == SENTINEL).all()) and (lp is None or bool((lp[n:] == SENTINEL).all())), "written behind the last row"
    assert not bool((acts[:n] == SENTINEL).any()) and not bool(torch.isnan(acts[:n]).any())
    return acts[:n], (None if lp is None else lp[:n])


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[0][0]}-{'-'.join(map(str, c[1]))}-{c[0][1]}")
def test_actions_are_the_plain_twins_bit_for_bit(case):
    """Deterministic: the bits of the plain policy with W3 = W_mu, b3 = b_mu, out_act = TANH.  Stochastic with W_ls = 0, b_ls = c
    (per action, the ends -20 and 2 among them): those of that policy with log_std = c, same seed and t.  The log-probability form
    returns the same actions.  b_ls = +5 gives the bits of 2, -30 those of -20 (actions and log-probability)."""
    import torch
    (n_in, n_u), hidden = case
    c = np.linspace(-20.0, 2.0, n_u).astype(np.float32)
    c[1:-1] = np.array([-1.5, -0.25, 0.5, -3.0, 1.25, -0.75])[: n_u - 2]
    sac, twin = const_std_actor(n_in, hidden, n_u, c)
    over, _ = const_std_actor(n_in, hidden, n_u, np.where(c >= 2.0, 5.0, np.where(c <= -20.0, -30.0, c)))
    for n in (1, 33, 129):
        env = P().env_for(n_in, n_u, n)
        try:
            a, p, o = env.make_sac_actor(sac, seed=11), env.make_policy(twin, seed=11), env.make_sac_actor(over, seed=11)
            rows = P().nan_rows(torch, n, n_in, seed=2)
            for stochastic in (False, True):
                got, _ = fwd(env, a, rows, t=5, stochastic=stochastic)
                want, _ = fwd(env, p, rows, t=5, stochastic=stochastic)
                assert np.array_equal(u32(got), u32(want)), (n, stochastic)
                got_lp, lp = fwd(env, a, rows, t=5, stochastic=stochastic, logp=True)
                assert np.array_equal(u32(got_lp), u32(got)) and not bool(torch.isnan(lp).any())
                o_a, o_lp = fwd(env, o, rows, t=5, stochastic=stochastic, logp=True)
                assert np.array_equal(u32(o_a), u32(got)) and np.array_equal(u32(o_lp), u32(lp)), "the clamp"
            det, _ = fwd(env, a, rows, t=5)
            sto, _ = fwd(env, a, rows, t=5, stochastic=True)
            sto6, _ = fwd(env, a, rows, t=6, stochastic=True)
            assert not np.array_equal(u32(det), u32(sto)) and not np.array_equal(u32(sto), u32(sto6))
        finally:
            env.close()


def device_normals(env, n_in, n_u, rows, seed, t):
    """the normals the per-env actors draw, as bits: a plain policy with W3 = 0, b3 = 0, log_std = 0 returns fmaf(1, z, 0) = z"""
    from gym_dockauv_amd.policy import MLPPolicy
    zero = MLPPolicy([(np.zeros((8, n_in)), np.zeros(8)), (np.zeros((n_u, 8)), np.zeros(n_u))], "tanh", "none", np.zeros(n_u))
    z, _ = fwd(env, env.make_policy(zero, seed=seed), rows, t=t, stochastic=True)
    return z.cpu().numpy()


def logp_errors(name, n=4096):
    """(device error, float32-NumPy error, max |x|) of the log-probability of case `name` (tests/test_sac_host.py: logp_cases)
    against forward_reference fed the device's own z; also checks the actions (scripts/sac_error.py records the figures)"""
    import torch
    mlp = H().logp_cases()[name]
    env = P().env_for(20, 6, n)
    try:
        rows = P().nan_rows(torch, n, 20, seed=4)
        obs = rows[:, :20].cpu().numpy()
        z = device_normals(env, 20, 6, rows, seed=13, t=9)
        ref = MLPPolicy_normals(13, n, 9, 6)
        assert np.abs(z - ref).max() <= P().EXPLORATION_CAP, "the recovered normals are not the Philox statement's"
        a, lp = fwd(env, env.make_sac_actor(mlp, seed=13), rows, t=9, stochastic=True, logp=True)
        a64, lp64, mu, ls = mlp.forward_reference(obs.astype(np.float64), z.astype(np.float64))
        a32, lp32 = mlp.forward_float32(obs, z)
        assert np.abs(a.cpu().numpy() - a64).max() <= FORWARD_BOUND
        dev = float(np.abs(lp.cpu().numpy().astype(np.float64) - lp64).max())
        f32 = float(np.abs(lp32.astype(np.float64) - lp64).max())
        return dev, f32, float(np.abs(mu + np.exp(ls) * z).max())
    finally:
        env.close()


def MLPPolicy_normals(seed, n, t, n_u, slot=2, offset=0):
    from gym_dockauv_amd.policy import MLPPolicy
    return MLPPolicy.normals_reference(seed, offset + np.arange(n), t, n_u, slot=slot)


@pytest.mark.parametrize("name", ["default", "wide_std"])
def test_log_prob_against_float64(name):
    """The device within 8 x the error of a float32 NumPy evaluation of the same expressions (the margin the policy tests give a
    reordered float32 chain), and under an absolute cap of 1e-3 so that the ratio cannot hide a broken correction."""
    dev, f32, reach = logp_errors(name)
    print(f"log-prob error, {name}: device {dev:.3e}, float32 NumPy {f32:.3e} (bound {8 * f32:.3e}, cap {LOGP_CAP:g}); max |x| = {reach:.2f}")
    assert f32 <= LOGP_CAP
    assert dev <= 8 * f32 and dev <= LOGP_CAP


def q_mlp(n_obs, n_u, hidden, seed):
    return P().make_mlp((n_obs + n_u, hidden, 1, "relu", "none"), seed=seed)


# one shape per (tiles of hidden layer 1, tiles of hidden layer 2): the 20 instantiations of each of the three kernels
ALL_TILES = [(h1, h2) if h2 else (h1,) for h1 in (17, 33, 96, 128) for h2 in (0, 32, 63, 65, 128)]


@pytest.mark.parametrize("hidden", ALL_TILES, ids=lambda h: "-".join(map(str, h)))
def test_every_instantiation_against_float64(hidden):
    """sac_actor_kernel, sac_actor_logp_kernel and q_kernel of every (MT1, MT2) on 33 rows (a tile and a lane) of the (20, 6) env:
    actions and q within 1e-5 of float64, the log-probability (float64 fed the device's own normals) within the absolute cap."""
    import torch
    n = 33
    env = P().env_for(20, 6, n)
    try:
        mlp = H().default_actor(20, hidden, 6, seed=50)
        rows = P().nan_rows(torch, n, 20, seed=3)
        obs = rows[:, :20].cpu().numpy().astype(np.float64)
        actor = env.make_sac_actor(mlp, seed=21)
        det, _ = fwd(env, actor, rows, t=1)
        assert np.abs(det.cpu().numpy() - mlp.forward_reference(obs)[0]).max() <= FORWARD_BOUND
        z = device_normals(env, 20, 6, rows, seed=21, t=1).astype(np.float64)
        a, lp = fwd(env, actor, rows, t=1, stochastic=True, logp=True)
        a64, lp64, _, _ = mlp.forward_reference(obs, z)
        assert np.abs(a.cpu().numpy() - a64).max() <= FORWARD_BOUND
        assert np.abs(lp.cpu().numpy() - lp64).max() <= LOGP_CAP
        qm = q_mlp(20, 6, hidden, seed=51)
        out = torch.full((n + 64,), SENTINEL, device="cuda")
        acts = a.contiguous()
        env.q_forward_device(env.make_q(qm), rows.data_ptr(), acts.data_ptr(), n, out.data_ptr(), obs_stride=22, stream=stream())
        torch.cuda.synchronize()
        assert bool((out[n:] == SENTINEL).all())
        ref = qm.forward_reference(np.concatenate([obs, acts.cpu().numpy().astype(np.float64)], axis=1))[:, 0]
        assert np.abs(out[:n].cpu().numpy() - ref).max() <= FORWARD_BOUND
    finally:
        env.close()


@pytest.mark.parametrize("n_obs,n_u,hidden", [(25, 6, (17,)), (25, 3, (64, 64)), (20, 6, (128, 128)), (36, 8, (64, 64))])
def test_q_dense_and_through_an_index(n_obs, n_u, hidden):
    """q against float64 (1e-5) on 1 / 33 / 129 rows, dense; then the same rows scattered into records of a wider stride (the
    replay ring's shape: [obs | next_obs | action | NaN ..]) and read through an index: the same bits, rows in any order, a poisoned
    record changes its own q only, nothing behind the last q is written."""
    import torch
    env = P().fan_env(n_obs, n_u, 4) if n_obs == 25 else P().env_for(n_obs, n_u, 4)
    try:
        mlp = q_mlp(n_obs, n_u, hidden, seed=3)
        q = env.make_q(mlp)
        g = torch.Generator(device="cuda")
        g.manual_seed(8)
        for n in (1, 33, 129):
            obs = (torch.rand((n, n_obs), device="cuda", generator=g) * 2 - 1).contiguous()
            act = (torch.rand((n, n_u), device="cuda", generator=g) * 2 - 1).contiguous()
            out = torch.full((n + 64,), SENTINEL, device="cuda")
            env.q_forward_device(q, obs.data_ptr(), act.data_ptr(), n, out.data_ptr(), stream=stream())
            torch.cuda.synchronize()
            assert bool((out[n:] == SENTINEL).all()) and not bool((out[:n] == SENTINEL).any())
            ref = mlp.forward_reference(torch.cat([obs, act], dim=1).cpu().numpy().astype(np.float64))[:, 0]
            err = float(np.abs(out[:n].cpu().numpy() - ref).max())
            print(f"Q {n_obs}+{n_u}-{hidden} n={n}: max |q - q_f64| = {err:.3e} (bound {FORWARD_BOUND:g})")
            assert err <= FORWARD_BOUND
            # records of stride R in a shuffled order, NaN everywhere else
            R = 2 * n_obs + n_u + 5
            perm = torch.randperm(n + 7, device="cuda", generator=g)[:n].contiguous()
            ring = torch.full((n + 7, R), float("nan"), device="cuda")
            ring[perm, :n_obs] = obs
            ring[perm, 2 * n_obs:2 * n_obs + n_u] = act
            out2 = torch.full((n + 64,), SENTINEL, device="cuda")
            env.q_forward_device(q, ring.data_ptr(), ring.data_ptr() + 8 * n_obs, n, out2.data_ptr(), obs_stride=R, act_stride=R,
                                 index_ptr=perm.data_ptr(), stream=stream())
            torch.cuda.synchronize()
            assert np.array_equal(u32(out2), u32(out)), n
            if n > 1:
                ring[perm[n // 2], 3] = 1e30       # (not NaN: the ReLU's fmaxf would swallow it)
                env.q_forward_device(q, ring.data_ptr(), ring.data_ptr() + 8 * n_obs, n, out2.data_ptr(), obs_stride=R, act_stride=R,
                                     index_ptr=perm.data_ptr(), stream=stream())
                torch.cuda.synchronize()
                keep = np.arange(n) != n // 2
                assert np.array_equal(u32(out2[:n])[keep], u32(out[:n])[keep]) and int(u32(out2[:n])[n // 2]) != int(u32(out[:n])[n // 2])
    finally:
        env.close()


def sac_env(n_obs, n_u, n_envs, max_timesteps=4, **kw):
    import bench
    import copy
    from gym_dockauv_amd.envs.torch_env import TorchDocking3d
    from gym_dockauv_amd.objects.vehicle_models import BlueROV2
    cid = {(20, 6): 3, (36, 3): 4, (36, 8): 2}[(n_obs, n_u)]
    wl = bench.workload(cid, n_envs)
    cfg = copy.deepcopy(wl["cfg"])
    cfg["max_timesteps"] = max_timesteps
    if n_u == 8:
        kw["vehicle_models"] = [BlueROV2(control_mode="direct")]
    env = TorchDocking3d(cfg, num_envs=n_envs, scenario=wl["scenario"], device_seed=9, **kw)
    assert (env.n_obs, env.n_u) == (n_obs, n_u)
    env.batch._gen = np.random.default_rng(5)
    env.reset()
    return env


def networks(env, hidden, seed=0):
    mlp = H().default_actor(env.n_obs, hidden, env.n_u, seed=20 + seed)
    q1, q2 = q_mlp(env.n_obs, env.n_u, hidden, seed=30 + seed), q_mlp(env.n_obs, env.n_u, hidden, seed=40 + seed)
    return mlp, q1, q2, env.make_sac_actor(mlp, seed=77), env.make_q(q1), env.make_q(q2)


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[0][0]}-{'-'.join(map(str, c[1]))}-{c[0][1]}")
def test_sac_target(case):
    """N = 200, rb.rollout with the actor fills the ring (max_timesteps 4: time limits among the dones).  For minibatches of 1, 33 and
    129 rows: the target from the ring through rb.index is the target on the sampled copies bit for bit (a2, logp2, q1, q2, y);
    q1 / q2 are dockauv_q_forward on (next_obs, a2) issued on their own; y is sac_target_reference of what the call left, with a
    host ent_coef and with a device log_ent_coef (0: alpha is exactly 1; -1.6: equal up to the last bit of expf); a2, logp2 and q
    against float64 with the slot-5 normals of the Philox statement; a row's outputs do not depend on the batch's length."""
    import torch
    from gym_dockauv_amd.policy import sac_target_reference
    (n_obs, n_u), hidden = case
    env = sac_env(n_obs, n_u, 200)
    try:
        mlp, q1m, q2m, actor, q1, q2 = networks(env, hidden)
        rb = env.make_replay_buffer(12 * 200, seed=5)
        rb.rollout(actor, 7, stochastic=True)
        ring = rb.storage.view(-1, rb.record_floats)
        gamma, alpha = 0.99, 0.2
        for B in (129, 33, 1):
            sm = rb.sample(B, want_index=True)
            dense = {k: v.clone() for k, v in [("y", env.sac_target(actor, q1, q2, sm, gamma, ent_coef=alpha, t=3))] + list(env.sac_buffers.items())}
            y_ring = env.sac_target(actor, q1, q2, rb, gamma, ent_coef=alpha, t=3)
            torch.cuda.synchronize()
            b = env.sac_buffers
            assert y_ring.shape == sm.rewards.shape and y_ring.data_ptr() == b["y"].data_ptr()
            for k in ("a2", "logp2", "q1", "q2", "y"):
                assert np.array_equal(u32(b[k]), u32(dense[k])), f"B={B}: {k} from the ring differs from the sampled copies"
                assert not bool(torch.isnan(b[k]).any())
            # the two Q launches are the public call on (next_obs, a2)
            for crit, k in ((q1, "q1"), (q2, "q2")):
                assert np.array_equal(u32(env.q_values(crit, sm.next_observations, b["a2"])), u32(b[k]))
                assert np.array_equal(u32(env.q_values(crit, ring[:, n_obs:2 * n_obs], ring[:, 2 * n_obs:2 * n_obs + n_u], rb.index)),
                                      u32(env.q_values(crit, sm.next_observations, sm.actions))), "q_values: ring against dense"
            # the last kernel
            h = {k: v.cpu().numpy() for k, v in b.items()}
            r, d = sm.rewards.cpu().numpy().reshape(-1), sm.dones.cpu().numpy().reshape(-1)
            assert np.array_equal(u32(h["y"]), u32(sac_target_reference(h["q1"], h["q2"], h["logp2"], r, d, gamma, ent_coef=alpha)))
            one = torch.zeros(1, device="cuda")
            y1 = env.sac_target(actor, q1, q2, sm, gamma, log_ent_coef=one, t=3).clone().cpu().numpy().reshape(-1)
            assert np.array_equal(u32(y1), u32(sac_target_reference(h["q1"], h["q2"], h["logp2"], r, d, gamma, ent_coef=1.0)))
            la = torch.full((1,), -1.6, device="cuda")
            y2 = env.sac_target(actor, q1, q2, sm, gamma, log_ent_coef=la, t=3).clone().cpu().numpy().reshape(-1)
            a_mid = np.float32(np.exp(np.float64(np.float32(-1.6))))
            cands = [sac_target_reference(h["q1"], h["q2"], h["logp2"], r, d, gamma, ent_coef=x)
                     for x in (np.nextafter(a_mid, np.float32(0)), a_mid, np.nextafter(a_mid, np.float32(1)))]
            assert any(np.array_equal(u32(y2), u32(c)) for c in cands), "log_ent_coef: alpha is not expf(log_ent_coef) to its last bit"
            # float64, with the Philox statement's slot-5 normals
            z = MLPPolicy_normals(77, B, 3, n_u, slot=5)
            nxt = sm.next_observations.cpu().numpy().astype(np.float64)
            a64, lp64, _, ls64 = mlp.forward_reference(nxt, z)
            # the normals here are the statement's, not the device's (the rows form has no call that returns them): the device's
            # deviate by dz <= the exploration bound, which moves x by std dz, a by at most that, and log_prob by at most
            # n_u (|z| + 2 std) dz (d/dz of -z^2 / 2 and of log(1 - tanh(x)^2), |d/dx| <= 2)
            dz = min(4 * P().recorded("exploration_max_dev"), P().EXPLORATION_CAP)
            std = float(np.exp(ls64).max())
            assert np.abs(h["a2"] - a64).max() <= FORWARD_BOUND + std * dz
            assert np.abs(h["logp2"] - lp64).max() <= LOGP_CAP + n_u * (float(np.abs(z).max()) + 2 * std) * dz
            xin = np.concatenate([nxt, h["a2"].astype(np.float64)], axis=1)
            assert np.abs(h["q1"] - q1m.forward_reference(xin)[:, 0]).max() <= FORWARD_BOUND
            assert np.abs(h["q2"] - q2m.forward_reference(xin)[:, 0]).max() <= FORWARD_BOUND
            if B == 129:
                keep = {k: v.copy() for k, v in h.items()}
                idx129 = rb.index.clone()
            if B == 33:
                # the first 33 rows of the 129-row batch, alone: same position, another n
                rb.index = idx129[:33].contiguous()
                env.sac_target(actor, q1, q2, rb, gamma, ent_coef=alpha, t=3)
                torch.cuda.synchronize()
                for k in ("a2", "logp2", "q1", "q2", "y"):
                    assert np.array_equal(u32(env.sac_buffers[k]), u32(keep[k][:33])), f"{k} depends on the batch's length"
        assert env.sac_target(actor, q1, q2, sm, gamma, ent_coef=alpha).data_ptr() == b["y"].data_ptr(), "a new buffer for a known shape"
    finally:
        env.close()


def test_slot5_normals_and_row_offset():
    """65 536 x 6 draws of the rows form (mu = 0, std = 1: a2 = tanh(z)) against tanh of the Philox statement's slot-5 normals
    within the recorded exploration bound of tests/test_gpu_policy.py plus tanh_'s own error (|d tanh / dz| <= 1); (row_offset, t)
    reproduces rows of a longer call; two t differ; slot 2 is another stream."""
    import torch
    from gym_dockauv_amd.policy import SquashedGaussianMLP
    n, n_obs, n_u = 65536, 20, 6
    env = P().env_for(n_obs, n_u, 4)
    try:
        zero = SquashedGaussianMLP([(np.zeros((8, n_obs)), np.zeros(8))], (np.zeros((n_u, 8)), np.zeros(n_u)), (np.zeros((n_u, 8)), np.zeros(n_u)), "tanh")
        actor = env.make_sac_actor(zero, seed=0xABCDEF0123)
        qm = q_mlp(n_obs, n_u, (17,), seed=1)
        q = env.make_q(qm)
        nxt = torch.zeros((n, n_obs), device="cuda")
        rd = torch.zeros((n,), device="cuda")

        def draw(rows, t, offset=0):
            o = {k: torch.full((rows + 8,) + s, SENTINEL, device="cuda") for k, s in (("a2", (n_u,)), ("logp2", ()), ("q1", ()), ("q2", ()), ("y", ()))}
            env.sac_target_device(actor, q, q, nxt.data_ptr(), rd.data_ptr(), rd.data_ptr(), rows, 0.99, o["a2"].data_ptr(),
                                  o["logp2"].data_ptr(), o["q1"].data_ptr(), o["q2"].data_ptr(), o["y"].data_ptr(), ent_coef=0.1, t=t,
                                  row_offset=offset, stream=stream())
            torch.cuda.synchronize()
            for v in o.values():
                assert bool((v[rows:] == SENTINEL).all()) and not bool((v[:rows] == SENTINEL).any())
            return o["a2"][:rows].cpu().numpy()

        a = draw(n, 7)
        bound = min(4 * P().recorded("exploration_max_dev"), P().EXPLORATION_CAP) + TANH_ERR
        dev = float(np.abs(a - np.tanh(MLPPolicy_normals(0xABCDEF0123, n, 7, n_u, slot=5))).max())
        print(f"slot-5 normals: max |a2 - tanh(z_ref)| = {dev:.3e} (bound {bound:.3e})")
        assert dev <= bound
        assert np.abs(a - np.tanh(MLPPolicy_normals(0xABCDEF0123, n, 7, n_u, slot=2))).max() > 0.1
        assert np.array_equal(u32(draw(129, 7, offset=1000)), u32(a[1000:1129])), "(row_offset, t) does not reproduce the rows"
        assert not np.array_equal(u32(draw(129, 8, offset=1000)), u32(a[1000:1129]))
    finally:
        env.close()


def test_rollout_is_the_steps_one_by_one():
    """rb.rollout(sac_actor, K = 7, stochastic) at N = 200 against a twin env: K x (dockauv_policy_forward, step(replay=rb)).
    Rows, actions and the ring as uint32."""
    import torch
    K = 7
    env, twin = sac_env(20, 6, 200), sac_env(20, 6, 200)
    try:
        mlp = H().default_actor(20, (64, 64), 6, seed=20)
        pol, t_pol = env.make_sac_actor(mlp, seed=3), twin.make_sac_actor(mlp, seed=3)
        rb, t_rb = env.make_replay_buffer(12 * 200, seed=5), twin.make_replay_buffer(12 * 200, seed=5)
        for call in range(2):                # (the second through the carry, wrapping the ring)
            obs, acts, reward, done = rb.rollout(pol, K, stochastic=True)
            for k in range(K):
                cur = twin._last_rows if twin._last_rows is not None else twin._packed[twin._i % len(twin._packed)]
                a = torch.full((200, 6), SENTINEL, device="cuda")
                twin.batch.policy_forward_device(t_pol, cur.data_ptr(), a.data_ptr(), t=twin._t, stochastic=True, stream=stream())
                o, r, d = twin.step(a, replay=t_rb)
                torch.cuda.synchronize()
                for name, x, y in (("obs", obs[k], o), ("actions", acts[k], a), ("reward", reward[k], r)):
                    assert np.array_equal(u32(x), u32(y)), f"call {call} step {k}: {name}"
                assert bool((done[k] == d).all())
            assert (rb.pos, rb.size) == (t_rb.pos, t_rb.size)
            assert np.array_equal(u32(rb.storage), u32(t_rb.storage)), f"call {call}: the ring"
        assert float(rb.storage[..., 2 * 20 + 6 + 1].sum()) > 0, "no done was stored"
        # evaluation takes the actor, deterministically
        mean, std = env.evaluate(pol, 200)
        assert np.isfinite(mean) and np.isfinite(std)
    finally:
        env.close()
        twin.close()


def test_refusals_on_a_live_handle():
    """What needs a handle: n_in / n_out against it, each role against the calls that must refuse it, by name."""
    import torch
    from gym_dockauv_amd import _capi
    from gym_dockauv_amd._capi import DockAUVError
    env = sac_env(20, 6, 64)
    try:
        b, lib, h = env.batch, env.batch._lib, env.batch._handle
        mlp, q1m, _, actor, q1, q2 = networks(env, (17,))
        plain = env.make_policy(P().make_mlp((20, (17,), 6, "tanh", "tanh"), seed=1, log_std=np.zeros(6)))
        value = env.make_value(P().make_mlp((20, (17,), 1, "tanh", "none"), seed=1))

        def refused(call, *needles):
            with pytest.raises(DockAUVError) as e:
                call()
            assert all(n in str(e.value) for n in needles), (needles, str(e.value))

        refused(lambda: b.make_q(P().make_mlp((25, (17,), 1, "relu", "none"))), "n_in", "n_obs + n_u")
        refused(lambda: b.make_q(P().make_mlp((20, (17,), 1, "relu", "none"))), "n_in")
        refused(lambda: b.make_sac_actor(H().default_actor(20, (17,), 3, seed=1)), "dockauv_sac_actor_desc.n_out")
        refused(lambda: b.make_sac_actor(H().default_actor(36, (17,), 6, seed=1)), "dockauv_sac_actor_desc.n_in")
        out = C.c_void_p()
        d = H().default_actor(133, (128, 128), 6, seed=1).host_desc()
        assert lib.dockauv_sac_actor_create(None, C.byref(d), C.byref(out)) == -1     # (valid on its own: only the handle is missing)
        rows = P().nan_rows(torch, 64, 20, seed=1)
        buf = torch.zeros((7 * 64 * 22,), device="cuda")
        ptr = buf.data_ptr()
        sac, qn = "squashed-Gaussian actor", "Q critic"
        # PPO's calls refuse the SAC actor, and the critic arguments refuse both roles
        refused(lambda: b.collect_device(actor, None, rows.data_ptr(), ptr, ptr, 1, 0.99, 0.95), sac)
        refused(lambda: b.collect_device(plain, q1, rows.data_ptr(), ptr, ptr, 1, 0.99, 0.95, values_ptr=ptr, advantages_ptr=ptr,
                                         returns_ptr=ptr), qn)
        refused(lambda: b.make_optim(actor), sac)
        refused(lambda: b.make_optim(plain, q1), qn)
        refused(lambda: b.policy_forward_rows_device(actor, rows.data_ptr(), 64, ptr), sac)
        refused(lambda: b.policy_forward_rows_device(q1, rows.data_ptr(), 64, ptr), qn)
        refused(lambda: b.policy_backward_device(actor, rows.data_ptr(), 64, ptr, [ptr] * 6), sac)
        refused(lambda: b.value_forward_device(q1, rows.data_ptr(), 64, ptr), qn)
        refused(lambda: b.policy_forward_device(q1, rows.data_ptr(), ptr), qn)
        refused(lambda: b.rollout_device(q1, rows.data_ptr(), ptr, ptr, 1), qn)
        io = _capi.PPOHeadIO()
        io.struct_size, io.n_rows, io.clip_range = C.sizeof(io), 64, 0.2
        assert lib.dockauv_ppo_head(h, actor.ptr, C.byref(io), None) == -1 and sac.encode() in lib.dockauv_last_error(h)
        # a plain tanh policy still has no log-probability; the SAC target takes only its own roles
        refused(lambda: b.policy_forward_logp_device(plain, rows.data_ptr(), ptr, ptr), "DOCKAUV_ACT_TANH")
        tgt = lambda a, c1, c2: b.sac_target_device(a, c1, c2, ptr, ptr, ptr, 4, 0.99, ptr, ptr, ptr, ptr, ptr, ent_coef=0.1)
        refused(lambda: tgt(plain, q1, q2), "not a squashed-Gaussian actor")
        refused(lambda: tgt(actor, value, q2), "q1_target is not a Q critic")
        refused(lambda: tgt(actor, q1, actor), "q2_target is not a Q critic")
        refused(lambda: b.q_forward_device(value, ptr, ptr, 4, ptr), "not a Q critic")
        refused(lambda: b.q_forward_device(q1, ptr, ptr, 4, ptr, obs_stride=19), "obs_stride")
        refused(lambda: b.q_forward_device(q1, ptr, ptr, 4, ptr, act_stride=5), "act_stride")
        # reloads: a Q critic through dockauv_policy_load, the actor through its own call only
        b.load_policy(q1, mlp=q1m)
        b.load_policy(actor, mlp=mlp)
        dd = plain.shape.__class__.from_buffer_copy(plain.shape)
        assert lib.dockauv_policy_load(actor.ptr, C.byref(dd), None) == -1 and b"dockauv_sac_actor_load" in lib.dockauv_last_error(h)
        sd = mlp.host_desc()
        assert lib.dockauv_sac_actor_load(plain.ptr, C.byref(sd), None) == -1 and b"not a squashed-Gaussian actor" in lib.dockauv_last_error(h)
        sd.n_hidden[0] = 18
        assert lib.dockauv_sac_actor_load(actor.ptr, C.byref(sd), None) == -1 and b"differ" in lib.dockauv_last_error(h)
        torch.cuda.synchronize()
    finally:
        env.close()


def test_load_from_device_tensors():
    """load_policy of both roles from device tensors: the next forward is that of an object created with those weights."""
    import torch
    env = sac_env(20, 6, 33)
    try:
        mlp_a, q_a, _, actor, q1, _ = networks(env, (64, 64), seed=0)
        mlp_b, q_b, _, actor_b, q1_b, _ = networks(env, (64, 64), seed=1)
        dev = lambda x: torch.as_tensor(x, device="cuda").contiguous()
        ts = [dev(a) for Wb in mlp_b.layers + [mlp_b.mu, mlp_b.log_std_head] for a in Wb]
        env.load_policy(actor, ts)
        env.load_policy(q1, [dev(a) for Wb in q_b.layers for a in Wb])
        rows = P().nan_rows(torch, 33, 20, seed=6)
        got, lp = fwd(env.batch, actor, rows, t=2, stochastic=True, logp=True)
        want, lp_b = fwd(env.batch, actor_b, rows, t=2, stochastic=True, logp=True)
        assert np.array_equal(u32(got), u32(want)) and np.array_equal(u32(lp), u32(lp_b))
        obs, act = rows[:, :20].contiguous(), got.contiguous()
        assert np.array_equal(u32(env.q_values(q1, obs, act)), u32(env.q_values(q1_b, obs, act)))
        assert np.array_equal(u32(env.q_values(q1, rows[:, :20], act)), u32(env.q_values(q1_b, obs, act))), "a strided observation view"
    finally:
        env.close()
