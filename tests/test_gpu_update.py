"""The whole update on a real MI355X (include/dockauv.h: dockauv_permutation, dockauv_ppo_update; TorchDocking3d.permutation /
ppo_train, DeviceAdam.steps): the permutation kernel bit for bit against its exact statement; ppo_train bit for bit against the
loop of its pieces (permutation, mlp_forward x 2, ppo_head_device, mlp_backward x 2, opt.step) on a second optimiser over cloned
tensors, with a critic and actor-only, with a minibatch that needs two groups of the head, and for two calls queued back to back
without a synchronisation; the clipped value loss against the float64 statement under the head's own bound; SB3's target_kl
early stop decided on the device, with the reconciled step count; every refusal on a live handle.  Outputs sit between
sentinels where the test owns them, every env is closed in `finally`.

The clipped value loss: observations U(-1, 1), the networks' own outputs as mean and v, the head's other inputs from
test_gpu_head.draw_head (rows off the ratio's clip edges), values_old = float32(v - N(0, 0.5)) with clip_range_vf 0.2, so that
the clamp is active on more than a quarter of the rows on each side.  A row whose float64 |v - v_old| lies within EDGE of the
clamp's edge may fall on the other side in float32: its v_old is redrawn from a slightly larger draw (at most 1 / 256 of it).
Bound, per output: max |x - x64| <= max(8 x e32, 4 ulp of max |x64|), e32 the error of the float32 NumPy restatement
(test_gpu_head.head_float32_numpy with the header's clipped value lines), test_gpu_head's floor for approx_kl.  grad_v stays
inside the library: the restatement's grad_v (IEEE float32 operations only, so the same bits) is checked through the critic's
gradients, which must be bit for bit those of mlp_backward on it.  Measured ratios: profiles/update/head_error.txt.
"""
import copy
import ctypes as C
from collections import namedtuple

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CLIP, VF, ENT = 0.2, 0.5, 0.01
CLIP_VF, VF_SIGMA = 0.2, 0.5
N_IN, N_U = 20, 6
Collected = namedtuple("Collected", ["obs", "actions", "reward", "done", "log_prob", "values", "advantages", "returns"])
KW = dict(clip_range=CLIP, vf_coef=VF, ent_coef=ENT)


def T():
    """the helpers of the backward tests: guarded, check_guards, bits, stream_of, SENTINEL, GUARD, P"""
    from tests import test_gpu_backward
    return test_gpu_backward


def H():
    from tests import test_gpu_head
    return test_gpu_head


def torch_env(num_envs=64):
    from gym_dockauv_amd.config.env_config import BASE_CONFIG
    from gym_dockauv_amd.envs.torch_env import TorchDocking3d
    cfg = copy.deepcopy(BASE_CONFIG)
    cfg["radar"].update(T().P().FANS[N_IN])
    env = TorchDocking3d(cfg, num_envs=num_envs, scenario="ObstaclesDocking3d", device_seed=7)
    assert (env.n_obs, env.n_u) == (N_IN, N_U)
    return env


def mlps(hidden=(64, 64), log_std=-0.5):
    P = T().P()
    return (P.make_mlp((N_IN, hidden, N_U, "tanh", "none"), seed=6, log_std=np.full(N_U, log_std)),
            P.make_mlp((N_IN, hidden, 1, "tanh", "none"), seed=7))


def learner(torch, actor_mlp, critic_mlp):
    a_net, c_net = H().sequential(torch, actor_mlp, torch.float32, "cuda"), H().sequential(torch, critic_mlp, torch.float32, "cuda")
    log_std = torch.tensor(actor_mlp.log_std, device="cuda", requires_grad=True)
    return a_net, c_net, log_std


def optimizer(env, policy, value, nets, critic=True):
    a_net, c_net, log_std = nets
    return env.make_optimizer(policy, value if critic else None, list(a_net.parameters()), log_std,
                              list(c_net.parameters()) if critic else None)


def loop_of_pieces(torch, env, opt, c, n_epochs, batch_size, lr, seed, first_epoch, stats, t_done=0, max_steps=None, load=True):
    """what one ppo_train queues, issued piece by piece on `opt`; stats [n_epochs, n_mb, >= 10] gets columns 0..9.  max_steps: stop
    after that many optimiser steps -- the pieces of the next minibatch are still run into opt.grads, unapplied (returns True)."""
    policy, value = opt.policy, opt.value
    K, N = int(c.actions.shape[0]), int(c.actions.shape[1])
    M = K * N
    rows = c.obs[:K]
    flat = lambda t: t.reshape(M, *t.shape[2:])
    if load:
        opt.load()
    steps = 0
    for e in range(n_epochs):
        perm = env.permutation(seed, first_epoch + e, M)
        for j in range((M + batch_size - 1) // batch_size):
            idx = perm[j * batch_size: (j + 1) * batch_size]
            B = int(idx.numel())
            mean = env.mlp_forward(policy, rows, idx)
            v = env.mlp_forward(value, rows, idx).view(-1) if value is not None else None
            grad_mean = torch.empty((B, N_U), device="cuda")
            grad_v = torch.empty((B,), device="cuda") if value is not None else None
            st = stats[e, j]
            env.batch.ppo_head_device(policy, B, mean.data_ptr(), 0 if v is None else v.data_ptr(), flat(c.actions).data_ptr(),
                                      flat(c.log_prob).data_ptr(), flat(c.advantages).data_ptr(),
                                      0 if v is None else flat(c.returns).data_ptr(), grad_mean.data_ptr(),
                                      0 if v is None else grad_v.data_ptr(), opt.grad_log_std.data_ptr(), st.data_ptr(), CLIP, VF, ENT,
                                      normalize_advantage=True, index_ptr=idx.data_ptr(), stream=T().stream_of(torch))
            env.mlp_backward(policy, rows, grad_mean, idx, out=opt.actor_grads)
            if value is not None:
                env.mlp_backward(value, rows, grad_v.view(-1, 1), idx, out=opt.critic_grads)
            if max_steps is not None and steps == max_steps:
                return True
            opt.step(lr, stats=st[8:10])
            steps += 1
    return False


def same(torch, xs, ys):
    return all(torch.equal(T().bits(x.detach()), T().bits(y.detach())) for x, y in zip(xs, ys))


def assert_same_state(torch, opt, opt2, what):
    assert same(torch, opt.params, opt2.params), f"{what}: the parameters differ from the loop of the pieces"
    (m, v, t), (m2, v2, t2) = opt.state(), opt2.state()
    assert same(torch, [m, v], [m2, v2]) and t == t2, f"{what}: the moments or the count differ from the loop of the pieces"


# ------------------------------------------------------------------------------------------------- the permutation
@pytest.mark.parametrize("n", [1, 2, 3, 63, 64, 65, 1000, 4097, 2 ** 20 + 1])
def test_permutation_equals_its_statement(n):
    """odd and even b, unequal halves, a last wave that is partly empty; the int64 output between sentinels"""
    import torch
    from gym_dockauv_amd.policy import MLPPolicy
    env = T().P().fan_env(N_IN, N_U, 64)
    try:
        guard = 32
        for seed, epoch in ((0, 0), (0x123456789ABCDEF, 2 ** 32 + 5)):
            buf = torch.full((n + 2 * guard,), -7, device="cuda", dtype=torch.int64)
            env.permutation_device(seed, epoch, n, buf[guard:].data_ptr(), stream=T().stream_of(torch))
            torch.cuda.synchronize()
            got = buf.cpu().numpy()
            assert (got[:guard] == -7).all() and (got[guard + n:] == -7).all(), "the kernel wrote outside out"
            assert np.array_equal(got[guard: guard + n], MLPPolicy.permutation_reference(seed, epoch, n)), (n, seed, epoch)
    finally:
        env.close()


# ------------------------------------------------------------------------------------------------- the loop of the pieces
@pytest.mark.parametrize("n_envs,batch,critic", [(64, 100, True), (64, 100, False), (320, 1100, True), (320, 1100, False)],
                         ids=["256rows-critic", "256rows-actor", "1280rows-critic", "1280rows-actor"])
def test_ppo_train_is_the_loop_of_its_pieces(n_envs, batch, critic):
    """2 epochs of minibatches of 100, 100, 56 rows, and of 1100 (two groups of the head) and 180 rows"""
    import torch
    env = torch_env(n_envs)
    try:
        actor_mlp, critic_mlp = mlps()
        policy, value = env.make_policy(actor_mlp, seed=3), env.make_value(critic_mlp)
        nets = [learner(torch, actor_mlp, critic_mlp) for _ in range(2)]
        env.load_policy(policy, nets[0][0], log_std=nets[0][2])
        env.reset()
        K, lr, seed = 4, 3e-3, 11
        c = env.collect(policy, value, K, gamma=0.99, gae_lambda=0.95)
        rows = c.obs[:K]
        n_mb = (K * n_envs + batch - 1) // batch

        opt = optimizer(env, policy, value, nets[0], critic)
        stats = env.ppo_train(opt, c, 2, batch, lr, seed=seed, first_epoch=5, **KW)
        torch.cuda.synchronize()
        assert tuple(stats.shape) == (2, n_mb, 12) and stats.device.type == "cuda"
        mean_after = env.mlp_forward(policy, rows).clone()
        v_after = env.mlp_forward(value, rows).clone()
        assert opt.steps() == 2 * n_mb

        opt2 = optimizer(env, policy, value, nets[1], critic)
        want = torch.zeros((2, n_mb, 10), device="cuda")
        loop_of_pieces(torch, env, opt2, c, 2, batch, lr, seed, 5, want)
        torch.cuda.synchronize()
        assert_same_state(torch, opt, opt2, "ppo_train")
        assert not same(torch, opt.params[:1], [torch.from_numpy(actor_mlp.layers[0][0]).cuda()]), "a parameter did not move"
        assert torch.equal(T().bits(stats[:, :, :10]), T().bits(want)), "stats columns 0..9 differ from the pieces'"
        s = stats.cpu().numpy()
        assert not np.isnan(s).any() and (s[:, :, 10] == 1.0).all()
        assert np.array_equal(s[:, :, 11].reshape(-1), np.arange(1, 2 * n_mb + 1, dtype=np.float32))
        if not critic:
            assert (s[:, :, 2] == 0).all()
        assert torch.equal(T().bits(env.mlp_forward(policy, rows)), T().bits(mean_after))
        assert torch.equal(T().bits(env.mlp_forward(value, rows)), T().bits(v_after))
    finally:
        env.close()


def test_two_updates_back_to_back_without_a_synchronisation():
    """two ppo_train calls queued on one stream, nothing between them: the loop of the pieces run for both"""
    import torch
    env = torch_env(64)
    try:
        actor_mlp, critic_mlp = mlps()
        policy, value = env.make_policy(actor_mlp, seed=3), env.make_value(critic_mlp)
        nets = [learner(torch, actor_mlp, critic_mlp) for _ in range(2)]
        env.load_policy(policy, nets[0][0], log_std=nets[0][2])
        env.reset()
        K, lr, seed, batch = 4, 3e-3, 2, 100
        c = env.collect(policy, value, K, gamma=0.99, gae_lambda=0.95)
        opt = optimizer(env, policy, value, nets[0])
        torch.cuda.synchronize()
        first = env.ppo_train(opt, c, 2, batch, lr, seed=seed, first_epoch=0, **KW)
        second = env.ppo_train(opt, c, 1, batch, 2 * lr, seed=seed, first_epoch=2, **KW)
        torch.cuda.synchronize()

        opt2 = optimizer(env, policy, value, nets[1])
        want = [torch.zeros((2, 3, 10), device="cuda"), torch.zeros((1, 3, 10), device="cuda")]
        loop_of_pieces(torch, env, opt2, c, 2, batch, lr, seed, 0, want[0])
        loop_of_pieces(torch, env, opt2, c, 1, batch, 2 * lr, seed, 2, want[1])
        torch.cuda.synchronize()
        assert_same_state(torch, opt, opt2, "two updates")
        for got, w in zip((first, second), want):
            assert torch.equal(T().bits(got[:, :, :10]), T().bits(w))
        assert np.array_equal(second.cpu().numpy()[0, :, 11], np.array([7, 8, 9], dtype=np.float32))
        assert opt.steps() == 9
    finally:
        env.close()


# ------------------------------------------------------------------------------------------------- clip_range_vf
def draw_values_old(v, n, seed, edge=None):
    """values_old float32 [n] = v - N(0, VF_SIGMA), the rows within `edge` of the clamp's edge redrawn from n + max(8, n / 16)
    draws: (values_old, rows redrawn, draws)"""
    edge = H().EDGE if edge is None else edge
    rng = np.random.default_rng(seed)
    draw = n + max(8, n // 16)
    delta = rng.normal(0.0, VF_SIGMA, draw)
    v64 = v.astype(np.float64)
    v_old = (v64 - delta[:n]).astype(np.float32)
    near = lambda vo, at: np.abs(np.abs(v64[at] - vo.astype(np.float64)) - CLIP_VF) < edge
    todo, spare, redrawn = np.flatnonzero(near(v_old, np.arange(n))), n, 0
    for r in todo:
        while True:
            assert spare < draw, "the spare draws ran out"
            cand = np.float32(v64[r] - delta[spare])
            spare += 1
            redrawn += 1
            if not near(np.array([cand]), np.array([r]))[0]:
                v_old[r] = cand
                break
    assert redrawn <= draw / 256.0, (redrawn, draw)
    d = v64 - v_old.astype(np.float64)
    assert (d > CLIP_VF).mean() >= 0.25 and (d < -CLIP_VF).mean() >= 0.25, "the clamp is active on too few rows"
    return v_old, redrawn, draw


def clipped_float32_numpy(d, v_old):
    """test_gpu_head.head_float32_numpy with the header's clipped value lines (IEEE float32 operations in the header's order)"""
    f = np.float32
    grad_mean, _, grad_log_std, stats = H().head_float32_numpy(d, True, True)
    n = d["v"].size
    dd = d["v"] - v_old
    vc = v_old + np.minimum(np.maximum(dd, f(-CLIP_VF)), f(CLIP_VF))
    dv = vc - d["returns"]
    grad_v = np.where(np.abs(dd) <= f(CLIP_VF), ((f(2) * f(VF)) * dv) / f(n), f(0)).astype(f)
    stats = stats.copy()
    stats[2] = f((dv * dv).sum(dtype=np.float64) / n)
    stats[0] = H().fma32(f(VF), stats[2], H().fma32(f(ENT), stats[3], stats[1]))
    for x in (dd, vc, dv, grad_v):
        assert x.dtype == f
    return grad_mean, grad_v, grad_log_std, stats


ROWS_BEYOND_ONE_PASS = 256 * 1024 + 33      # test_gpu_head.ROWS_BEYOND_ONE_PASS: a second pass of the head's group 0


@pytest.mark.parametrize("n", [257, ROWS_BEYOND_ONE_PASS])
def test_clipped_value_loss_against_float64(n):
    """one minibatch of n rows through ppo_train with clip_range_vf"""
    import torch
    from gym_dockauv_amd.policy import MLPPolicy
    assert ROWS_BEYOND_ONE_PASS == H().ROWS_BEYOND_ONE_PASS
    env = torch_env(64)
    try:
        actor_mlp, critic_mlp = mlps(log_std=0.0)
        rng = np.random.default_rng(n)
        draw = n + max(8, n // 16)
        cand = rng.uniform(-1, 1, (draw, N_IN)).astype(np.float32)
        d, _, _, kept = H().draw_head(n, N_U, seed=12 + n, mean=actor_mlp.forward_reference(cand.astype(np.float64)), edge=1e-4,
                                      want_kept=True)
        actor_mlp.log_std = d["log_std"]
        packed = np.full((2, n, N_IN + 2), np.nan, dtype=np.float32)
        packed[0, :, :N_IN] = cand[kept]
        packed[1, :, :N_IN] = 0.0
        policy, value = env.make_policy(actor_mlp), env.make_value(critic_mlp)
        opt = optimizer(env, policy, value, learner(torch, actor_mlp, critic_mlp))
        rows_t = torch.from_numpy(packed).cuda()
        obs = rows_t[:, :, :N_IN]
        # the networks' own outputs are the head's mean and v (the same kernel, the same weights: the same bits as inside the call)
        d["mean"] = env.mlp_forward(policy, obs[:1]).cpu().numpy()
        d["v"] = env.mlp_forward(value, obs[:1]).view(-1).cpu().numpy()
        v_old, redrawn, drawn = draw_values_old(d["v"], n, seed=n + 1)
        print(f"head clip_vf rows{n}: {redrawn} of {drawn} values_old redrawn")
        dev = lambda a, *tail: torch.from_numpy(a).cuda().view(1, n, *tail)
        vals = torch.zeros((2, n), device="cuda")
        vals[0] = torch.from_numpy(v_old).cuda()
        c = Collected(obs, dev(d["actions"], N_U), None, None, dev(d["log_prob_old"]), vals, dev(d["advantages"]), dev(d["returns"]))

        seed, epoch = 9, 3
        perm = MLPPolicy.permutation_reference(seed, epoch, n)
        pos = {k: (a if k == "log_std" else np.ascontiguousarray(a[perm])) for k, a in d.items()}     # in the minibatch's order
        f32 = clipped_float32_numpy(pos, v_old[perm])
        ref = MLPPolicy.ppo_head_reference(pos["mean"], pos["v"], pos["actions"], pos["log_prob_old"], pos["advantages"], pos["returns"],
                                           pos["log_std"], CLIP, VF, ENT, clip_range_vf=CLIP_VF, values_old=v_old[perm])
        plain = MLPPolicy.ppo_head_reference(pos["mean"], pos["v"], pos["actions"], pos["log_prob_old"], pos["advantages"],
                                             pos["returns"], pos["log_std"], CLIP, VF, ENT)
        assert abs(plain[3][2] - ref[3][2]) > 1e-3, "the clamp does not change the value loss"
        idx = torch.from_numpy(perm).cuda()
        want_critic = [g.clone() for g in env.mlp_backward(value, obs[:1], torch.from_numpy(f32[1]).cuda().view(-1, 1), idx)]

        stats = env.ppo_train(opt, c, 1, n, 3e-4, clip_range_vf=CLIP_VF, seed=seed, first_epoch=epoch, **KW)
        torch.cuda.synchronize()
        s = stats.cpu().numpy()[0, 0]
        assert s[10] == 1.0 and s[11] == 1.0 and s[8] > 0
        assert same(torch, opt.critic_grads, want_critic), "grad_v is not the header's float32 expression (seen through the critic's gradients)"
        label = f"clip_vf_rows{n}"
        pairs = [("grad_v", f32[1], f32[1], ref[1])]
        pairs += [(f"stats.{name}", s[k: k + 1], f32[3][k: k + 1], ref[3][k: k + 1]) for k, name in enumerate(H().STAT_NAMES)]
        for name, dv, f, r in pairs:
            e_dev = float(np.abs(dv.astype(np.float64) - r).max())
            e_np = float(np.abs(f.astype(np.float64) - r).max())
            floor = 4.0 * float(np.spacing(np.float32(np.abs(r).max())))
            if name == "stats.approx_kl":
                floor = H().KL_FLOOR_ULPS * float(np.spacing(np.float32(H().f64_ratio(pos).max())))
            bound = max(8.0 * e_np, floor)
            print(f"head {label} {name}: device {e_dev:.3e}, float32 NumPy {e_np:.3e}, bound {bound:.3e}, "
                  f"ratio {e_dev / max(e_np, floor / 8.0):.2f}")
            assert e_dev <= bound, (name, e_dev, e_np, bound)
        assert s[5] == np.float32(ref[3][5])
    finally:
        env.close()


# ------------------------------------------------------------------------------------------------- target_kl
def test_target_kl_stops_on_the_device():
    import torch
    env = torch_env(64)
    try:
        actor_mlp, critic_mlp = mlps()
        policy, value = env.make_policy(actor_mlp, seed=3), env.make_value(critic_mlp)
        nets = [learner(torch, actor_mlp, critic_mlp) for _ in range(3)]
        env.load_policy(policy, nets[0][0], log_std=nets[0][2])
        env.reset()
        K, lr, seed, batch, epochs = 4, 3e-3, 4, 100, 3
        c = env.collect(policy, value, K, gamma=0.99, gae_lambda=0.95)
        free = env.ppo_train(optimizer(env, policy, value, nets[0]), c, epochs, batch, lr, seed=seed, **KW)
        torch.cuda.synchronize()
        free = free.cpu().numpy().reshape(-1, 12)
        kl = free[:, 4]
        s = next(i for i in range(2, kl.size) if kl[i] > kl[:i].max() + 4 * np.spacing(np.float32(max(abs(kl[i]), abs(kl[:i].max())))))
        threshold = 0.5 * (float(kl[s]) + float(kl[:s].max()))
        target_kl = np.float32(threshold / 1.5)
        assert kl[:s].max() < np.float32(1.5) * target_kl < kl[s], "the threshold does not separate the two statistics in float32"
        print(f"target_kl: approx_kl {kl}, stop at minibatch {s}, target_kl {target_kl}")

        opt = optimizer(env, policy, value, nets[1])
        got = env.ppo_train(opt, c, epochs, batch, lr, target_kl=float(target_kl), seed=seed, **KW)
        opt2 = optimizer(env, policy, value, nets[2])
        want = torch.zeros((epochs, 3, 10), device="cuda")
        torch.cuda.synchronize()
        got = got.cpu().numpy().reshape(-1, 12)
        assert np.array_equal(got[:, 10], np.array([1.0] * s + [0.0] * (kl.size - s), dtype=np.float32))
        assert np.array_equal(got[:s, 11], np.arange(1, s + 1, dtype=np.float32))
        assert not got[s:, 8:].any(), "columns 8..11 of a minibatch that was not applied"
        assert np.array_equal(got[: s + 1, :8].view(np.int32), free[: s + 1, :8].view(np.int32)), "the head's statistics up to the stop"
        assert np.array_equal(got[:s, 8:10].view(np.int32), free[:s, 8:10].view(np.int32))
        assert not np.isnan(got).any() and (got[s:, 4] != 0).all(), "the minibatches after the stop still report the head's statistics"
        assert opt.steps() == s

        # the loop stopped after s steps; its next minibatch's gradients are in opt2.grads, unapplied
        assert loop_of_pieces(torch, env, opt2, c, epochs, batch, lr, seed, 0, want, max_steps=s)
        torch.cuda.synchronize()
        assert_same_state(torch, opt, opt2, "target_kl")
        # one further step on the same gradients: the reconciled count gives step s + 1's bias corrections
        for g, g2 in zip(opt.grads, opt2.grads):
            g.copy_(g2)
        opt.step(lr)
        opt2.step(lr)
        torch.cuda.synchronize()
        assert_same_state(torch, opt, opt2, "the step after the stop")
        assert opt.steps() == s + 1
    finally:
        env.close()


# ------------------------------------------------------------------------------------------------- refusals
def test_refusals_on_a_live_handle():
    """One refusal per line of the header's lists, each before any device call and naming its field; nothing is written."""
    import torch
    from gym_dockauv_amd import _capi
    lib = _capi.load_library()
    env, other = torch_env(64), torch_env(64)
    try:
        actor_mlp, critic_mlp = mlps(hidden=(5,))
        policy, value = env.make_policy(actor_mlp), env.make_value(critic_mlp)
        nets = learner(torch, actor_mlp, critic_mlp)
        opt, opt_actor = optimizer(env, policy, value, nets), optimizer(env, policy, value, nets, critic=False)
        handle, foreign = env.batch._handle, other.batch._handle
        M = 256
        g = T().guarded
        rows = torch.zeros((M, N_IN + 2), device="cuda")
        actions, logp, adv, ret, vold = (torch.zeros(M * N_U, device="cuda"),) + tuple(torch.zeros(M, device="cuda") for _ in range(4))
        stats_buf, stats = g(torch, 3 * 12)
        perm_buf = torch.full((64 + 16,), -7, device="cuda", dtype=torch.int64)
        before = [p.detach().clone() for p in opt.params]

        def perm(h=handle, n=64, out=perm_buf.data_ptr()):
            rc = lib.dockauv_permutation(h, 1, 2, n, C.c_void_p(out), None)
            return rc, lib.dockauv_last_error(h)

        for kwargs, word in ((dict(h=None), b"null handle"), (dict(out=None), b"out is NULL"), (dict(n=0), b"n 0 must be >= 1"),
                             (dict(n=-3), b"must be >= 1"), (dict(n=2 ** 31 + 1), b"must be <= 2^31")):
            rc, msg = perm(**kwargs)
            assert rc == -1 and word in msg, (kwargs, rc, msg)

        def update(h=handle, o=opt, null_io=False, with_critic=True, patch=None, **over):
            io = _capi.PPOUpdateIO()
            io.struct_size = C.sizeof(_capi.PPOUpdateIO)
            io.normalize_advantage = 1
            io.rows, io.actions, io.log_prob_old = rows.data_ptr(), actions.data_ptr(), logp.data_ptr()
            io.advantages, io.returns, io.values_old = adv.data_ptr(), ret.data_ptr(), vold.data_ptr()
            io.n_rows, io.batch_size, io.n_epochs = M, 100, 1
            io.clip_range, io.vf_coef, io.ent_coef = CLIP, VF, ENT
            io.opt.struct_size = C.sizeof(_capi.OptimIO)
            io.opt.lr = 1e-3
            for i, k in enumerate(opt._six(opt.actor_params)):
                io.opt.actor_params[i], io.opt.actor_grads[i] = k or None, opt._six(opt.actor_grads)[i] or None
                if with_critic:
                    io.opt.critic_params[i], io.opt.critic_grads[i] = opt._six(opt.critic_params)[i] or None, opt._six(opt.critic_grads)[i] or None
            io.opt.log_std, io.opt.grad_log_std = opt.log_std.data_ptr(), opt.grad_log_std.data_ptr()
            io.stats = stats.data_ptr()
            for k, val in over.items():
                setattr(io, k, val)
            if patch:
                patch(io)
            rc = lib.dockauv_ppo_update(h, None if o is None else o.handle.ptr, None if null_io else C.byref(io), None)
            return rc, lib.dockauv_last_error(h)

        def opt_field(name, val):
            def patch(io):
                setattr(io.opt, name, val)
            return patch

        def opt_slot(name, i, val):
            def patch(io):
                getattr(io.opt, name)[i] = val
            return patch

        cases = [(dict(h=None), b"null handle"), (dict(o=None), b"null optimiser"), (dict(null_io=True), b"io is NULL"),
                 (dict(struct_size=16), b"dockauv_ppo_update_io.struct_size"), (dict(h=foreign), b"another handle"),
                 (dict(n_rows=0), b"n_rows"), (dict(n_rows=2 ** 31 + 1), b"n_rows"), (dict(batch_size=0), b"batch_size"),
                 (dict(n_epochs=0), b"n_epochs"), (dict(batch_size=255), b"one row"), (dict(clip_range=0.0), b"clip_range"),
                 (dict(clip_range_vf=-0.1), b"clip_range_vf"), (dict(target_kl=-0.1), b"target_kl"),
                 (dict(target_kl=float("nan")), b"target_kl"),
                 (dict(rows=None), b"rows is NULL"), (dict(actions=None), b"actions is NULL"),
                 (dict(log_prob_old=None), b"log_prob_old is NULL"), (dict(advantages=None), b"advantages is NULL"),
                 (dict(returns=None), b"returns is NULL"), (dict(clip_range_vf=0.2, values_old=None), b"values_old is NULL"),
                 (dict(o=opt_actor, with_critic=False, clip_range_vf=0.2), b"no critic"), (dict(stats=None), b"stats is NULL"),
                 (dict(patch=opt_field("stats", stats.data_ptr())), b"opt.stats must be NULL"),
                 (dict(patch=opt_field("struct_size", 8)), b"dockauv_optim_io.struct_size"),
                 (dict(patch=opt_field("lr", -1.0)), b"lr"), (dict(patch=opt_field("log_std", None)), b"log_std is NULL"),
                 (dict(patch=opt_field("grad_log_std", None)), b"grad_log_std is NULL"),
                 (dict(patch=opt_slot("actor_params", 0, None)), b"actor_params[0]"),
                 (dict(patch=opt_slot("critic_grads", 4, None)), b"critic_grads[4]"),
                 (dict(with_critic=False), b"critic_params[0]"), (dict(o=opt_actor), b"must be NULL")]
        for kwargs, word in cases:
            rc, msg = update(**kwargs)
            assert rc == -1 and word in msg, (kwargs, rc, msg)
        env.batch.synchronize()
        assert bool((perm_buf == -7).all()) and bool((stats == T().SENTINEL).all()), "a refused call wrote"
        assert all(torch.equal(x, y.detach()) for x, y in zip(before, opt.params)), "a refused call moved a parameter"
        assert opt.steps() == 0 and opt_actor.steps() == 0, "a refused call counted"
        # the good calls
        rc, msg = perm()
        assert rc == 0, (rc, msg)
        logp.fill_(-5.0)
        rc, msg = update(normalize_advantage=0)
        assert rc == 0, (rc, msg)
        rc, msg = update(o=opt_actor, with_critic=False, normalize_advantage=0, returns=None)
        assert rc == 0, (rc, msg)
        env.batch.synchronize()
        T().check_guards(stats_buf, 36, "stats")
        assert bool((perm_buf[64:] == -7).all()) and sorted(perm_buf[:64].tolist()) == list(range(64))
        assert opt.steps() == 3 and opt_actor.steps() == 3
    finally:
        env.close()
        other.close()
