"""The optimiser on a real MI355X (include/dockauv.h: dockauv_optim_*; TorchDocking3d.make_optimizer / ppo_update): three
consecutive clipped Adam steps on given gradients against the float64 statement (MLPPolicy.adam_reference) for a 20-5-6, a
36-64-64-3 and a 36-128-128-8 network, each with and without the critic, in the clipped, the unclipped and the unclipping
(max_grad_norm <= 0) regime with a learning rate that changes between the steps; the bitwise properties (two optimisers, zero
gradients, coef == 1 against no clipping, the repack against an explicit load_policy through the forward kernel and through the
head's grad_log_std); ppo_update bit for bit against the same loop written from ppo_minibatch and opt.step, and one minibatch
step against float64 autograd of the loop body of INTEGRATION.md section 6 followed by adam_reference; every refusal on a live
handle.  Every parameter array and stats sit between sentinels and, like every gradient array, start 4 bytes off 8-byte
alignment; every batch is closed in `finally`.

Bound, per array (each parameter tensor, its slice of m and of v) and for norm and coef: max |x - x64| <= max(8 x e32, 4 ulp of
max |x64|), e32 the error of a float32 NumPy restatement (adam_float32_numpy: the header's expression order, float64 only for
the sum of squares) against float64.  The measured ratios device error / max(e32, floor / 8): profiles/update/optim_error.txt
(scripts/optim_error.py on the helpers of this file; the tests print them as well).
"""
import copy
import ctypes as C
from collections import namedtuple

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHAPES = [(20, (5,), 6), (36, (64, 64), 3), (36, (128, 128), 8)]
BETAS, EPS = (0.9, 0.999), 1e-5
# (gradient norm, learning rate) of the three steps: with max_grad_norm 0.5 the first is clipped to a quarter, the second sits
# just above the threshold, the third is not clipped
STEPS = ((2.0, 3e-4), (0.6, 1e-3), (0.1, 1e-4))
CLIP, VF, ENT = 0.2, 0.5, 0.01
# norm and coef of a step whose gradients the DEVICE computed (test_one_minibatch_step_against_float64_autograd) need another
# floor than 4 ulp of their own size.  There the norm is the length of a gradient vector that two float32 backward passes -- the
# device's and float32 torch's on the CPU -- summed over 256 rows in different orders: it can be off by as much as the length of
# that vector's error (| |a| - |b| | <= |a - b|), and being ONE number it is one draw of that error on either side, which nothing
# averages: float32 torch happened to land 6.8e-9 from float64, the device 1.86e-7 and 1.26e-7 in two runs with the rows in
# different orders, against 4 ulp = 2.38e-7 -- ratios 6.23 and 4.23, too close to 8 to be a property of the code.  coef =
# max_grad_norm / (norm + 1e-6) is a function of the norm alone and carries the norm's error times |d coef / d norm| =
# coef / (norm + 1e-6) on top of its own rounding: 2.45e-7 at coef 0.81 against the same 2.38e-7, ratio 8.23, in the first run.
# So in that test the floor of the norm is 4 ulp plus GRAD_ERROR_LENGTH = the length of (float32 torch's gradients - float64's),
# the restatement's own error as a vector (measured: see the test's print), and the floor of coef is 4 ulp plus the norm's floor
# times coef / (norm + 1e-6); the factor 8 on e32 stays.  On given gradients (test_three_steps_against_float64) norm and coef keep
# the plain floor: every ratio there came out 1.00.
NORM_FLOOR_FROM_GRADIENT_ERROR = True


def T():
    """the helpers of the backward tests: guarded, check_guards, shifted_rows, bits, stream_of, SENTINEL, GUARD, P"""
    from tests import test_gpu_backward
    return test_gpu_backward


def H():
    from tests import test_gpu_head
    return test_gpu_head


def shape_id(case):
    (n_in, hidden, n_u), critic = case
    return f"{n_in}-{'-'.join(map(str, hidden))}-{n_u}-{'critic' if critic else 'nocritic'}"


CASES = [(s, c) for s in SHAPES for c in (True, False)]


def guarded_shifted(torch, n):
    """T().guarded with the n floats 4 bytes off 8-byte alignment: (whole buffer, the n floats in its middle)"""
    t = T()
    buf = torch.full((n + 2 * t.GUARD + 1,), t.SENTINEL, device="cuda")[1:]
    mid = buf[t.GUARD: t.GUARD + n]
    assert mid.data_ptr() % 8 == 4
    return buf, mid


def dev_view(torch, ptr, n):
    from gym_dockauv_amd.parallel import _DevArray
    return torch.as_tensor(_DevArray(ptr, (n,), "<f4"), device="cuda")


class Nets:
    """the arrays of one actor, its log_std and (optionally) one critic: host float32 lists in the optimiser's order and the
    MLPPolicy objects"""

    def __init__(self, shape, critic, seed):
        n_in, hidden, n_u = shape
        rng = np.random.default_rng(seed)
        self.shape, self.has_critic = shape, critic
        self.actor = T().P().make_mlp((n_in, hidden, n_u, "tanh", "none"), seed=seed, log_std=rng.uniform(-1, 0.3, n_u))
        self.critic = T().P().make_mlp((n_in, hidden, 1, "tanh", "none"), seed=seed + 1) if critic else None
        self.arrays = [a for Wb in self.actor.layers for a in Wb] + [self.actor.log_std]
        self.n_actor = len(self.arrays) - 1
        if critic:
            self.arrays += [a for Wb in self.critic.layers for a in Wb]
        self.names = [f"actor.{n}" for n in self.layer_names(self.actor)] + ["log_std"] + \
                     ([f"critic.{n}" for n in self.layer_names(self.critic)] if critic else [])

    @staticmethod
    def layer_names(mlp):
        return ["W1", "b1", "W2", "b2", "W3", "b3"] if len(mlp.layers) == 3 else ["W1", "b1", "W3", "b3"]

    def draw_grads(self, rng, norm):
        g = [rng.normal(size=a.shape) for a in self.arrays]
        scale = norm / np.sqrt(sum((x * x).sum() for x in g))
        return [np.ascontiguousarray(x * scale, dtype=np.float32) for x in g]


class DeviceSide:
    """guarded device copies of a Nets' arrays, an actor and a critic on `env`, and one dockauv_optim over them"""

    def __init__(self, torch, env, nets, max_grad_norm, betas=BETAS, eps=EPS):
        self.torch, self.env, self.nets = torch, env, nets
        self.bufs = [guarded_shifted(torch, a.size) for a in nets.arrays]
        for (_, mid), a in zip(self.bufs, nets.arrays):
            mid.copy_(torch.from_numpy(a.reshape(-1)))
        self.stats_buf = guarded_shifted(torch, 2)
        self.policy = env.make_policy(nets.actor)
        self.value = env.make_value(nets.critic) if nets.has_critic else None
        # (the actor's log_std came with the host arrays: has_log_std is set)
        self.opt = env.make_optim(self.policy, self.value, betas=betas, eps=eps, max_grad_norm=max_grad_norm)
        self.lens = [a.size for a in nets.arrays]

    def six(self, ptrs):
        ptrs = list(ptrs)
        if len(ptrs) == 4:
            ptrs[2:2] = [0, 0]
        return ptrs

    def ptr_sets(self, tensors):
        na = self.nets.n_actor
        ptrs = [t.data_ptr() for t in tensors]
        return self.six(ptrs[:na]), ptrs[na], (self.six(ptrs[na + 1:]) if self.nets.has_critic else None)

    def step(self, grads, lr, want_stats=True):
        """one dockauv_optim_step on host gradients (copied to the device 4 bytes off 8-byte alignment); returns (norm, coef)"""
        torch = self.torch
        g_dev = [T().shifted_rows(torch, torch.from_numpy(g.reshape(-1)).cuda()) for g in grads]
        ap, ls, cp = self.ptr_sets([mid for _, mid in self.bufs])
        ag, gls, cg = self.ptr_sets(g_dev)
        self.env.optim_step_device(self.opt, lr, ap, ls, ag, gls, cp, cg, stats_ptr=self.stats_buf[1].data_ptr() if want_stats else 0,
                                   stream=T().stream_of(torch))
        torch.cuda.synchronize()
        for g, h in zip(g_dev, grads):
            assert np.array_equal(g.cpu().numpy().view(np.int32), h.reshape(-1).view(np.int32)), "a gradient array was written"
        self.check_guards()
        st = self.stats_buf[1].cpu().numpy()
        return float(st[0]), float(st[1])

    def check_guards(self):
        for (buf, mid), name in zip(self.bufs, self.nets.names):
            T().check_guards(buf, mid.numel(), name)
        T().check_guards(self.stats_buf[0], 2, "stats")

    def params(self):
        return [mid.cpu().numpy().reshape(a.shape) for (_, mid), a in zip(self.bufs, self.nets.arrays)]

    def moments(self):
        m_ptr, v_ptr, n, t = self.env.optim_state(self.opt)
        assert n == sum(self.lens)
        out = []
        for ptr in (m_ptr, v_ptr):
            flat = dev_view(self.torch, ptr, n).cpu().numpy()
            out.append([x.reshape(a.shape) for x, a in zip(np.split(flat, np.cumsum(self.lens)[:-1]), self.nets.arrays)])
        return out[0], out[1], t


def fma32(a, b, c):
    return H().fma32(np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32), c)


def adam_float32_numpy(params, grads, m, v, t, lr, betas, eps, max_grad_norm):
    """the definition of the header in float32 NumPy arrays, float64 only for the sum of squares and for the host scalars"""
    f = np.float32
    total = sum(float((g.astype(np.float64) ** 2).sum()) for g in grads)
    norm = f(np.sqrt(total))
    coef = min(f(1), f(max_grad_norm) / (norm + f(1e-6))) if max_grad_norm > 0 else f(1)
    c1, c2, b2 = f(1.0 - betas[0]), f(1.0 - betas[1]), f(betas[1])
    step_size, rsq = f(lr / (1.0 - betas[0] ** t)), f(1.0 / np.sqrt(1.0 - betas[1] ** t))
    new_p, new_m, new_v = [], [], []
    for p, g, a, b in zip(params, grads, m, v):
        g = g * f(coef)
        a = fma32(c1, g - a, a)
        b = fma32(c2 * g, g, b2 * b)
        denom = fma32(np.sqrt(b), rsq, f(eps))
        p = p - step_size * (a / denom)
        for x in (g, a, b, denom, p):
            assert x.dtype == f
        new_p.append(p)
        new_m.append(a)
        new_v.append(b)
    return new_p, new_m, new_v, f(norm), f(coef)


def judge(label, name, dev, f32, ref, extra_floor=0.0):
    """(device error, float32 NumPy error, bound, ratio) of one array; prints the figures.  extra_floor: added to the floor of
    4 ulp (NORM_FLOOR_FROM_GRADIENT_ERROR: the two outputs that have one)"""
    dev, f32, ref = (np.asarray(x, dtype=np.float64).reshape(-1) for x in (dev, f32, ref))
    assert dev.shape == ref.shape and not np.isnan(dev).any(), (label, name)
    e_dev, e_np = float(np.abs(dev - ref).max()), float(np.abs(f32 - ref).max())
    floor = 4.0 * float(np.spacing(np.float32(np.abs(ref).max()))) + extra_floor
    bound = max(8.0 * e_np, floor)
    ratio = e_dev / max(e_np, floor / 8.0)
    print(f"optim {label} {name}: device {e_dev:.3e}, float32 NumPy {e_np:.3e}, bound {bound:.3e}, ratio {ratio:.2f}")
    return e_dev, e_np, bound, ratio


def three_steps_case(case, max_grad_norm, env=None):
    """[(label, array name, device error, float32 NumPy error, bound, ratio)] over three consecutive steps"""
    import torch
    from gym_dockauv_amd.policy import MLPPolicy
    shape, critic = case
    nets = Nets(shape, critic, seed=11)
    own = env is None
    if own:
        env = T().P().fan_env(shape[0], shape[2], 64)
    res = []
    try:
        side = DeviceSide(torch, env, nets, max_grad_norm)
        rng = np.random.default_rng(5)
        zeros = lambda: [np.zeros(a.shape) for a in nets.arrays]
        p64, m64, v64 = [a.astype(np.float64) for a in nets.arrays], zeros(), zeros()
        p32, m32, v32 = list(nets.arrays), [z.astype(np.float32) for z in zeros()], [z.astype(np.float32) for z in zeros()]
        for t, (norm_target, lr) in enumerate(STEPS, start=1):
            grads = nets.draw_grads(rng, norm_target)
            norm_dev, coef_dev = side.step(grads, lr)
            p64, m64, v64, norm64, coef64 = MLPPolicy.adam_reference(p64, grads, m64, v64, t, lr, BETAS, EPS, max_grad_norm)
            p32, m32, v32, norm32, coef32 = adam_float32_numpy(p32, grads, m32, v32, t, lr, BETAS, EPS, max_grad_norm)
            if max_grad_norm > 0:
                assert (coef64 < 1.0) == (norm_target > max_grad_norm), "the step is not in the regime it is meant for"
            else:
                assert coef64 == 1.0 and coef_dev == 1.0
            m_dev, v_dev, steps = side.moments()
            assert steps == t
            label = f"{shape_id(case)}_mgn{max_grad_norm:g}_step{t}"
            res.append((label, "norm") + judge(label, "norm", [norm_dev], [norm32], [norm64]))
            res.append((label, "coef") + judge(label, "coef", [coef_dev], [coef32], [coef64]))
            for kind, dev, f32, ref in (("p", side.params(), p32, p64), ("m", m_dev, m32, m64), ("v", v_dev, v32, v64)):
                for name, d, f, r in zip(nets.names, dev, f32, ref):
                    res.append((label, f"{kind}.{name}") + judge(label, f"{kind}.{name}", d, f, r))
    finally:
        if own:
            env.close()
    return res


@pytest.mark.parametrize("case", CASES, ids=shape_id)
def test_three_steps_against_float64(case):
    """max_grad_norm 0.5: a clipped step, one just above the threshold, an unclipped one; max_grad_norm 0: no clipping; the
    learning rate changes between the steps."""
    env = T().P().fan_env(case[0][0], case[0][2], 64)
    worst = (0.0, "")
    try:
        for max_grad_norm in (0.5, 0.0):
            for label, name, e_dev, e_np, bound, ratio in three_steps_case(case, max_grad_norm, env):
                worst = max(worst, (ratio, f"{label} {name}"))
                assert e_dev <= bound, (label, name, e_dev, e_np, bound)
    finally:
        env.close()
    print(f"optim {shape_id(case)}: largest ratio device error / max(e32, floor / 8) = {worst[0]:.2f} ({worst[1]})")


def head_rows_for(log_std, n, n_u, seed):
    """test_gpu_head.draw_head with the actions and old log-probabilities moved to `log_std` (the actor's, which the head reads):
    the same normals and the same spread of the ratios"""
    from gym_dockauv_amd.policy import MLPPolicy
    d, _, _ = H().draw_head(n, n_u, seed=seed)
    ls_d, ls = d["log_std"].astype(np.float64), np.asarray(log_std, dtype=np.float64)
    mean = d["mean"].astype(np.float64)
    z = (d["actions"].astype(np.float64) - mean) * np.exp(-ls_d)
    noise = MLPPolicy.log_prob_reference(z, ls_d) - d["log_prob_old"].astype(np.float64)
    d["actions"] = np.ascontiguousarray(mean + np.exp(ls) * z, dtype=np.float32)
    d["log_prob_old"] = np.ascontiguousarray(MLPPolicy.log_prob_reference(z, ls) - noise, dtype=np.float32)
    d["log_std"] = np.ascontiguousarray(ls, dtype=np.float32)
    return d


def same_bits(a, b):
    return all(np.array_equal(np.ascontiguousarray(x).view(np.int32), np.ascontiguousarray(y).view(np.int32)) for x, y in zip(a, b))


@pytest.mark.parametrize("case", CASES, ids=shape_id)
def test_bitwise_properties(case):
    """Two optimisers on equal inputs; zero gradients; coef == 1 against max_grad_norm <= 0; the repack against load_policy."""
    import torch
    shape, critic = case
    n_in, _, n_u = shape
    nets = Nets(shape, critic, seed=21)
    env = T().P().fan_env(n_in, n_u, 64)
    try:
        rng = np.random.default_rng(9)
        g_big, g_small = nets.draw_grads(rng, 3.0), nets.draw_grads(rng, 0.1)
        a, b = DeviceSide(torch, env, nets, 0.5), DeviceSide(torch, env, nets, 0.5)
        for side in (a, b):
            assert side.step(g_big, 3e-4)[1] < 1.0
            assert side.step(g_small, 1e-3)[1] == 1.0
        assert same_bits(a.params(), b.params()), "two optimisers differ in the parameters"
        (ma, va, ta), (mb, vb, tb) = a.moments(), b.moments()
        assert ta == tb == 2 and same_bits(ma, mb) and same_bits(va, vb), "two optimisers differ in the moments"
        assert not same_bits(a.params(), nets.arrays)

        zero = DeviceSide(torch, env, nets, 0.5)
        norm, coef = zero.step([np.zeros_like(x) for x in nets.arrays], 1e-3)
        assert norm == 0.0 and coef == 1.0
        assert same_bits(zero.params(), nets.arrays), "zero gradients moved a parameter"
        mz, vz, _ = zero.moments()
        assert all(not x.any() for x in mz + vz)

        clip, free = DeviceSide(torch, env, nets, 0.5), DeviceSide(torch, env, nets, 0.0)
        assert clip.step(g_small, 1e-3)[1] == 1.0 and free.step(g_small, 1e-3)[1] == 1.0
        assert same_bits(clip.params(), free.params()) and same_bits(clip.moments()[0], free.moments()[0]) \
            and same_bits(clip.moments()[1], free.moments()[1]), "coef == 1 differs from no clipping"

        # the repack: the networks of `side` hold the updated weights and log_std without a load_policy
        side = DeviceSide(torch, env, nets, 0.5)
        rows, _, _ = T().make_rows(torch, nets.actor, 65, seed=4)
        d = head_rows_for(nets.actor.log_std, 65, n_u, seed=2)
        pols = [side.policy] + ([side.value] if critic else [])
        fwd = lambda: [T().run_forward_rows(torch, env, p, rows, 65).cpu().numpy() for p in pols]
        head = lambda: H().run_head(torch, env, side.policy, d, True, False)
        before, head_before = fwd(), head()
        side.step(g_big, 1e-2)
        after, head_after = fwd(), head()
        ap, ls, cp = side.ptr_sets([mid for _, mid in side.bufs])
        env.load_policy(side.policy, device_ptrs=ap, log_std_ptr=ls, stream=T().stream_of(torch))
        if critic:
            env.load_policy(side.value, device_ptrs=cp, stream=T().stream_of(torch))
        loaded, head_loaded = fwd(), head()
        for x, y, z in zip(before, after, loaded):
            assert not np.array_equal(x, y), "the step did not reach the network"
            assert np.array_equal(y.view(np.int32), z.view(np.int32)), "the repack differs from load_policy of the updated arrays"
        assert not np.array_equal(head_before[2], head_after[2]) and head_before[3][3] != head_after[3][3], \
            "the step did not reach the actor's log_std"
        for y, z in zip(head_after, head_loaded):
            if y is not None:
                assert np.array_equal(y.view(np.int32), z.view(np.int32)), "the repacked log_std differs from load_policy's"
        for s in (a, b, zero, clip, free, side):
            s.check_guards()
    finally:
        env.close()


# ------------------------------------------------------------------------------------------------- ppo_update
Collected = namedtuple("Collected", ["obs", "actions", "reward", "done", "log_prob", "values", "advantages", "returns"])
N_IN, N_U = 20, 6


def torch_env():
    from gym_dockauv_amd.config.env_config import BASE_CONFIG
    from gym_dockauv_amd.envs.torch_env import TorchDocking3d
    cfg = copy.deepcopy(BASE_CONFIG)
    cfg["radar"].update(T().P().FANS[N_IN])
    env = TorchDocking3d(cfg, num_envs=64, scenario="ObstaclesDocking3d", device_seed=7)
    assert (env.n_obs, env.n_u) == (N_IN, N_U)
    return env


def learner(torch, actor_mlp, critic_mlp):
    a_net, c_net = H().sequential(torch, actor_mlp, torch.float32, "cuda"), H().sequential(torch, critic_mlp, torch.float32, "cuda")
    log_std = torch.tensor(actor_mlp.log_std, device="cuda", requires_grad=True)
    return a_net, c_net, log_std


def test_ppo_update_is_the_loop_of_its_pieces():
    """2 epochs x 3 minibatches (100, 100 and 56 of 4 x 64 rows): ppo_update bit for bit against ppo_minibatch, a copy of every
    .grad into opt.grads and opt.step, with the same generator seed; stats [2, 3, 10] with the head's bits in front."""
    import torch
    env = torch_env()
    try:
        actor_mlp = T().P().make_mlp((N_IN, (64, 64), N_U, "tanh", "none"), seed=6, log_std=np.full(N_U, -0.5))
        critic_mlp = T().P().make_mlp((N_IN, (64, 64), 1, "tanh", "none"), seed=7)
        policy, value = env.make_policy(actor_mlp, seed=3), env.make_value(critic_mlp)
        nets = [learner(torch, actor_mlp, critic_mlp) for _ in range(2)]
        env.load_policy(policy, nets[0][0], log_std=nets[0][2])
        env.reset()
        K, N = 4, 64
        c = env.collect(policy, value, K, gamma=0.99, gae_lambda=0.95)
        kw = dict(clip_range=CLIP, vf_coef=VF, ent_coef=ENT)
        lr = 3e-3

        a_net, c_net, log_std = nets[0]
        opt = env.make_optimizer(policy, value, list(a_net.parameters()), log_std, list(c_net.parameters()))
        gen = torch.Generator(device="cuda")
        gen.manual_seed(3)
        stats = env.ppo_update(opt, c, 2, 100, lr, generator=gen, **kw)
        torch.cuda.synchronize()
        assert tuple(stats.shape) == (2, 3, 10) and stats.device.type == "cuda"
        got = [p.detach().clone() for p in list(a_net.parameters()) + [log_std] + list(c_net.parameters())]
        # the networks hold the last step's weights: the forward kernel gives what a load of the updated tensors gives
        mean_after = env.mlp_forward(policy, c.obs[:K]).clone()
        v_after = env.mlp_forward(value, c.obs[:K]).clone()

        a_net, c_net, log_std = nets[1]
        a_params, c_params = list(a_net.parameters()), list(c_net.parameters())
        opt2 = env.make_optimizer(policy, value, a_params, log_std, c_params)
        gen.manual_seed(3)
        rows = c.obs[:K]
        flat = lambda t: t.reshape(K * N, *t.shape[2:])
        want_stats = torch.zeros((2, 3, 10), device="cuda")
        for e in range(2):
            perm = torch.randperm(K * N, device="cuda", generator=gen)
            for j, idx in enumerate(perm.split(100)):
                st = env.ppo_minibatch(policy, value, a_params, log_std, c_params, flat(c.actions), flat(c.log_prob), flat(c.advantages),
                                       flat(c.returns), rows, idx, **kw)
                for g, p in zip(opt2.grads, a_params + [log_std] + c_params):
                    g.copy_(p.grad)
                want_stats[e, j, :8] = st
                opt2.step(lr, stats=want_stats[e, j, 8:])
        torch.cuda.synchronize()
        assert [int(x.numel()) for x in perm.split(100)] == [100, 100, 56]
        want = [p.detach() for p in a_params + [log_std] + c_params]
        for x, y, p0 in zip(got, want, [a for Wb in actor_mlp.layers for a in Wb] + [actor_mlp.log_std] + [a for Wb in critic_mlp.layers for a in Wb]):
            assert torch.equal(T().bits(x), T().bits(y)), "ppo_update differs from the loop of its pieces"
            assert not np.array_equal(x.cpu().numpy(), p0), "a parameter did not move"
        assert torch.equal(T().bits(stats), T().bits(want_stats))
        s = stats.cpu().numpy()
        assert not np.isnan(s).any() and (s[:, :, 8] > 0).all() and (s[:, :, 9] > 0).all() and (s[:, :, 9] <= 1).all()
        env.load_policy(policy, a_net, log_std=log_std)
        env.load_policy(value, c_net)
        assert torch.equal(T().bits(env.mlp_forward(policy, rows)), T().bits(mean_after))
        assert torch.equal(T().bits(env.mlp_forward(value, rows)), T().bits(v_after))
    finally:
        env.close()


def test_one_minibatch_step_against_float64_autograd():
    """One ppo_update minibatch of 256 rows (a hand-made collection from test_gpu_head.draw_head, rows off the clip edges) against
    float64 autograd of the section-6 body on the CPU followed by adam_reference; e32: the same body in float32 torch on the CPU
    followed by adam_float32_numpy.  The bound of the module's docstring, per parameter tensor and for the norm and coef."""
    import torch
    from gym_dockauv_amd.policy import MLPPolicy
    env = torch_env()
    try:
        K, N, lr = 4, 64, 3e-4
        n = K * N
        actor_mlp = T().P().make_mlp((N_IN, (64, 64), N_U, "tanh", "none"), seed=6, log_std=np.zeros(N_U))
        critic_mlp = T().P().make_mlp((N_IN, (64, 64), 1, "tanh", "none"), seed=7)
        rng = np.random.default_rng(11)
        draw = n + max(8, n // 16)
        cand = rng.uniform(-1, 1, (draw, N_IN)).astype(np.float32)
        d, _, _, kept = H().draw_head(n, N_U, seed=12, mean=actor_mlp.forward_reference(cand.astype(np.float64)), edge=1e-4, want_kept=True)
        actor_mlp.log_std = d["log_std"]
        packed = np.full((K + 1, N, N_IN + 2), np.nan, dtype=np.float32)
        packed[:K, :, :N_IN] = cand[kept].reshape(K, N, N_IN)
        packed[K, :, :N_IN] = 0.0

        p_new, norm, coef, grads_of = {}, {}, {}, {}
        for kind, dt in (("f32", torch.float32), ("f64", torch.float64)):
            a_net, c_net = H().sequential(torch, actor_mlp, dt, "cpu"), H().sequential(torch, critic_mlp, dt, "cpu")
            ls = torch.tensor(d["log_std"], dtype=dt, requires_grad=True)
            g = lambda x: torch.from_numpy(x).to(dt)
            loss, _, _ = H().section6_body(torch, a_net, c_net, ls, g(cand[kept]), g(d["actions"]), g(d["log_prob_old"]),
                                           g(d["advantages"]), g(d["returns"]))
            loss.backward()
            ps = list(a_net.parameters()) + [ls] + list(c_net.parameters())
            params, grads = [p.detach().numpy() for p in ps], [p.grad.numpy() for p in ps]
            grads_of[kind] = [g.astype(np.float64) for g in grads]
            zeros = [np.zeros(p.shape, dtype=params[0].dtype) for p in params]
            step = MLPPolicy.adam_reference if kind == "f64" else adam_float32_numpy
            p_new[kind], _, _, norm[kind], coef[kind] = step(params, grads, zeros, zeros, 1, lr, BETAS, EPS, 0.5)

        policy, value = env.make_policy(actor_mlp), env.make_value(critic_mlp)
        a_net, c_net, log_std = learner(torch, actor_mlp, critic_mlp)
        opt = env.make_optimizer(policy, value, list(a_net.parameters()), log_std, list(c_net.parameters()))
        rows_t = torch.from_numpy(packed).cuda()
        dev = lambda a, *tail: torch.from_numpy(a).cuda().view(K, N, *tail)
        c = Collected(rows_t[:, :, :N_IN], dev(d["actions"], N_U), None, None, dev(d["log_prob_old"]), None, dev(d["advantages"]),
                      dev(d["returns"]))
        gen = torch.Generator(device="cuda")
        gen.manual_seed(5)
        stats = env.ppo_update(opt, c, 1, n, lr, clip_range=CLIP, vf_coef=VF, ent_coef=ENT, generator=gen)
        torch.cuda.synchronize()
        assert tuple(stats.shape) == (1, 1, 10)
        got = [p.detach().cpu().numpy() for p in list(a_net.parameters()) + [log_std] + list(c_net.parameters())]
        names = [f"actor.{x}" for x in ("W1", "b1", "W2", "b2", "W3", "b3")] + ["log_std"] + [f"critic.{x}" for x in ("W1", "b1", "W2", "b2", "W3", "b3")]
        s = stats.cpu().numpy()[0, 0]
        checks = [("norm", [s[8]], [norm["f32"]], [norm["f64"]]), ("coef", [s[9]], [coef["f32"]], [coef["f64"]])]
        checks += [(f"p.{nm}", x, f, r) for nm, x, f, r in zip(names, got, p_new["f32"], p_new["f64"])]
        grad_error_length = float(np.sqrt(sum(((a - b) ** 2).sum() for a, b in zip(grads_of["f32"], grads_of["f64"]))))
        print(f"optim ppo_update_one_minibatch: length of float32 torch's gradient error {grad_error_length:.3e}")
        extra_of = {}
        if NORM_FLOOR_FROM_GRADIENT_ERROR:
            extra_of["norm"] = grad_error_length
            extra_of["coef"] = (4.0 * float(np.spacing(np.float32(norm["f64"]))) + grad_error_length) * coef["f64"] / (norm["f64"] + 1e-6)
        for name, x, f, r in checks:
            extra = extra_of.get(name, 0.0)
            e_dev, e_np, bound, ratio = judge("ppo_update_one_minibatch", name, x, f, r, extra)
            assert e_dev <= bound, (name, e_dev, e_np, bound)
    finally:
        env.close()


def test_ppo_update_refuses_a_last_minibatch_of_one_row():
    import torch
    env = torch_env()
    try:
        actor_mlp = T().P().make_mlp((N_IN, (5,), N_U, "tanh", "none"), seed=6, log_std=np.zeros(N_U))
        critic_mlp = T().P().make_mlp((N_IN, (5,), 1, "tanh", "none"), seed=7)
        policy, value = env.make_policy(actor_mlp), env.make_value(critic_mlp)
        a_net, c_net, log_std = learner(torch, actor_mlp, critic_mlp)
        opt = env.make_optimizer(policy, value, list(a_net.parameters()), log_std, list(c_net.parameters()))
        env.load_policy(policy, a_net, log_std=log_std)
        env.reset()
        c = env.collect(policy, value, 4, gamma=0.99, gae_lambda=0.95)
        before = [p.detach().clone() for p in opt.params]
        with pytest.raises(ValueError, match="one row"):
            env.ppo_update(opt, c, 1, 255, 3e-4, clip_range=CLIP, vf_coef=VF, ent_coef=ENT)
        with pytest.raises(ValueError):
            env.make_optimizer(policy, None, list(a_net.parameters()), log_std, list(c_net.parameters()))
        with pytest.raises(ValueError):
            env.make_optimizer(policy, value, list(a_net.parameters())[:-1], log_std, list(c_net.parameters()))
        with pytest.raises(ValueError):
            opt.step(3e-4, stats=torch.zeros(3, device="cuda"))
        torch.cuda.synchronize()
        assert all(torch.equal(x, y) for x, y in zip(before, opt.params)), "a refused call moved a parameter"
        stats = env.ppo_update(opt, c, 1, 255, 3e-4, clip_range=CLIP, vf_coef=VF, ent_coef=ENT, normalize_advantage=False)
        assert tuple(stats.shape) == (1, 2, 10)
        # actor only
        opt_a = env.make_optimizer(policy, None, list(a_net.parameters()), log_std, None)
        assert len(opt_a.grads) == 5
        opt_a.step(3e-4)
        torch.cuda.synchronize()
    finally:
        env.close()


def test_refusals_on_a_live_handle():
    """One refusal per line of the header's list, each before any device call and naming its field; then the good calls."""
    import torch
    from gym_dockauv_amd import _capi
    lib = _capi.load_library()
    P = T().P()
    env, other = P.fan_env(20, 6, 64), P.fan_env(20, 6, 64)
    try:
        nets = Nets((20, (5,), 6), True, seed=1)
        actor, critic = env.make_policy(nets.actor), env.make_value(nets.critic)
        no_std = env.make_policy(P.make_mlp((20, (5,), 6, "tanh", "none"), seed=3))
        foreign_actor, foreign_critic = other.make_policy(nets.actor), other.make_value(nets.critic)

        def create(handle=env._handle, a=actor, c=critic, null_desc=False, null_out=False, **over):
            d = _capi.OptimDesc()
            d.struct_size = C.sizeof(_capi.OptimDesc)
            d.beta1, d.beta2, d.eps, d.max_grad_norm = 0.9, 0.999, 1e-5, 0.5
            for k, val in over.items():
                setattr(d, k, val)
            out = C.c_void_p()
            rc = lib.dockauv_optim_create(handle, None if a is None else a.ptr, None if c is None else c.ptr,
                                          None if null_desc else C.byref(d), None if null_out else C.byref(out))
            return rc, lib.dockauv_last_error(handle), out

        for kwargs, word in ((dict(handle=None), b"null handle"), (dict(a=None), b"null actor"), (dict(null_desc=True), b"desc is NULL"),
                             (dict(null_out=True), b"out is NULL"), (dict(struct_size=8), b"struct_size"), (dict(a=critic), b"is a critic"),
                             (dict(c=actor), b"is an actor"), (dict(a=foreign_actor), b"another handle"),
                             (dict(c=foreign_critic), b"another handle"), (dict(a=no_std), b"log_std"), (dict(beta1=1.0), b"beta1"),
                             (dict(beta1=-0.1), b"beta1"), (dict(beta2=1.0), b"beta2"), (dict(beta2=float("nan")), b"beta2"),
                             (dict(eps=0.0), b"eps"), (dict(eps=-1e-5), b"eps")):
            rc, msg, out = create(**kwargs)
            assert rc == -1 and word in msg and not out.value, (kwargs, rc, msg)
        rc, msg, opt = create()
        assert rc == 0 and opt.value, (rc, msg)
        rc, msg, opt_actor_only = create(c=None)
        assert rc == 0 and opt_actor_only.value, (rc, msg)

        params = [torch.from_numpy(a.reshape(-1).copy()).cuda() for a in nets.arrays]
        grads = [torch.full_like(p, 0.01) for p in params]
        stats = torch.zeros(2, device="cuda")
        before = [p.clone() for p in params]
        slot = {0: 0, 1: 1, 2: 4, 3: 5}     # W1 b1 W3 b3 of the one-hidden-layer networks

        def step(handle=env._handle, o=opt, null_io=False, with_critic=True, patch=None, **over):
            io = _capi.OptimIO()
            io.struct_size = C.sizeof(_capi.OptimIO)
            io.lr = 1e-3
            for i in range(4):
                io.actor_params[slot[i]], io.actor_grads[slot[i]] = params[i].data_ptr(), grads[i].data_ptr()
                if with_critic:
                    io.critic_params[slot[i]], io.critic_grads[slot[i]] = params[5 + i].data_ptr(), grads[5 + i].data_ptr()
            io.log_std, io.grad_log_std, io.stats = params[4].data_ptr(), grads[4].data_ptr(), stats.data_ptr()
            for k, val in over.items():
                setattr(io, k, val)
            if patch:
                patch(io)
            rc = lib.dockauv_optim_step(handle, o, None if null_io else C.byref(io), None)
            return rc, lib.dockauv_last_error(handle)

        def setter(field, i, val):
            def patch(io):
                getattr(io, field)[i] = val
            return patch

        spare = torch.zeros(8, device="cuda").data_ptr()
        cases = [(dict(handle=None), b"null handle"), (dict(o=None), b"null optimiser"), (dict(null_io=True), b"io is NULL"),
                 (dict(struct_size=16), b"struct_size"), (dict(handle=other._handle), b"another handle"),
                 (dict(lr=-1e-3), b"lr"), (dict(lr=float("nan")), b"lr"), (dict(lr=float("inf")), b"lr"),
                 (dict(log_std=None), b"log_std is NULL"), (dict(grad_log_std=None), b"grad_log_std is NULL"),
                 (dict(grad_log_std=params[4].data_ptr()), b"grad_log_std is the log_std pointer"),
                 (dict(with_critic=False), b"critic_params[0]"),
                 (dict(o=opt_actor_only), b"critic_params[0] (W1) must be NULL")]
        for field in ("actor_params", "actor_grads", "critic_params", "critic_grads"):
            for i in (0, 1, 4, 5):
                cases.append((dict(patch=setter(field, i, None)), f"{field}[{i}]".encode()))
            for i in (2, 3):
                cases.append((dict(patch=setter(field, i, spare)), f"{field}[{i}]".encode()))
        for who, first in (("actor", 0), ("critic", 5)):
            cases.append((dict(patch=setter(f"{who}_grads", 0, params[first].data_ptr())), f"{who}_grads[0] (W1) is the params pointer".encode()))
        for kwargs, word in cases:
            rc, msg = step(**kwargs)
            assert rc == -1 and word in msg, (kwargs, rc, msg)
        env.synchronize()
        steps = C.c_longlong(-1)
        assert lib.dockauv_optim_state(opt, None, None, None, C.byref(steps)) == 0 and steps.value == 0, "a refused step counted"
        assert all(torch.equal(x, y) for x, y in zip(before, params)) and not bool(stats.any()), "a refused call wrote"
        rc, msg = step()
        assert rc == 0, (rc, msg)
        rc, msg = step(o=opt_actor_only, with_critic=False, stats=None)
        assert rc == 0, (rc, msg)
        env.synchronize()
        assert lib.dockauv_optim_state(opt, None, None, None, C.byref(steps)) == 0 and steps.value == 1
        assert float(stats[0]) > 0 and not any(torch.equal(x, y) for x, y in zip(before, params))
        assert lib.dockauv_optim_destroy(opt) == 0 and lib.dockauv_optim_destroy(opt_actor_only) == 0
    finally:
        env.close()
        other.close()
