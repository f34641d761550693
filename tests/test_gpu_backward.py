"""The MLP backward and the gathered forward on a real MI355X (include/dockauv.h: dockauv_policy_backward,
dockauv_policy_forward_rows; TorchDocking3d.mlp_forward / mlp_backward / mlp_apply): every policy_backward_kernel<MT1, MT2> against
the float64 statement (MLPPolicy.backward_reference) at 1, 33 and 129 rows, more rows than the bounded grid covers in one pass,
the bitwise properties (two calls, a gather against the dense copy, duplicates, NaN rows outside the index), forward_rows bit for
bit against policy_forward and value_forward, a PPO-shaped loss through mlp_apply against float64 autograd on the CPU, and
refusals on a live handle.  The reward and done columns of every row are NaN; every output sits between sentinels; the rows
start 4 bytes off 8-byte alignment.  Every batch is closed in `finally`.

Bound, per gradient tensor: max |g - g64| <= max(8 x e32, 4 ulp of max |g64|), e32 the error of a float32 NumPy restatement of
the same case against float64 (backward_float32_numpy).  The measured ratios: profiles/update/backward_error.txt (written by
scripts/backward_error.py from the helpers of this file; the tests print them as well).  Measured on an MI355X: the largest
ratio device error / max(e32, floor / 8) over all cases is 3.87 with np.tanh in the restatement (25-96-63-3 tanh, one row, dW3)
and 3.17 with the kernel's tanh form, so the restatement keeps np.tanh.
"""
import copy
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SENTINEL = -7.0
GUARD = 32                    # sentinel floats in front of and behind every output
RELU_MARGIN = 1e-5            # a unit whose float64 pre-activation is closer to zero may switch sides in float32
# the float32 restatement's tanh: "libm" = np.tanh in float32 (half an ulp); "kernel" = the kernel's own form
# 1 - 2 / (exp(2 x) + 1) evaluated in float32 (absolute error up to ~3e-7)
TANH_FORM = "libm"
# rows one pass of the bounded grid covers with the 64-64 networks: 256 groups (dockauv_device.h: kBwdMaxGroups, one per CU) x
# 64 rows a pass (two hidden tiles -> two row tiles of 32, BackwardLayout::rt); 33 more rows: a second pass of one group, with a
# full row tile and a single lane of the next
ROWS_BEYOND_ONE_PASS = 256 * 64 + 33


def P():
    """the helpers of the policy tests: make_mlp, fan_env, nan_rows, TILE_PAIRS, WIDE, WIDEST, FORWARD_BOUND"""
    from tests import test_gpu_policy
    return test_gpu_policy


def stream_of(torch):
    return torch.cuda.current_stream().cuda_stream


def bits(x):
    import torch
    return x.contiguous().view(torch.int32)


def shape_id(s):
    return f"{s[0]}-{'-'.join(map(str, s[1]))}-{s[2]}-{s[3]}-{s[4]}"


def guarded(torch, n):
    """(whole buffer, the n floats in its middle)"""
    buf = torch.full((n + 2 * GUARD,), SENTINEL, device="cuda")
    return buf, buf[GUARD: GUARD + n]


def check_guards(buf, n, what):
    assert bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[GUARD + n:] == SENTINEL).all()), f"the kernel wrote outside {what}"


def shifted_rows(torch, rows):
    """a copy of `rows` that starts one float behind an allocation's start: 4-byte and not 8-byte aligned"""
    d = torch.empty(rows.numel() + 1, device="cuda")[1:].view(rows.shape)
    d.copy_(rows)
    assert d.data_ptr() % 8 == 4
    return d


def draw_rows(mlp, n, seed):
    """n packed rows on the host (observation columns U(-1, 1) from NumPy's generator, reward / done NaN).  For a relu network
    the rows with a hidden unit whose float64 pre-activation lies within RELU_MARGIN of zero are dropped from a slightly larger
    draw, decided here from the float64 forward; returns (rows float32 [n, n_in + 2], rows dropped, rows drawn)."""
    n_in = mlp.n_in
    draw = n + max(8, n // 16)
    cand = np.full((draw, n_in + 2), np.nan, dtype=np.float32)
    cand[:, :n_in] = np.random.default_rng(seed).uniform(-1, 1, (draw, n_in)).astype(np.float32)
    keep = np.ones(draw, dtype=bool)
    if mlp.hidden_act == "relu":
        x = cand[:, :n_in].astype(np.float64)
        for W, b in mlp.layers[:-1]:
            pre = x @ W.astype(np.float64).T + b.astype(np.float64)
            keep &= ~(np.abs(pre) < RELU_MARGIN).any(axis=1)
            x = np.maximum(pre, 0.0)
    idx = np.flatnonzero(keep)[:n]
    assert idx.size == n
    return cand[idx], int((~keep).sum()), draw


def make_rows(torch, mlp, n, seed):
    """draw_rows on the device, 4 bytes off 8-byte alignment: (rows, rows dropped, rows drawn)"""
    rows, dropped, draw = draw_rows(mlp, n, seed)
    return shifted_rows(torch, torch.from_numpy(rows).cuda()), dropped, draw


def make_grad_out(torch, n, n_out, seed):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    return torch.randn((n, n_out), device="cuda", generator=g).contiguous()


def device_policy(env, mlp):
    return env.make_value(mlp) if (mlp.n_out == 1 and mlp.n_out != env.n_u) else env.make_policy(mlp)


def run_backward(torch, env, pol, mlp, rows, grad_out, index=None):
    """dockauv_policy_backward into guarded buffers; returns the gradients as device tensors in layer order"""
    shapes = [s for W, b in mlp.layers for s in (W.shape, b.shape)]
    bufs = [guarded(torch, int(np.prod(s))) for s in shapes]
    ptrs = [v.data_ptr() for _, v in bufs]
    if len(ptrs) == 4:
        ptrs[2:2] = [0, 0]
    n = grad_out.shape[0]
    env.policy_backward_device(pol, rows.data_ptr(), n, grad_out.data_ptr(), ptrs, index_ptr=0 if index is None else index.data_ptr(),
                               stream=stream_of(torch))
    torch.cuda.synchronize()
    out = []
    for (buf, v), s in zip(bufs, shapes):
        check_guards(buf, v.numel(), "a gradient array")
        assert not bool((v == SENTINEL).any()), "a gradient entry was not written"
        out.append(v.clone().view(*s))
    return out


def run_forward_rows(torch, env, pol, rows, n, index=None):
    buf, v = guarded(torch, n * pol.n_out)
    env.policy_forward_rows_device(pol, rows.data_ptr(), n, v.data_ptr(), index_ptr=0 if index is None else index.data_ptr(),
                                   stream=stream_of(torch))
    torch.cuda.synchronize()
    check_guards(buf, v.numel(), "out")
    return v.clone().view(n, pol.n_out)


def tanh_kernel_form(x):
    """the kernel's tanh in float32 NumPy: 1 - 2 / (exp(2 x) + 1)"""
    x = x.astype(np.float32)
    return (np.float32(1.0) - np.float32(2.0) / (np.exp(np.float32(2.0) * x) + np.float32(1.0))).astype(np.float32)


def backward_float32_numpy(mlp, x, g, tanh_form=None):
    """the definition of the header in plain float32 NumPy arrays"""
    form = tanh_form or TANH_FORM
    x, g = x.astype(np.float32), g.astype(np.float32)
    hs = [x]
    for W, b in mlp.layers[:-1]:
        pre = hs[-1] @ W.T + b
        if mlp.hidden_act == "relu":
            hs.append(np.maximum(pre, np.float32(0.0)))
        else:
            hs.append(np.tanh(pre) if form == "libm" else tanh_kernel_form(pre))
    grads = []
    for i in range(len(mlp.layers) - 1, -1, -1):
        grads[:0] = [g.T @ hs[i], g.sum(axis=0)]
        if i > 0:
            h = hs[i]
            g = (g @ mlp.layers[i][0]) * (np.float32(1.0) - h * h if mlp.hidden_act == "tanh" else (h > 0).astype(np.float32))
    assert all(a.dtype == np.float32 for a in grads)
    return grads


def names_of(mlp):
    return ["dW1", "db1", "dW2", "db2", "dW3", "db3"] if len(mlp.layers) == 3 else ["dW1", "db1", "dW3", "db3"]


def compare(mlp, x32, g32, got, label, tanh_form=None):
    """[(name, device error, float32 NumPy error, bound)] of the gradients `got` (NumPy float32) for observations x32 and upstream
    gradients g32; prints each figure"""
    ref = mlp.backward_reference(x32.astype(np.float64), g32.astype(np.float64))
    f32 = backward_float32_numpy(mlp, x32, g32, tanh_form)
    rows = []
    for name, d, f, r in zip(names_of(mlp), got, f32, ref):
        assert d.shape == r.shape and not np.isnan(d).any(), (label, name, "NaN: a reward / done column or an unwritten row got in")
        e_dev = float(np.abs(d.astype(np.float64) - r).max())
        e_np = float(np.abs(f.astype(np.float64) - r).max())
        floor = 4.0 * float(np.spacing(np.float32(np.abs(r).max())))
        bound = max(8.0 * e_np, floor)
        print(f"backward {label} {name}: device {e_dev:.3e}, float32 NumPy {e_np:.3e}, bound {bound:.3e}, "
              f"ratio {e_dev / max(e_np, floor / 8.0):.2f}")
        rows.append((name, e_dev, e_np, bound))
    return rows


def backward_case(shape, n_rows, seed=1, tanh_form=None, env=None):
    """one shape at one row count: (rows of compare(), relu rows dropped, rows drawn)"""
    import torch
    mlp = P().make_mlp(shape, seed=seed)
    own = env is None
    if own:
        env = P().fan_env(shape[0], 6 if shape[2] == 1 else shape[2], 64)
    try:
        pol = device_policy(env, mlp)
        rows, dropped, draw = make_rows(torch, mlp, n_rows, seed=2 + n_rows)
        g = make_grad_out(torch, n_rows, shape[2], seed=5 + n_rows)
        got = [t.cpu().numpy() for t in run_backward(torch, env, pol, mlp, rows, g)]
        env.destroy_policy(pol)
        x32, g32 = rows[:, : shape[0]].cpu().numpy(), g.cpu().numpy()
    finally:
        if own:
            env.close()
    return compare(mlp, x32, g32, got, f"{shape_id(shape)} rows {n_rows}", tanh_form), dropped, draw


# one critic (a single output) per hidden depth, and observations wider than the two dW1 tiles a wave keeps in registers (133
# columns: five tiles of 32 for two hidden tiles, the third of a wave is accumulated in LDS)
CRITICS = [(20, (64,), 1, "tanh", "none"), (36, (64, 64), 1, "tanh", "none")]
WIDE_OBS = (133, (33, 32), 6, "relu", "none")


ROW_COUNTS = (1, 33, 129)


def all_cases():
    return P().TILE_PAIRS + [P().WIDE] + CRITICS + [WIDE_OBS]


@pytest.mark.parametrize("shape", all_cases(), ids=shape_id)
def test_every_instantiation_against_float64(shape):
    """Each of the 20 (MT1, MT2) instantiations (TILE_PAIRS), the widest hidden layers (WIDE), a critic per hidden depth and the
    wide-observation path at 1 row (one lane), 33 and 129 rows (a group plus a lane).  The seeds' relu rows next to a kink were
    counted on the CPU: scripts/backward_error.py --relu-rows."""
    env = P().fan_env(shape[0], 6 if shape[2] == 1 else shape[2], 64)
    n_dropped = n_drawn = 0
    try:
        for n_rows in ROW_COUNTS:
            res, dropped, draw = backward_case(shape, n_rows, env=env)
            n_dropped, n_drawn = n_dropped + dropped, n_drawn + draw
            for name, e_dev, e_np, bound in res:
                assert e_dev <= bound, (shape, n_rows, name, e_dev, e_np, bound)
        # the gathered forward of the same instantiation (policy_rows_kernel<MT1, MT2>): the pre-activation output against float64
        import torch
        from gym_dockauv_amd.policy import MLPPolicy
        mlp = P().make_mlp(shape, seed=1)
        pol = device_policy(env, mlp)
        rows, _, _ = make_rows(torch, mlp, 129, seed=2)
        index = torch.arange(128, -1, -1, device="cuda")
        out = run_forward_rows(torch, env, pol, rows, 129, index=index).cpu().numpy().astype(np.float64)
        ref = MLPPolicy(mlp.layers, mlp.hidden_act, "none").forward_reference(rows[:, : shape[0]].cpu().numpy().astype(np.float64))
        err = float(np.abs(out - ref[::-1]).max())
        print(f"forward_rows {shape_id(shape)} rows 129 reversed: max |out - out_f64| = {err:.3e} (bound {P().FORWARD_BOUND:g})")
        assert err <= P().FORWARD_BOUND, (shape, err)
    finally:
        env.close()
    # relu: at most 2 % of the rows drawn for this shape (187 over the three row counts) had a unit next to its kink
    assert n_dropped <= 0.02 * n_drawn, (shape, n_dropped, n_drawn)


@pytest.mark.parametrize("shape", [(20, (64, 64), 6, "tanh", "none"), (20, (64, 64), 1, "tanh", "none")], ids=["actor", "critic"])
def test_more_rows_than_one_pass_of_the_grid(shape):
    """ROWS_BEYOND_ONE_PASS rows: groups 0 .. 255 walk one pass each, group 0 a second one with 33 live rows."""
    res, _, _ = backward_case(shape, ROWS_BEYOND_ONE_PASS)
    for name, e_dev, e_np, bound in res:
        assert e_dev <= bound, (name, e_dev, e_np, bound)


@pytest.mark.parametrize("shape", [(20, (64, 64), 6, "tanh", "none"), (36, (128,), 1, "relu", "none")], ids=shape_id)
def test_bitwise_properties(shape):
    """Two calls give the same bits; a random index of 1 000 out of 4 096 rows gives the bits of those rows copied densely in
    that order; an index with duplicates equals the dense batch with the rows repeated; the rows outside the index are all NaN."""
    import torch
    mlp = P().make_mlp(shape, seed=1)
    env = P().fan_env(shape[0], 6 if shape[2] == 1 else shape[2], 64)
    try:
        pol = device_policy(env, mlp)
        n_in = shape[0]
        rows, dropped, draw = make_rows(torch, mlp, 4096, seed=3)
        assert dropped <= 0.02 * draw, (dropped, draw)
        gen = torch.Generator(device="cuda")
        gen.manual_seed(9)
        index = torch.randperm(4096, device="cuda", generator=gen)[:1000].contiguous()
        assert index.dtype == torch.int64
        g = make_grad_out(torch, 1000, shape[2], seed=4)
        dense = shifted_rows(torch, rows[index].contiguous())
        poisoned = rows.clone()
        outside = torch.ones(4096, dtype=torch.bool, device="cuda")
        outside[index] = False
        poisoned[outside] = float("nan")
        poisoned = shifted_rows(torch, poisoned)
        a = run_backward(torch, env, pol, mlp, dense, g)
        b = run_backward(torch, env, pol, mlp, dense, g)
        c = run_backward(torch, env, pol, mlp, poisoned, g, index=index)
        for x, y, z in zip(a, b, c):
            assert not torch.isnan(x).any() and float(x.abs().max()) > 0
            assert torch.equal(bits(x), bits(y)), "two calls differ"
            assert torch.equal(bits(x), bits(z)), "the gather differs from the dense copy"
        dup = index.clone()
        dup[1::3] = dup[0]
        dup[500:520] = dup[777]
        d = run_backward(torch, env, pol, mlp, shifted_rows(torch, rows[dup].contiguous()), g)
        e = run_backward(torch, env, pol, mlp, rows, g, index=dup)
        for x, y in zip(d, e):
            assert torch.equal(bits(x), bits(y)), "an index with duplicates differs from the repeated rows"
        assert not torch.equal(bits(a[0]), bits(d[0]))
        # forward_rows through the same index: the bits of the dense rows
        f_dense = run_forward_rows(torch, env, pol, dense, 1000)
        f_index = run_forward_rows(torch, env, pol, poisoned, 1000, index=index)
        assert not torch.isnan(f_dense).any() and torch.equal(bits(f_dense), bits(f_index))
        # a zero upstream gradient: exact zeros
        for t in run_backward(torch, env, pol, mlp, dense, torch.zeros_like(g)):
            assert not bool(t.any())
    finally:
        env.close()


@pytest.mark.parametrize("n_in,n_out", [(20, 6), (36, 3)])
def test_forward_rows_is_policy_forward_and_value_forward_bitwise(n_in, n_out):
    """forward_rows of an actor (raw output) and of a critic against dockauv_policy_forward (deterministic) and
    dockauv_value_forward on the same rows, dense and through an index, bit for bit; for an actor with a tanh output it is the
    float64 pre-activation within FORWARD_BOUND."""
    import torch
    from gym_dockauv_amd.policy import MLPPolicy
    N = 1000 + 33
    env = P().fan_env(n_in, n_out, N)
    try:
        actor_mlp = P().make_mlp((n_in, (64, 64), n_out, "tanh", "none"), seed=1, log_std=np.full(n_out, -0.5))
        critic_mlp = P().make_mlp((n_in, (96,), 1, "relu", "none"), seed=2)
        squashed_mlp = P().make_mlp((n_in, (33, 65), n_out, "tanh", "tanh"), seed=3)
        actor, critic, squashed = env.make_policy(actor_mlp, seed=5), env.make_value(critic_mlp), env.make_policy(squashed_mlp)
        rows = shifted_rows(torch, P().nan_rows(torch, N, n_in, seed=2))
        acts = torch.full((N, n_out), SENTINEL, device="cuda")
        env.policy_forward_device(actor, rows.data_ptr(), acts.data_ptr(), t=3, stochastic=False, stream=stream_of(torch))
        vals = torch.full((N,), SENTINEL, device="cuda")
        env.value_forward_device(critic, rows.data_ptr(), N, vals.data_ptr(), stream=stream_of(torch))
        torch.cuda.synchronize()
        a = run_forward_rows(torch, env, actor, rows, N)
        v = run_forward_rows(torch, env, critic, rows, N)
        assert not torch.isnan(a).any() and not torch.isnan(v).any()
        assert torch.equal(bits(a), bits(acts)) and torch.equal(bits(v[:, 0]), bits(vals))
        gen = torch.Generator(device="cuda")
        gen.manual_seed(1)
        index = torch.randint(0, N, (517,), device="cuda", generator=gen)
        assert torch.equal(bits(run_forward_rows(torch, env, actor, rows, 517, index=index)), bits(acts[index]))
        assert torch.equal(bits(run_forward_rows(torch, env, critic, rows, 517, index=index)[:, 0]), bits(vals[index]))
        # a single row
        assert torch.equal(bits(run_forward_rows(torch, env, actor, rows, 1, index=index[5:6].contiguous())), bits(acts[index[5:6]]))
        # tanh output: forward_rows stops before it
        pre = run_forward_rows(torch, env, squashed, rows, N).cpu().numpy().astype(np.float64)
        raw = MLPPolicy(squashed_mlp.layers, "tanh", "none")
        err = float(np.abs(pre - raw.forward_reference(rows[:, :n_in].cpu().numpy().astype(np.float64))).max())
        print(f"forward_rows {n_in}-33-65-{n_out} tanh output: max |out - pre-activation_f64| = {err:.3e} (bound {P().FORWARD_BOUND:g})")
        assert err <= P().FORWARD_BOUND
        assert float(np.abs(pre).max()) > 0.05
    finally:
        env.close()


def ppo_loss(torch, out, value, actions, logp_old, adv, ret, log_std, clip=0.2, vf_coef=0.5, ent_coef=0.01):
    """SB3's PPO loss on one minibatch: clipped surrogate, value loss, entropy bonus"""
    dist = torch.distributions.Normal(out, log_std.exp())
    ratio = (dist.log_prob(actions).sum(-1) - logp_old).exp()
    surrogate = -torch.min(ratio * adv, ratio.clamp(1 - clip, 1 + clip) * adv).mean()
    return surrogate + vf_coef * ((ret - value) ** 2).mean() - ent_coef * dist.entropy().sum(-1).mean(), ratio


def test_mlp_apply_ppo_loss_against_float64_autograd():
    """One minibatch of a real collect (config 3, 256 envs, K = 8): the PPO loss with the actor and the critic through mlp_apply,
    then each parameter's .grad against the .grad of the same loss on nn.Sequential in float64 on the CPU; the learner's
    parameters are the collecting ones plus a perturbation, so that the ratios spread and some are clipped.  Rows whose float64
    ratio lies within 1e-4 of a clip edge are left out of the minibatch (the edge may fall on the other side in float32).  Bound
    as above, e32 from the same loss on nn.Sequential in float32 on the CPU."""
    import torch
    import bench
    from gym_dockauv_amd.envs.torch_env import TorchDocking3d
    N, K, B = 256, 8, 512
    wl = bench.workload(3, N)
    env = TorchDocking3d(copy.deepcopy(wl["cfg"]), num_envs=N, scenario=wl["scenario"], device_seed=9)
    try:
        env.batch._gen = np.random.default_rng(5)
        env.reset()
        actor_mlp = P().make_mlp((20, (64, 64), 6, "tanh", "none"), seed=6, log_std=np.full(6, -0.5))
        critic_mlp = P().make_mlp((20, (64, 64), 1, "tanh", "none"), seed=7)
        actor, critic = env.make_policy(actor_mlp, seed=3), env.make_value(critic_mlp)
        c = env.collect(actor, critic, K, gamma=0.99, gae_lambda=0.95)
        torch.cuda.synchronize()
        assert not torch.isnan(c.obs).any()

        def seq(mlp, dtype, device):
            mods = []
            for i, (W, b) in enumerate(mlp.layers):
                lin = torch.nn.Linear(W.shape[1], W.shape[0])
                with torch.no_grad():
                    lin.weight.copy_(torch.from_numpy(W))
                    lin.bias.copy_(torch.from_numpy(b))
                mods += [lin] + ([torch.nn.Tanh()] if i < len(mlp.layers) - 1 else [])
            return torch.nn.Sequential(*mods).to(dtype=dtype, device=device)

        rng = np.random.default_rng(8)
        from gym_dockauv_amd.policy import MLPPolicy
        perturb = lambda m: MLPPolicy([(W + rng.normal(0, 0.02, W.shape), b + rng.normal(0, 0.02, b.shape)) for W, b in m.layers],
                                      m.hidden_act, m.out_act)
        learn_a, learn_c = perturb(actor_mlp), perturb(critic_mlp)
        nets = {kind: (seq(learn_a, dt, dev), seq(learn_c, dt, dev))
                for kind, dt, dev in (("gpu", torch.float32, "cuda"), ("f32", torch.float32, "cpu"), ("f64", torch.float64, "cpu"))}
        log_std0 = np.full(6, -0.45, dtype=np.float32)

        obs = c.obs[:K]                                   # [K, N, 20]: a view of the packed buffer
        flat = lambda t: t.reshape(K * N, *t.shape[2:])
        data = dict(obs=flat(obs), actions=flat(c.actions), logp=flat(c.log_prob), adv=flat(c.advantages), ret=flat(c.returns))
        adv = data["adv"]
        data["adv"] = (adv - adv.mean()) / (adv.std() + 1e-8)

        def cpu_loss(kind, index):
            dt = torch.float32 if kind == "f32" else torch.float64
            a, cr = nets[kind]
            d = {k: v[index].cpu().to(dt) for k, v in data.items()}
            ls = torch.tensor(log_std0, dtype=dt, requires_grad=True)
            loss, ratio = ppo_loss(torch, a(d["obs"]), cr(d["obs"])[:, 0], d["actions"], d["logp"], d["adv"], d["ret"], ls)
            return loss, ratio, ls

        gen = torch.Generator(device="cuda")
        gen.manual_seed(2)
        index = torch.randperm(K * N, device="cuda", generator=gen)[: B + 64]
        with torch.no_grad():
            _, ratio64, _ = cpu_loss("f64", index)
        near = ((ratio64 - 0.8).abs() < 1e-4) | ((ratio64 - 1.2).abs() < 1e-4)
        assert int(near.sum()) <= 8
        index = index[(~near).cuda()][:B].contiguous()
        assert index.numel() == B
        clipped = float(((ratio64 < 0.8) | (ratio64 > 1.2)).double().mean())
        assert 0.02 < clipped < 0.98, f"share of clipped rows {clipped}: the case must exercise both branches"

        grads = {}
        for kind in ("f32", "f64"):
            loss, _, ls = cpu_loss(kind, index)
            loss.backward()
            grads[kind] = [p.grad.numpy().astype(np.float64) for net in nets[kind] for p in net.parameters()] + [ls.grad.numpy().astype(np.float64)]

        a_net, c_net = nets["gpu"]
        log_std = torch.tensor(log_std0, device="cuda", requires_grad=True)
        env.load_policy(actor, a_net, log_std=log_std)
        index_in, obs_in = index.clone().requires_grad_(False), obs
        out = env.mlp_apply(actor, list(a_net.parameters()), obs_in, index_in)
        value = env.mlp_apply(critic, list(c_net.parameters()), obs_in, index_in)[:, 0]
        assert tuple(out.shape) == (B, 6) and out.requires_grad and value.requires_grad
        loss, _ = ppo_loss(torch, out, value, data["actions"][index], data["logp"][index], data["adv"][index], data["ret"][index], log_std)
        loss.backward()
        torch.cuda.synchronize()
        assert obs_in.grad is None and index_in.grad is None and not obs_in.requires_grad
        got = [p.grad.cpu().numpy().astype(np.float64) for net in (a_net, c_net) for p in net.parameters()] + [log_std.grad.cpu().numpy().astype(np.float64)]
        names = [f"{who}.{n}" for who in ("actor", "critic") for n in ("W1", "b1", "W2", "b2", "W3", "b3")] + ["log_std"]
        for name, d, f, r in zip(names, got, grads["f32"], grads["f64"]):
            e_dev, e_np = float(np.abs(d - r).max()), float(np.abs(f - r).max())
            bound = max(8.0 * e_np, 4.0 * float(np.spacing(np.float32(np.abs(r).max()))))
            print(f"mlp_apply PPO loss {name}: device {e_dev:.3e}, float32 torch on the CPU {e_np:.3e}, bound {bound:.3e}")
            assert e_dev <= bound, (name, e_dev, e_np, bound)
        # the collecting weights are the learner's now: the next collect runs with them
        env.collect(actor, critic, K, gamma=0.99, gae_lambda=0.95)
        torch.cuda.synchronize()
    finally:
        env.close()


def test_refusals_on_a_live_handle():
    import torch
    from gym_dockauv_amd import _capi
    lib = _capi.load_library()
    env, other = P().fan_env(20, 6, 64), P().fan_env(20, 6, 64)
    try:
        mlp = P().make_mlp((20, (64, 64), 6, "tanh", "none"), seed=1)
        one = P().make_mlp((20, (64,), 6, "tanh", "none"), seed=1)
        pol, pol_one, foreign = env.make_policy(mlp), env.make_policy(one), other.make_policy(mlp)
        rows = P().nan_rows(torch, 64, 20, seed=2)
        g = make_grad_out(torch, 64, 6, seed=1)
        outs = [torch.zeros(n, device="cuda") for n in (64 * 20, 64, 64 * 64, 64, 6 * 64, 6)]

        def call(p, n_rows=64, struct_size=None, drop=()):
            gr = _capi.PolicyGrads()
            gr.struct_size = C.sizeof(_capi.PolicyGrads) if struct_size is None else struct_size
            for f, t in zip(("dW1", "db1", "dW2", "db2", "dW3", "db3"), outs):
                setattr(gr, f, None if f in drop else t.data_ptr())
            rc = lib.dockauv_policy_backward(env._handle, p.ptr, rows.data_ptr(), None, n_rows, g.data_ptr(), C.byref(gr), None)
            return rc, lib.dockauv_last_error(env._handle)

        rc, msg = call(pol, struct_size=24)
        assert rc == -1 and b"struct_size" in msg, (rc, msg)
        rc, msg = call(pol, drop=("dW2",))
        assert rc == -1 and b"dW2" in msg, (rc, msg)
        rc, msg = call(pol, drop=("db2",))
        assert rc == -1 and b"dW2/db2" in msg, (rc, msg)
        rc, msg = call(pol_one, drop=("dW2", "db2"))          # one hidden layer: taken
        assert rc == 0, (rc, msg)
        rc, msg = call(pol, n_rows=0)
        assert rc == -1 and b"n_rows" in msg, (rc, msg)
        rc, msg = call(foreign)
        assert rc == -1 and b"another handle" in msg, (rc, msg)
        out = torch.zeros((64, 6), device="cuda")
        rc = lib.dockauv_policy_forward_rows(env._handle, foreign.ptr, rows.data_ptr(), None, 64, out.data_ptr(), None)
        assert rc == -1 and b"another handle" in lib.dockauv_last_error(env._handle)
        rc = lib.dockauv_policy_forward_rows(env._handle, pol.ptr, rows.data_ptr(), None, 0, out.data_ptr(), None)
        assert rc == -1 and b"n_rows" in lib.dockauv_last_error(env._handle)
        rc, msg = call(pol)                                   # ... and the good call goes through
        assert rc == 0, (rc, msg)
        env.synchronize()
    finally:
        env.close()
        other.close()
    # the widest shape dockauv_policy_create accepts: the forward's packed weights fit the LDS, the backward's images do not
    wide = P().fan_env(133, 6, 64)
    try:
        mlp = P().make_mlp(P().WIDEST, seed=1)
        pol = wide.make_policy(mlp)
        rows = P().nan_rows(torch, 64, 133, seed=2)
        g = make_grad_out(torch, 64, 6, seed=1)
        with pytest.raises(_capi.DockAUVError, match="LDS"):
            run_backward(torch, wide, pol, mlp, rows, g)
        assert not torch.isnan(run_forward_rows(torch, wide, pol, rows, 64)).any()     # forward_rows takes it
    finally:
        wide.close()
