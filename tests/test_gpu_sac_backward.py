"""The networks' share of SAC's gradient half on a real MI355X (include/dockauv.h: dockauv_sac_actor_forward_rows,
dockauv_sac_actor_backward, dockauv_q_backward; TorchDocking3d.sac_actor_heads / sac_actor_backward / q_backward / sac_actor_apply /
q_apply): every sac_actor_heads_kernel, sac_actor_backward_kernel, q_backward_kernel and q_backward_dx_kernel <MT1, MT2> at 33 rows
against float64; Q parameter gradients and grad_actions at 1, 33 and 129 rows on four (n_obs, n_u) and beyond one pass of the
bounded grid; the bitwise properties (two calls, the replay ring's records through an index against the dense rows, duplicates,
NaN records outside the index); the form without parameter gradients (the bits of the other form, no workspace); the heads bit
for bit against the two plain twins' dockauv_policy_forward_rows; one SAC step end to end through sac_actor_apply / q_apply against
the same graph in float64 on the CPU; refusals on a live handle.  The helpers are those of tests/test_gpu_backward.py: guarded
outputs between sentinels, rows 4 bytes off 8-byte alignment with NaN behind the observation (and action) columns, draw_rows'
ReLU margin, backward_float32_numpy as the float32 restatement.  Every env is closed in `finally`.

Bound, per output tensor (the project's, tests/test_gpu_backward.py): max |g - g64| <= max(8 x e32, 4 ulp of max |g64|), e32 the
error of a float32 restatement of the same case against float64.  The measured ratios: profiles/sac/backward_error.txt (written by
scripts/sac_backward_error.py from the helpers of this file; the tests print them as well).
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FORWARD_BOUND = 1e-5          # tests/test_gpu_policy.py: the project's float32 bar
MIN_GAP = 1e-4                # |q1 - q2| below this may order the other way in float32 (ten times FORWARD_BOUND)
ROW_COUNTS = (1, 33, 129)
# one shape per (tiles of hidden layer 1, tiles of hidden layer 2): the 20 instantiations of each of the four kernels
ALL_TILES = [(h1, h2) if h2 else (h1,) for h1 in (17, 33, 96, 128) for h2 in (0, 32, 63, 65, 128)]
# (n_obs, n_u, hidden, hidden_act) of the Q cases: 25 is odd, so one layer-1 k step takes a column from each source
Q_CASES = [(20, 6, (64, 64), "relu"), (36, 3, (128, 128), "relu"), (36, 8, (128, 128), "relu"), (25, 6, (33, 65), "tanh")]
NET_SEED, ROW_SEED = 3, 7     # the relu rows next to a kink these seeds drop were counted on the CPU, well inside draw_rows' cap


def B():
    """the helpers of the backward tests: guarded, check_guards, shifted_rows, draw_rows, make_rows, backward_float32_numpy, bits"""
    from tests import test_gpu_backward
    return test_gpu_backward


def P():
    from tests import test_gpu_policy
    return test_gpu_policy


def stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def q_mlp(n_obs, n_u, hidden, act, seed=NET_SEED):
    return P().make_mlp((n_obs + n_u, hidden, 1, act, "none"), seed=seed)


def sac_mlp(n_obs, n_u, hidden, act, seed=NET_SEED):
    """a squashed-Gaussian actor whose hidden layers and mu head are make_mlp's (so draw_rows' drops are that network's), with a
    log_std head of the same initialisation from another stream"""
    from gym_dockauv_amd.policy import SquashedGaussianMLP
    base = P().make_mlp((n_obs, hidden, n_u, act, "none"), seed=seed)
    rng = np.random.default_rng(1000 + seed)
    n_last, b = hidden[-1], 1.0 / np.sqrt(hidden[-1])
    return SquashedGaussianMLP(base.layers[:-1], base.layers[-1], (rng.uniform(-b, b, (n_u, n_last)), rng.uniform(-b, b, n_u)), act)


def input_grad_float32_numpy(mlp, x, g):
    """dL/dx of backward_float32_numpy's pass in plain float32 NumPy arrays"""
    x, g = x.astype(np.float32), g.astype(np.float32)
    hs = [x]
    for W, b in mlp.layers[:-1]:
        pre = hs[-1] @ W.T + b
        hs.append(np.maximum(pre, np.float32(0.0)) if mlp.hidden_act == "relu" else np.tanh(pre))
    for i in range(len(mlp.layers) - 1, -1, -1):
        g = g @ mlp.layers[i][0]
        if i > 0:
            h = hs[i]
            g = g * (np.float32(1.0) - h * h if mlp.hidden_act == "tanh" else (h > 0).astype(np.float32))
    assert g.dtype == np.float32
    return g


def compare_named(names, got, f32, ref, label):
    """[(name, device error, float32 error, bound)] per output tensor; prints each figure"""
    rows = []
    for name, d, f, r in zip(names, got, f32, ref):
        d, f, r = np.asarray(d, dtype=np.float64), np.asarray(f, dtype=np.float64), np.asarray(r, dtype=np.float64)
        assert d.shape == r.shape and not np.isnan(d).any(), (label, name, "NaN: a column behind the row or an unwritten entry got in")
        e_dev, e_np = float(np.abs(d - r).max()), float(np.abs(f - r).max())
        floor = 4.0 * float(np.spacing(np.float32(np.abs(r).max())))
        bound = max(8.0 * e_np, floor)
        print(f"sac backward {label} {name}: device {e_dev:.3e}, float32 {e_np:.3e}, bound {bound:.3e}, "
              f"ratio {e_dev / max(e_np, floor / 8.0):.2f}")
        rows.append((name, e_dev, e_np, bound))
    return rows


def assert_within(rows, label):
    for name, e_dev, e_np, bound in rows:
        assert e_dev <= bound, (label, name, e_dev, e_np, bound)


def layer_names(n_hidden, tail):
    return ["dW1", "db1", "dW2", "db2"][: 2 * n_hidden] + tail


# ------------------------------------------------------------------------------------------ guarded calls on device pointers
def run_heads(torch, env, actor, rows, n, stride, index=None):
    buf, v = B().guarded(torch, n * 2 * env.n_u)
    env.sac_actor_forward_rows_device(actor, rows.data_ptr(), n, v.data_ptr(), row_stride=stride,
                                      index_ptr=0 if index is None else index.data_ptr(), stream=stream())
    torch.cuda.synchronize()
    B().check_guards(buf, v.numel(), "out")
    assert not bool((v == B().SENTINEL).any()), "an output entry was not written"
    return v.clone().view(n, 2 * env.n_u)


def run_actor_backward(torch, env, actor, mlp, rows, grad_out, stride, index=None):
    """dockauv_sac_actor_backward into guarded buffers: (dW1, db1[, dW2, db2], dW_mu, db_mu, dW_ls, db_ls) as device tensors"""
    shapes = [s for W, b in mlp.layers for s in (W.shape, b.shape)] + [mlp.mu[0].shape, mlp.mu[1].shape] * 2
    bufs = [B().guarded(torch, int(np.prod(s))) for s in shapes]
    ptrs = [v.data_ptr() for _, v in bufs]
    if len(ptrs) == 6:
        ptrs[2:2] = [0, 0]
    env.sac_actor_backward_device(actor, rows.data_ptr(), grad_out.shape[0], grad_out.data_ptr(), ptrs, row_stride=stride,
                                  index_ptr=0 if index is None else index.data_ptr(), stream=stream())
    torch.cuda.synchronize()
    out = []
    for (buf, v), s in zip(bufs, shapes):
        B().check_guards(buf, v.numel(), "a gradient array")
        assert not bool((v == B().SENTINEL).any()), "a gradient entry was not written"
        out.append(v.clone().view(*s))
    return out


def run_q_backward(torch, env, q, mlp, obs_ptr, act_ptr, grad_q, obs_stride, act_stride, params=True, dx=True, index=None):
    """dockauv_q_backward into guarded buffers: ([dW1, db1[, dW2, db2], dW3, db3] or None, grad_actions [n, n_u] or None)"""
    n = grad_q.shape[0]
    shapes = [s for W, b in mlp.layers for s in (W.shape, b.shape)]
    bufs = [B().guarded(torch, int(np.prod(s))) for s in shapes] if params else None
    ptrs = None
    if params:
        ptrs = [v.data_ptr() for _, v in bufs]
        if len(ptrs) == 4:
            ptrs[2:2] = [0, 0]
    da_buf, da = B().guarded(torch, n * env.n_u) if dx else (None, None)
    env.q_backward_device(q, obs_ptr, act_ptr, n, grad_q.data_ptr(), grad_ptrs=ptrs, grad_actions_ptr=da.data_ptr() if dx else 0,
                          obs_stride=obs_stride, act_stride=act_stride, index_ptr=0 if index is None else index.data_ptr(), stream=stream())
    torch.cuda.synchronize()
    grads = None
    if params:
        grads = []
        for (buf, v), s in zip(bufs, shapes):
            B().check_guards(buf, v.numel(), "a gradient array")
            assert not bool((v == B().SENTINEL).any()), "a gradient entry was not written"
            grads.append(v.clone().view(*s))
    if dx:
        B().check_guards(da_buf, da.numel(), "grad_actions")
        assert not bool((da == B().SENTINEL).any()), "an entry of grad_actions was not written"
        da = da.clone().view(n, env.n_u)
    return grads, da


# ------------------------------------------------------------------------------------------ cases against float64
def q_case(env, n_obs, n_u, hidden, act, n_rows, label=None):
    """dockauv_q_backward (parameters and grad_actions in one call) of one shape at one row count on records [obs | action | NaN NaN]:
    rows of compare_named()"""
    import torch
    mlp = q_mlp(n_obs, n_u, hidden, act)
    q = env.make_q(mlp)
    n_in = n_obs + n_u
    rows, _, _ = B().make_rows(torch, mlp, n_rows, seed=ROW_SEED)
    g = B().make_grad_out(torch, n_rows, 1, seed=5 + n_rows)
    grads, da = run_q_backward(torch, env, q, mlp, rows.data_ptr(), rows.data_ptr() + 4 * n_obs, g.view(-1), n_in + 2, n_in + 2)
    env.destroy_policy(q)
    x32, g32 = rows[:, :n_in].cpu().numpy(), g.cpu().numpy()
    x64, g64 = x32.astype(np.float64), g32.astype(np.float64)
    ref = list(mlp.backward_reference(x64, g64)) + [mlp.backward_input_reference(x64, g64)[:, n_obs:]]
    f32 = B().backward_float32_numpy(mlp, x32, g32) + [input_grad_float32_numpy(mlp, x32, g32)[:, n_obs:]]
    got = [t.cpu().numpy() for t in grads] + [da.cpu().numpy()]
    label = label or f"Q {n_obs}+{n_u}-{'-'.join(map(str, hidden))}-1 {act} rows {n_rows}"
    return compare_named(layer_names(len(hidden), ["dW3", "db3", "grad_actions"]), got, f32, ref, label)


def actor_case(env, n_obs, n_u, hidden, act, n_rows, label=None):
    """dockauv_sac_actor_backward of one shape at one row count on packed rows: rows of compare_named()"""
    import torch
    mlp = sac_mlp(n_obs, n_u, hidden, act)
    actor = env.make_sac_actor(mlp)
    both = mlp._both_heads()
    rows, _, _ = B().make_rows(torch, both, n_rows, seed=ROW_SEED)
    g = B().make_grad_out(torch, n_rows, 2 * n_u, seed=5 + n_rows)
    got = [t.cpu().numpy() for t in run_actor_backward(torch, env, actor, mlp, rows, g, n_obs + 2)]
    env.destroy_policy(actor)
    x32, g32 = rows[:, :n_obs].cpu().numpy(), g.cpu().numpy()
    ref = mlp.backward_reference(x32.astype(np.float64), g32.astype(np.float64))
    *hid, dW, db = B().backward_float32_numpy(both, x32, g32)
    f32 = hid + [dW[:n_u], db[:n_u], dW[n_u:], db[n_u:]]
    label = label or f"actor {n_obs}-{'-'.join(map(str, hidden))}-{n_u} {act} rows {n_rows}"
    return compare_named(layer_names(len(hidden), ["dW_mu", "db_mu", "dW_ls", "db_ls"]), got, f32, ref, label)


@pytest.mark.parametrize("hidden", ALL_TILES, ids=lambda h: "-".join(map(str, h)))
def test_every_instantiation_at_33_rows(hidden):
    """sac_actor_heads_kernel, sac_actor_backward_kernel, q_backward_kernel and q_backward_dx_kernel of every (MT1, MT2) on 33 rows
    (a tile and a lane) of the (20, 6) env, tanh and relu, against float64; the form without parameter gradients gives the bits
    of the other form's grad_actions, and the call without grad_actions the bits of its parameter gradients."""
    import torch
    n, n_obs, n_u = 33, 20, 6
    env = P().fan_env(n_obs, n_u, 64)
    try:
        for act in ("tanh", "relu"):
            assert_within(actor_case(env, n_obs, n_u, hidden, act, n), (hidden, act))
            assert_within(q_case(env, n_obs, n_u, hidden, act, n), (hidden, act))
            # the heads of the same instantiation against float64, through a reversed index
            mlp = sac_mlp(n_obs, n_u, hidden, act)
            actor = env.make_sac_actor(mlp)
            rows, _, _ = B().make_rows(torch, mlp._both_heads(), n, seed=ROW_SEED)
            index = torch.arange(n - 1, -1, -1, device="cuda")
            out = run_heads(torch, env, actor, rows, n, n_obs + 2, index=index).cpu().numpy().astype(np.float64)
            err = float(np.abs(out - mlp.heads_reference(rows[:, :n_obs].cpu().numpy().astype(np.float64))[::-1]).max())
            print(f"sac heads 20-{'-'.join(map(str, hidden))}-6 {act} rows 33 reversed: max |out - out_f64| = {err:.3e} (bound {FORWARD_BOUND:g})")
            assert err <= FORWARD_BOUND, (hidden, act, err)
            # the three forms of the Q backward on the same rows
            qm = q_mlp(n_obs, n_u, hidden, act)
            q = env.make_q(qm)
            qrows, _, _ = B().make_rows(torch, qm, n, seed=ROW_SEED)
            g = B().make_grad_out(torch, n, 1, seed=9).view(-1)
            args = (torch, env, q, qm, qrows.data_ptr(), qrows.data_ptr() + 4 * n_obs, g, n_obs + n_u + 2, n_obs + n_u + 2)
            both_p, both_a = run_q_backward(*args)
            _, only_a = run_q_backward(*args, params=False)
            only_p, _ = run_q_backward(*args, dx=False)
            assert torch.equal(B().bits(only_a), B().bits(both_a)), "grad_actions without parameters differs"
            for x, y in zip(only_p, both_p):
                assert torch.equal(B().bits(x), B().bits(y)), "parameter gradients without grad_actions differ"
    finally:
        env.close()


@pytest.mark.parametrize("case", Q_CASES, ids=lambda c: f"{c[0]}+{c[1]}-{'-'.join(map(str, c[2]))}-{c[3]}")
def test_q_gradients_against_float64(case):
    """Parameter gradients and grad_actions at 1 row (a lane), 33 and 129 rows (a group and a lane) on four (n_obs, n_u); the odd
    n_obs puts the two sources into one k step; 36 + 8 with 128-128 is the widest Q critic of the shipped configurations."""
    n_obs, n_u, hidden, act = case
    env = P().fan_env(n_obs, n_u, 64)
    try:
        for n_rows in ROW_COUNTS:
            assert_within(q_case(env, n_obs, n_u, hidden, act, n_rows), (case, n_rows))
    finally:
        env.close()


def test_q_more_rows_than_one_pass_of_the_grid():
    """256 * 64 + 33 rows at 64-64: groups 0 .. 255 walk one pass each, group 0 a second one with a full row tile and one lane."""
    env = P().fan_env(20, 6, 64)
    try:
        assert_within(q_case(env, 20, 6, (64, 64), "relu", B().ROWS_BEYOND_ONE_PASS), "beyond one pass")
    finally:
        env.close()


@pytest.mark.parametrize("n_rows", ROW_COUNTS + (256 * 64 + 33,))
def test_actor_backward_against_float64(n_rows):
    """20-128-128-6 relu (one row tile a pass: 16 417 rows are 514 passes on 256 groups) at 1, 33, 129 and 256 * 64 + 33 rows."""
    env = P().fan_env(20, 6, 64)
    try:
        assert_within(actor_case(env, 20, 6, (128, 128), "relu", n_rows), n_rows)
    finally:
        env.close()


def test_actor_backward_splits_the_two_heads():
    """grad_out zero in the log-std columns: dW_ls and db_ls are exact zeros and the other arrays have the bits of the call
    repeated; the same with the roles swapped; and each head's arrays are those of a call that carries both (the k order of a
    hidden unit's delta takes the two heads' rows in turn, so the hidden layers are compared against float64 only)."""
    import torch
    n, n_obs, n_u, hidden = 129, 20, 6, (64, 64)
    env = P().fan_env(n_obs, n_u, 64)
    try:
        mlp = sac_mlp(n_obs, n_u, hidden, "tanh")
        actor = env.make_sac_actor(mlp)
        rows, _, _ = B().make_rows(torch, mlp._both_heads(), n, seed=ROW_SEED)
        g = B().make_grad_out(torch, n, 2 * n_u, seed=4)
        full = run_actor_backward(torch, env, actor, mlp, rows, g, n_obs + 2)
        for head, (zero_from, keep_from) in enumerate(((n_u, 0), (0, n_u))):
            gz = g.clone()
            gz[:, zero_from: zero_from + n_u] = 0.0
            a = run_actor_backward(torch, env, actor, mlp, rows, gz, n_obs + 2)
            b = run_actor_backward(torch, env, actor, mlp, rows, gz, n_obs + 2)
            for x, y in zip(a, b):
                assert torch.equal(B().bits(x), B().bits(y)), "two calls differ"
            dead, live = (a[6:8], a[4:6]) if head == 0 else (a[4:6], a[6:8])
            assert not bool(dead[0].any()) and not bool(dead[1].any()), "the head without an upstream gradient is not exactly zero"
            want = full[4:6] if head == 0 else full[6:8]
            assert float(live[0].abs().max()) > 0
            for x, y in zip(live, want):
                assert torch.equal(B().bits(x), B().bits(y)), "a head's own gradients depend on the other head's columns"
            # the hidden layers of the one-head call against float64 with the other head's columns zero
            x32, g32 = rows[:, :n_obs].cpu().numpy(), gz.cpu().numpy()
            ref = mlp.backward_reference(x32.astype(np.float64), g32.astype(np.float64))
            *hid, dW, db = B().backward_float32_numpy(mlp._both_heads(), x32, g32)
            assert_within(compare_named(layer_names(2, []), [t.cpu().numpy() for t in a[:4]], hid, ref[:4], f"actor, head {head} alone"), head)
    finally:
        env.close()


@pytest.mark.parametrize("n_obs,n_u,hidden", [(36, 3, (17,)), (20, 6, (64, 64)), (36, 8, (128, 128))])
def test_heads_are_the_two_plain_twins_bit_for_bit(n_obs, n_u, hidden):
    """mu is dockauv_policy_forward_rows of the plain twin (W3 = W_mu), the raw log_std that of a plain policy with W3 = W_ls,
    b3 = b_ls: dense and through an index with duplicates, the rows' reward / done columns NaN."""
    import torch
    from gym_dockauv_amd.policy import MLPPolicy
    N = 517
    env = P().fan_env(n_obs, n_u, 64)
    try:
        mlp = sac_mlp(n_obs, n_u, hidden, "relu")
        actor = env.make_sac_actor(mlp)
        twin_mu = env.make_policy(mlp.plain_twin("none"))
        twin_ls = env.make_policy(MLPPolicy(mlp.layers + [mlp.log_std_head], mlp.hidden_act, "none"))
        rows = B().shifted_rows(torch, P().nan_rows(torch, N, n_obs, seed=2))
        heads = run_heads(torch, env, actor, rows, N, n_obs + 2)
        assert not torch.isnan(heads).any()
        mu, ls = B().run_forward_rows(torch, env, twin_mu, rows, N), B().run_forward_rows(torch, env, twin_ls, rows, N)
        assert torch.equal(B().bits(heads[:, :n_u]), B().bits(mu)) and torch.equal(B().bits(heads[:, n_u:]), B().bits(ls))
        gen = torch.Generator(device="cuda")
        gen.manual_seed(1)
        index = torch.randint(0, N, (131,), device="cuda", generator=gen)
        hi = run_heads(torch, env, actor, rows, 131, n_obs + 2, index=index)
        assert torch.equal(B().bits(hi), B().bits(heads[index]))
        assert torch.equal(B().bits(run_heads(torch, env, actor, rows, 1, n_obs + 2, index=index[7:8].contiguous())), B().bits(heads[index[7:8]]))
        assert float(heads[:, n_u:].abs().max()) > 0.05
    finally:
        env.close()


def ring_of(torch, n_obs, n_u, obs, act, slots, gen):
    """records of the replay ring's shape [obs | next_obs | action | NaN ..] in a shuffled order, NaN everywhere else:
    (ring [slots, R], the int64 index of the n rows)"""
    n = obs.shape[0]
    R = 2 * n_obs + n_u + 5
    perm = torch.randperm(slots, device="cuda", generator=gen)[:n].contiguous()
    ring = torch.full((slots, R), float("nan"), device="cuda")
    ring[perm, :n_obs] = obs
    ring[perm, 2 * n_obs: 2 * n_obs + n_u] = act
    return ring, perm


def test_gather_from_the_ring_is_the_dense_call_bit_for_bit():
    """The same rows scattered into records of the ring's stride and read through an index give the bits of the dense call (Q:
    parameters and grad_actions; the actor: heads and gradients); a duplicated index entry counts twice; the records outside the
    index are all NaN; two identical calls give identical bits."""
    import torch
    n, n_obs, n_u, hidden = 1000, 20, 6, (64, 64)
    env = P().fan_env(n_obs, n_u, 64)
    try:
        qm, am = q_mlp(n_obs, n_u, hidden, "relu"), sac_mlp(n_obs, n_u, hidden, "relu")
        q, actor = env.make_q(qm), env.make_sac_actor(am)
        gen = torch.Generator(device="cuda")
        gen.manual_seed(9)
        obs = (torch.rand((n, n_obs), device="cuda", generator=gen) * 2 - 1).contiguous()
        act = (torch.rand((n, n_u), device="cuda", generator=gen) * 2 - 1).contiguous()
        gq = B().make_grad_out(torch, n, 1, seed=4).view(-1)
        ga = B().make_grad_out(torch, n, 2 * n_u, seed=5)
        ring, index = ring_of(torch, n_obs, n_u, obs, act, 4096, gen)
        R = ring.shape[1]
        dup = torch.arange(n, device="cuda")
        dup[1::3] = 0
        dup[500:520] = 777

        def q_dense(o, a):
            return run_q_backward(torch, env, q, qm, o.data_ptr(), a.data_ptr(), gq, n_obs, n_u)

        def q_ring(ix):
            return run_q_backward(torch, env, q, qm, ring.data_ptr(), ring.data_ptr() + 8 * n_obs, gq, R, R, index=ix)

        def same(x, y, what):
            xs, ys = (list(x[0]) + [x[1]], list(y[0]) + [y[1]]) if isinstance(x, tuple) else (list(x), list(y))
            for s, t in zip(xs, ys):
                assert not torch.isnan(s).any() and float(s.abs().max()) > 0
                assert torch.equal(B().bits(s), B().bits(t)), what

        d = q_dense(obs, act)
        same(d, q_dense(obs, act), "two Q calls differ")
        same(d, q_ring(index), "the Q gather differs from the dense rows")
        d2 = q_dense(obs[dup].contiguous(), act[dup].contiguous())
        same(d2, q_ring(index[dup].contiguous()), "a Q index with duplicates differs from the repeated rows")
        assert not torch.equal(B().bits(d[0][0]), B().bits(d2[0][0]))

        a_dense = lambda o: run_actor_backward(torch, env, actor, am, o, ga, n_obs)
        a_ring = lambda ix: run_actor_backward(torch, env, actor, am, ring, ga, R, index=ix)
        e = a_dense(obs)
        same(e, a_dense(obs), "two actor calls differ")
        same(e, a_ring(index), "the actor gather differs from the dense rows")
        same(a_dense(obs[dup].contiguous()), a_ring(index[dup].contiguous()), "an actor index with duplicates differs from the repeated rows")
        h = run_heads(torch, env, actor, obs, n, n_obs)
        assert torch.equal(B().bits(h), B().bits(run_heads(torch, env, actor, ring, n, R, index=index)))
        # a zero upstream gradient: exact zeros
        z = run_q_backward(torch, env, q, qm, obs.data_ptr(), act.data_ptr(), torch.zeros_like(gq), n_obs, n_u)
        assert not any(bool(t.any()) for t in z[0]) and not bool(z[1].any())
    finally:
        env.close()


def test_form_without_parameter_gradients():
    """grads == NULL: grad_actions has the bits of the call that also asks for parameters, dense and through the ring's index and
    beyond one pass of the grid; the critic's partial workspace stays NULL through any number of such calls, is allocated by the
    first call with parameters and stays that allocation afterwards."""
    import torch
    n, n_obs, n_u, hidden = B().ROWS_BEYOND_ONE_PASS, 20, 6, (64, 64)
    env = P().fan_env(n_obs, n_u, 64)
    try:
        qm = q_mlp(n_obs, n_u, hidden, "relu")
        q = env.make_q(qm)
        gen = torch.Generator(device="cuda")
        gen.manual_seed(3)
        obs = (torch.rand((n, n_obs), device="cuda", generator=gen) * 2 - 1).contiguous()
        act = (torch.rand((n, n_u), device="cuda", generator=gen) * 2 - 1).contiguous()
        gq = B().make_grad_out(torch, n, 1, seed=4).view(-1)
        args = (torch, env, q, qm, obs.data_ptr(), act.data_ptr(), gq, n_obs, n_u)
        assert env.backward_workspace(q) == (0, 0)
        _, a0 = run_q_backward(*args, params=False)
        _, a1 = run_q_backward(*args, params=False)
        assert env.backward_workspace(q) == (0, 0), "the form without parameter gradients allocated a workspace"
        grads, a2 = run_q_backward(*args)
        ptr, floats = env.backward_workspace(q)
        n_params = sum(W.size + b.size for W, b in qm.layers)
        assert ptr != 0 and floats == 256 * n_params
        assert float(a0.abs().max()) > 0 and not torch.isnan(a0).any()
        assert torch.equal(B().bits(a0), B().bits(a1)) and torch.equal(B().bits(a0), B().bits(a2))
        ring, index = ring_of(torch, n_obs, n_u, obs[:1000], act[:1000], 2048, gen)
        R = ring.shape[1]
        _, a3 = run_q_backward(torch, env, q, qm, ring.data_ptr(), ring.data_ptr() + 8 * n_obs, gq[:1000].contiguous(), R, R, params=False, index=index)
        _, a4 = run_q_backward(torch, env, q, qm, obs.data_ptr(), act.data_ptr(), gq[:1000].contiguous(), n_obs, n_u, params=False)
        assert torch.equal(B().bits(a3), B().bits(a4))
        run_q_backward(*args)
        assert env.backward_workspace(q) == (ptr, floats), "a later call allocated again"
        # the actor's: allocated by its first backward, both heads counted
        am = sac_mlp(n_obs, n_u, hidden, "relu")
        actor = env.make_sac_actor(am)
        assert env.backward_workspace(actor) == (0, 0)
        run_heads(torch, env, actor, obs, 64, n_obs)
        assert env.backward_workspace(actor) == (0, 0)
        run_actor_backward(torch, env, actor, am, obs, B().make_grad_out(torch, 64, 2 * n_u, seed=1), n_obs)
        ap, af = env.backward_workspace(actor)
        assert ap != 0 and af == 256 * (sum(W.size + b.size for W, b in am.layers) + 2 * (am.mu[0].size + am.mu[1].size))
    finally:
        env.close()


# ------------------------------------------------------------------------------------------ one SAC step end to end
def sac_losses(torch, actor_fn, q_fns, obs, act, y, z, log_alpha, n_u):
    """SB3 1.5's SAC.train on one minibatch with the normals given: (critic_loss, actor_loss, ent_coef_loss, heads, a).
    actor_fn(obs) -> [B, 2 n_u] = (mu | raw log_std); q_fns[i](obs, actions, learn) -> [B]."""
    heads = actor_fn(obs)
    heads.retain_grad()
    mu, ls = heads[:, :n_u], heads[:, n_u:].clamp(-20.0, 2.0)
    std = ls.exp()
    x = mu + std * z
    a = torch.tanh(x)
    a.retain_grad()
    logp = torch.distributions.Normal(mu, std).log_prob(x).sum(dim=1) - torch.log(1.0 - a ** 2 + 1e-6).sum(dim=1)
    ent_coef = log_alpha.detach().exp()
    ent_coef_loss = -(log_alpha * (logp - float(n_u)).detach()).mean()
    mse = torch.nn.functional.mse_loss
    critic_loss = 0.5 * sum(mse(qf(obs, act, True), y) for qf in q_fns)
    q_pi = torch.min(q_fns[0](obs, a, False), q_fns[1](obs, a, False))
    actor_loss = (ent_coef * logp - q_pi).mean()
    return critic_loss, actor_loss, ent_coef_loss, heads, a


def functional_nets(torch, am, qms, dtype, device):
    """leaves and callables of the same three networks through torch.nn.functional.linear"""
    F = torch.nn.functional
    t = lambda x: torch.tensor(np.asarray(x), dtype=dtype, device=device, requires_grad=True)
    ap = [t(v) for Wb in am.layers + [am.mu, am.log_std_head] for v in Wb]
    qps = [[t(v) for Wb in qm.layers for v in Wb] for qm in qms]

    def actor_fn(obs):
        h = obs
        for i in range(len(am.layers)):
            h = torch.relu(F.linear(h, ap[2 * i], ap[2 * i + 1]))
        return torch.cat([F.linear(h, ap[-4], ap[-3]), F.linear(h, ap[-2], ap[-1])], dim=1)

    def q_fn(ps):
        def f(obs, a, learn):
            h = torch.cat([obs, a], dim=1)
            for i in range(len(ps) // 2 - 1):
                h = torch.relu(F.linear(h, ps[2 * i], ps[2 * i + 1]))
            return F.linear(h, ps[-2], ps[-1])[:, 0]
        return f

    return ap, qps, actor_fn, [q_fn(ps) for ps in qps]


def reference_gradients(torch, am, qms, data, dtype, device, n_u):
    """every gradient of the step from the functional graph: parameter gradients of the critic loss (critics), of the actor loss
    (actor), of the ent_coef loss (log_ent_coef), and the actor loss's gradients on the heads and on the sampled action"""
    ap, qps, actor_fn, q_fns = functional_nets(torch, am, qms, dtype, device)
    d = {k: v.to(dtype=dtype, device=device) for k, v in data.items()}
    log_alpha = torch.tensor(np.log(0.2), dtype=dtype, device=device, requires_grad=True)
    critic_loss, actor_loss, ent_loss, heads, a = sac_losses(torch, actor_fn, q_fns, d["obs"], d["act"], d["y"], d["z"], log_alpha, n_u)
    gq = torch.autograd.grad(critic_loss, [p for ps in qps for p in ps])
    g_alpha = torch.autograd.grad(ent_loss, [log_alpha])
    actor_loss.backward()
    out = [g for g in gq] + [p.grad for p in ap] + [heads.grad[:, :n_u], heads.grad[:, n_u:], a.grad, g_alpha[0].reshape(1)]
    return [g.detach().cpu().numpy().astype(np.float64) for g in out], heads.detach(), a.detach()


def test_one_sac_step_end_to_end():
    """B = 129 on the (20, 6) env, 64-64 relu: SB3 1.5's critic loss, actor loss and ent_coef loss formed in torch on the device from
    sac_actor_apply / q_apply outputs with the normals given.  The gradients on mu, on the raw log_std and on the sampled action,
    and every parameter gradient (the critics' from the critic loss, the actor's from the actor loss, log_ent_coef's), against the
    same graph in float64 on the CPU; e32 from the same graph in float32 torch.nn.functional.linear on the device.  Rows are kept
    whose float64 hidden pre-activations (all three networks, on the replayed and on the sampled action) stay RELU_MARGIN off zero
    and whose |q1 - q2| on the sampled action is at least MIN_GAP: a kink may fall on the other side in float32."""
    import torch
    from tests.test_gpu_sac import sac_env
    n_obs, n_u, hidden, want = 20, 6, (64, 64), 129
    am = sac_mlp(n_obs, n_u, hidden, "relu", seed=11)
    qms = [q_mlp(n_obs, n_u, hidden, "relu", seed=12), q_mlp(n_obs, n_u, hidden, "relu", seed=13)]
    rng = np.random.default_rng(17)
    cand = want + 32
    obs, act = rng.uniform(-1, 1, (cand, n_obs)).astype(np.float32), rng.uniform(-1, 1, (cand, n_u)).astype(np.float32)
    z, y = rng.standard_normal((cand, n_u)).astype(np.float32), rng.standard_normal(cand).astype(np.float32)

    def pre_ok(layers, x):
        keep = np.ones(x.shape[0], dtype=bool)
        for W, b in layers:
            pre = x @ W.astype(np.float64).T + b.astype(np.float64)
            keep &= ~(np.abs(pre) < B().RELU_MARGIN).any(axis=1)
            x = np.maximum(pre, 0.0)
        return keep

    o64 = obs.astype(np.float64)
    a_pi, _, _, ls64 = am.forward_reference(o64, z.astype(np.float64))
    keep = pre_ok(am.layers, o64) & (np.abs(ls64) < 2.0 - 1e-3).all(axis=1)
    q_pi = []
    for qm in qms:
        keep &= pre_ok(qm.layers[:-1], np.concatenate([o64, act.astype(np.float64)], axis=1))
        keep &= pre_ok(qm.layers[:-1], np.concatenate([o64, a_pi], axis=1))
        q_pi.append(qm.forward_reference(np.concatenate([o64, a_pi], axis=1))[:, 0])
    keep &= np.abs(q_pi[0] - q_pi[1]) >= MIN_GAP
    idx = np.flatnonzero(keep)[:want]
    assert idx.size == want, (idx.size, "rows off every kink")
    assert 0.05 < float((q_pi[0] < q_pi[1])[idx].mean()) < 0.95, "both critics must be the minimum on some rows"
    data = {k: torch.from_numpy(v[idx]) for k, v in dict(obs=obs, act=act, z=z, y=y).items()}

    ref, _, _ = reference_gradients(torch, am, qms, data, torch.float64, "cpu", n_u)
    f32, _, _ = reference_gradients(torch, am, qms, data, torch.float32, "cuda", n_u)

    env = sac_env(n_obs, n_u, 64)
    try:
        actor, q1, q2 = env.make_sac_actor(am), env.make_q(qms[0]), env.make_q(qms[1])
        leaf = lambda x: torch.tensor(np.asarray(x), dtype=torch.float32, device="cuda", requires_grad=True)
        ap = [leaf(v) for Wb in am.layers + [am.mu, am.log_std_head] for v in Wb]
        qps = [[leaf(v) for Wb in qm.layers for v in Wb] for qm in qms]
        d = {k: v.cuda().contiguous() for k, v in data.items()}
        log_alpha = torch.tensor(np.log(0.2), dtype=torch.float32, device="cuda", requires_grad=True)
        q_fns = [lambda o, a, learn, c=c, ps=ps: env.q_apply(c, ps if learn else None, o, a) for c, ps in ((q1, qps[0]), (q2, qps[1]))]
        critic_loss, actor_loss, ent_loss, heads, a = sac_losses(torch, lambda o: env.sac_actor_apply(actor, ap, o), q_fns,
                                                                 d["obs"], d["act"], d["y"], d["z"], log_alpha, n_u)
        assert tuple(heads.shape) == (want, 2 * n_u) and heads.requires_grad
        critic_loss.backward()
        actor_loss.backward()
        ent_loss.backward()
        torch.cuda.synchronize()
        assert d["obs"].grad is None and d["act"].grad is None
        got = [p.grad for ps in qps for p in ps] + [p.grad for p in ap] + [heads.grad[:, :n_u], heads.grad[:, n_u:], a.grad, log_alpha.grad.reshape(1)]
        got = [g.detach().cpu().numpy().astype(np.float64) for g in got]
        names = [f"q{i}.{n}" for i in (1, 2) for n in ("W1", "b1", "W2", "b2", "W3", "b3")]
        names += [f"actor.{n}" for n in ("W1", "b1", "W2", "b2", "W_mu", "b_mu", "W_ls", "b_ls")] + ["d mu", "d log_std", "d action", "log_ent_coef"]
        assert len(got) == len(ref) == len(f32) == len(names)
        assert_within(compare_named(names, got, f32, ref, "SAC step B=129"), "SAC step")
    finally:
        env.close()


# ------------------------------------------------------------------------------------------ refusals
def test_refusals_on_a_live_handle():
    """Each new call refuses the three other roles by name, objects of another handle, strides below the widths, and (Q) both
    outputs NULL; two-layer networks need dW2 / db2; the good calls go through.  A shape over the 160 KiB is refused with the
    bytes in the message, and the shapes the issue names fit."""
    import torch
    from gym_dockauv_amd import _capi
    lib = _capi.load_library()
    n_obs, n_u, n = 20, 6, 64
    env, other = P().fan_env(n_obs, n_u, 64), P().fan_env(n_obs, n_u, 64)
    try:
        am, qm = sac_mlp(n_obs, n_u, (64, 64), "relu"), q_mlp(n_obs, n_u, (64, 64), "relu")
        plain = env.make_policy(P().make_mlp((n_obs, (64, 64), n_u, "tanh", "none"), seed=1))
        value = env.make_value(P().make_mlp((n_obs, (64, 64), 1, "tanh", "none"), seed=1))
        actor, q, foreign_a, foreign_q = env.make_sac_actor(am), env.make_q(qm), other.make_sac_actor(am), other.make_q(qm)
        rows = P().nan_rows(torch, n, n_obs, seed=2)
        act = torch.zeros((n, n_u), device="cuda")
        out = torch.zeros((n, 2 * n_u), device="cuda")
        g12, g1 = B().make_grad_out(torch, n, 2 * n_u, seed=1), B().make_grad_out(torch, n, 1, seed=1).view(-1)
        bufs = [torch.zeros(k, device="cuda") for k in (64 * 26, 64, 64 * 64, 64, 6 * 64, 6, 6 * 64, 6)]
        err = lambda: lib.dockauv_last_error(env._handle)

        def heads(p, stride=n_obs + 2):
            io = _capi.SacRowsIO()
            io.struct_size, io.row_stride, io.rows, io.n_rows, io.out = C.sizeof(io), stride, rows.data_ptr(), n, out.data_ptr()
            return lib.dockauv_sac_actor_forward_rows(env._handle, p.ptr, C.byref(io), None), err()

        def actor_bwd(p, stride=n_obs + 2, drop=()):
            io = _capi.SacActorBackwardIO()
            io.struct_size, io.row_stride, io.rows, io.n_rows, io.grad_out = C.sizeof(io), stride, rows.data_ptr(), n, g12.data_ptr()
            for f, t in zip(("dW1", "db1", "dW2", "db2", "dW_mu", "db_mu", "dW_ls", "db_ls"), bufs):
                setattr(io, f, None if f in drop else t.data_ptr())
            return lib.dockauv_sac_actor_backward(env._handle, p.ptr, C.byref(io), None), err()

        def q_bwd(p, obs_stride=n_obs + 2, act_stride=n_u, params=True, dx=True, drop=()):
            io = _capi.QBackwardIO()
            io.struct_size, io.obs_stride, io.act_stride, io.n_rows = C.sizeof(io), obs_stride, act_stride, n
            io.obs, io.actions, io.grad_q = rows.data_ptr(), act.data_ptr(), g1.data_ptr()
            io.grad_actions = out.data_ptr() if dx else None
            gr = _capi.PolicyGrads()
            gr.struct_size = C.sizeof(gr)
            for f, t in zip(("dW1", "db1", "dW2", "db2", "dW3", "db3"), bufs):
                setattr(gr, f, None if f in drop else t.data_ptr())
            if params:
                io.grads = C.pointer(gr)
            return lib.dockauv_q_backward(env._handle, p.ptr, C.byref(io), None), err()

        for call, own in ((heads, actor), (actor_bwd, actor), (q_bwd, q)):
            others = {"plain actor": plain, "value critic": value, "Q critic": q, "squashed-Gaussian actor": actor}
            for name, p in others.items():
                if p is own:
                    continue
                rc, msg = call(p)
                assert rc == -1 and b"the policy is a " + name.encode() in msg, (call.__name__, name, rc, msg)
            rc, msg = call(own)
            assert rc == 0, (call.__name__, rc, msg)
        for call, p in ((heads, foreign_a), (actor_bwd, foreign_a), (q_bwd, foreign_q)):
            rc, msg = call(p)
            assert rc == -1 and b"another handle" in msg, (rc, msg)
        rc, msg = heads(actor, stride=n_obs - 1)
        assert rc == -1 and b"dockauv_sac_rows_io.row_stride" in msg and b"n_obs 20" in msg, (rc, msg)
        rc, msg = actor_bwd(actor, stride=n_obs - 1)
        assert rc == -1 and b"dockauv_sac_actor_backward_io.row_stride" in msg, (rc, msg)
        rc, msg = q_bwd(q, obs_stride=n_obs - 1)
        assert rc == -1 and b"dockauv_q_backward_io.obs_stride" in msg, (rc, msg)
        rc, msg = q_bwd(q, act_stride=n_u - 1)
        assert rc == -1 and b"dockauv_q_backward_io.act_stride" in msg and b"n_u 6" in msg, (rc, msg)
        rc, msg = q_bwd(q, params=False, dx=False)
        assert rc == -1 and b"both NULL" in msg, (rc, msg)
        rc, msg = q_bwd(q, drop=("dW2",))
        assert rc == -1 and b"dW2/db2" in msg, (rc, msg)
        rc, msg = actor_bwd(actor, drop=("db2",))
        assert rc == -1 and b"db2 is NULL" in msg, (rc, msg)
        rc, msg = q_bwd(q, params=False)
        assert rc == 0, (rc, msg)
        # dockauv_policy_backward and dockauv_policy_forward_rows go on refusing both SAC roles
        for p, word in ((actor, b"squashed-Gaussian actor"), (q, b"Q critic")):
            rc = lib.dockauv_policy_forward_rows(env._handle, p.ptr, rows.data_ptr(), None, n, out.data_ptr(), None)
            assert rc == -1 and word in err()
        env.synchronize()
    finally:
        env.close()
        other.close()
    # LDS: 36-128-128 with the 16-row output tile and 44-128-128 for Q fit; the widest shapes the create calls accept do not
    for n_obs, n_u in ((36, 8), (133, 6)):
        wide = P().fan_env(n_obs, n_u, 64)
        try:
            am, qm = sac_mlp(n_obs, n_u, (128, 128), "relu"), q_mlp(n_obs, n_u, (128, 128), "relu")
            actor, q = wide.make_sac_actor(am), wide.make_q(qm)
            rows, _, _ = B().make_rows(torch, qm, 33, seed=ROW_SEED)
            ga, gq = B().make_grad_out(torch, 33, 2 * n_u, seed=1), B().make_grad_out(torch, 33, 1, seed=1).view(-1)
            stride = n_obs + n_u + 2
            if n_obs == 36:
                run_actor_backward(torch, wide, actor, am, rows, ga, stride)
                run_q_backward(torch, wide, q, qm, rows.data_ptr(), rows.data_ptr() + 4 * n_obs, gq, stride, stride)
            else:
                with pytest.raises(_capi.DockAUVError, match=r"needs \d{6} B of LDS for n_in 133"):
                    run_actor_backward(torch, wide, actor, am, rows, ga, stride)
                for params in (True, False):
                    with pytest.raises(_capi.DockAUVError, match=r"needs \d{6} B of LDS for n_in 139"):
                        run_q_backward(torch, wide, q, qm, rows.data_ptr(), rows.data_ptr() + 4 * n_obs, gq, stride, stride, params=params)
                assert not torch.isnan(run_heads(torch, wide, actor, rows, 33, stride)).any()     # the forward takes it
        finally:
            wide.close()
