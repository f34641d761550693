"""The PPO head on a real MI355X (include/dockauv.h: dockauv_ppo_head; TorchDocking3d.ppo_head / ppo_minibatch): every output
against the float64 statement (MLPPolicy.ppo_head_reference) at 1 row (no normalisation), 2, 63, 64, 65 and 257 rows and at more
rows than the bounded grid covers in one pass, for the action counts of both vehicles (6, 3) and of direct thruster control
(8), with and without normalisation, with and without the critic, dense and through an index that permutes and holds
duplicates; the bitwise properties (two calls, index against dense, NaN outside the index); ppo_minibatch against float64
autograd of the loop body of INTEGRATION.md section 6 on the CPU; and every refusal on a live handle.  Every input array starts
4 bytes off 8-byte alignment, every output sits between sentinels, every batch is closed in `finally`.

Inputs: mean U(-1, 1); log_std U(-1, 0.3); actions = mean + exp(log_std) z; log_prob_old = float32(float64 log-probability -
N(0, 0.3)); advantages 100 + N(0, 1); returns and v N(0, 1).  A row whose float64 ratio lies within EDGE of 1 +- clip may fall on
the other side in float32: such rows are replaced from a slightly larger draw (at most 1 / 256 of it; 3 of 65 569 on the CPU).
From 257 rows on each of the four regimes -- ratio above 1 + clip or below 1 - clip, times live or clipped (the sign of the
normalised advantage) -- holds at least 5 % of the rows (9.7 % to 14.8 % on the CPU).

Bound, per output (grad_mean, grad_v, grad_log_std and each entry of stats): max |x - x64| <= max(8 x e32, 4 ulp of max |x64|),
e32 the error of a float32 NumPy restatement (head_float32_numpy: the header's expression order, float64 only for the sums over
the rows) against float64; for approx_kl the floor is 4 ulp of the largest ratio (KL_FLOOR_ULPS: why); clip_fraction matches
exactly.  The measured ratios device error / max(e32, floor / 8):
profiles/update/head_error.txt (scripts/head_error.py on the helpers of this file; the tests print them as well).
"""
import copy
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CLIP, VF, ENT = 0.2, 0.5, 0.01
EDGE = 1e-5
# rows one pass of the bounded grid covers: 256 groups (dockauv_device.h: kBwdMaxGroups) x 1 024 rows a group takes per pass
# (kHeadPassRows: 256 lanes x 4 rows in flight); 33 more: a second pass of group 0 with half a wave of live rows
ROWS_BEYOND_ONE_PASS = 256 * 1024 + 33
ROW_COUNTS = (1, 2, 63, 64, 65, 257)
# approx_kl alone needs another floor than 4 ulp of its own size.  It is the mean of (ratio - 1) - lr: a difference of float32
# numbers of the size of the ratio (1 to 3 here) that leaves a few hundredths, so each row carries the rounding of expf -- up to
# an ulp of the RATIO, 1.2e-7 -- whatever the size of the result, and over a handful of rows nothing averages it away.  The
# restatement's own error is one draw of the same quantity and came out 9.36 times smaller than the device's at 2 rows and
# n_u = 8 (5.4e-8 against 5.8e-9; 6.03 at 64 rows, n_u = 3) with the floor at 4 ulp of approx_kl; every other output stayed
# below 3.  So the floor of approx_kl is 4 ulp of the largest ratio in the minibatch; the factor 8 on e32 stays.
KL_FLOOR_ULPS = 4.0
STAT_NAMES = ("loss", "policy_loss", "value_loss", "entropy_loss", "approx_kl", "clip_fraction", "adv_mean", "adv_std")
ENVS = {6: 20, 3: 36, 8: 36}          # n_u -> n_obs of a fan_env that has it (BlueROV2, LAUV, BlueROV2 with direct thrusters)


def B_():
    """the helpers of the backward tests: guarded, check_guards, shifted_rows, bits, stream_of, SENTINEL, P"""
    from tests import test_gpu_backward
    return test_gpu_backward


def f64_ratio(d):
    from gym_dockauv_amd.policy import MLPPolicy
    ls = d["log_std"].astype(np.float64)
    z = (d["actions"].astype(np.float64) - d["mean"].astype(np.float64)) * np.exp(-ls)
    return np.exp(MLPPolicy.log_prob_reference(z, ls) - d["log_prob_old"].astype(np.float64))


def draw_head(n, n_u, seed, mean=None, edge=EDGE, want_kept=False):
    """One minibatch of n rows as float32 arrays (keys mean, v, actions, log_prob_old, advantages, returns, log_std); the rows
    within `edge` of a clip edge are replaced from a draw of n + max(8, n / 16) rows (`mean`: that many rows of given means).
    Returns (arrays, rows replaced, rows drawn), with want_kept also which rows of the draw the n rows are."""
    from gym_dockauv_amd.policy import MLPPolicy
    rng = np.random.default_rng(seed)
    draw = n + max(8, n // 16)
    if mean is None:
        mean = rng.uniform(-1, 1, (draw, n_u))
    assert mean.shape == (draw, n_u)
    log_std = rng.uniform(-1, 0.3, n_u)
    z = rng.normal(size=(draw, n_u))
    d = dict(mean=mean, v=rng.normal(size=draw), actions=mean + np.exp(log_std) * z,
             log_prob_old=MLPPolicy.log_prob_reference(z, log_std) - rng.normal(0, 0.3, draw),
             advantages=100 + rng.normal(size=draw), returns=rng.normal(size=draw), log_std=log_std)
    d = {k: np.ascontiguousarray(a, dtype=np.float32) for k, a in d.items()}
    ratio = f64_ratio(d)
    near = (np.abs(ratio - (1 + CLIP)) < edge) | (np.abs(ratio - (1 - CLIP)) < edge)
    keep = np.flatnonzero(~near)[:n]
    assert keep.size == n
    replaced = int(near[: keep[-1] + 1].sum())
    assert replaced <= draw / 256.0, (replaced, draw)
    out = {k: (a if k == "log_std" else np.ascontiguousarray(a[keep])) for k, a in d.items()}
    if n >= 257:
        adv = out["advantages"].astype(np.float64)
        up, r = adv > adv.mean(), ratio[keep]
        for name, mask in (("high clipped", (r > 1 + CLIP) & up), ("high live", (r > 1 + CLIP) & ~up),
                           ("low live", (r < 1 - CLIP) & up), ("low clipped", (r < 1 - CLIP) & ~up)):
            assert mask.mean() >= 0.05, (name, mask.mean())
    return (out, replaced, draw, keep) if want_kept else (out, replaced, draw)


def with_duplicates(d, n):
    """the minibatch with some positions repeating another position's whole row (what an index with duplicates addresses)"""
    src = np.arange(n)
    if n >= 63:
        src[1::5] = 0
        src[n // 2: n // 2 + 3] = n - 1
    return {k: (a if k == "log_std" else np.ascontiguousarray(a[src])) for k, a in d.items()}, src


def scatter(d, src, seed):
    """row arrays of n + 37 rows, NaN everywhere but at the slots an index addresses: (row arrays, index); position r reads slot
    index[r], positions that repeat a row share its slot, the slots are a random permutation"""
    n = src.size
    slots = np.random.default_rng(seed).permutation(n + 37)[:n]
    index = slots[src].astype(np.int64)
    rows = {}
    for k in ("actions", "log_prob_old", "advantages", "returns"):
        a = np.full((n + 37,) + d[k].shape[1:], np.nan, dtype=np.float32)
        a[index] = d[k]
        rows[k] = a
    return rows, index


def fma32(a, b, c):
    """fmaf on float32 arrays: the product of two float32 is exact in float64"""
    return (a.astype(np.float64) * b.astype(np.float64) + np.asarray(c, dtype=np.float32).astype(np.float64)).astype(np.float32)


def head_float32_numpy(d, normalize, critic):
    """the definition of the header in float32 NumPy arrays, float64 only for the sums over the rows (each rounded once).
    m and s: the float32 squares are centred on the float32 minibatch mean.  That is the header's form as long as one group
    takes all the rows (up to 1 024: its centre is m itself); with more groups the library centres each group's squares on that
    group's own float32 mean and moves them to m in float64, which this restatement does not spell out -- both are float32
    squares of deviations of the same size summed in float64, so e32 measures the same rounding.  Only
    test_more_rows_than_one_pass_of_the_grid has more than one group."""
    f = np.float32
    mean, a, lpo, adv, ls = d["mean"], d["actions"], d["log_prob_old"], d["advantages"], d["log_std"]
    n, n_u = mean.shape
    m, s = f(0), f(1)
    if normalize:
        m = f(adv.sum(dtype=np.float64) / n)
        dc = adv - m
        s = f(np.sqrt((dc * dc).sum(dtype=np.float64) / (n - 1)))
        adv = (adv - m) / (s + f(1e-8))
    inv_std = np.exp(-ls)
    z = (a - mean) * inv_std
    term = fma32(f(-0.5) * z, z, -(ls + f(0.918938533)))
    halves = []
    for cols in (range(0, min(4, n_u)), range(4, n_u)):
        acc = np.zeros(n, dtype=f)
        for j in cols:
            acc = acc + term[:, j]
        halves.append(acc)
    lr = (halves[0] + halves[1]) - lpo
    ratio = np.exp(lr)
    lo, hi = f(1) - f(CLIP), f(1) + f(CLIP)
    live = ~(((adv > 0) & (ratio > hi)) | ((adv < 0) & (ratio < lo)))
    surr = np.minimum(ratio * adv, np.minimum(np.maximum(ratio, lo), hi) * adv)
    g = np.where(live, -(adv * ratio) / f(n), f(0)).astype(f)
    grad_mean = (g[:, None] * z) * inv_std
    grad_log_std = (g[:, None] * fma32(z, z, f(-1))).sum(axis=0, dtype=np.float64).astype(f) - f(ENT)
    grad_v, value_loss = None, f(0)
    if critic:
        dv = d["v"] - d["returns"]
        grad_v = ((f(2) * f(VF)) * dv) / f(n)
        value_loss = f((dv * dv).sum(dtype=np.float64) / n)
    policy_loss = f(-surr.sum(dtype=np.float64) / n)
    e = f(0)
    for j in range(n_u):
        e = e + (f(1.418938533) + ls[j])
    entropy_loss = -e
    loss = fma32(f(VF), value_loss, fma32(f(ENT), entropy_loss, policy_loss))
    stats = np.array([loss, policy_loss, value_loss, entropy_loss, f(((ratio - f(1)) - lr).sum(dtype=np.float64) / n),
                      f((np.abs(ratio - f(1)) > f(CLIP)).sum(dtype=np.float64) / n), m, s], dtype=f)
    for x in (grad_mean, grad_log_std, z, lr, ratio, g):
        assert x.dtype == f
    return grad_mean, grad_v, grad_log_std, stats


def reference(d, normalize, critic):
    from gym_dockauv_amd.policy import MLPPolicy
    return MLPPolicy.ppo_head_reference(d["mean"], d["v"] if critic else None, d["actions"], d["log_prob_old"], d["advantages"],
                                        d["returns"], d["log_std"], CLIP, VF, ENT, normalize_advantage=normalize)


def make_actor(env, n_u, log_std):
    """an actor on `env` whose device log_std is `log_std` (the head reads nothing else of it)"""
    mlp = B_().P().make_mlp((env.n_observations, (17,), n_u, "tanh", "none"), seed=1, log_std=log_std)
    return env.make_policy(mlp)


def run_head(torch, env, actor, d, normalize, critic, rows=None, index=None):
    """dockauv_ppo_head into guarded buffers, every float input 4 bytes off 8-byte alignment; `rows` / `index`: the row arrays and
    the int64 index to read them through (default: the minibatch's own arrays, dense).  Returns NumPy (grad_mean, grad_v or
    None, grad_log_std, stats)."""
    T = B_()
    n, n_u = d["mean"].shape
    dev = lambda a: T.shifted_rows(torch, torch.from_numpy(a).cuda())
    src = rows if rows is not None else d
    t = {k: dev(d[k]) for k in ("mean", "v")}
    t.update({k: dev(src[k]) for k in ("actions", "log_prob_old", "advantages", "returns")})
    idx = None if index is None else torch.from_numpy(index).cuda()
    bufs = {"grad_mean": T.guarded(torch, n * n_u), "grad_v": T.guarded(torch, n), "grad_log_std": T.guarded(torch, n_u),
            "stats": T.guarded(torch, 8)}
    ptr = lambda name: bufs[name][1].data_ptr()
    env.ppo_head_device(actor, n, t["mean"].data_ptr(), t["v"].data_ptr() if critic else 0, t["actions"].data_ptr(),
                        t["log_prob_old"].data_ptr(), t["advantages"].data_ptr(), t["returns"].data_ptr() if critic else 0,
                        ptr("grad_mean"), ptr("grad_v") if critic else 0, ptr("grad_log_std"), ptr("stats"), CLIP, VF, ENT,
                        normalize_advantage=normalize, index_ptr=0 if idx is None else idx.data_ptr(), stream=T.stream_of(torch))
    torch.cuda.synchronize()
    out = []
    for name in ("grad_mean", "grad_v", "grad_log_std", "stats"):
        buf, v = bufs[name]
        T.check_guards(buf, v.numel(), name)
        if name == "grad_v" and not critic:
            assert bool((v == T.SENTINEL).all()), "grad_v was written without a critic"
            out.append(None)
            continue
        assert not bool((v == T.SENTINEL).any()), f"an entry of {name} was not written"
        out.append(v.cpu().numpy().reshape(n, n_u) if name == "grad_mean" else v.cpu().numpy())
    return out


def compare(d, normalize, critic, got, label):
    """[(output, device error, float32 NumPy error, bound, ratio)] for the device's `got`; prints each figure"""
    ref, f32 = reference(d, normalize, critic), head_float32_numpy(d, normalize, critic)
    pairs = [(name, got[i], f32[i], ref[i]) for i, name in enumerate(("grad_mean", "grad_v", "grad_log_std")) if ref[i] is not None]
    pairs += [(f"stats.{name}", got[3][k: k + 1], f32[3][k: k + 1], ref[3][k: k + 1]) for k, name in enumerate(STAT_NAMES)]
    res = []
    for name, dv, f, r in pairs:
        assert dv.shape == r.shape and not np.isnan(dv).any(), (label, name, "NaN: a row outside the minibatch got in")
        e_dev = float(np.abs(dv.astype(np.float64) - r).max())
        e_np = float(np.abs(f.astype(np.float64) - r).max())
        floor = 4.0 * float(np.spacing(np.float32(np.abs(r).max())))
        if name == "stats.approx_kl":
            floor = KL_FLOOR_ULPS * float(np.spacing(np.float32(f64_ratio(d).max())))
        bound = max(8.0 * e_np, floor)
        ratio = e_dev / max(e_np, floor / 8.0)
        print(f"head {label} {name}: device {e_dev:.3e}, float32 NumPy {e_np:.3e}, bound {bound:.3e}, ratio {ratio:.2f}")
        res.append((name, e_dev, e_np, bound, ratio))
    # a row counts as clipped or not: the same count in float32 and float64, so the same float32 quotient
    assert got[3][5] == np.float32(ref[3][5]), (label, "clip_fraction", got[3][5], ref[3][5])
    return res


def head_case(n_u, n, normalize, critic, indexed, env=None, actors=None):
    """one case: the rows of compare()"""
    import torch
    d, _, _ = draw_head(n, n_u, seed=7 * n + n_u)
    rows = index = None
    if indexed:
        d, src = with_duplicates(d, n)
        rows, index = scatter(d, src, seed=n)
    own = env is None
    if own:
        env = B_().P().fan_env(ENVS[n_u], n_u, 64)
    try:
        key = d["log_std"].tobytes()
        actors = {} if actors is None else actors
        if key not in actors:
            actors[key] = make_actor(env, n_u, d["log_std"])
        got = run_head(torch, env, actors[key], d, normalize, critic, rows, index)
    finally:
        if own:
            env.close()
    label = f"n_u{n_u}_rows{n}_{'norm' if normalize else 'raw'}_{'critic' if critic else 'nocritic'}_{'index' if indexed else 'dense'}"
    return compare(d, normalize, critic, got, label)


def variants(n):
    return [(nm, cr, ix) for nm in ((True, False) if n >= 2 else (False,)) for cr in (True, False) for ix in (False, True)]


@pytest.mark.parametrize("n_u", [6, 3, 8])
def test_against_float64(n_u):
    """Every row count below one pass, each with and without normalisation (one row: without), with and without the critic, dense
    and through an index with duplicates."""
    env = B_().P().fan_env(ENVS[n_u], n_u, 64)
    worst, actors = (0.0, ""), {}
    try:
        for n in ROW_COUNTS:
            for normalize, critic, indexed in variants(n):
                for name, e_dev, e_np, bound, ratio in head_case(n_u, n, normalize, critic, indexed, env, actors):
                    worst = max(worst, (ratio, f"rows {n} {name}"))
                    assert e_dev <= bound, (n_u, n, normalize, critic, indexed, name, e_dev, e_np, bound)
    finally:
        env.close()
    print(f"head n_u {n_u}: largest ratio device error / max(e32, floor / 8) = {worst[0]:.2f} ({worst[1]})")


@pytest.mark.parametrize("normalize,critic,indexed", [(True, True, True), (True, False, False), (False, True, False)])
def test_more_rows_than_one_pass_of_the_grid(normalize, critic, indexed):
    """ROWS_BEYOND_ONE_PASS rows: groups 0 .. 255 walk one pass each, group 0 a second one with 33 live rows.  The only cases
    whose advantage moments come from more than one group's partial (head_float32_numpy: how its e32 relates to that form)."""
    for name, e_dev, e_np, bound, ratio in head_case(6, ROWS_BEYOND_ONE_PASS, normalize, critic, indexed):
        assert e_dev <= bound, (name, e_dev, e_np, bound)


@pytest.mark.parametrize("n", [257, 5000])
def test_bitwise_properties(n):
    """Two calls give the same bits; rows through an index (a permutation with duplicates, NaN in every row-array entry outside
    it) give the bits of the same rows laid out densely; without the critic grad_v stays untouched."""
    import torch
    env = B_().P().fan_env(20, 6, 64)
    try:
        d, _, _ = draw_head(n, 6, seed=3)
        d, src = with_duplicates(d, n)
        rows, index = scatter(d, src, seed=4)
        assert np.unique(index).size < n and np.isnan(rows["advantages"]).sum() > 37
        actor = make_actor(env, 6, d["log_std"])
        for normalize, critic in ((True, True), (False, False)):
            a = run_head(torch, env, actor, d, normalize, critic)
            b = run_head(torch, env, actor, d, normalize, critic)
            c = run_head(torch, env, actor, d, normalize, critic, rows, index)
            for name, x, y, z in zip(("grad_mean", "grad_v", "grad_log_std", "stats"), a, b, c):
                if x is None:
                    assert y is None and z is None
                    continue
                assert not np.isnan(x).any() and float(np.abs(x).max()) > 0
                assert np.array_equal(x.view(np.int32), y.view(np.int32)), f"two calls differ in {name}"
                assert np.array_equal(x.view(np.int32), z.view(np.int32)), f"the index differs from the dense rows in {name}"
    finally:
        env.close()


def sequential(torch, mlp, dtype, device):
    mods = []
    for i, (W, b) in enumerate(mlp.layers):
        lin = torch.nn.Linear(W.shape[1], W.shape[0])
        with torch.no_grad():
            lin.weight.copy_(torch.from_numpy(W))
            lin.bias.copy_(torch.from_numpy(b))
        mods += [lin] + ([torch.nn.Tanh()] if i < len(mlp.layers) - 1 else [])
    return torch.nn.Sequential(*mods).to(dtype=dtype, device=device)


def section6_body(torch, actor, critic, log_std, obs, actions, logp_old, adv, ret):
    """the loop body of INTEGRATION.md section 6: (loss, stats[:6] as tensors)"""
    mean, v = actor(obs), critic(obs)[:, 0]
    dist = torch.distributions.Normal(mean, log_std.exp())
    lr = dist.log_prob(actions).sum(-1) - logp_old
    ratio = lr.exp()
    a = (adv - adv.mean()) / (adv.std() + 1e-8)
    policy_loss = -torch.min(ratio * a, ratio.clamp(1 - CLIP, 1 + CLIP) * a).mean()
    value_loss = ((ret - v) ** 2).mean()
    entropy_loss = -dist.entropy().sum(-1).mean()
    loss = policy_loss + VF * value_loss + ENT * entropy_loss
    return loss, [loss, policy_loss, value_loss, entropy_loss, ((ratio - 1) - lr).mean(), ((ratio - 1).abs() > CLIP).to(loss.dtype).mean()], ratio


def test_ppo_minibatch_against_float64_autograd():
    """A 25-64-64-6 actor and a 25-64-64-1 critic, 257 rows through an index: every .grad and stats within the rule above of
    float64 autograd of the section-6 body on the CPU (e32: the same body in float32 torch on the CPU); a second call replaces
    .grad instead of adding to it."""
    import torch
    from gym_dockauv_amd.config.env_config import BASE_CONFIG
    from gym_dockauv_amd.envs.torch_env import TorchDocking3d
    T = B_()
    n_in, n_u, n, M = 25, 6, 257, 400
    cfg = copy.deepcopy(BASE_CONFIG)
    cfg["radar"].update(T.P().FANS[n_in])
    env = TorchDocking3d(cfg, num_envs=64, scenario="ObstaclesDocking3d", device_seed=7)
    try:
        assert (env.n_obs, env.n_u) == (n_in, n_u)
        actor_mlp = T.P().make_mlp((n_in, (64, 64), n_u, "tanh", "none"), seed=6, log_std=np.zeros(n_u))
        critic_mlp = T.P().make_mlp((n_in, (64, 64), 1, "tanh", "none"), seed=7)
        policy, value = env.make_policy(actor_mlp), env.make_value(critic_mlp)
        rng = np.random.default_rng(11)
        packed = np.full((M, n_in + 2), np.nan, dtype=np.float32)
        packed[:, :n_in] = rng.uniform(-1, 1, (M, n_in))
        # the means are the actor's own on `pool` rows of the packed buffer; a float32 mean moves a ratio by up to ~1e-5, so
        # the band round the clip edges is 1e-4 here (tests/test_gpu_backward.py: the same figure for the same reason)
        pool = rng.permutation(M)[: n + max(8, n // 16)]
        d, _, _, kept = draw_head(n, n_u, seed=12, mean=actor_mlp.forward_reference(packed[pool, :n_in].astype(np.float64)),
                                  edge=1e-4, want_kept=True)
        index = pool[kept].astype(np.int64)
        arrays = {}
        for k in ("actions", "log_prob_old", "advantages", "returns"):
            a = np.full((M,) + d[k].shape[1:], np.nan, dtype=np.float32)
            a[index] = d[k]
            arrays[k] = a
        log_std0 = d["log_std"]

        grads, stats = {}, {}
        for kind, dt in (("f32", torch.float32), ("f64", torch.float64)):
            a_net, c_net = sequential(torch, actor_mlp, dt, "cpu"), sequential(torch, critic_mlp, dt, "cpu")
            ls = torch.tensor(log_std0, dtype=dt, requires_grad=True)
            g = lambda x: torch.from_numpy(x[index]).to(dt)
            loss, st, ratio = section6_body(torch, a_net, c_net, ls, g(packed[:, :n_in]), g(arrays["actions"]), g(arrays["log_prob_old"]),
                                     g(arrays["advantages"]), g(arrays["returns"]))
            loss.backward()
            ratio_max = float(ratio.detach().max())
            grads[kind] = [p.grad.numpy().astype(np.float64) for net in (a_net, c_net) for p in net.parameters()] + [ls.grad.numpy().astype(np.float64)]
            adv = arrays["advantages"][index].astype(np.float64)
            stats[kind] = np.array([float(s.detach()) for s in st] + ([adv.mean(), adv.std(ddof=1)] if kind == "f64" else
                                                                      [np.float32(adv.mean()), np.float32(adv.std(ddof=1))]), dtype=np.float64)

        a_net, c_net = sequential(torch, actor_mlp, torch.float32, "cuda"), sequential(torch, critic_mlp, torch.float32, "cuda")
        log_std = torch.tensor(log_std0, device="cuda", requires_grad=True)
        dev = {k: T.shifted_rows(torch, torch.from_numpy(a).cuda()) for k, a in arrays.items()}
        rows_t, index_t = torch.from_numpy(packed).cuda(), torch.from_numpy(index).cuda()
        params = list(a_net.parameters()) + list(c_net.parameters()) + [log_std]
        for p in params:
            p.grad = torch.full_like(p, 3.0)          # what a second call must replace
        call = lambda: env.ppo_minibatch(policy, value, list(a_net.parameters()), log_std, list(c_net.parameters()), dev["actions"],
                                         dev["log_prob_old"], dev["advantages"], dev["returns"], rows_t, index_t,
                                         clip_range=CLIP, vf_coef=VF, ent_coef=ENT)
        st1 = call()
        first = [p.grad.clone() for p in params]
        st2 = call()
        torch.cuda.synchronize()
        assert tuple(st1.shape) == (8,) and st1.device.type == "cuda"
        for p, g1 in zip(params, first):
            assert p.grad.shape == p.shape and torch.equal(T.bits(p.grad), T.bits(g1)), "a second call changed .grad: accumulated?"
        assert torch.equal(T.bits(st1), T.bits(st2))
        got = [p.grad.cpu().numpy().astype(np.float64) for p in params] + [st1.cpu().numpy().astype(np.float64)[k: k + 1] for k in range(8)]
        f32 = grads["f32"] + [stats["f32"][k: k + 1] for k in range(8)]
        f64 = grads["f64"] + [stats["f64"][k: k + 1] for k in range(8)]
        names = [f"{who}.{nm}" for who in ("actor", "critic") for nm in ("W1", "b1", "W2", "b2", "W3", "b3")] + ["log_std"] + \
                [f"stats.{s}" for s in STAT_NAMES]
        for name, dv, f, r in zip(names, got, f32, f64):
            e_dev, e_np = float(np.abs(dv - r).max()), float(np.abs(f - r).max())
            floor = 4.0 * float(np.spacing(np.float32(np.abs(r).max())))
            if name == "stats.approx_kl":
                floor = KL_FLOOR_ULPS * float(np.spacing(np.float32(ratio_max)))
            bound = max(8.0 * e_np, floor)
            print(f"ppo_minibatch {name}: device {e_dev:.3e}, float32 torch on the CPU {e_np:.3e}, bound {bound:.3e}, "
                  f"ratio {e_dev / max(e_np, floor / 8.0):.2f}")
            assert e_dev <= bound, (name, e_dev, e_np, bound)
    finally:
        env.close()


def test_torch_ppo_head_validates_and_matches_the_c_call():
    """TorchDocking3d.ppo_head: the tensors of the direct call, and a ValueError for a wrong device, dtype, shape or layout."""
    import torch
    from gym_dockauv_amd.config.env_config import BASE_CONFIG
    from gym_dockauv_amd.envs.torch_env import TorchDocking3d
    env = TorchDocking3d(copy.deepcopy(BASE_CONFIG), num_envs=64, scenario="ObstaclesDocking3d", device_seed=7)
    try:
        n_u, n = env.n_u, 65
        d, _, _ = draw_head(n, n_u, seed=5)
        actor = make_actor(env.batch, n_u, d["log_std"])
        t = {k: torch.from_numpy(a).cuda() for k, a in d.items()}
        args = lambda **over: [over.get(k, t[k]) for k in ("mean", "v", "actions", "log_prob_old", "advantages", "returns")]
        kw = dict(clip_range=CLIP, vf_coef=VF, ent_coef=ENT)
        gm, gv, gls, stats = env.ppo_head(actor, *args(), **kw)
        torch.cuda.synchronize()
        want = run_head(torch, env.batch, actor, d, True, True)
        for x, y in zip((gm, gv, gls, stats), want):
            assert np.array_equal(x.cpu().numpy().view(np.int32).reshape(-1), y.view(np.int32).reshape(-1))
        gm, gv, gls, stats = env.ppo_head(actor, *args(v=None), **kw)
        assert gv is None and float(stats[2]) == 0.0
        for bad in (dict(mean=t["mean"].cpu()), dict(mean=t["mean"].double()), dict(mean=t["mean"][:, :3]), dict(v=t["v"][:-1]),
                    dict(actions=t["actions"].t().contiguous().t()), dict(log_prob_old=t["log_prob_old"][:-1]),
                    dict(advantages=t["advantages"].double()), dict(returns=t["returns"][::2])):
            with pytest.raises(ValueError):
                env.ppo_head(actor, *args(**bad), **kw)
        with pytest.raises(ValueError):
            env.ppo_head(actor, *args(), index=torch.arange(n, device="cuda", dtype=torch.int32), **kw)
        with pytest.raises(ValueError):
            env.ppo_head(actor, t["mean"][:1], t["v"][:1], t["actions"][:1], t["log_prob_old"][:1], t["advantages"][:1], t["returns"][:1], **kw)
    finally:
        env.close()


def test_refusals_on_a_live_handle():
    """One refusal per line of the header's list, each before any device call and naming its field; then the good call."""
    import torch
    from gym_dockauv_amd import _capi
    lib = _capi.load_library()
    T = B_()
    env, other = T.P().fan_env(20, 6, 64), T.P().fan_env(20, 6, 64)
    try:
        n = 64
        d, _, _ = draw_head(n, 6, seed=1)
        actor = make_actor(env, 6, d["log_std"])
        critic = env.make_value(T.P().make_mlp((20, (17,), 1, "tanh", "none"), seed=2))
        no_std = env.make_policy(T.P().make_mlp((20, (17,), 6, "tanh", "none"), seed=3))
        squashed = env.make_policy(T.P().make_mlp((20, (17,), 6, "tanh", "tanh"), seed=4, log_std=d["log_std"]))
        foreign = make_actor(other, 6, d["log_std"])
        t = {k: torch.from_numpy(a).cuda() for k, a in d.items()}
        outs = {"grad_mean": torch.zeros(n * 6, device="cuda"), "grad_v": torch.zeros(n, device="cuda"),
                "grad_log_std": torch.zeros(6, device="cuda"), "stats": torch.zeros(8, device="cuda")}

        def call(p=actor, handle=env._handle, drop=(), null_io=False, **over):
            io = _capi.PPOHeadIO()
            io.struct_size = C.sizeof(_capi.PPOHeadIO)
            io.normalize_advantage, io.n_rows = 1, n
            io.clip_range, io.vf_coef, io.ent_coef = CLIP, VF, ENT
            for f in ("mean", "v", "actions", "log_prob_old", "advantages", "returns"):
                setattr(io, f, None if f in drop else t[f].data_ptr())
            for f, o in outs.items():
                setattr(io, f, None if f in drop else o.data_ptr())
            for k, val in over.items():
                setattr(io, k, val)
            rc = lib.dockauv_ppo_head(handle, None if p is None else p.ptr, None if null_io else C.byref(io), None)
            return rc, lib.dockauv_last_error(handle)

        for kwargs, word in ((dict(handle=None), b"null handle"), (dict(p=None), b"null actor"), (dict(null_io=True), b"io is NULL"),
                             (dict(p=critic), b"critic"), (dict(p=no_std), b"log_std"), (dict(p=squashed), b"DOCKAUV_ACT_TANH"),
                             (dict(p=foreign), b"another handle"), (dict(struct_size=112), b"struct_size"),
                             (dict(n_rows=0), b"n_rows"), (dict(n_rows=1), b"n_rows"), (dict(clip_range=0.0), b"clip_range"),
                             (dict(clip_range=-0.2), b"clip_range"), (dict(drop=("mean",)), b"mean"),
                             (dict(drop=("actions",)), b"actions"), (dict(drop=("log_prob_old",)), b"log_prob_old"),
                             (dict(drop=("advantages",)), b"advantages"), (dict(drop=("returns",)), b"returns"),
                             (dict(drop=("grad_mean",)), b"grad_mean"), (dict(drop=("grad_log_std",)), b"grad_log_std"),
                             (dict(drop=("stats",)), b"stats"), (dict(drop=("v",)), b"grad_v"), (dict(drop=("grad_v",)), b"grad_v")):
            rc, msg = call(**kwargs)
            assert rc == -1 and word in msg, (kwargs, rc, msg)
        assert not any(bool(o.any()) for o in outs.values()), "a refused call wrote an output"
        rc, msg = call(n_rows=1, normalize_advantage=0)            # one row without normalisation: taken
        assert rc == 0, (rc, msg)
        rc, msg = call(drop=("v", "grad_v", "returns"))            # no critic: taken, returns is not needed
        assert rc == 0, (rc, msg)
        rc, msg = call()                                           # ... and the good call goes through
        assert rc == 0, (rc, msg)
        env.synchronize()
        assert bool(outs["stats"].any()) and not bool(torch.isnan(outs["stats"]).any())
    finally:
        env.close()
        other.close()
