"""SAC's loss head on a real MI355X (include/dockauv.h: dockauv_sac_sample, dockauv_sac_critic_head, dockauv_sac_actor_head,
dockauv_sac_ent_coef_step; TorchDocking3d.sac_sample / sac_critic_head / sac_actor_head / ent_coef_step / sac_gradients): the
sample bit for bit against dockauv_sac_target's draw, dense and through an index; the critic head bit for bit and its sums
against float64; the actor head on crafted heads against float64 under the project's bound; three chained ent_coef steps bit for
bit against the float32 statement; the bitwise properties; refusals on a live handle; and the whole gradient half of one SAC step
(sac_gradients) against the same graph in float64 on the CPU.  n_u = 3 (the lo sum only), 6 (lo and hi) and 8 (both full) on the
(36, 3), (20, 6) and (36, 8) envs of tests/test_gpu_sac.py; B = 1, 33, 129 and 1 324 = 1 024 + 300: the three calls with sums are one
group of 1 024 lanes, so there lanes 0 .. 299 take a second row and the second pass is partial.  Outputs go into guarded buffers
between sentinels, inputs are slices of NaN-filled buffers (tests/test_gpu_backward.py: guarded, check_guards).  The four calls
keep no workspace, so there is none to watch; the refusal test checks that they allocate none of the backward's either.

Bound of the actor head, per output (the project's, tests/test_gpu_backward.py): max |g - g64| <= max(8 x e32, 4 ulp of max |g64|).
g64: sac_actor_head_reference with the normals of normals_reference(.., slot=SAC_ROWS_STREAM); e32: the error of the float32
restatement sac_actor_head_float32 fed normals_float32 (the kernel's own float32 Box-Muller restated: the rounding of u1 near 1 is
the largest single term of the device's deviation, see normals_reference).  The measured ratios: profiles/sac/head_error.txt
(scripts/sac_head_error.py on the helpers of this file; the tests print them as well).
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROW_COUNTS = (1, 33, 129, 1024 + 300)
CASES = [((36, 3), (64, 64)), ((20, 6), (17,)), ((36, 8), (128, 128))]     # (n_obs, n_u), hidden
ACTOR_SEED = 77
RECORD = {}                   # the figures of the last end-to-end case, for scripts/sac_head_error.py
ids = lambda c: f"{c[0][0]}-{'-'.join(map(str, c[1]))}-{c[0][1]}"


def B_():
    from tests import test_gpu_backward
    return test_gpu_backward


def S():
    from tests import test_gpu_sac
    return test_gpu_sac


def SB():
    from tests import test_gpu_sac_backward
    return test_gpu_sac_backward


def HH():
    from tests import test_sac_head_host
    return test_sac_head_host


def stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def bits(x):
    return B_().bits(x)


def ulp32(x):
    return float(np.spacing(np.float32(abs(float(x)))))


def in_nan(torch, x):
    """a contiguous device copy of float32 array x that sits inside a NaN-filled buffer"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    buf = torch.full((x.size + 64,), float("nan"), device="cuda")
    v = buf[32: 32 + x.size].view(*x.shape)
    v.copy_(torch.from_numpy(x))
    return v


def out_of(torch, bufs, shapes, what):
    outs = []
    for (buf, v), s in zip(bufs, shapes):
        B_().check_guards(buf, v.numel(), what)
        assert not bool((v == B_().SENTINEL).any()), f"an entry of {what} was not written"
        outs.append(v.clone().view(*s))
    return outs


# ------------------------------------------------------------------------------------------ guarded calls on device pointers
def run_sample(torch, env, actor, heads, t, row_offset=0):
    n, n_u = heads.shape[0], env.n_u
    bufs = [B_().guarded(torch, n * n_u), B_().guarded(torch, n)]
    env.batch.sac_sample_device(actor, heads.data_ptr(), n, bufs[0][1].data_ptr(), bufs[1][1].data_ptr(), t=t, row_offset=row_offset, stream=stream())
    torch.cuda.synchronize()
    return out_of(torch, bufs, [(n, n_u), (n,)], "a / logp")


def run_critic_head(torch, env, q, q1, q2, y):
    n = q1.shape[0]
    bufs = [B_().guarded(torch, n), B_().guarded(torch, n), B_().guarded(torch, 6)]
    env.batch.sac_critic_head_device(q, q1.data_ptr(), q2.data_ptr(), y.data_ptr(), n, *[v.data_ptr() for _, v in bufs], stream=stream())
    torch.cuda.synchronize()
    return out_of(torch, bufs, [(n,), (n,), (6,)], "grad_q / stats")


def run_actor_head(torch, env, actor, heads, q1, q2, dq1, dq2, t, row_offset=0, ent_coef=None, log_ent_coef=None):
    n, n_u = heads.shape[0], env.n_u
    bufs = [B_().guarded(torch, n * 2 * n_u), B_().guarded(torch, 4)]
    env.batch.sac_actor_head_device(actor, heads.data_ptr(), q1.data_ptr(), q2.data_ptr(), dq1.data_ptr(), dq2.data_ptr(), n,
                                    bufs[0][1].data_ptr(), bufs[1][1].data_ptr(), ent_coef=0.0 if ent_coef is None else ent_coef,
                                    log_ent_coef_ptr=0 if log_ent_coef is None else log_ent_coef.data_ptr(), t=t, row_offset=row_offset,
                                    stream=stream())
    torch.cuda.synchronize()
    return out_of(torch, bufs, [(n, 2 * n_u), (4,)], "grad_out / stats")


def run_ent_coef_step(torch, env, state, logp, step, lr, target, betas=(0.9, 0.999), eps=1e-8):
    """one step on a guarded copy of `state`: (new state, before, stats) as device tensors"""
    bufs = [B_().guarded(torch, 3), B_().guarded(torch, 1), B_().guarded(torch, 4)]
    bufs[0][1].copy_(state)
    env.batch.sac_ent_coef_step_device(bufs[0][1].data_ptr(), logp.data_ptr(), logp.shape[0], step, lr, target, betas=betas, eps=eps,
                                       before_ptr=bufs[1][1].data_ptr(), stats_ptr=bufs[2][1].data_ptr(), stream=stream())
    torch.cuda.synchronize()
    return out_of(torch, bufs, [(3,), (1,), (4,)], "state / before / stats")


def rows_normals(n, t, n_u, row_offset=0, f32=False):
    from gym_dockauv_amd.policy import MLPPolicy, SAC_ROWS_STREAM
    fn = MLPPolicy.normals_float32 if f32 else MLPPolicy.normals_reference
    return fn(ACTOR_SEED, row_offset + np.arange(n), t, n_u, slot=SAC_ROWS_STREAM)


def networks(env, hidden):
    am = SB().sac_mlp(env.n_obs, env.n_u, hidden, "relu", seed=11)
    qm = SB().q_mlp(env.n_obs, env.n_u, hidden, "relu", seed=12)
    return am, qm, env.make_sac_actor(am, seed=ACTOR_SEED), env.make_q(qm)


# ------------------------------------------------------------------------------------------ the sample
@pytest.mark.parametrize("case", CASES, ids=ids)
def test_sample_is_the_targets_draw_bit_for_bit(case):
    """a and logp of dockauv_sac_actor_forward_rows + dockauv_sac_sample are the a2 and logp2 dockauv_sac_target writes for the same
    rows, t and row_offset, at every B: dense, and with the rows scattered over records of another stride behind an index.
    Another t gives other normals; two calls give the same bits."""
    import torch
    (n_obs, n_u), hidden = case
    env = S().sac_env(n_obs, n_u, 64)
    try:
        am, qm, actor, q = networks(env, hidden)
        gen = torch.Generator(device="cuda")
        gen.manual_seed(3)
        for B in ROW_COUNTS:
            t, off = 5 + B, 1000 * B
            obs = (torch.rand((B, n_obs), device="cuda", generator=gen) * 2 - 1).contiguous()
            rd = torch.zeros((B,), device="cuda")
            R, slots = n_obs + 3, 2 * B + 7
            perm = torch.randperm(slots, device="cuda", generator=gen)[:B].contiguous()
            ring = torch.full((slots, R), float("nan"), device="cuda")
            ring[perm, :n_obs] = obs
            ring[perm, n_obs:n_obs + 2] = 0.0
            for index in (None, perm):
                rows, stride = (obs, n_obs) if index is None else (ring, R)
                iptr = 0 if index is None else index.data_ptr()
                hb, heads = B_().guarded(torch, B * 2 * n_u)
                env.batch.sac_actor_forward_rows_device(actor, rows.data_ptr(), B, heads.data_ptr(), row_stride=stride, index_ptr=iptr, stream=stream())
                heads = heads.view(B, 2 * n_u)
                a, logp = run_sample(torch, env, actor, heads, t, off)
                o = {k: torch.zeros((B,) + s, device="cuda") for k, s in (("a2", (n_u,)), ("logp2", ()), ("q1", ()), ("q2", ()), ("y", ()))}
                rew, done, cs = (rd, rd, 1) if index is None else (ring[:, n_obs], ring[:, n_obs + 1], R)
                env.batch.sac_target_device(actor, q, q, rows.data_ptr(), rew.data_ptr(), done.data_ptr(), B, 0.99, o["a2"].data_ptr(),
                                            o["logp2"].data_ptr(), o["q1"].data_ptr(), o["q2"].data_ptr(), o["y"].data_ptr(), ent_coef=0.2,
                                            t=t, row_offset=off, next_obs_stride=stride, column_stride=cs, index_ptr=iptr, stream=stream())
                torch.cuda.synchronize()
                assert not bool(torch.isnan(a).any()) and not bool(torch.isnan(logp).any())
                assert torch.equal(bits(a), bits(o["a2"])), (B, index is None, "a differs from the target's a2")
                assert torch.equal(bits(logp), bits(o["logp2"])), (B, index is None, "logp differs from the target's logp2")
            a_again, logp_again = run_sample(torch, env, actor, heads, t, off)
            assert torch.equal(bits(a), bits(a_again)) and torch.equal(bits(logp), bits(logp_again)), "two calls differ"
            a_other, _ = run_sample(torch, env, actor, heads, t + 1, off)
            assert not torch.equal(bits(a), bits(a_other)), "another t gave the same normals"
            a_wrap, _ = run_sample(torch, env, actor, heads, t + 2 ** 32, off + 2 ** 32)
            assert torch.equal(bits(a), bits(a_wrap)), "the counter takes t and row_offset + i mod 2^32"
            if B == 129:
                # rows 40 .. 72 alone at their row_offset: a row's draw is its counter's, not its position's in the launch
                a_part, lp_part = run_sample(torch, env, actor, heads[40:73].contiguous(), t, off + 40)
                assert torch.equal(bits(a_part), bits(a[40:73])) and torch.equal(bits(lp_part), bits(logp[40:73]))
                # the torch wrapper is the same call
                wa, wl = env.sac_sample(actor, heads.contiguous(), t, row_offset=off)
                torch.cuda.synchronize()
                assert torch.equal(bits(wa), bits(a)) and torch.equal(bits(wl), bits(logp))
    finally:
        env.close()


# ------------------------------------------------------------------------------------------ the critic head
@pytest.mark.parametrize("B", ROW_COUNTS)
def test_critic_head(B):
    """grad_q1 / grad_q2 are the float32 statement bit for bit (a subtraction and a division: exact IEEE); mse1 / mse2 within 1
    float32 ulp of the float64 mean of the float32 squares (non-negative terms: nothing cancels; one rounding of an exact-to-
    float64 sum); the means of q1, q2, y within 4 ulp of max |q|; critic_loss is 0.5f * (mse1 + mse2) of the device's own two;
    two calls give the same bits; the NaN around the inputs does not get in."""
    import torch
    from gym_dockauv_amd.policy import sac_critic_head_float32
    env = S().sac_env(20, 6, 64)
    try:
        _, _, _, q = networks(env, (17,))
        rng = np.random.default_rng(B)
        q1, q2, y = (rng.standard_normal(B).astype(np.float32) * np.float32(3) for _ in range(3))
        d = [in_nan(torch, x) for x in (q1, q2, y)]
        g1, g2, stats = run_critic_head(torch, env, q, *d)
        again = run_critic_head(torch, env, q, *d)
        for x, z in zip((g1, g2, stats), again):
            assert torch.equal(bits(x), bits(z)), "two calls differ"
        f1, f2, fs = sac_critic_head_float32(q1, q2, y)
        assert np.array_equal(g1.cpu().numpy().view(np.uint32), f1.view(np.uint32)), "grad_q1"
        assert np.array_equal(g2.cpu().numpy().view(np.uint32), f2.view(np.uint32)), "grad_q2"
        st = stats.cpu().numpy()
        assert not np.isnan(st).any()
        sq = [((x - y) * (x - y)).astype(np.float64).mean() for x in (q1, q2)]
        for k, want in ((1, sq[0]), (2, sq[1])):
            print(f"critic head B={B} mse{k}: device {st[k]:.9g}, float64 {want:.17g}, ulp {ulp32(want):.3e}")
            assert abs(float(st[k]) - want) <= ulp32(want), (k, st[k], want)
        assert st[0] == np.float32(0.5) * (st[1] + st[2])
        scale = max(float(np.abs(x).max()) for x in (q1, q2, y))
        for k, x in ((3, q1), (4, q2), (5, y)):
            want = x.astype(np.float64).mean()
            print(f"critic head B={B} mean {k}: device {st[k]:.9g}, float64 {want:.17g}, 4 ulp of max |q| {4 * ulp32(scale):.3e}")
            assert abs(float(st[k]) - want) <= 4 * ulp32(scale)
        if B == 129:
            w1, w2, ws = env.sac_critic_head(q, d[0], d[1], d[2])
            torch.cuda.synchronize()
            assert torch.equal(bits(w1), bits(g1)) and torch.equal(bits(w2), bits(g2)) and torch.equal(bits(ws), bits(stats))
    finally:
        env.close()


# ------------------------------------------------------------------------------------------ the actor head
def actor_head_case(env, actor, B, t=9, row_offset=70, ent_coef=0.2, label=None):
    """dockauv_sac_actor_head on crafted heads at B rows: (rows of compare_named(), what the checks behind need)"""
    import torch
    from gym_dockauv_amd.policy import sac_actor_head_float32, sac_actor_head_reference
    n_u = env.n_u
    rng = np.random.default_rng(1000 * n_u + B)
    heads = HH().crafted_heads(rng, B, n_u)
    q1, q2 = (rng.standard_normal(B).astype(np.float32) for _ in range(2))
    tie = B // 2
    q2[tie] = q1[tie]
    dq1, dq2 = (rng.standard_normal((B, n_u)).astype(np.float32) for _ in range(2))
    dev = [in_nan(torch, x) for x in (heads, q1, q2, dq1, dq2)]
    g, stats = run_actor_head(torch, env, actor, *dev, t, row_offset, ent_coef=ent_coef)
    z64, z32 = rows_normals(B, t, n_u, row_offset), rows_normals(B, t, n_u, row_offset, f32=True)
    r_g, r_s, _, _ = sac_actor_head_reference(heads, z64, q1, q2, dq1, dq2, ent_coef=ent_coef)
    f_g, f_s, _, _ = sac_actor_head_float32(heads, z32, q1, q2, dq1, dq2, ent_coef=ent_coef)
    gh, sh = g.cpu().numpy(), stats.cpu().numpy()
    label = label or f"n_u {n_u} rows {B}"
    rows = SB().compare_named(["d mu", "d raw log-std", "actor_loss", "mean logp"],
                              [gh[:, :n_u], gh[:, n_u:], sh[0:1], sh[1:2]], [f_g[:, :n_u], f_g[:, n_u:], f_s[0:1], f_s[1:2]],
                              [r_g[:, :n_u], r_g[:, n_u:], r_s[0:1], r_s[1:2]], "actor head " + label)
    return rows, dict(heads=heads, q1=q1, q2=q2, dq1=dq1, dq2=dq2, dev=dev, g=g, stats=stats, z64=z64, tie=tie, r_s=r_s)


@pytest.mark.parametrize("case", CASES, ids=ids)
def test_actor_head(case):
    """Against float64 under the project's bound at every B; entries of the raw log-std gradient outside the clamp are exact 0.0f, on
    both edges they are not; the row with q1_pi == q2_pi takes dq1; |x| reaches 12, where s underflows against the 1e-6;
    log_ent_coef = 0 gives exactly the bits of ent_coef = 1.0f; two calls give the same bits; mean min q within 4 ulp of max |q|."""
    import torch
    (n_obs, n_u), hidden = case
    env = S().sac_env(n_obs, n_u, 64)
    try:
        _, _, actor, _ = networks(env, hidden)
        for B in ROW_COUNTS:
            rows, c = actor_head_case(env, actor, B)
            SB().assert_within(rows, (n_u, B))
            raw = c["heads"][:, n_u:]
            g_ls = c["g"].cpu().numpy()[:, n_u:]
            outside = (raw < -20) | (raw > 2)
            assert (g_ls[outside].view(np.uint32) == 0).all(), "outside the clamp the gradient must be exactly +0.0f"
            assert (g_ls[~outside] != 0).all(), "inside the clamp, both edges included, the gradient is not zero"
            if B >= 33:
                for cond, what in ((raw < -20, "below -20"), (raw > 2, "above 2"), (raw == -20, "exactly -20"), (raw == 2, "exactly 2"),
                                   ((raw > -20) & (raw < 2), "inside")):
                    assert cond.any(axis=0).all(), f"not every column holds a raw log-std {what}"
                x = c["heads"][:, :n_u] + np.exp(np.clip(raw, -20, 2).astype(np.float64)) * c["z64"]
                assert float(np.abs(x).max()) >= 12.0
            st = c["stats"].cpu().numpy()
            assert st[3] == np.float32(0.2)
            mq = np.minimum(c["q1"], c["q2"]).astype(np.float64).mean()
            assert abs(float(st[2]) - mq) <= 4 * ulp32(max(np.abs(c["q1"]).max(), np.abs(c["q2"]).max()))
            again = run_actor_head(torch, env, actor, *c["dev"], 9, 70, ent_coef=0.2)
            assert torch.equal(bits(again[0]), bits(c["g"])) and torch.equal(bits(again[1]), bits(c["stats"])), "two calls differ"
            # the tie: the row's gradient is that of q1 < q2 (dq1), and not that of q2 < q1
            tie = c["tie"]
            for shift, same in ((1.0, True), (-1.0, False)):
                q2s = c["q2"].copy()
                q2s[tie] += np.float32(shift)
                gs, _ = run_actor_head(torch, env, actor, c["dev"][0], c["dev"][1], in_nan(torch, q2s), c["dev"][3], c["dev"][4], 9, 70, ent_coef=0.2)
                assert torch.equal(bits(gs[tie]), bits(c["g"][tie])) == same, "a tie must take dq1"
            # log_ent_coef = 0 is ent_coef = 1.0f
            one = run_actor_head(torch, env, actor, *c["dev"], 9, 70, ent_coef=1.0)
            zero = run_actor_head(torch, env, actor, *c["dev"], 9, 70, log_ent_coef=torch.zeros(1, device="cuda"))
            assert torch.equal(bits(one[0]), bits(zero[0])) and torch.equal(bits(one[1]), bits(zero[1]))
            assert float(one[1][3]) == 1.0 and not torch.equal(bits(one[0]), bits(c["g"]))
            if B == 129:
                wg, ws = env.sac_actor_head(actor, c["dev"][0], 9, c["dev"][1], c["dev"][2], c["dev"][3], c["dev"][4], ent_coef=0.2, row_offset=70)
                torch.cuda.synchronize()
                assert torch.equal(bits(wg), bits(c["g"])) and torch.equal(bits(ws), bits(c["stats"]))
                # logp is the sample's: its mean, formed on the host as the kernel forms it, is stats[1] bit for bit
                _, logp = run_sample(torch, env, actor, c["dev"][0], 9, 70)
                lp = logp.cpu().numpy()
                assert abs(int(np.float32(lp.astype(np.float64).sum() / B).view(np.uint32)) - int(st[1].view(np.uint32))) <= 1
    finally:
        env.close()


# ------------------------------------------------------------------------------------------ the entropy coefficient
@pytest.mark.parametrize("init", [1.0, 0.1])
def test_ent_coef_three_chained_steps(init):
    """state and before are the float32 statement bit for bit given the device's own mean (stats[2]); that mean is within 1 ulp of
    the float64 mean of the float32 terms (logp in (-5, -1), target_entropy -6: all terms negative, nothing cancels); stats[1] is
    expf(log_ent_coef before) to one bit, stats[0] = -(p_before * mean) and stats[3] the new p, exactly.  B = 129, 1 324 and 1."""
    import torch
    from gym_dockauv_amd.policy import ent_coef_step_float32
    env = S().sac_env(20, 6, 64)
    try:
        lr, target = 3e-3, -6.0
        state = env.ent_coef_state(init)
        torch.cuda.synchronize()
        want = np.array([np.log(init), 0, 0], dtype=np.float32)
        assert np.array_equal(state.cpu().numpy().view(np.uint32), want.view(np.uint32))
        rng = np.random.default_rng(int(init * 10))
        for step, B in ((1, 129), (2, 1324), (3, 1)):
            logp = rng.uniform(-5.0, -1.0, B).astype(np.float32)
            d_logp = in_nan(torch, logp)
            new, before, stats = run_ent_coef_step(torch, env, state, d_logp, step, lr, target)
            again = run_ent_coef_step(torch, env, state, d_logp, step, lr, target)
            for x, z in zip((new, before, stats), again):
                assert torch.equal(bits(x), bits(z)), "two calls differ"
            st, s0 = stats.cpu().numpy(), state.cpu().numpy()
            assert before.cpu().numpy().view(np.uint32)[0] == s0.view(np.uint32)[0], "before is not log_ent_coef as it was"
            mean64 = (logp + np.float32(target)).astype(np.float64).mean()
            print(f"ent_coef step {step} B={B}: mean device {st[2]:.9g}, float64 {mean64:.17g}, ulp {ulp32(mean64):.3e}")
            assert abs(float(st[2]) - mean64) <= ulp32(mean64)
            f_state, f_loss = ent_coef_step_float32(s0, st[2], step, lr)
            assert np.array_equal(new.cpu().numpy().view(np.uint32), f_state.view(np.uint32)), (step, new.cpu().numpy(), f_state)
            assert st[0].view(np.uint32) == np.float32(f_loss).view(np.uint32) and st[3].view(np.uint32) == f_state[0].view(np.uint32)
            e = np.float32(np.exp(np.float64(s0[0])))
            assert st[1] in (np.nextafter(e, np.float32(0)), e, np.nextafter(e, np.float32(np.inf))), (st[1], e)
            if step == 2:
                # the torch wrapper is the same call, in place
                s2, b2 = state.clone(), torch.zeros(1, device="cuda")
                ws = env.ent_coef_step(s2, d_logp, step, lr, target_entropy=target, before=b2)
                torch.cuda.synchronize()
                assert torch.equal(bits(s2), bits(new)) and torch.equal(bits(ws), bits(stats)) and torch.equal(bits(b2), bits(before))
            state = new
        assert float(state[0]) < np.log(init), "logp + target_entropy < 0 everywhere (more entropy than the target): the coefficient shrinks"
    finally:
        env.close()


# ------------------------------------------------------------------------------------------ refusals
def test_refusals_on_a_live_handle():
    """A plain actor, a value critic and a Q critic as `actor` are each refused by dockauv_sac_sample and dockauv_sac_actor_head, a
    squashed-Gaussian actor (and the two others) as `q1_critic` by dockauv_sac_critic_head; objects of another handle are refused;
    the overlap of grad_out with dq at the handle's n_u is refused; the good calls go through and allocate none of the
    backward's workspace."""
    import torch
    from gym_dockauv_amd import _capi
    lib = _capi.load_library()
    n_obs, n_u, n = 20, 6, 64
    env, other = S().sac_env(n_obs, n_u, 64), S().sac_env(n_obs, n_u, 64)
    try:
        am, qm = SB().sac_mlp(n_obs, n_u, (64, 64), "relu"), SB().q_mlp(n_obs, n_u, (64, 64), "relu")
        plain = env.make_policy(SB().P().make_mlp((n_obs, (64, 64), n_u, "tanh", "none"), seed=1))
        value = env.make_value(SB().P().make_mlp((n_obs, (64, 64), 1, "tanh", "none"), seed=1))
        actor, q, foreign_a, foreign_q = env.make_sac_actor(am), env.make_q(qm), other.make_sac_actor(am), other.make_q(qm)
        z = lambda *s: torch.zeros(s, device="cuda")
        heads, a, logp, q1, q2, y, g1, g2 = z(n, 2 * n_u), z(n, n_u), z(n), z(n), z(n), z(n), z(n), z(n)
        dq = z(2 * n * n_u)              # dq1 | dq2
        grad_out, st6, st4 = z(n, 2 * n_u), z(6), z(4)
        err = lambda: lib.dockauv_last_error(env.batch._handle)

        def sample(p):
            io = _capi.SacSampleIO()
            io.struct_size, io.n_rows, io.heads, io.a, io.logp = C.sizeof(io), n, heads.data_ptr(), a.data_ptr(), logp.data_ptr()
            return lib.dockauv_sac_sample(env.batch._handle, p.ptr, C.byref(io), None), err()

        def critic_head(p):
            io = _capi.SacCriticHeadIO()
            io.struct_size, io.n_rows, io.q1, io.q2, io.y = C.sizeof(io), n, q1.data_ptr(), q2.data_ptr(), y.data_ptr()
            io.grad_q1, io.grad_q2, io.stats = g1.data_ptr(), g2.data_ptr(), st6.data_ptr()
            return lib.dockauv_sac_critic_head(env.batch._handle, p.ptr, C.byref(io), None), err()

        def actor_head(p, grad_out_ptr=None):
            io = _capi.SacActorHeadIO()
            io.struct_size, io.n_rows, io.ent_coef, io.heads = C.sizeof(io), n, 0.2, heads.data_ptr()
            io.q1_pi, io.q2_pi, io.dq1, io.dq2 = q1.data_ptr(), q2.data_ptr(), dq.data_ptr(), dq.data_ptr() + 4 * n * n_u
            io.grad_out, io.stats = grad_out_ptr or grad_out.data_ptr(), st4.data_ptr()
            return lib.dockauv_sac_actor_head(env.batch._handle, p.ptr, C.byref(io), None), err()

        roles = {"plain actor": plain, "value critic": value, "Q critic": q, "squashed-Gaussian actor": actor}
        for call, own in ((sample, actor), (actor_head, actor), (critic_head, q)):
            for name, p in roles.items():
                if p is own:
                    continue
                rc, msg = call(p)
                assert rc == -1 and b"the policy is a " + name.encode() in msg, (call.__name__, name, rc, msg)
            rc, msg = call(own)
            assert rc == 0, (call.__name__, rc, msg)
        for call, p in ((sample, foreign_a), (actor_head, foreign_a), (critic_head, foreign_q)):
            rc, msg = call(p)
            assert rc == -1 and b"another handle" in msg, (rc, msg)
        # grad_out [n][2 n_u] one row of dq2 in front of dq2's end: clear at one action a row, an overlap at the handle's six
        rc, msg = actor_head(actor, grad_out_ptr=dq.data_ptr() + 4 * (2 * n * n_u - n_u))
        assert rc == -1 and b"dockauv_sac_actor_head_io.grad_out overlaps dq" in msg, (rc, msg)
        torch.cuda.synchronize()
        assert env.batch.backward_workspace(actor) == (0, 0) and env.batch.backward_workspace(q) == (0, 0)
    finally:
        env.close()
        other.close()


# ------------------------------------------------------------------------------------------ sac_gradients end to end
def device_rows_normals(torch, env, actor, B, t, row_offset=0):
    """The normals the rows form draws, from the device itself: with heads = 0 (mu 0, std 1), alpha = 0 and dq = 1 the actor head
    writes d mu = gx = -s / B and d raw log-std = fmaf(gx, z, -0) = gx z rounded once, so z = their quotient to 2^-24 relative."""
    n_u = env.n_u
    zf = lambda *s: torch.zeros(s, device="cuda")
    g, _ = run_actor_head(torch, env, actor, zf(B, 2 * n_u), zf(B), zf(B), torch.ones((B, n_u), device="cuda"), torch.ones((B, n_u), device="cuda"),
                          t, row_offset, ent_coef=0.0)
    g = g.cpu().numpy().astype(np.float64)
    assert (g[:, :n_u] < 0).all()
    return g[:, n_u:] / g[:, :n_u]


def test_sac_gradients_end_to_end():
    """B = 129 on the (20, 6) env, 64-64 relu: sac_gradients on ReplaySamples (and, bit for bit, on the same rows behind an index in
    a replay ring) against sac_losses / reference_gradients of tests/test_gpu_sac_backward.py in float64 on the CPU with the device's
    normals and the device's y: every parameter gradient of the three networks, grad_out (d mu, d raw log-std) and the ent_coef
    gradient -mean(logp + target_entropy) from ent_coef_step's stats, under the project's bound with e32 from the same graph in
    float32 torch.  Row rules as there: MIN_GAP on |q1 - q2| at the sampled action, draw_rows' ReLU margin on every hidden
    pre-activation, the clamp inactive; the row of position p is the next candidate that passes them with position p's normals,
    so all 129 positions are filled."""
    import torch
    from gym_dockauv_amd.replay import ReplaySamples
    n_obs, n_u, hidden, want, t = 20, 6, (64, 64), 129, 4
    am = SB().sac_mlp(n_obs, n_u, hidden, "relu", seed=11)
    qms = [SB().q_mlp(n_obs, n_u, hidden, "relu", seed=12), SB().q_mlp(n_obs, n_u, hidden, "relu", seed=13)]
    tms = [SB().q_mlp(n_obs, n_u, hidden, "relu", seed=14), SB().q_mlp(n_obs, n_u, hidden, "relu", seed=15)]
    rng = np.random.default_rng(17)
    cand = want + 64
    obs, act = rng.uniform(-1, 1, (cand, n_obs)).astype(np.float32), rng.uniform(-1, 1, (cand, n_u)).astype(np.float32)
    nxt, rew = rng.uniform(-1, 1, (cand, n_obs)).astype(np.float32), rng.standard_normal((cand, 1)).astype(np.float32)
    done = (rng.uniform(size=(cand, 1)) < 0.2).astype(np.float32)

    env = S().sac_env(n_obs, n_u, 64)
    try:
        actor = env.make_sac_actor(am, seed=ACTOR_SEED)
        q1, q2, q1t, q2t = (env.make_q(m) for m in qms + tms)
        z = device_rows_normals(torch, env, actor, want, 2 * t + 1)
        assert np.abs(z - rows_normals(want, 2 * t + 1, n_u)).max() <= SB().P().EXPLORATION_CAP, "the recovered normals are not the Philox statement's"

        def pre_ok(layers, x):
            for W, b in layers:
                pre = x @ W.astype(np.float64).T + b.astype(np.float64)
                if (np.abs(pre) < B_().RELU_MARGIN).any():
                    return False
                x = np.maximum(pre, 0.0)
            return True

        def row_ok(c, zp):
            o64, a64 = obs[c:c + 1].astype(np.float64), act[c:c + 1].astype(np.float64)
            a_pi, _, _, ls64 = am.forward_reference(o64, zp[None, :])
            heads = am.heads_reference(o64)
            if not pre_ok(am.layers, o64) or not (np.abs(heads[:, n_u:]) < 2.0 - 1e-3).all():
                return False
            qp = []
            for qm in qms:
                if not pre_ok(qm.layers[:-1], np.concatenate([o64, a64], axis=1)) or not pre_ok(qm.layers[:-1], np.concatenate([o64, a_pi], axis=1)):
                    return False
                qp.append(float(qm.forward_reference(np.concatenate([o64, a_pi], axis=1))[0, 0]))
            return abs(qp[0] - qp[1]) >= SB().MIN_GAP

        idx, c = [], 0
        for p in range(want):
            while c < cand and not row_ok(c, z[p]):
                c += 1
            assert c < cand, (p, "ran out of candidate rows off every kink")
            idx.append(c)
            c += 1
        idx = np.array(idx)
        dev = lambda x: torch.from_numpy(np.ascontiguousarray(x[idx])).cuda().contiguous()
        sm = ReplaySamples(dev(obs), dev(act), dev(nxt), dev(done), dev(rew))

        state = env.ent_coef_state(0.2)
        g = env.sac_gradients(actor, q1, q2, q1t, q2t, sm, 0.99, t, log_ent_coef=state[:1])
        ent_stats = env.ent_coef_step(state.clone(), g.logp, 1, 3e-4)
        torch.cuda.synchronize()
        # the target's draw is dockauv_sac_target's at counter 2 t, the sample's at 2 t + 1
        keep = {k: v.clone() for k, v in (("logp", g.logp), ("grad_out", g.grad_out), ("y", g.y), ("critic_stats", g.critic_stats), ("actor_stats", g.actor_stats))}
        y_alone = env.sac_target(actor, q1t, q2t, sm, 0.99, log_ent_coef=state[:1], t=2 * t).clone().view(-1)
        heads = env.sac_actor_heads(actor, sm.observations)
        a_alone, logp_alone = env.sac_sample(actor, heads, 2 * t + 1)
        torch.cuda.synchronize()
        assert torch.equal(bits(y_alone), bits(keep["y"])) and torch.equal(bits(logp_alone), bits(keep["logp"]))

        data = dict(obs=sm.observations.cpu(), act=sm.actions.cpu(), y=keep["y"].cpu(), z=torch.from_numpy(z))
        ref, _, a_ref = SB().reference_gradients(torch, am, qms, data, torch.float64, "cpu", n_u)
        f32, _, _ = SB().reference_gradients(torch, am, qms, data, torch.float32, "cuda", n_u)
        q_pi = [qm.forward_reference(np.concatenate([data["obs"].numpy().astype(np.float64), a_ref.numpy()], axis=1))[:, 0] for qm in qms]
        assert 0.05 < float((q_pi[0] < q_pi[1]).mean()) < 0.95, "both critics must be the minimum on some rows"
        drop = lambda xs: xs[:20] + xs[20:22] + xs[23:]          # (reference_gradients' "d action" has no counterpart here)
        got = list(g.q1) + list(g.q2) + list(g.actor) + [keep["grad_out"][:, :n_u], keep["grad_out"][:, n_u:], -ent_stats[2:3]]
        got = [x.detach().cpu().numpy().astype(np.float64) for x in got]
        names = [f"q{i}.{n}" for i in (1, 2) for n in ("W1", "b1", "W2", "b2", "W3", "b3")]
        names += [f"actor.{n}" for n in ("W1", "b1", "W2", "b2", "W_mu", "b_mu", "W_ls", "b_ls")] + ["d mu", "d log_std", "log_ent_coef"]
        ref, f32 = drop(ref), drop(f32)
        assert len(got) == len(ref) == len(f32) == len(names) == 23
        rows = RECORD["sac_gradients_B129"] = SB().compare_named(names, got, f32, ref, "sac_gradients B=129")
        SB().assert_within(rows, "sac_gradients")

        # the same rows behind an index in a replay ring: the same bits; and a second call reuses the buffers
        rb = env.make_replay_buffer(8 * 64, seed=5)
        ring = rb.storage.view(-1, rb.record_floats)
        gen = torch.Generator(device="cuda")
        gen.manual_seed(2)
        perm = torch.randperm(ring.shape[0], device="cuda", generator=gen)[:want].contiguous()
        ring.fill_(float("nan"))
        o3 = 2 * n_obs + n_u
        ring[perm, :n_obs], ring[perm, n_obs:2 * n_obs], ring[perm, 2 * n_obs:o3] = sm.observations, sm.next_observations, sm.actions
        ring[perm, o3], ring[perm, o3 + 1], ring[perm, o3 + 2] = sm.rewards[:, 0], sm.dones[:, 0], 0.0
        rb.index, rb.last_samples = perm, sm
        g2 = env.sac_gradients(actor, q1, q2, q1t, q2t, rb, 0.99, t, log_ent_coef=state[:1], out=(g.q1, g.q2, g.actor))
        torch.cuda.synchronize()
        assert g2.logp.data_ptr() == g.logp.data_ptr() and g2.q1[0].data_ptr() == g.q1[0].data_ptr()
        for k in keep:
            assert torch.equal(bits(getattr(g2, k)), bits(keep[k])), f"{k} through the ring differs"
        for x, w in zip(list(g2.q1) + list(g2.q2) + list(g2.actor), got[:20]):
            assert np.array_equal(x.cpu().numpy().astype(np.float64), w), "a gradient through the ring differs"
    finally:
        env.close()
