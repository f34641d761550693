"""CPU: the surface of SAC's loss head and its statements (include/dockauv.h: dockauv_sac_sample, dockauv_sac_critic_head,
dockauv_sac_actor_head, dockauv_sac_ent_coef_step; gym_dockauv_amd/policy.py: sac_critic_head_reference, sac_actor_head_reference,
ent_coef_step_reference and their float32 restatements).  The four symbols are declared, bound once and exported and the ABI is
still 3; the four io structs have the layout of their ctypes mirrors; every refusal that needs no live handle fires with a NULL
handle and pointers that are never dereferenced, the field named (roles and foreign handles: tests/test_gpu_sac_head.py); the
float64 statements are float64 torch autograd on SB3's formulas as they are written -- Normal(mu, std).log_prob(x),
log(1 - a^2 + 1e-6), torch.min, clamp; mse_loss; torch.optim.Adam on one scalar over three steps -- and the float32 restatements
stay within float32's reach of them.

Bounds.  Statement against autograd: both sides are float64 evaluations of the same formulas, so they agree to float64 rounding;
1e-9 relative to the largest entry leaves room for the cancellation of 1 - a^2 against the 1e-6 (an absolute error of 1e-16 in
1 - a^2 over 1e-6 is 1e-10).  Restatement against statement: FORWARD_BOUND = 1e-5 relative to the largest entry, the project's
float32 bar (tests/test_gpu_policy.py): every output is a chain of a few dozen float32 operations (2^-24 = 6e-8 each) through
exp, tanh and log at arguments of a few units."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dockauv.h")

NEW_SYMBOLS = ["dockauv_sac_sample", "dockauv_sac_critic_head", "dockauv_sac_actor_head", "dockauv_sac_ent_coef_step"]
NEW_STRUCTS = {"dockauv_sac_sample_io": "SacSampleIO", "dockauv_sac_critic_head_io": "SacCriticHeadIO",
               "dockauv_sac_actor_head_io": "SacActorHeadIO", "dockauv_sac_ent_coef_io": "SacEntCoefIO"}
RTOL = 1e-9
FORWARD_BOUND = 1e-5


@pytest.fixture(scope="module")
def lib():
    from gym_dockauv_amd.csrc import build
    build.build()
    from gym_dockauv_amd import _capi
    return _capi.load_library()


def test_symbols_declared_bound_and_exported(lib):
    from gym_dockauv_amd import _capi
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(dockauv_[a-z0-9_]+)\s*\(", text))
    bound = [s[0] for s in _capi.SYMBOLS]
    for n in NEW_SYMBOLS:
        assert n in declared and bound.count(n) == 1 and hasattr(lib, n), n
    assert declared == set(bound), "header and binding declare different symbols"
    for s in NEW_STRUCTS:
        assert re.search(rf"typedef\s+struct\s+{s}\b", text), s
    assert _capi.ABI_VERSION == 3 and lib.dockauv_abi_version() == 3
    assert re.search(r"#define\s+DOCKAUV_ABI_VERSION\s+3\b", text)
    assert "dockauv_sac_head.hip" in open(os.path.join(ROOT, "gym_dockauv_amd", "csrc", "build.py")).read()


def test_struct_layouts_match_c(tmp_path):
    from gym_dockauv_amd import _capi
    items, want = [], []
    for cname, pyname in NEW_STRUCTS.items():
        mirror = getattr(_capi, pyname)
        items.append(f"sizeof({cname})")
        want.append(C.sizeof(mirror))
        for f in mirror._fields_:
            items.append(f"offsetof({cname}, {f[0]})")
            want.append(getattr(mirror, f[0]).offset)
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(void) {\n%s  return 0;\n}\n'
                   % (HEADER, "".join(f'  printf("%zu\\n", (size_t){it});\n' for it in items)))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-o", str(exe), str(src)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    assert got == want


def test_io_blocks_refused_before_any_device_call(lib):
    from gym_dockauv_amd import _capi
    fake = C.c_void_p(8)          # never dereferenced: something else is refused first
    err = lambda: lib.dockauv_last_error(None)
    # fake arrays far enough apart not to overlap at 4 rows of at most 16 floats
    addr = lambda k: 4096 * (k + 1)

    def sample_io(change, needle):
        io = _capi.SacSampleIO()
        io.struct_size, io.n_rows, io.heads, io.a, io.logp = C.sizeof(io), 4, addr(0), addr(1), addr(2)
        change(io)
        rc = lib.dockauv_sac_sample(None, fake, C.byref(io), None)
        assert rc == -1 and needle in err(), (needle, rc, err())

    sample_io(lambda io: setattr(io, "struct_size", 8), b"dockauv_sac_sample_io.struct_size")
    sample_io(lambda io: setattr(io, "n_rows", 0), b"dockauv_sac_sample_io.n_rows")
    sample_io(lambda io: setattr(io, "n_rows", -2), b"dockauv_sac_sample_io.n_rows")
    for f in ("heads", "a", "logp"):
        sample_io(lambda io, f=f: setattr(io, f, None), b"dockauv_sac_sample_io." + f.encode() + b" is NULL")
    sample_io(lambda io: None, b"null handle")          # a valid block gets as far as the handle
    assert lib.dockauv_sac_sample(None, None, None, None) == -1 and b"io is NULL" in err()
    io = _capi.SacSampleIO()
    io.struct_size, io.n_rows, io.heads, io.a, io.logp = C.sizeof(io), 4, addr(0), addr(1), addr(2)
    assert lib.dockauv_sac_sample(None, None, C.byref(io), None) == -1 and b"null actor" in err()

    def critic_io(change, needle, policy=fake):
        io = _capi.SacCriticHeadIO()
        io.struct_size, io.n_rows = C.sizeof(io), 4
        for k, f in enumerate(("q1", "q2", "y", "grad_q1", "grad_q2", "stats")):
            setattr(io, f, addr(k))
        change(io)
        rc = lib.dockauv_sac_critic_head(None, policy, C.byref(io), None)
        assert rc == -1 and needle in err(), (needle, rc, err())

    critic_io(lambda io: setattr(io, "struct_size", 16), b"dockauv_sac_critic_head_io.struct_size")
    critic_io(lambda io: setattr(io, "n_rows", 0), b"dockauv_sac_critic_head_io.n_rows")
    for f in ("q1", "q2", "y", "grad_q1", "grad_q2", "stats"):
        critic_io(lambda io, f=f: setattr(io, f, None), b"dockauv_sac_critic_head_io." + f.encode() + b" is NULL")
    critic_io(lambda io: setattr(io, "grad_q1", io.q1), b"dockauv_sac_critic_head_io.grad_q1 overlaps q1")
    critic_io(lambda io: setattr(io, "grad_q2", io.y + 12), b"dockauv_sac_critic_head_io.grad_q2 overlaps y")      # the last float
    critic_io(lambda io: setattr(io, "grad_q2", io.y + 16), b"null handle")                                       # just behind it
    critic_io(lambda io: setattr(io, "stats", io.q2 - 20), b"dockauv_sac_critic_head_io.stats overlaps q2")       # stats [6] reaches in
    critic_io(lambda io: setattr(io, "grad_q2", io.grad_q1), b"dockauv_sac_critic_head_io.grad_q1 overlaps grad_q2")
    critic_io(lambda io: None, b"null handle")
    critic_io(lambda io: None, b"null critic", policy=None)
    assert lib.dockauv_sac_critic_head(None, None, None, None) == -1 and b"io is NULL" in err()

    def actor_io(change, needle, policy=fake):
        io = _capi.SacActorHeadIO()
        io.struct_size, io.n_rows, io.ent_coef = C.sizeof(io), 4, 0.2
        for k, f in enumerate(("heads", "q1_pi", "q2_pi", "dq1", "dq2", "grad_out", "stats")):
            setattr(io, f, addr(k))
        change(io)
        rc = lib.dockauv_sac_actor_head(None, policy, C.byref(io), None)
        assert rc == -1 and needle in err(), (needle, rc, err())

    actor_io(lambda io: setattr(io, "struct_size", 16), b"dockauv_sac_actor_head_io.struct_size")
    actor_io(lambda io: setattr(io, "n_rows", 0), b"dockauv_sac_actor_head_io.n_rows")
    actor_io(lambda io: setattr(io, "ent_coef", float("nan")), b"dockauv_sac_actor_head_io.ent_coef is NaN")
    actor_io(lambda io: (setattr(io, "ent_coef", float("nan")), setattr(io, "log_ent_coef", addr(9))), b"null handle")   # (unread then)
    for f in ("heads", "q1_pi", "q2_pi", "dq1", "dq2", "grad_out", "stats"):
        actor_io(lambda io, f=f: setattr(io, f, None), b"dockauv_sac_actor_head_io." + f.encode() + b" is NULL")
    actor_io(lambda io: setattr(io, "grad_out", io.heads), b"dockauv_sac_actor_head_io.grad_out overlaps heads")
    actor_io(lambda io: setattr(io, "grad_out", io.dq2), b"dockauv_sac_actor_head_io.grad_out overlaps dq2")
    actor_io(lambda io: setattr(io, "stats", io.q1_pi), b"dockauv_sac_actor_head_io.stats overlaps q1_pi")
    actor_io(lambda io: (setattr(io, "log_ent_coef", addr(9)), setattr(io, "stats", addr(9))), b"dockauv_sac_actor_head_io.stats overlaps log_ent_coef")
    actor_io(lambda io: setattr(io, "stats", io.grad_out + 4), b"dockauv_sac_actor_head_io.grad_out overlaps stats")
    actor_io(lambda io: None, b"null handle")
    actor_io(lambda io: None, b"null actor", policy=None)
    assert lib.dockauv_sac_actor_head(None, None, None, None) == -1 and b"io is NULL" in err()

    def ent_io(change, needle):
        io = _capi.SacEntCoefIO()
        io.struct_size, io.n_rows, io.step, io.target_entropy = C.sizeof(io), 4, 1, -6.0
        io.lr, io.beta1, io.beta2, io.eps = 3e-4, 0.9, 0.999, 1e-8
        io.state, io.logp, io.before, io.stats = addr(0), addr(1), addr(2), addr(3)
        change(io)
        rc = lib.dockauv_sac_ent_coef_step(None, C.byref(io), None)
        assert rc == -1 and needle in err(), (needle, rc, err())

    ent_io(lambda io: setattr(io, "struct_size", 8), b"dockauv_sac_ent_coef_io.struct_size")
    ent_io(lambda io: setattr(io, "n_rows", 0), b"dockauv_sac_ent_coef_io.n_rows")
    ent_io(lambda io: setattr(io, "step", 0), b"dockauv_sac_ent_coef_io.step")
    for bad in (-1e-3, float("inf"), float("nan")):
        ent_io(lambda io, bad=bad: setattr(io, "lr", bad), b"dockauv_sac_ent_coef_io.lr")
    for f in ("beta1", "beta2"):
        for bad in (-0.1, 1.0, float("nan")):
            ent_io(lambda io, f=f, bad=bad: setattr(io, f, bad), b"dockauv_sac_ent_coef_io." + f.encode())
    for bad in (0.0, -1e-8, float("nan")):
        ent_io(lambda io, bad=bad: setattr(io, "eps", bad), b"dockauv_sac_ent_coef_io.eps")
    ent_io(lambda io: setattr(io, "state", None), b"dockauv_sac_ent_coef_io.state is NULL")
    ent_io(lambda io: setattr(io, "logp", None), b"dockauv_sac_ent_coef_io.logp is NULL")
    for off in (0, 4, 8):
        ent_io(lambda io, off=off: setattr(io, "before", io.state + off), b"dockauv_sac_ent_coef_io.before overlaps state")
    ent_io(lambda io: setattr(io, "before", io.state + 12), b"null handle")
    ent_io(lambda io: setattr(io, "stats", io.state - 4), b"dockauv_sac_ent_coef_io.stats overlaps state")
    ent_io(lambda io: (setattr(io, "before", None), setattr(io, "stats", None)), b"null handle")      # both are optional
    ent_io(lambda io: (setattr(io, "lr", 0.0), setattr(io, "beta1", 0.0)), b"null handle")            # the closed ends
    assert lib.dockauv_sac_ent_coef_step(None, None, None) == -1 and b"io is NULL" in err()


# ------------------------------------------------------------------------------------------ the statements
def _t(x, grad=False):
    import torch
    return torch.tensor(np.asarray(x), dtype=torch.float64, requires_grad=grad)


def _close(got, want, what, rtol=RTOL):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    scale = max(float(np.abs(want).max()), 1e-300)
    err = float(np.abs(got - want).max()) / scale
    print(f"{what}: max relative difference {err:.2e} (bound {rtol:g})")
    assert err <= rtol, (what, err)


def crafted_heads(rng, B, n_u, low_mu_zero=False):
    """heads [B, 2 n_u] float32 whose every raw log-std column holds values below -20, above 2, exactly -20.0 and 2.0, and inside
    (nine rows a column, B >= 9), and a row with |mu| = 12.5 and std = exp(-6), so that |x| passes 12 whatever z is.
    ``low_mu_zero``: mu = 0 wherever the log-std is -20 or a float32 step above it (see test_actor_head_statement_is_float64_autograd)."""
    mu = rng.uniform(-3.0, 3.0, (B, n_u))
    raw = rng.uniform(-6.0, 1.5, (B, n_u))
    for j in range(n_u):
        rows = rng.permutation(B)[:9] if B >= 9 else np.arange(B).repeat(9)[:9]
        for r, v in zip(rows, (-20.0, 2.0, -20.5, -31.0, 2.25, 7.0, np.nextafter(np.float32(-20.0), np.float32(0.0)),
                               np.nextafter(np.float32(2.0), np.float32(0.0)), -6.0)):
            raw[r, j] = v
        mu[rows[8], j] = 12.5 * (-1) ** j
    if low_mu_zero:
        mu[raw < -19.0] = 0.0
    return np.concatenate([mu, raw], axis=1).astype(np.float32)


def actor_case(n_u, B=65, seed=0, low_mu_zero=False):
    rng = np.random.default_rng(100 * n_u + seed)
    heads = crafted_heads(rng, B, n_u, low_mu_zero)
    z = rng.standard_normal((B, n_u))
    if low_mu_zero:
        z[heads[:, n_u:] < -19.0] *= 1e-3
    # two critics that are functions of the action: q_k(a) = c_k + a . w_k + 0.5 a^2 . v_k, so dq_k / da = w_k + a v_k
    cw = [(rng.standard_normal(B), rng.standard_normal((B, n_u)), rng.standard_normal((B, n_u))) for _ in range(2)]
    return heads, z, cw


@pytest.mark.parametrize("n_u", [3, 6, 8])
@pytest.mark.parametrize("alpha_as", ["ent_coef", "log_ent_coef"])
def test_actor_head_statement_is_float64_autograd(n_u, alpha_as):
    """sac_actor_head_reference against autograd through SB3's actor loss as it is written, rows with the raw log-std below -20,
    above 2 and exactly on both edges included.  Where the log-std is -20, clamped or one float32 step inside (std = 2e-9), the rows have mu = 0 and normals
    of a thousandth: autograd sends -(x - mu) / std^2 = -z / std, some 1e9 at |z| of a unit, into mu along two paths that cancel,
    and adds the rest of d loss / d x to the first before the second takes it away again -- an absolute error of an ulp of
    alpha z / (B std), 2e-10 against entries of 0.04 (measured: 2e-9 to 5e-9 relative), and with |mu| of a few units x - mu =
    (mu + std z) - mu loses eight digits on top.  That is the yardstick's error: the statement never forms either.  The mask and
    the edge at -20.0 are held on those rows all the same.  The GPU tests, whose yardstick is the statement, keep |mu| up to 3
    and unit normals there."""
    import torch
    from gym_dockauv_amd.policy import sac_actor_head_reference
    heads, z, cw = actor_case(n_u, low_mu_zero=True)
    B = heads.shape[0]
    raw = heads[:, n_u:]
    assert (raw < -20).any(axis=0).all() and (raw > 2).any(axis=0).all() and (raw == -20).any(axis=0).all() and (raw == 2).any(axis=0).all()
    kw = dict(ent_coef=0.2) if alpha_as == "ent_coef" else dict(log_ent_coef=np.log(0.2))
    alpha = float(np.float32(0.2)) if alpha_as == "ent_coef" else float(np.exp(np.float64(np.float32(np.log(0.2)))))

    h = _t(heads, grad=True)
    mu, ls = h[:, :n_u], h[:, n_u:].clamp(-20.0, 2.0)
    std = ls.exp()
    x = mu + std * _t(z)
    a = torch.tanh(x)
    logp = torch.distributions.Normal(mu, std).log_prob(x).sum(dim=1) - torch.log(1.0 - a ** 2 + 1e-6).sum(dim=1)
    qs = [_t(c) + (a * _t(w)).sum(dim=1) + 0.5 * (a ** 2 * _t(v)).sum(dim=1) for c, w, v in cw]
    loss = (alpha * logp - torch.min(qs[0], qs[1])).mean()
    loss.backward()
    assert float(x.detach().abs().max()) > 12.0

    a64 = a.detach().numpy()
    dq = [w + a64 * v for _, w, v in cw]
    q = [t.detach().numpy() for t in qs]
    g, stats, a_ref, logp_ref = sac_actor_head_reference(heads, z, q[0], q[1], dq[0], dq[1], **kw)
    _close(a_ref, a64, "a")
    _close(logp_ref, logp.detach().numpy(), "logp")
    _close(g[:, :n_u], h.grad.numpy()[:, :n_u], "grad_out, mu")
    _close(g[:, n_u:], h.grad.numpy()[:, n_u:], "grad_out, raw log-std")
    _close(g, h.grad.numpy(), "grad_out")
    outside = (raw < -20) | (raw > 2)
    assert (g[:, n_u:][outside] == 0.0).all() and (g[:, n_u:][~outside] != 0.0).all(), "the clamp's mask: zero outside, the edges inside"
    _close(stats, [float(loss.detach()), float(logp.detach().mean()), float(torch.min(qs[0], qs[1]).detach().mean()), alpha], "stats")
    with pytest.raises(ValueError):
        sac_actor_head_reference(heads, z, q[0], q[1], dq[0], dq[1])
    with pytest.raises(ValueError):
        sac_actor_head_reference(heads, z, q[0], q[1], dq[0], dq[1], ent_coef=0.2, log_ent_coef=0.0)


def test_actor_head_tie_goes_to_critic_one():
    from gym_dockauv_amd.policy import sac_actor_head_float32, sac_actor_head_reference
    heads, z, cw = actor_case(6, B=9)
    q1 = np.arange(9, dtype=np.float32)
    q2 = q1.copy()
    q2[::2] += 1.0
    q2[1] -= 1.0
    dq1, dq2 = cw[0][1], cw[1][1]
    for fn in (sac_actor_head_reference, sac_actor_head_float32):
        g = fn(heads, z, q1, q2, dq1, dq2, ent_coef=0.0)[0]
        only1 = fn(heads, z, q1, q1 + 1, dq1, dq2, ent_coef=0.0)[0]
        only2 = fn(heads, z, q1, q1 - 1, dq1, dq2, ent_coef=0.0)[0]
        assert (g[3] == only1[3]).all() and (g[0] == only1[0]).all(), "a tie, and q1 < q2, take dq1"
        assert (g[1] == only2[1]).all() and not (g[1] == only1[1]).all(), "q2 < q1 takes dq2"


def test_critic_head_statement_is_float64_autograd():
    import torch
    from gym_dockauv_amd.policy import sac_critic_head_reference
    rng = np.random.default_rng(5)
    for B in (1, 33, 129):
        q1, q2, y = (rng.standard_normal(B) * 3 for _ in range(3))
        t1, t2 = _t(q1, grad=True), _t(q2, grad=True)
        mse = torch.nn.functional.mse_loss
        loss = 0.5 * sum(mse(t, _t(y)) for t in (t1, t2))
        loss.backward()
        g1, g2, stats = sac_critic_head_reference(q1, q2, y)
        _close(g1, t1.grad.numpy(), f"grad_q1 B={B}")
        _close(g2, t2.grad.numpy(), f"grad_q2 B={B}")
        _close(stats, [float(loss.detach()), float(mse(t1, _t(y)).detach()), float(mse(t2, _t(y)).detach()), q1.mean(), q2.mean(), y.mean()], f"stats B={B}")


@pytest.mark.parametrize("init", [1.0, 0.1])
def test_ent_coef_statement_is_torch_adam_over_three_steps(init):
    import torch
    from gym_dockauv_amd.policy import ent_coef_step_reference
    rng = np.random.default_rng(8)
    lr, betas, eps, target = 3e-3, (0.9, 0.999), 1e-8, -6.0
    p = torch.tensor(np.log(init), dtype=torch.float64, requires_grad=True)
    opt = torch.optim.Adam([p], lr=lr, betas=betas, eps=eps)
    state = np.array([np.log(init), 0.0, 0.0])
    for step in (1, 2, 3):
        logp = rng.standard_normal(129) * 2 + step
        opt.zero_grad()
        before = float(p.detach())
        loss = -(p * _t(logp + target)).mean()
        loss.backward()
        opt.step()
        state, stats = ent_coef_step_reference(state, logp, step, lr, target, betas, eps)
        _close(state[0], float(p.detach()), f"log_ent_coef after step {step}")
        _close(state[1], float(opt.state[p]["exp_avg"]), f"m after step {step}")
        _close(state[2], float(opt.state[p]["exp_avg_sq"]), f"v after step {step}")
        _close(stats, [float(loss.detach()), np.exp(before), float((logp + target).mean()), float(p.detach())], f"stats of step {step}")
    with pytest.raises(ValueError):
        ent_coef_step_reference(state, logp, 0, lr, target)


@pytest.mark.parametrize("n_u", [3, 6, 8])
def test_float32_restatements_stay_within_float32_of_the_statements(n_u):
    from gym_dockauv_amd import policy as P
    heads, z, cw = actor_case(n_u, B=129, seed=1)
    rng = np.random.default_rng(n_u)
    q1, q2 = (rng.standard_normal(129).astype(np.float32) for _ in range(2))
    dq1, dq2 = (rng.standard_normal((129, n_u)).astype(np.float32) for _ in range(2))
    z32 = z.astype(np.float32)
    g64, s64, a64, lp64 = P.sac_actor_head_reference(heads, z32, q1, q2, dq1, dq2, ent_coef=0.2)
    g32, s32, a32, lp32 = P.sac_actor_head_float32(heads, z32, q1, q2, dq1, dq2, ent_coef=0.2)
    assert all(t.dtype == np.float32 for t in (g32, s32, a32, lp32))
    for name, x, y in (("grad_out, mu", g32[:, :n_u], g64[:, :n_u]), ("grad_out, raw log-std", g32[:, n_u:], g64[:, n_u:]), ("a", a32, a64),
                       ("logp", lp32, lp64), ("stats", s32, s64)):
        _close(x, y, f"actor head float32 {name}", rtol=FORWARD_BOUND)
    raw = heads[:, n_u:]
    outside = (raw < -20) | (raw > 2)
    assert (g32[:, n_u:][outside] == 0.0).all() and (g32[:, n_u:][~outside] != 0.0).all()
    # log_ent_coef = 0 is ent_coef = 1 bit for bit
    one = P.sac_actor_head_float32(heads, z32, q1, q2, dq1, dq2, ent_coef=1.0)
    zero = P.sac_actor_head_float32(heads, z32, q1, q2, dq1, dq2, log_ent_coef=0.0)
    assert all((x.view(np.int32) == y.view(np.int32)).all() for x, y in zip(one, zero))

    y = rng.standard_normal(129).astype(np.float32)
    r1, r2, rs = P.sac_critic_head_reference(q1, q2, y)
    f1, f2, fs = P.sac_critic_head_float32(q1, q2, y)
    for name, x, ref in (("grad_q1", f1, r1), ("grad_q2", f2, r2), ("stats", fs, rs)):
        assert x.dtype == np.float32
        _close(x, ref, f"critic head float32 {name}", rtol=FORWARD_BOUND)

    state64, state32 = np.array([np.log(0.1), 0.0, 0.0]), np.array([np.log(0.1), 0.0, 0.0], dtype=np.float32)
    for step in (1, 2, 3):
        logp = (lp32 + np.float32(step)).astype(np.float32)
        state64, st64 = P.ent_coef_step_reference(state64, logp, step, 3e-3, -float(n_u))
        mean = P.ent_coef_mean_float32(logp, -float(n_u))
        state32, loss32 = P.ent_coef_step_float32(state32, mean, step, 3e-3)
        assert state32.dtype == np.float32 and state32.shape == (3,)
        _close(mean, st64[2], f"ent_coef mean, step {step}", rtol=FORWARD_BOUND)
        _close(state32, state64, f"ent_coef state after step {step}", rtol=FORWARD_BOUND)
        _close(loss32, st64[0], f"ent_coef_loss of step {step}", rtol=FORWARD_BOUND)


def test_header_and_records_know_the_new_calls():
    full = " ".join(re.sub(r"\n \*", "\n", open(HEADER).read()).split())
    # the paragraph that listed what is missing: the first two items are provided now and name their calls, the last two remain
    m = re.search(r"the loss head \(.*?\) and ent_coef itself \((dockauv_[a-z_]+)\)", full)
    assert m and m.group(1) == "dockauv_sac_ent_coef_step", "the header's SAC paragraph does not name the loss head's calls"
    for n in NEW_SYMBOLS[:3]:
        assert n in m.group(0), n
    rest = full[m.end():]
    assert re.match(r"[^.]*\.\s+What remains outside it: the optimiser for these roles and the Polyak update", rest), rest[:200]
    cov = open(os.path.join(ROOT, "profiles", "coverage", "kernels.txt")).read()
    usage = open(os.path.join(ROOT, "profiles", "sac", "kernel_usage.txt")).read()
    for k in ("sac_sample_kernel", "sac_critic_head_kernel", "sac_actor_head_kernel", "ent_coef_step_kernel"):
        assert re.search(rf"^{k} launched test_gpu_sac_head", cov, flags=re.M), k
        assert k in usage, k
