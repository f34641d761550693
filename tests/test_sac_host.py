"""CPU: the surface of the SAC forward half and its NumPy statements (include/dockauv.h: dockauv_sac_actor_*, dockauv_q_*,
dockauv_sac_target; gym_dockauv_amd/policy.py: SquashedGaussianMLP, sac_target_reference).  The new symbols are declared, bound and
exported and the ABI is still 3; the three new structs have the layout of their ctypes mirrors; descriptors and io blocks are
refused with the field named before a handle or a device is looked at; ``forward_reference`` is SB3's formulas (against an
independent torch float64 restatement, 1e-12 on rows with |x| <= 6, and default-initialised heads keep every row inside that);
``sac_target_reference`` is its float64 form to 1e-6 relative; and the float32 NumPy evaluation of the kernel's log-probability
expressions stays under the 1e-3 cap the GPU test puts on the device (what needs a live handle -- n_in against n_obs + n_u, n_out
against n_u, each role against the calls that must refuse it -- is in tests/test_gpu_sac.py)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dockauv.h")

SAC_SYMBOLS = ["dockauv_q_create", "dockauv_q_forward", "dockauv_sac_actor_create", "dockauv_sac_actor_load", "dockauv_sac_target"]
LOGP_CAP = 1e-3


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
    for n in SAC_SYMBOLS:
        assert n in declared and bound.count(n) == 1 and hasattr(lib, n), n
    assert declared == set(bound), "header and binding declare different symbols"
    # call-like names in the header's comments are functions that exist
    assert set(re.findall(r"\b(dockauv_[a-z0-9_]+)\s*\(", open(HEADER).read())) == declared
    assert _capi.ABI_VERSION == 3 and lib.dockauv_abi_version() == 3
    assert re.search(r"#define\s+DOCKAUV_ABI_VERSION\s+3\b", text)


def test_struct_layouts_match_c(tmp_path):
    from gym_dockauv_amd import _capi
    structs = {"dockauv_sac_actor_desc": _capi.SacActorDesc, "dockauv_q_io": _capi.QIO, "dockauv_sac_target_io": _capi.SacTargetIO,
               "dockauv_policy_desc": _capi.PolicyDesc}
    items, want = [], []
    for cname, mirror in structs.items():
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
    assert [f[0] for f in _capi.SacTargetIO._fields_][-5:] == ["a2", "logp2", "q1", "q2", "y"]


def _actor_desc(hidden=(64, 64), n_in=20, n_out=6):
    from gym_dockauv_amd.policy import SquashedGaussianMLP
    rng = np.random.default_rng(0)
    layers, n = [], n_in
    for w in hidden:
        layers.append((rng.standard_normal((w, n)), rng.standard_normal(w)))
        n = w
    mlp = SquashedGaussianMLP(layers, (rng.standard_normal((n_out, n)), np.zeros(n_out)), (np.zeros((n_out, n)), np.zeros(n_out)))
    return mlp, mlp.host_desc(seed=3)


def test_descriptors_and_io_refused_before_any_device_call(lib):
    from gym_dockauv_amd import _capi
    from gym_dockauv_amd.policy import MLPPolicy
    out = C.c_void_p()
    fake = C.c_void_p(8)          # never dereferenced: something else is refused first
    err = lambda: lib.dockauv_last_error(None)

    def actor(change, needle):
        mlp, d = _actor_desc()
        change(d)
        rc = lib.dockauv_sac_actor_create(None, C.byref(d), C.byref(out))
        assert rc == -1 and not out.value and needle in err(), (needle, rc, err())

    actor(lambda d: setattr(d, "struct_size", d.struct_size - 8), b"dockauv_sac_actor_desc.struct_size")
    actor(lambda d: d.n_hidden.__setitem__(0, 129), b"n_hidden[0]")
    actor(lambda d: d.n_hidden.__setitem__(1, 129), b"n_hidden[1]")
    actor(lambda d: setattr(d, "n_out", 9), b"dockauv_sac_actor_desc.n_out")
    actor(lambda d: setattr(d, "n_out", 0), b"dockauv_sac_actor_desc.n_out")
    actor(lambda d: setattr(d, "hidden_act", 0), b"hidden_act")
    actor(lambda d: setattr(d, "precision", 1), b"precision")
    actor(lambda d: setattr(d, "W_mu", None), b"W_mu is NULL")
    actor(lambda d: setattr(d, "b_ls", None), b"b_ls is NULL")
    actor(lambda d: setattr(d, "W2", None), b"W2 is NULL")
    actor(lambda d: None, b"null handle")             # a valid descriptor gets as far as the handle
    assert lib.dockauv_sac_actor_create(None, None, C.byref(out)) == -1 and b"null" in err()
    assert lib.dockauv_sac_actor_load(None, None, None) == -1 and b"null policy" in err()

    # a Q critic's descriptor is a dockauv_policy_desc: its own fields first, then the handle
    rng = np.random.default_rng(1)
    q = MLPPolicy([(rng.standard_normal((64, 26)), np.zeros(64)), (rng.standard_normal((1, 64)), np.zeros(1))], "relu", "none")
    d = q.host_desc()
    d.struct_size -= 4
    assert lib.dockauv_q_create(None, C.byref(d), C.byref(out)) == -1 and b"dockauv_policy_desc.struct_size" in err()
    d = q.host_desc()
    d.n_hidden[0] = 129
    assert lib.dockauv_q_create(None, C.byref(d), C.byref(out)) == -1 and b"n_hidden[0]" in err()
    d = q.host_desc()
    d.n_out = 2
    assert lib.dockauv_q_create(None, C.byref(d), C.byref(out)) == -1 and b"a critic has one output" in err()
    d = q.host_desc()
    d.out_act = _capi.ACT_TANH
    assert lib.dockauv_q_create(None, C.byref(d), C.byref(out)) == -1 and b"out_act" in err()
    d = q.host_desc()
    assert lib.dockauv_q_create(None, C.byref(d), C.byref(out)) == -1 and b"null handle" in err() and not out.value

    def qio(change, needle):
        io = _capi.QIO()
        io.struct_size, io.obs_stride, io.act_stride, io.n_rows = C.sizeof(io), 20, 6, 4
        io.obs = io.actions = io.q = 8
        change(io)
        rc = lib.dockauv_q_forward(None, fake, C.byref(io), None)
        assert rc == -1 and needle in err(), (needle, rc, err())

    qio(lambda io: setattr(io, "struct_size", 8), b"dockauv_q_io.struct_size")
    qio(lambda io: setattr(io, "n_rows", 0), b"dockauv_q_io.n_rows")
    qio(lambda io: setattr(io, "obs", None), b"dockauv_q_io.obs is NULL")
    qio(lambda io: setattr(io, "actions", None), b"dockauv_q_io.actions is NULL")
    qio(lambda io: setattr(io, "q", None), b"dockauv_q_io.q is NULL")
    qio(lambda io: None, b"null handle")
    assert lib.dockauv_q_forward(None, None, None, None) == -1 and b"io is NULL" in err()

    def tio(change, needle):
        io = _capi.SacTargetIO()
        io.struct_size, io.next_obs_stride, io.column_stride, io.gamma, io.ent_coef, io.n_rows = C.sizeof(io), 20, 1, 0.99, 0.2, 4
        io.next_obs = io.rewards = io.dones = io.a2 = io.logp2 = io.q1 = io.q2 = io.y = 8
        change(io)
        rc = lib.dockauv_sac_target(None, fake, fake, fake, C.byref(io), None)
        assert rc == -1 and needle in err(), (needle, rc, err())

    tio(lambda io: setattr(io, "struct_size", 16), b"dockauv_sac_target_io.struct_size")
    tio(lambda io: setattr(io, "n_rows", 0), b"dockauv_sac_target_io.n_rows")
    tio(lambda io: setattr(io, "gamma", 1.5), b"dockauv_sac_target_io.gamma")
    tio(lambda io: setattr(io, "gamma", -0.1), b"dockauv_sac_target_io.gamma")
    tio(lambda io: setattr(io, "gamma", float("nan")), b"dockauv_sac_target_io.gamma")
    tio(lambda io: setattr(io, "ent_coef", float("nan")), b"ent_coef is NaN")
    tio(lambda io: setattr(io, "column_stride", 0), b"column_stride")
    for f in ("next_obs", "rewards", "dones", "a2", "logp2", "q1", "q2", "y"):
        tio(lambda io, f=f: setattr(io, f, None), b"dockauv_sac_target_io." + f.encode() + b" is NULL")
    tio(lambda io: None, b"null handle")
    assert lib.dockauv_sac_target(None, None, None, None, None, None) == -1 and b"io is NULL" in err()


def default_actor(n_in, hidden, n_out, seed, ls_scale=1.0):
    """torch's default initialisation of every Linear (weights and biases U(+-1 / sqrt(fan_in))); the log_std head x ls_scale"""
    from gym_dockauv_amd.policy import SquashedGaussianMLP
    rng = np.random.default_rng(seed)
    lin = lambda o, i: (rng.uniform(-1, 1, (o, i)) / np.sqrt(i), rng.uniform(-1, 1, o) / np.sqrt(i))
    layers, n = [], n_in
    for w in hidden:
        layers.append(lin(w, n))
        n = w
    mu, ls = lin(n_out, n), lin(n_out, n)
    return SquashedGaussianMLP(layers, mu, (ls[0] * ls_scale, ls[1] * ls_scale), "relu")


@pytest.mark.parametrize("n_u", [3, 6, 8])
def test_forward_reference_is_sb3s_formulas(n_u):
    """torch.distributions.Normal, torch.tanh and log(1 - a^2 + 1e-6) in float64 on 1 000 rows: 1e-12 on rows with |x| <= 6,
    and default-initialised heads keep every row inside that."""
    import torch
    mlp = default_actor(20, (64, 64), n_u, seed=n_u)
    rng = np.random.default_rng(10 + n_u)
    obs = rng.uniform(-1, 1, (1000, 20))
    z = rng.standard_normal((1000, n_u))
    a, lp, mu, ls = mlp.forward_reference(obs, z)
    t = lambda x: torch.as_tensor(np.asarray(x), dtype=torch.float64)
    h = t(obs)
    for W, b in mlp.layers:
        h = torch.relu(h @ t(W).T + t(b))
    mu_t = h @ t(mlp.mu[0]).T + t(mlp.mu[1])
    ls_t = torch.clamp(h @ t(mlp.log_std_head[0]).T + t(mlp.log_std_head[1]), -20, 2)
    dist = torch.distributions.Normal(mu_t, ls_t.exp())
    x_t = mu_t + ls_t.exp() * t(z)
    a_t = torch.tanh(x_t)
    lp_t = dist.log_prob(x_t).sum(dim=1) - torch.log(1 - a_t ** 2 + 1e-6).sum(dim=1)
    inside = (x_t.abs().max(dim=1).values <= 6).numpy()
    assert inside.all(), "a default-initialised head left |x| <= 6"
    assert np.abs(a - a_t.numpy()).max() <= 1e-12 and np.abs(mu - mu_t.numpy()).max() <= 1e-12 and np.abs(ls - ls_t.numpy()).max() <= 1e-12
    assert np.abs(lp - lp_t.numpy())[inside].max() <= 1e-12
    # deterministic: z = 0
    a0, lp0, _, _ = mlp.forward_reference(obs)
    assert np.abs(a0 - torch.tanh(mu_t).numpy()).max() <= 1e-12
    assert np.abs(lp0 - (dist.log_prob(mu_t).sum(dim=1) - torch.log(1 - torch.tanh(mu_t) ** 2 + 1e-6).sum(dim=1)).numpy()).max() <= 1e-12


def logp_cases():
    """the two cases of the log-probability error (tests/test_gpu_sac.py, scripts/sac_error.py): default-initialised networks,
    and the log_std head scaled so that some |x| reach about 8"""
    return {"default": default_actor(20, (64, 64), 6, seed=21), "wide_std": default_actor(20, (64, 64), 6, seed=21, ls_scale=3.0)}


def test_float32_numpy_log_prob_stays_under_the_cap():
    """The float32 NumPy evaluation of the kernel's expressions against forward_reference on both cases: under the absolute cap
    of 1e-3 the GPU test holds the device to (so that cap can be met at all); the second case does reach |x| of about 8."""
    rng = np.random.default_rng(5)
    obs = rng.uniform(-1, 1, (4096, 20)).astype(np.float32)
    z = rng.standard_normal((4096, 6)).astype(np.float32)
    reach = {}
    for name, mlp in logp_cases().items():
        _, lp64, mu, ls = mlp.forward_reference(obs, z)
        a32, lp32 = mlp.forward_float32(obs, z)
        err = float(np.abs(lp32.astype(np.float64) - lp64).max())
        reach[name] = float(np.abs(mu + np.exp(ls) * z).max())
        print(f"float32 NumPy log-prob error, {name}: {err:.3e} (cap {LOGP_CAP:g}); max |x| = {reach[name]:.2f}")
        assert err <= LOGP_CAP, (name, err)
        assert np.abs(a32 - mlp.forward_reference(obs, z)[0]).max() <= 1e-5
    assert reach["default"] <= 6 and 7.0 <= reach["wide_std"] <= 9.0, reach


def test_sac_target_reference():
    from gym_dockauv_amd.policy import sac_target_reference
    rng = np.random.default_rng(9)
    n = 5000
    q1, q2, lp = (rng.standard_normal(n).astype(np.float32) * 10 for _ in range(3))
    r = rng.standard_normal(n).astype(np.float32)
    d = (rng.random(n) < 0.2).astype(np.float32)
    gamma, alpha = 0.99, 0.37
    y = sac_target_reference(q1, q2, lp, r, d, gamma, ent_coef=alpha)
    assert y.dtype == np.float32 and y.shape == (n,)
    f = lambda x: x.astype(np.float64)
    want = f(r) + float(np.float32(gamma)) * (1 - f(d)) * (np.minimum(f(q1), f(q2)) - float(np.float32(alpha)) * f(lp))
    assert np.all(np.abs(y - want) <= 1e-6 * np.maximum(np.abs(want), 1.0))
    assert np.array_equal(y[d == 1].view(np.uint32), r[d == 1].view(np.uint32)), "a done row's target is its reward"
    # alpha from log_ent_coef is alpha given directly
    log_alpha = np.float32(-1.25)
    a = np.float32(np.exp(np.float64(log_alpha)))
    assert np.array_equal(sac_target_reference(q1, q2, lp, r, d, gamma, log_ent_coef=log_alpha).view(np.uint32),
                          sac_target_reference(q1, q2, lp, r, d, gamma, ent_coef=a).view(np.uint32))
    with pytest.raises(ValueError):
        sac_target_reference(q1, q2, lp, r, d, gamma)
    with pytest.raises(ValueError):
        sac_target_reference(q1, q2, lp, r, d, gamma, ent_coef=0.1, log_ent_coef=0.0)


def test_from_torch_reads_an_sb3_style_actor():
    import torch
    from gym_dockauv_amd.policy import SquashedGaussianMLP

    class Actor(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.latent_pi = torch.nn.Sequential(torch.nn.Linear(20, 48), torch.nn.ReLU(), torch.nn.Linear(48, 33), torch.nn.ReLU())
            self.mu, self.log_std = torch.nn.Linear(33, 6), torch.nn.Linear(33, 6)

    torch.manual_seed(0)
    m = Actor()
    mlp = SquashedGaussianMLP.from_torch(m)
    assert (mlp.n_in, mlp.n_hidden, mlp.n_out, mlp.hidden_act) == (20, [48, 33], 6, "relu")
    sd = SquashedGaussianMLP.from_torch(m.state_dict())
    for (W, b), (W2, b2) in zip(mlp.layers + [mlp.mu, mlp.log_std_head], sd.layers + [sd.mu, sd.log_std_head]):
        assert np.array_equal(W, W2) and np.array_equal(b, b2)
    obs = torch.rand(50, 20, dtype=torch.float64) * 2 - 1
    md = Actor().double()
    md.load_state_dict({k: v.double() for k, v in m.state_dict().items()})
    assert np.abs(mlp.forward_reference(obs.numpy())[2] - md.mu(md.latent_pi(obs)).detach().numpy()).max() <= 1e-12
    twin = mlp.plain_twin()
    assert twin.out_act == "tanh" and np.abs(twin.forward_reference(obs.numpy()) - mlp.forward_reference(obs.numpy())[0]).max() <= 1e-15


def test_rows_stream_normals_are_slot_5():
    from gym_dockauv_amd.policy import MLPPolicy, SAC_ROWS_STREAM
    assert SAC_ROWS_STREAM == 5
    a = MLPPolicy.normals_reference(77, np.arange(64), 3, 6, slot=SAC_ROWS_STREAM)
    assert not np.array_equal(a, MLPPolicy.normals_reference(77, np.arange(64), 3, 6))
    assert np.array_equal(MLPPolicy.normals_reference(77, np.arange(64), 3, 6), MLPPolicy.normals_reference(77, np.arange(64), 3, 6, slot=2))
    assert np.array_equal(a[10:20], MLPPolicy.normals_reference(77, 10 + np.arange(10), 3, 6, slot=5)), "row_offset adds to the row"
    assert not np.array_equal(a, MLPPolicy.normals_reference(77, np.arange(64), 4, 6, slot=5))
