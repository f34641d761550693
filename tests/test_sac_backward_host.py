"""CPU: the surface of the networks' share of SAC's gradient half and its float64 statements (include/dockauv.h:
dockauv_sac_actor_forward_rows, dockauv_sac_actor_backward, dockauv_q_backward; gym_dockauv_amd/policy.py:
SquashedGaussianMLP.heads_reference / backward_reference, MLPPolicy.backward_input_reference).  The new symbols are declared, bound
and exported and the ABI is still 3; the new structs have the layout of their ctypes mirrors; every NULL pointer, wrong
struct_size, n_rows < 1 and stride below every row width is refused with the field named before a handle or a device is looked
at (what needs a live handle -- strides against n_obs / n_u, each role against the calls that must refuse it, the LDS bound -- is
in tests/test_gpu_sac_backward.py); and the three statements are float64 torch autograd's gradients to 1e-12 relative: both sides
are float64 evaluations of the same formulas."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dockauv.h")

NEW_SYMBOLS = ["dockauv_sac_actor_forward_rows", "dockauv_sac_actor_backward", "dockauv_q_backward"]
WORKSPACE = "dockauv_policy_backward_workspace"
RTOL = 1e-12


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
    for n in NEW_SYMBOLS + [WORKSPACE]:
        assert n in declared and bound.count(n) == 1 and hasattr(lib, n), n
    assert declared == set(bound), "header and binding declare different symbols"
    for s in ("dockauv_sac_rows_io", "dockauv_sac_actor_backward_io", "dockauv_q_backward_io"):
        assert re.search(rf"typedef\s+struct\s+{s}\b", text), s
    assert _capi.ABI_VERSION == 3 and lib.dockauv_abi_version() == 3
    assert re.search(r"#define\s+DOCKAUV_ABI_VERSION\s+3\b", text)
    # the paragraph that said the gradient half is missing now says what remains
    full = " ".join(re.sub(r"\n \*", "\n", open(HEADER).read()).split())
    assert "is not in the library" not in full
    for word in ("the loss head", "ent_coef itself", "the optimiser for these roles", "the Polyak update"):
        assert word in full, word


def test_struct_layouts_match_c(tmp_path):
    from gym_dockauv_amd import _capi
    structs = {"dockauv_sac_rows_io": _capi.SacRowsIO, "dockauv_sac_actor_backward_io": _capi.SacActorBackwardIO,
               "dockauv_q_backward_io": _capi.QBackwardIO, "dockauv_policy_grads": _capi.PolicyGrads}
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


def test_io_blocks_refused_before_any_device_call(lib):
    from gym_dockauv_amd import _capi
    fake = C.c_void_p(8)          # never dereferenced: something else is refused first
    err = lambda: lib.dockauv_last_error(None)

    def rows_io(change, needle):
        io = _capi.SacRowsIO()
        io.struct_size, io.row_stride, io.n_rows = C.sizeof(io), 20, 4
        io.rows = io.out = 8
        change(io)
        rc = lib.dockauv_sac_actor_forward_rows(None, fake, C.byref(io), None)
        assert rc == -1 and needle in err(), (needle, rc, err())

    rows_io(lambda io: setattr(io, "struct_size", 8), b"dockauv_sac_rows_io.struct_size")
    rows_io(lambda io: setattr(io, "n_rows", 0), b"dockauv_sac_rows_io.n_rows")
    rows_io(lambda io: setattr(io, "row_stride", 0), b"dockauv_sac_rows_io.row_stride")
    rows_io(lambda io: setattr(io, "rows", None), b"dockauv_sac_rows_io.rows is NULL")
    rows_io(lambda io: setattr(io, "out", None), b"dockauv_sac_rows_io.out is NULL")
    rows_io(lambda io: None, b"null handle")          # a valid block gets as far as the handle
    assert lib.dockauv_sac_actor_forward_rows(None, None, None, None) == -1 and b"io is NULL" in err()
    io = _capi.SacRowsIO()
    io.struct_size, io.row_stride, io.n_rows, io.rows, io.out = C.sizeof(io), 20, 4, 8, 8
    assert lib.dockauv_sac_actor_forward_rows(None, None, C.byref(io), None) == -1 and b"null actor" in err()

    def actor_io(change, needle):
        io = _capi.SacActorBackwardIO()
        io.struct_size, io.row_stride, io.n_rows = C.sizeof(io), 20, 4
        for f, _ in _capi.SacActorBackwardIO._fields_[2:]:
            if f != "n_rows" and f != "row_index":
                setattr(io, f, 8)
        change(io)
        rc = lib.dockauv_sac_actor_backward(None, fake, C.byref(io), None)
        assert rc == -1 and needle in err(), (needle, rc, err())

    actor_io(lambda io: setattr(io, "struct_size", 16), b"dockauv_sac_actor_backward_io.struct_size")
    actor_io(lambda io: setattr(io, "n_rows", 0), b"dockauv_sac_actor_backward_io.n_rows")
    actor_io(lambda io: setattr(io, "n_rows", -3), b"dockauv_sac_actor_backward_io.n_rows")
    actor_io(lambda io: setattr(io, "row_stride", 0), b"dockauv_sac_actor_backward_io.row_stride")
    for f in ("rows", "grad_out", "dW1", "db1", "dW_mu", "db_mu", "dW_ls", "db_ls"):
        actor_io(lambda io, f=f: setattr(io, f, None), b"dockauv_sac_actor_backward_io." + f.encode() + b" is NULL")
    actor_io(lambda io: None, b"null handle")
    actor_io(lambda io: (setattr(io, "dW2", None), setattr(io, "db2", None)), b"null handle")   # (whether they are needed: the actor decides)
    assert lib.dockauv_sac_actor_backward(None, None, None, None) == -1 and b"io is NULL" in err()

    def q_io(change, needle, with_grads=True):
        io = _capi.QBackwardIO()
        io.struct_size, io.obs_stride, io.act_stride, io.n_rows = C.sizeof(io), 20, 6, 4
        io.obs = io.actions = io.grad_q = io.grad_actions = 8
        g = _capi.PolicyGrads()
        g.struct_size = C.sizeof(g)
        g.dW1 = g.db1 = g.dW2 = g.db2 = g.dW3 = g.db3 = 8
        if with_grads:
            io.grads = C.pointer(g)
        change(io, g)
        rc = lib.dockauv_q_backward(None, fake, C.byref(io), None)
        assert rc == -1 and needle in err(), (needle, rc, err())

    q_io(lambda io, g: setattr(io, "struct_size", 8), b"dockauv_q_backward_io.struct_size")
    q_io(lambda io, g: setattr(io, "n_rows", 0), b"dockauv_q_backward_io.n_rows")
    q_io(lambda io, g: setattr(io, "obs_stride", 0), b"dockauv_q_backward_io.obs_stride")
    q_io(lambda io, g: setattr(io, "act_stride", 0), b"dockauv_q_backward_io.act_stride")
    for f in ("obs", "actions", "grad_q"):
        q_io(lambda io, g, f=f: setattr(io, f, None), b"dockauv_q_backward_io." + f.encode() + b" is NULL")
    q_io(lambda io, g: setattr(io, "grad_actions", None), b"grads and grad_actions are both NULL", with_grads=False)
    q_io(lambda io, g: setattr(g, "struct_size", 8), b"dockauv_policy_grads.struct_size")
    for f in ("dW1", "db1", "dW3", "db3"):
        q_io(lambda io, g, f=f: setattr(g, f, None), b"dockauv_policy_grads: dW1/db1/dW3/db3")
    q_io(lambda io, g: None, b"null handle")
    q_io(lambda io, g: None, b"null handle", with_grads=False)                     # grad_actions alone is a valid request
    q_io(lambda io, g: setattr(io, "grad_actions", None), b"null handle")          # ... and so are the parameters alone
    assert lib.dockauv_q_backward(None, None, None, None) == -1 and b"io is NULL" in err()
    assert lib.dockauv_policy_backward_workspace(None, None, None) == -1 and b"null policy" in err()


def _t(x):
    import torch
    return torch.tensor(np.asarray(x), dtype=torch.float64)


def _close(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    scale = max(float(np.abs(want).max()), 1e-300)
    err = float(np.abs(got - want).max()) / scale
    print(f"{what}: max relative difference {err:.2e}")
    assert err <= RTOL, (what, err)


@pytest.mark.parametrize("hidden,act,n_u", [((64, 64), "relu", 6), ((33,), "tanh", 3), ((48, 40), "tanh", 8)])
def test_actor_statements_are_float64_autograd(hidden, act, n_u):
    """heads_reference and backward_reference against autograd through an nn.Sequential with mu / log_std heads in float64."""
    import torch
    from tests.test_sac_host import default_actor
    mlp = default_actor(20, hidden, n_u, seed=3 + n_u)
    mlp.hidden_act = act
    rng = np.random.default_rng(n_u)
    obs, g = rng.uniform(-1, 1, (257, 20)), rng.standard_normal((257, 2 * n_u))
    mods = []
    for W, b in mlp.layers:
        lin = torch.nn.Linear(W.shape[1], W.shape[0]).double()
        with torch.no_grad():
            lin.weight.copy_(_t(W)), lin.bias.copy_(_t(b))
        mods += [lin, torch.nn.ReLU() if act == "relu" else torch.nn.Tanh()]
    latent = torch.nn.Sequential(*mods)
    heads = []
    for W, b in (mlp.mu, mlp.log_std_head):
        lin = torch.nn.Linear(W.shape[1], W.shape[0]).double()
        with torch.no_grad():
            lin.weight.copy_(_t(W)), lin.bias.copy_(_t(b))
        heads.append(lin)
    h = latent(_t(obs))
    out = torch.cat([heads[0](h), heads[1](h)], dim=1)
    _close(mlp.heads_reference(obs), out.detach().numpy(), "heads_reference")
    (out * _t(g)).sum().backward()
    want = [p.grad.numpy() for p in latent.parameters()] + [p.grad.numpy() for lin in heads for p in lin.parameters()]
    got = mlp.backward_reference(obs, g)
    assert len(got) == len(want) == 2 * len(hidden) + 4
    for name, a, b in zip(("dW1", "db1", "dW2", "db2")[: 2 * len(hidden)] + ("dW_mu", "db_mu", "dW_ls", "db_ls"), got, want):
        _close(a, b, f"backward_reference {name}")


@pytest.mark.parametrize("hidden,act,n_obs,n_u", [((64, 64), "relu", 20, 6), ((40,), "tanh", 25, 6), ((128, 128), "relu", 36, 8)])
def test_backward_input_reference_is_float64_autograd(hidden, act, n_obs, n_u):
    """dL/dx of a Q critic on x = cat([obs, a]) against autograd in float64; its action columns are what dockauv_q_backward's
    grad_actions states, and backward_reference on the same x the parameter gradients."""
    import torch
    from gym_dockauv_amd.policy import MLPPolicy
    rng = np.random.default_rng(n_obs)
    widths = [n_obs + n_u] + list(hidden) + [1]
    layers = [(rng.uniform(-1, 1, (o, i)) / np.sqrt(i), rng.uniform(-1, 1, o) / np.sqrt(i)) for i, o in zip(widths[:-1], widths[1:])]
    q = MLPPolicy(layers, act, "none")
    obs, a, g = rng.uniform(-1, 1, (129, n_obs)), rng.uniform(-1, 1, (129, n_u)), rng.standard_normal((129, 1))
    mods = []
    for i, (W, b) in enumerate(q.layers):
        lin = torch.nn.Linear(W.shape[1], W.shape[0]).double()
        with torch.no_grad():
            lin.weight.copy_(_t(W)), lin.bias.copy_(_t(b))
        mods += [lin] + ([torch.nn.ReLU() if act == "relu" else torch.nn.Tanh()] if i < len(q.layers) - 1 else [])
    net = torch.nn.Sequential(*mods)
    to, ta = _t(obs), _t(a).requires_grad_(True)
    x = torch.cat([to, ta], dim=1)
    x.retain_grad()
    (net(x) * _t(g)).sum().backward()
    x64 = np.concatenate([obs, a], axis=1)
    dx = q.backward_input_reference(x64, g)
    _close(dx, x.grad.numpy(), "backward_input_reference")
    _close(dx[:, n_obs:], ta.grad.numpy(), "backward_input_reference, action columns")
    for name, got, p in zip(("dW1", "db1", "dW2", "db2", "dW3", "db3") if len(hidden) == 2 else ("dW1", "db1", "dW3", "db3"),
                            q.backward_reference(x64, g), net.parameters()):
        _close(got, p.grad.numpy(), f"backward_reference {name}")
