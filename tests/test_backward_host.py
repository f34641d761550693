"""CPU-only checks of the MLP backward's surface (include/dockauv.h: dockauv_policy_forward_rows, dockauv_policy_backward,
dockauv_policy_grads): MLPPolicy.backward_reference against torch float64 autograd, exact zeros for a zero upstream gradient,
the declarations with the ABI version unchanged, the ctypes mirror of dockauv_policy_grads against the C struct, and refusals
before any device call."""
import ctypes as C
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dockauv.h")
NEW = ["dockauv_policy_forward_rows", "dockauv_policy_backward"]


@pytest.fixture(scope="module")
def lib():
    from gym_dockauv_amd.csrc import build
    build.build()
    from gym_dockauv_amd import _capi
    return _capi.load_library()


def _mlp(n_in, hidden, n_out, act, seed):
    from gym_dockauv_amd.policy import MLPPolicy
    rng = np.random.default_rng(seed)
    layers, n = [], n_in
    for w in list(hidden) + [n_out]:
        b = 1.0 / np.sqrt(n)
        layers.append((rng.uniform(-b, b, (w, n)), rng.uniform(-b, b, w)))
        n = w
    return MLPPolicy(layers, act, "none")


CASES = [(hidden, act, n_out, rows) for hidden, act, n_out, rows in
         itertools.product([(17,), (64,), (128,), (17, 64), (64, 64), (128, 17), (128, 128)], ["tanh", "relu"], [1, 6], [1, 257])]


@pytest.mark.parametrize("hidden,act,n_out,rows", CASES, ids=lambda v: "-".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_backward_reference_is_torch_autograd(hidden, act, n_out, rows):
    """The float64 statement against torch's float64 autograd of the same float32 weights: one and two hidden layers, tanh and
    relu, widths 17 / 64 / 128, 1 and 6 outputs, 1 and 257 rows; 1e-12 relative to the largest entry of each gradient."""
    import torch
    mlp = _mlp(20, hidden, n_out, act, seed=3)
    rng = np.random.default_rng(4)
    x = rng.uniform(-1, 1, (rows, 20))
    g = rng.normal(size=(rows, n_out))
    got = mlp.backward_reference(x, g)
    mods, params = [], []
    for i, (W, b) in enumerate(mlp.layers):
        lin = torch.nn.Linear(W.shape[1], W.shape[0]).double()
        with torch.no_grad():
            lin.weight.copy_(torch.from_numpy(W.astype(np.float64)))
            lin.bias.copy_(torch.from_numpy(b.astype(np.float64)))
        mods.append(lin)
        params += [lin.weight, lin.bias]
        if i < len(mlp.layers) - 1:
            mods.append(torch.nn.Tanh() if act == "tanh" else torch.nn.ReLU())
    out = torch.nn.Sequential(*mods)(torch.from_numpy(x))
    assert np.abs(out.detach().numpy() - mlp.forward_reference(x)).max() <= 1e-12
    out.backward(torch.from_numpy(g))
    assert len(got) == len(params)
    for mine, p in zip(got, params):
        want = p.grad.numpy()
        assert mine.dtype == np.float64 and mine.shape == want.shape
        assert np.abs(mine - want).max() <= 1e-12 * np.abs(want).max(), (mine.shape, np.abs(mine - want).max())


def test_zero_upstream_gradient_gives_exact_zeros():
    for hidden, act in (((64, 64), "tanh"), ((17,), "relu")):
        mlp = _mlp(20, hidden, 6, act, seed=1)
        x = np.random.default_rng(0).uniform(-1, 1, (33, 20))
        for gr in mlp.backward_reference(x, np.zeros((33, 6))):
            assert not gr.any()


def test_reference_rejects_mismatched_batches():
    mlp = _mlp(20, (64, 64), 6, "tanh", seed=1)
    with pytest.raises(ValueError):
        mlp.backward_reference(np.zeros((4, 20)), np.zeros((5, 6)))


def test_new_symbols_declared_bound_exported(lib):
    from gym_dockauv_amd import _capi
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(dockauv_[a-z0-9_]+)\s*\(", text))
    bound = {s[0] for s in _capi.SYMBOLS}
    for n in NEW:
        assert n in declared, f"{n} not declared in include/dockauv.h"
        assert n in bound, f"{n} not in _capi.SYMBOLS"
        assert hasattr(lib, n), f"{n} not exported by libdockauv.so"
    assert re.search(r"typedef\s+struct\s+dockauv_policy_grads\b", text)
    # the change only adds symbols: the ABI version stays
    assert re.search(r"#define\s+DOCKAUV_ABI_VERSION\s+3\b", text) and lib.dockauv_abi_version() == 3


def test_policy_grads_layout_matches_c(tmp_path):
    from gym_dockauv_amd import _capi
    fields = [f[0] for f in _capi.PolicyGrads._fields_]
    assert fields == ["struct_size", "reserved", "dW1", "db1", "dW2", "db2", "dW3", "db3"]
    src = tmp_path / "layout.c"
    src.write_text(f'''
#include <stdio.h>
#include <stddef.h>
#include "{HEADER}"
int main(void) {{
  printf("%zu", sizeof(dockauv_policy_grads));
''' + "".join(f'  printf(" %zu", offsetof(dockauv_policy_grads, {f}));\n' for f in fields) + '''  printf("\\n");
  return 0;
}''')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-o", str(exe), str(src)])
    out = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    got = [C.sizeof(_capi.PolicyGrads)] + [getattr(_capi.PolicyGrads, f).offset for f in fields]
    assert out == got


def _grads(**over):
    from gym_dockauv_amd import _capi
    g = _capi.PolicyGrads()
    g.struct_size = C.sizeof(_capi.PolicyGrads)
    for f in ("dW1", "db1", "dW2", "db2", "dW3", "db3"):
        setattr(g, f, 8)          # never dereferenced: the call is refused first
    for k, v in over.items():
        setattr(g, k, v)
    return g


def test_null_arguments_refused_without_a_device(lib):
    """Both entry points return DOCKAUV_E_INVALID (-1) on a NULL handle, policy or buffer, a row count below 1 and a gradient
    struct of the wrong size -- without a handle, so nothing can have touched a device."""
    err = lambda: lib.dockauv_last_error(None)
    fake = C.c_void_p(8)   # never dereferenced: the call is refused first
    # forward_rows
    assert lib.dockauv_policy_forward_rows(None, fake, fake, None, 128, fake, None) == -1 and b"null handle" in err()
    assert lib.dockauv_policy_forward_rows(None, fake, fake, fake, 128, fake, None) == -1 and b"null handle" in err()
    assert lib.dockauv_policy_forward_rows(None, None, fake, None, 128, fake, None) == -1 and b"null policy" in err()
    assert lib.dockauv_policy_forward_rows(None, fake, None, None, 128, fake, None) == -1 and b"NULL" in err()
    assert lib.dockauv_policy_forward_rows(None, fake, fake, None, 128, None, None) == -1 and b"NULL" in err()
    assert lib.dockauv_policy_forward_rows(None, fake, fake, None, 0, fake, None) == -1 and b"n_rows" in err()
    # backward
    g = _grads()
    assert lib.dockauv_policy_backward(None, fake, fake, None, 128, fake, C.byref(g), None) == -1 and b"null handle" in err()
    assert lib.dockauv_policy_backward(None, None, fake, None, 128, fake, C.byref(g), None) == -1 and b"null policy" in err()
    assert lib.dockauv_policy_backward(None, fake, None, None, 128, fake, C.byref(g), None) == -1 and b"NULL" in err()
    assert lib.dockauv_policy_backward(None, fake, fake, None, 128, None, C.byref(g), None) == -1 and b"NULL" in err()
    assert lib.dockauv_policy_backward(None, fake, fake, None, 128, fake, None, None) == -1 and b"NULL" in err()
    assert lib.dockauv_policy_backward(None, fake, fake, None, 0, fake, C.byref(g), None) == -1 and b"n_rows" in err()
    assert lib.dockauv_policy_backward(None, fake, fake, None, -5, fake, C.byref(g), None) == -1 and b"n_rows" in err()
    g = _grads(struct_size=8)
    assert lib.dockauv_policy_backward(None, fake, fake, None, 128, fake, C.byref(g), None) == -1 and b"struct_size" in err()
    for f in ("dW1", "db1", "dW3", "db3"):
        g = _grads(**{f: None})
        assert lib.dockauv_policy_backward(None, fake, fake, None, 128, fake, C.byref(g), None) == -1 and b"dW1/db1/dW3/db3" in err(), f
    # dW2 / db2 may be NULL (one hidden layer): the next complaint is the handle
    g = _grads(dW2=None, db2=None)
    assert lib.dockauv_policy_backward(None, fake, fake, None, 128, fake, C.byref(g), None) == -1 and b"null handle" in err()
