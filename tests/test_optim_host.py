"""CPU-only checks of the optimiser's surface (include/dockauv.h: dockauv_optim_create / _destroy / _step / _state):
MLPPolicy.adam_reference against torch's clip_grad_norm_ + torch.optim.Adam(eps=1e-5) in float64 over three steps, the
declarations with the ABI version unchanged, the ctypes mirrors of dockauv_optim_desc and dockauv_optim_io against the C structs,
and the refusal of a NULL handle without a device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dockauv.h")
NEW = ("dockauv_optim_create", "dockauv_optim_destroy", "dockauv_optim_step", "dockauv_optim_state")


@pytest.fixture(scope="module")
def lib():
    from gym_dockauv_amd.csrc import build
    build.build()
    from gym_dockauv_amd import _capi
    return _capi.load_library()


def shapes_20_5():
    """the tensors of a 20-5-6 actor with log_std and a 20-5-1 critic, in the optimiser's order"""
    return [(5, 20), (5,), (6, 5), (6,), (6,), (5, 20), (5,), (1, 5), (1,)]


@pytest.mark.parametrize("max_grad_norm", [0.5, 0.0])
def test_adam_reference_is_torch(max_grad_norm):
    """Three consecutive steps; the gradients are N(0, 1) scaled so that step 1 clips (norm 2), step 2 sits near the edge above
    it (0.6) and step 3 does not clip (0.1).  1e-12 relative to the largest entry of each array."""
    import torch
    from gym_dockauv_amd.policy import MLPPolicy
    rng = np.random.default_rng(5)
    shapes = shapes_20_5()
    p0 = [rng.normal(size=s) for s in shapes]
    p0_copy = [p.copy() for p in p0]
    t_params = [torch.tensor(p, dtype=torch.float64, requires_grad=True) for p in p0]
    opt = torch.optim.Adam(t_params, lr=3e-4, eps=1e-5)
    params, m, v = p0, [np.zeros(s) for s in shapes], [np.zeros(s) for s in shapes]
    coefs = []
    for t, (target, lr) in enumerate(((2.0, 3e-4), (0.6, 1e-3), (0.1, 3e-4)), start=1):
        grads = [rng.normal(size=s) for s in shapes]
        scale = target / np.sqrt(sum((g * g).sum() for g in grads))
        grads = [g * scale for g in grads]
        for tp, g in zip(t_params, grads):
            tp.grad = torch.tensor(g, dtype=torch.float64)
        for group in opt.param_groups:
            group["lr"] = lr
        want_norm = float(torch.nn.utils.clip_grad_norm_(t_params, max_grad_norm)) if max_grad_norm > 0 else target
        opt.step()
        params, m, v, norm, coef = MLPPolicy.adam_reference(params, grads, m, v, t, lr, (0.9, 0.999), 1e-5, max_grad_norm)
        coefs.append(coef)
        assert abs(norm - want_norm) <= 1e-12 * want_norm and abs(norm - target) <= 1e-12 * target
        for i, tp in enumerate(t_params):
            st = opt.state[tp]
            for name, got, want in (("param", params[i], tp.detach().numpy()), ("m", m[i], st["exp_avg"].numpy()),
                                    ("v", v[i], st["exp_avg_sq"].numpy())):
                assert got.dtype == np.float64 and got.shape == want.shape
                assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max(), (t, i, name, np.abs(got - want).max())
    if max_grad_norm > 0:
        assert coefs[0] < 0.26 and coefs[1] < 1.0 and coefs[2] == 1.0, coefs
    else:
        assert coefs == [1.0, 1.0, 1.0]
    # nothing was changed in place
    assert all(np.array_equal(a, b) for a, b in zip(p0, p0_copy))


def test_adam_reference_rejects_bad_input():
    from gym_dockauv_amd.policy import MLPPolicy
    a = [np.zeros((2, 3)), np.zeros(3)]
    with pytest.raises(ValueError):
        MLPPolicy.adam_reference(a, a[:1], a, a, 1, 1e-3)
    with pytest.raises(ValueError):
        MLPPolicy.adam_reference(a, [np.zeros((3, 2)), np.zeros(3)], a, a, 1, 1e-3)
    with pytest.raises(ValueError):
        MLPPolicy.adam_reference(a, a, a, a, 0, 1e-3)


def test_symbols_declared_bound_exported(lib):
    from gym_dockauv_amd import _capi
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(dockauv_[a-z0-9_]+)\s*\(", text))
    for name in NEW:
        assert name in declared, f"{name} not declared in include/dockauv.h"
        assert name in {s[0] for s in _capi.SYMBOLS}, f"{name} not in _capi.SYMBOLS"
        assert hasattr(lib, name), f"{name} not exported by libdockauv.so"
    assert re.search(r"typedef\s+struct\s+dockauv_optim_desc\b", text) and re.search(r"typedef\s+struct\s+dockauv_optim_io\b", text)
    assert re.search(r"typedef\s+struct\s+dockauv_optim_s\s*\*\s*dockauv_optim\s*;", text)
    # the change only adds structs and functions: the ABI version stays
    assert re.search(r"#define\s+DOCKAUV_ABI_VERSION\s+3\b", text) and lib.dockauv_abi_version() == 3 and _capi.ABI_VERSION == 3


def test_the_optimiser_no_longer_stays_with_the_learner():
    """the header, INTEGRATION.md and the README describe the optimiser as part of the library"""
    for path in (HEADER, os.path.join(ROOT, "INTEGRATION.md"), os.path.join(ROOT, "README.md")):
        text = " ".join(open(path).read().split())
        assert "dockauv_optim_step" in text or "ppo_update" in text, path
        for old in ("optimiser step stay with the learner", "the optimiser stay in torch", "optimiser stay in torch",
                    "Not part of the library: gradient-norm clipping"):
            assert old not in text, (path, old)


@pytest.mark.parametrize("struct,mirror", [("dockauv_optim_desc", "OptimDesc"), ("dockauv_optim_io", "OptimIO")])
def test_struct_layout_matches_c(tmp_path, struct, mirror):
    from gym_dockauv_amd import _capi
    cls = getattr(_capi, mirror)
    fields = [f[0] for f in cls._fields_]
    want = {"OptimDesc": ["struct_size", "reserved", "beta1", "beta2", "eps", "max_grad_norm", "reserved1"],
            "OptimIO": ["struct_size", "reserved", "lr", "actor_params", "log_std", "actor_grads", "grad_log_std", "critic_params",
                        "critic_grads", "stats"]}[mirror]
    assert fields == want
    src = tmp_path / "layout.c"
    src.write_text(f'''
#include <stdio.h>
#include <stddef.h>
#include "{HEADER}"
int main(void) {{
  printf("%zu", sizeof({struct}));
''' + "".join(f'  printf(" %zu", offsetof({struct}, {f}));\n' for f in fields) + '''  printf("\\n");
  return 0;
}''')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-o", str(exe), str(src)])
    out = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    got = [C.sizeof(cls)] + [getattr(cls, f).offset for f in fields]
    assert out == got


def test_null_handle_refused_without_a_device(lib):
    from gym_dockauv_amd import _capi
    fake = C.c_void_p(8)   # never dereferenced: the calls are refused first
    d = _capi.OptimDesc()
    d.struct_size = C.sizeof(_capi.OptimDesc)
    d.beta1, d.beta2, d.eps, d.max_grad_norm = 0.9, 0.999, 1e-5, 0.5
    out = C.c_void_p(123)
    assert lib.dockauv_optim_create(None, fake, fake, C.byref(d), C.byref(out)) == -1
    assert b"null handle" in lib.dockauv_last_error(None)
    assert lib.dockauv_optim_create(None, None, None, None, None) == -1 and b"null handle" in lib.dockauv_last_error(None)
    io = _capi.OptimIO()
    io.struct_size = C.sizeof(_capi.OptimIO)
    assert lib.dockauv_optim_step(None, fake, C.byref(io), None) == -1 and b"null handle" in lib.dockauv_last_error(None)
    assert lib.dockauv_optim_step(None, None, None, None) == -1 and b"null handle" in lib.dockauv_last_error(None)
    assert lib.dockauv_optim_state(None, None, None, None, None) == -1 and b"null optimiser" in lib.dockauv_last_error(None)
    assert lib.dockauv_optim_destroy(None) == 0
