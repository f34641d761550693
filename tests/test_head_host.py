"""CPU-only checks of the PPO head's surface (include/dockauv.h: dockauv_ppo_head, dockauv_ppo_head_io):
MLPPolicy.ppo_head_reference against torch float64 autograd of the loss as INTEGRATION.md section 6 builds it, the declaration
with the ABI version unchanged, the ctypes mirror of dockauv_ppo_head_io against the C struct, and the refusal of a NULL handle
without a device."""
import ctypes as C
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dockauv.h")
CLIP, VF, ENT = 0.2, 0.5, 0.01


@pytest.fixture(scope="module")
def lib():
    from gym_dockauv_amd.csrc import build
    build.build()
    from gym_dockauv_amd import _capi
    return _capi.load_library()


def draw(B, n_u, seed):
    """a minibatch whose ratios spread over both clip edges: (mean, v, actions, log_prob_old, advantages, returns, log_std)"""
    from gym_dockauv_amd.policy import MLPPolicy
    rng = np.random.default_rng(seed)
    mean = rng.uniform(-1, 1, (B, n_u))
    log_std = rng.uniform(-1, 0.3, n_u)
    z = rng.normal(size=(B, n_u))
    actions = mean + np.exp(log_std) * z
    lpo = MLPPolicy.log_prob_reference(z, log_std) - rng.normal(0, 0.3, B)
    return mean, rng.normal(size=B), actions, lpo, 100 + rng.normal(size=B), rng.normal(size=B), log_std


def torch_head(mean, v, actions, lpo, adv, ret, log_std, normalize):
    """the loop body of INTEGRATION.md section 6 in float64: (grad_mean, grad_v, grad_log_std, stats[:6])"""
    import torch
    t = lambda x: torch.from_numpy(np.asarray(x, dtype=np.float64))
    mean_t, ls = t(mean).requires_grad_(), t(log_std).requires_grad_()
    v_t = None if v is None else t(v).requires_grad_()
    dist = torch.distributions.Normal(mean_t, ls.exp())
    lr = dist.log_prob(t(actions)).sum(-1) - t(lpo)
    ratio = lr.exp()
    a = t(adv)
    if normalize:
        a = (a - a.mean()) / (a.std() + 1e-8)
    policy_loss = -torch.min(ratio * a, ratio.clamp(1 - CLIP, 1 + CLIP) * a).mean()
    value_loss = ((t(ret) - v_t) ** 2).mean() if v is not None else torch.zeros((), dtype=torch.float64)
    entropy_loss = -dist.entropy().sum(-1).mean()
    loss = policy_loss + VF * value_loss + ENT * entropy_loss
    loss.backward()
    stats = [loss, policy_loss, value_loss, entropy_loss, ((ratio - 1) - lr).mean(), ((ratio - 1).abs() > CLIP).double().mean()]
    return (mean_t.grad.numpy(), None if v is None else v_t.grad.numpy(), ls.grad.numpy(), np.array([float(s.detach()) for s in stats]))


@pytest.mark.parametrize("B,n_u,normalize,critic", list(itertools.product([2, 257], [1, 4], [True, False], [True, False])))
def test_ppo_head_reference_is_torch_autograd(B, n_u, normalize, critic):
    """1e-12 relative to the largest entry of each output, on Normal / torch.min / clamp / .std() as section 6 uses them."""
    from gym_dockauv_amd.policy import MLPPolicy
    mean, v, actions, lpo, adv, ret, log_std = draw(B, n_u, seed=B + n_u)
    if not critic:
        v = None
    got = MLPPolicy.ppo_head_reference(mean, v, actions, lpo, adv, ret, log_std, CLIP, VF, ENT, normalize_advantage=normalize)
    want = torch_head(mean, v, actions, lpo, adv, ret, log_std, normalize)
    assert (got[1] is None) == (not critic)
    for name, g, w in zip(("grad_mean", "grad_v", "grad_log_std", "stats"), got[:3] + (got[3][:6],), want):
        if w is None:
            continue
        assert g.dtype == np.float64 and g.shape == w.shape, name
        assert np.abs(g - w).max() <= 1e-12 * np.abs(w).max(), (name, np.abs(g - w).max(), np.abs(w).max())
    a = np.asarray(adv)
    m, s = (a.mean(), a.std(ddof=1)) if normalize else (0.0, 1.0)
    assert abs(got[3][6] - m) <= 1e-12 * max(abs(m), 1.0) and abs(got[3][7] - s) <= 1e-12 * s
    if B == 257:
        assert 0.05 < got[3][5] < 0.95, "the draw must reach both sides of the clip range"


def test_reference_rejects_bad_shapes():
    from gym_dockauv_amd.policy import MLPPolicy
    mean, v, actions, lpo, adv, ret, log_std = draw(5, 3, seed=1)
    with pytest.raises(ValueError):
        MLPPolicy.ppo_head_reference(mean, v, actions, lpo[:4], adv, ret, log_std, CLIP, VF, ENT)
    with pytest.raises(ValueError):
        MLPPolicy.ppo_head_reference(mean[:1], v[:1], actions[:1], lpo[:1], adv[:1], ret[:1], log_std, CLIP, VF, ENT)


def test_symbol_declared_bound_exported(lib):
    from gym_dockauv_amd import _capi
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(dockauv_[a-z0-9_]+)\s*\(", text))
    assert "dockauv_ppo_head" in declared, "dockauv_ppo_head not declared in include/dockauv.h"
    assert "dockauv_ppo_head" in {s[0] for s in _capi.SYMBOLS}, "dockauv_ppo_head not in _capi.SYMBOLS"
    assert hasattr(lib, "dockauv_ppo_head"), "dockauv_ppo_head not exported by libdockauv.so"
    assert re.search(r"typedef\s+struct\s+dockauv_ppo_head_io\b", text)
    # the change only adds a struct and a function: the ABI version stays
    assert re.search(r"#define\s+DOCKAUV_ABI_VERSION\s+3\b", text) and lib.dockauv_abi_version() == 3 and _capi.ABI_VERSION == 3


def test_ppo_head_io_layout_matches_c(tmp_path):
    from gym_dockauv_amd import _capi
    fields = [f[0] for f in _capi.PPOHeadIO._fields_]
    assert fields == ["struct_size", "normalize_advantage", "mean", "v", "actions", "log_prob_old", "advantages", "returns",
                      "row_index", "n_rows", "clip_range", "vf_coef", "ent_coef", "reserved", "grad_mean", "grad_v",
                      "grad_log_std", "stats"]
    src = tmp_path / "layout.c"
    src.write_text(f'''
#include <stdio.h>
#include <stddef.h>
#include "{HEADER}"
int main(void) {{
  printf("%zu", sizeof(dockauv_ppo_head_io));
''' + "".join(f'  printf(" %zu", offsetof(dockauv_ppo_head_io, {f}));\n' for f in fields) + '''  printf("\\n");
  return 0;
}''')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-o", str(exe), str(src)])
    out = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    got = [C.sizeof(_capi.PPOHeadIO)] + [getattr(_capi.PPOHeadIO, f).offset for f in fields]
    assert out == got


def test_null_handle_refused_without_a_device(lib):
    from gym_dockauv_amd import _capi
    io = _capi.PPOHeadIO()
    io.struct_size = C.sizeof(_capi.PPOHeadIO)
    fake = C.c_void_p(8)   # never dereferenced: the call is refused first
    assert lib.dockauv_ppo_head(None, fake, C.byref(io), None) == -1 and b"null handle" in lib.dockauv_last_error(None)
    assert lib.dockauv_ppo_head(None, None, None, None) == -1 and b"null handle" in lib.dockauv_last_error(None)
