"""CPU-only checks of the whole-update entry points (include/dockauv.h: dockauv_permutation, dockauv_ppo_update): the exact
statement of the permutation (MLPPolicy.permutation_reference) as a permutation and against NumPy's own shuffle in a chi-square
table, the ctypes mirror of dockauv_ppo_update_io against a C program compiled from the header, the refusals that need no
device, ppo_head_reference with clip_range_vf against float64 torch autograd of SB3's value-loss lines, and the documents."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dockauv.h")
SIZES = (1, 2, 3, 5, 63, 64, 65, 1000, 4096, 4097, 100_000)


@pytest.fixture(scope="module")
def lib():
    from gym_dockauv_amd.csrc import build
    build.build()
    from gym_dockauv_amd import _capi
    return _capi.load_library()


def perm(seed, epoch, n):
    from gym_dockauv_amd.policy import MLPPolicy
    return MLPPolicy.permutation_reference(seed, epoch, n)


@pytest.mark.parametrize("n", SIZES)
def test_permutation_reference_is_a_permutation(n):
    p = perm(3, 5, n)
    assert p.dtype == np.int64 and p.shape == (n,)
    assert np.array_equal(np.sort(p), np.arange(n)), "not a permutation of range(n)"
    assert np.array_equal(p, perm(3, 5, n)), "not deterministic"


def test_permutation_reference_depends_on_epoch_and_seed():
    n = 4096
    base = perm(0, 0, n)
    for other, what in ((perm(0, 1, n), "epoch"), (perm(1, 0, n), "seed"), (perm(1 << 32, 0, n), "the seed's high word")):
        same = float((base == other).mean())
        assert same < 0.01, (what, same)
    assert np.array_equal(perm(0, 1 << 32 | 1, n), perm(0, 1, n)), "the epoch enters mod 2^32"
    with pytest.raises(ValueError):
        perm(0, 0, 0)
    with pytest.raises(ValueError):
        perm(0, 0, (1 << 31) + 1)


def chi_square(perms, n):
    """the chi-square statistic of the 16 x 16 table (position bucket, value bucket) pooled over `perms`"""
    bucket = np.arange(n) * 16 // n
    table = np.zeros((16, 16))
    for p in perms:
        np.add.at(table, (bucket, bucket[p]), 1.0)
    per = np.bincount(bucket, minlength=16).astype(np.float64)
    expected = np.outer(per, per) * (len(perms) / n)
    return float(((table - expected) ** 2 / expected).sum())


@pytest.mark.parametrize("n", [256, 1000])
def test_permutation_reference_is_as_uniform_as_numpy(n):
    """64 permutations (seeds 0..7 x epochs 0..7) against the largest statistic of 300 batches of 64 NumPy permutations"""
    mine = chi_square([perm(s, e, n) for s in range(8) for e in range(8)], n)
    rng = np.random.default_rng(1)
    theirs = [chi_square([rng.permutation(n) for _ in range(64)], n) for _ in range(300)]
    print(f"permutation n {n}: chi-square {mine:.1f}; NumPy mean {np.mean(theirs):.1f}, max {max(theirs):.1f}")
    assert mine <= max(theirs), (mine, max(theirs))


def test_update_io_layout_matches_c(tmp_path):
    from gym_dockauv_amd import _capi
    fields = [name for name, _ in _capi.PPOUpdateIO._fields_]
    src = tmp_path / "layout.c"
    prints = "\n".join(f'  printf("%zu\\n", offsetof(dockauv_ppo_update_io, {f}));' for f in fields)
    src.write_text(f'''
#include <stdio.h>
#include <stddef.h>
#include "{HEADER}"
int main(void) {{
  printf("%zu\\n", sizeof(dockauv_ppo_update_io));
{prints}
  return 0;
}}''')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-o", str(exe), str(src)])
    out = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    got = [C.sizeof(_capi.PPOUpdateIO)] + [getattr(_capi.PPOUpdateIO, f).offset for f in fields]
    assert out == got
    assert _capi.PPOUpdateIO.opt.size == C.sizeof(_capi.OptimIO)


def test_null_arguments_refused_without_a_device(lib):
    from gym_dockauv_amd import _capi
    io = _capi.PPOUpdateIO()
    io.struct_size = C.sizeof(_capi.PPOUpdateIO)
    fake = C.c_void_p(8)   # never dereferenced: the calls are refused first
    err = lambda: lib.dockauv_last_error(None)
    assert lib.dockauv_permutation(None, 0, 0, 16, fake, None) == -1 and b"dockauv_permutation: null handle" in err()
    assert lib.dockauv_permutation(None, 0, 0, 0, None, None) == -1 and b"dockauv_permutation: null handle" in err()
    assert lib.dockauv_ppo_update(None, fake, C.byref(io), None) == -1 and b"dockauv_ppo_update: null handle" in err()
    assert lib.dockauv_ppo_update(None, None, None, None) == -1 and b"dockauv_ppo_update: null handle" in err()


def value_case():
    """v, v_old, returns with rows inside the clamp, outside it on both sides and exactly on both edges (c = 0.25 and
    offsets that are exact in binary, so that float64 sees |v - v_old| == c)"""
    rng = np.random.default_rng(4)
    c = 0.25
    offs = np.concatenate([rng.uniform(-0.2, 0.2, 9), rng.uniform(0.3, 1.0, 7), -rng.uniform(0.3, 1.0, 7), [c, -c, c, -c]])
    v_old = np.round(rng.normal(size=offs.size) * 8) / 8
    v = v_old + offs
    assert ((v - v_old)[-4:] == [c, -c, c, -c]).all()
    return c, v, v_old, rng.normal(size=offs.size)


def test_head_reference_with_clip_range_vf_against_torch_autograd():
    import torch
    from gym_dockauv_amd.policy import MLPPolicy
    c, v, v_old, ret = value_case()
    n, n_u, vf = v.size, 3, 0.5
    rng = np.random.default_rng(5)
    mean, ls = rng.uniform(-1, 1, (n, n_u)), rng.uniform(-1, 0.3, n_u)
    actions = mean + np.exp(ls) * rng.normal(size=(n, n_u))
    lpo, adv = rng.normal(size=n) - 3.0, rng.normal(size=n)
    args = (mean, v, actions, lpo, adv, ret, ls, 0.2, vf, 0.01)
    old = MLPPolicy.ppo_head_reference(*args)
    for kw in ({}, dict(clip_range_vf=None, values_old=None), dict(clip_range_vf=0.0, values_old=v_old), dict(clip_range_vf=None, values_old=v_old)):
        same = MLPPolicy.ppo_head_reference(*args, **kw)
        assert all(np.array_equal(a, b) for a, b in zip(old, same)), "the defaults changed the head's reference"
    _, grad_v, _, stats = MLPPolicy.ppo_head_reference(*args, clip_range_vf=c, values_old=v_old)

    # SB3's lines (ppo.py): values_pred = old + clamp(values - old, -c, c); value_loss = F.mse_loss(returns, values_pred)
    tv = torch.tensor(v, dtype=torch.float64, requires_grad=True)
    t_old, t_ret = torch.tensor(v_old, dtype=torch.float64), torch.tensor(ret, dtype=torch.float64)
    pred = t_old + torch.clamp(tv - t_old, -c, c)
    value_loss = torch.nn.functional.mse_loss(t_ret, pred)
    (vf * value_loss).backward()
    assert abs(stats[2] - value_loss.item()) <= 1e-15 * max(1.0, value_loss.item())
    assert np.abs(grad_v - tv.grad.numpy()).max() <= 1e-16
    assert abs(stats[0] - (old[3][0] + vf * (value_loss.item() - old[3][2]))) <= 1e-14
    d = v - v_old
    assert (grad_v[np.abs(d) > c] == 0).all() and (grad_v[np.abs(d) <= c] != 0).all()
    assert (grad_v[-4:] != 0).all(), "a row exactly on the clamp's edge has the unclamped gradient (torch.clamp's backward)"
    for a, b in zip(old[:1] + old[2:3], MLPPolicy.ppo_head_reference(*args, clip_range_vf=c, values_old=v_old)[0:3:2]):
        assert np.array_equal(a, b), "clip_range_vf touched the policy's gradients"
    with pytest.raises(ValueError):
        MLPPolicy.ppo_head_reference(*args, clip_range_vf=c)


def test_values_old_draw_of_the_gpu_test_stays_within_its_cap():
    """the draw tests/test_gpu_update.py feeds the clipped value loss: at most 1 / 256 of it is redrawn for lying within EDGE
    of the clamp's edge, and the clamp is active on a quarter of the rows on each side (asserted inside)"""
    from tests import test_gpu_update as G
    for n in (257, G.ROWS_BEYOND_ONE_PASS):
        v = np.random.default_rng(n).normal(size=n).astype(np.float32)
        v_old, redrawn, draw = G.draw_values_old(v, n, seed=n + 1)
        print(f"values_old n {n}: {redrawn} of {draw} redrawn")
        assert v_old.dtype == np.float32 and redrawn <= draw / 256.0


def test_documented(lib):
    """the header states the network, the value clamp and the stop rule; INTEGRATION.md, the README, DESIGN.md and the kernel
    records know the new entry points"""
    text = " ".join(open(HEADER).read().replace("\n *", "\n").split())
    for phrase in ("b = max(2, bit_length(n - 1))", "t = ((R + k_r) mod 2^32) * 0xD2511F53", "f = (f ^ (f >> 15)) mod 2^w",
                   "counter (q, epoch mod 2^32, 0, 3)", "it has no bound and cannot hang",
                   "vc = v_old + fminf(fmaxf(d, -c), c)", "(fabsf(d) <= c) ? ((2.0f * vf_coef) * dv) / (float)B : 0.0f",
                   "approx_kl > 1.5f * target_kl", "on the frozen weights", "the count is PENDING",
                   "stats [n_epochs][J][12]"):
        assert phrase in text, phrase
    for entry in ("dockauv_optim_step", "dockauv_optim_state"):
        at = text.index(f"int {entry}(")
        assert "pending" in text[max(0, at - 6000): at], f"{entry} does not document the pending count"
    for path in ("INTEGRATION.md", "README.md", "DESIGN.md"):
        doc = open(os.path.join(ROOT, path)).read()
        assert "dockauv_ppo_update" in doc and "dockauv_permutation" in doc, path
    assert "## 7G. The whole update in one call" in open(os.path.join(ROOT, "DESIGN.md")).read()
    cov = open(os.path.join(ROOT, "profiles", "coverage", "kernels.txt")).read()
    usage = open(os.path.join(ROOT, "profiles", "update", "kernel_usage.txt")).read()
    for k in ("permutation_kernel", "update_begin_kernel", "HeadArgsVf", "HeadArgsGate", "AdamArgsCtl"):
        assert k in cov, k
        assert k in usage, k
