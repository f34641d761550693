"""
Reward normalisation, host side (no GPU): the NumPy statement of dockauv_rewnorm_scan (gym_dockauv_amd/normalize.py:
reward_normalize_reference) against a literal transcription of SB3 1.5's VecNormalize / RunningMeanStd loop, frozen mode, and the C
surface: symbols declared, bound and exported, the ctypes mirror of dockauv_rewnorm_io, refusals by name before any device call,
the signature of ``collect``, the documents.  `crafted` below is also what tests/test_gpu_rewnorm.py feeds the kernels.
"""
import ctypes as C
import inspect
import math
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dockauv.h")
NEW = ["dockauv_rewnorm_create", "dockauv_rewnorm_destroy", "dockauv_rewnorm_state", "dockauv_rewnorm_reset", "dockauv_rewnorm_scan",
       "dockauv_gae_normalized", "dockauv_collect_normalized"]
TERMINAL = (400.0, -200.0, -100.0, -300.0)   # w_goal, w_deltad_max / w_Theta_max, w_t_max, w_col of config/env_config.py


@pytest.fixture(scope="module")
def lib():
    from gym_dockauv_amd.csrc import build
    build.build()
    from gym_dockauv_amd import _capi
    return _capi.load_library()


# ------------------------------------------------------------------------------------------------------- crafted inputs
def crafted(K, N, n_obs, seed, first_last=True):
    """(rows float32 [K, N, n_obs + 2], reward float32 [K, N], done bool [K, N]): reward U(-1, 1) plus, where done, a terminal
    term drawn from {400, -200, -100, -300}; done with p = 0.15 plus dones at k = 0 (envs 0-3) and k = K - 1 (envs 4-7) and none
    at all for env 8 (N > 8); observation columns NaN (never read)."""
    rng = np.random.default_rng(seed)
    reward = rng.uniform(-1, 1, (K, N))
    done = rng.random((K, N)) < 0.15
    if first_last:
        done[0, 0:4] = True
        done[K - 1, 4:8] = True
    if N > 8:
        done[:, 8] = False
    reward = (reward + np.where(done, rng.choice(TERMINAL, (K, N)), 0.0)).astype(np.float32)
    rows = np.full((K, N, n_obs + 2), np.nan, dtype=np.float32)
    rows[:, :, n_obs] = reward
    rows[:, :, n_obs + 1] = done
    return rows, reward, done


# ------------------------------------------------------------------------------------------------------- SB3, transcribed
class RunningMeanStd:
    """stable_baselines3/common/running_mean_std.py (1.5), scalar shape"""

    def __init__(self, epsilon=1e-4):
        self.mean = np.float64(0.0)
        self.var = np.float64(1.0)
        self.count = epsilon

    def update(self, arr):
        batch_mean = np.mean(arr, axis=0)
        batch_var = np.var(arr, axis=0)
        batch_count = arr.shape[0]
        self.update_from_moments(batch_mean, batch_var, batch_count)

    def update_from_moments(self, batch_mean, batch_var, batch_count):
        delta = batch_mean - self.mean
        tot_count = self.count + batch_count
        new_mean = self.mean + delta * batch_count / tot_count
        m_a = self.var * self.count
        m_b = batch_var * batch_count
        m_2 = m_a + m_b + np.square(delta) * self.count * batch_count / (self.count + batch_count)
        new_var = m_2 / (self.count + batch_count)
        new_count = batch_count + self.count
        self.mean = new_mean
        self.var = new_var
        self.count = new_count


def sb3_loop(reward, done, gamma, clip_reward, epsilon, rms, returns):
    """VecNormalize.step_wait with norm_reward=True, norm_obs=False, one call per row of `reward`: the returns carry is float32
    (as the device keeps it), the statistics see it in float64.  Returns (normalised rewards float32 [K, N], den [K], returns)."""
    out = np.zeros(reward.shape, dtype=np.float32)
    den = np.zeros(reward.shape[0])
    for k in range(reward.shape[0]):
        returns = returns * np.float32(gamma) + reward[k]
        assert returns.dtype == np.float32
        rms.update(returns.astype(np.float64))
        den[k] = np.sqrt(rms.var + epsilon)
        # (a VecEnv hands SB3 float64 rewards: the float32 words of the rows, widened)
        out[k] = np.clip(reward[k].astype(np.float64) / np.sqrt(rms.var + epsilon), -clip_reward, clip_reward)
        returns[done[k]] = 0
    return out, den, returns


def test_reference_is_sb3s_loop():
    """K = 19, 19, 1 steps of N = 200 on one state, so that episodes span both boundaries: mean, var and every step's den agree to
    1e-13 relative, count exactly, the normalised rewards to the last float32 bit but where the two float64 quotients straddle a
    rounding boundary (adjacent floats)."""
    from gym_dockauv_amd.normalize import INITIAL_STATE, RewardNormalizer, reward_normalize_reference
    assert RewardNormalizer.reward_normalize_reference is reward_normalize_reference
    N, gamma, clip, eps = 200, 0.99, 10.0, 1e-8
    rms, returns = RunningMeanStd(), np.zeros(N, dtype=np.float32)
    state, carry = np.array(INITIAL_STATE), np.zeros(N, dtype=np.float32)
    rel = lambda a, b: abs(a - b) / abs(b)
    spanned = 0
    for i, K in enumerate((19, 19, 1)):
        _, reward, done = crafted(K, N, 4, seed=70 + i, first_last=K > 1)
        if K > 1:
            assert done[0, 0:4].all() and done[K - 1, 4:8].all() and not done[:, 8].any()
        spanned += int((carry != 0).sum())
        want, want_den, returns = sb3_loop(reward, done, gamma, clip, eps, rms, returns)
        ref = reward_normalize_reference(reward, done, gamma, clip, eps, state, carry)
        state, carry = ref["state"], ref["carry"]
        assert np.array_equal(carry.view(np.int32), returns.view(np.int32)), "the carries differ"
        assert rel(state[0], rms.mean) <= 1e-13 and rel(state[1], rms.var) <= 1e-13, (state, rms.mean, rms.var)
        assert state[2] == rms.count and round(state[2]) == N * (19 * i + K)
        assert (np.abs(ref["step_stats"][:, 3] - want_den) <= 1e-13 * want_den).all()
        assert ref["reward_norm"].dtype == np.float32 and ref["discounted"].dtype == np.float32
        ulps = np.abs(ref["reward_norm"].view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))
        assert ulps.max() <= 1 and (ulps == 0).mean() > 0.99
        assert np.abs(ref["reward_norm"]).max() <= clip
    assert spanned >= N // 2, "hardly an episode spans a scan boundary"
    assert state[1] > 100.0, "returns in the hundreds: the variance must show it"


def test_frozen_mode_changes_neither_state_nor_carry():
    from gym_dockauv_amd.normalize import reward_normalize_reference
    N, K = 50, 7
    _, reward, done = crafted(K, N, 4, seed=3)
    state = np.array([1.5, 900.0, 4000.0001, 0.0])
    carry = np.random.default_rng(1).uniform(-50, 50, N).astype(np.float32)
    s0, c0 = state.copy(), carry.copy()
    ref = reward_normalize_reference(reward, done, 0.99, 2.0, 1e-8, state, carry, training=False)
    assert np.array_equal(state, s0) and np.array_equal(carry, c0)
    assert np.array_equal(ref["state"][:3], s0[:3]) and np.array_equal(ref["carry"].view(np.int32), c0.view(np.int32))
    den = math.sqrt(900.0 + 1e-8)
    assert (ref["step_stats"][:, 3] == den).all() and not ref["step_stats"][:, :3].any() and not ref["discounted"].any()
    want = np.clip(reward.astype(np.float64) / den, -2.0, 2.0).astype(np.float32)
    assert np.array_equal(ref["reward_norm"].view(np.int32), want.view(np.int32))
    assert (np.abs(ref["reward_norm"]) == 2.0).sum() == done.sum()       # (terminal rewards only: 100 / 30 > 2 > 1 / 30)
    # a training scan from the same state moves both
    moved = reward_normalize_reference(reward, done, 0.99, 2.0, 1e-8, state, carry)
    assert moved["state"][2] == s0[2] + K * N and not np.array_equal(moved["carry"], c0)
    with pytest.raises(ValueError):
        reward_normalize_reference(reward, done[:3], 0.99, 2.0, 1e-8, state, carry)
    with pytest.raises(ValueError):
        reward_normalize_reference(reward, done, 0.99, 0.0, 1e-8, state, carry)
    with pytest.raises(ValueError):
        reward_normalize_reference(reward, done, 1.5, 2.0, 1e-8, state, carry)


def test_discounted_return_is_two_float32_roundings():
    """ret = carry * gamma + reward with a rounded product: on inputs where the fused form gives another float32, the statement
    gives the two-rounding one"""
    from gym_dockauv_amd.normalize import reward_normalize_reference
    rng = np.random.default_rng(0)
    N = 4096
    carry = rng.uniform(-300, 300, N).astype(np.float32)
    reward = rng.uniform(-1, 1, (1, N)).astype(np.float32)
    g = np.float32(0.99)
    two = (carry * g).astype(np.float32) + reward[0]
    fused = (carry.astype(np.float64) * np.float64(g) + reward[0].astype(np.float64)).astype(np.float32)   # (exact product)
    assert (two != fused).sum() > N // 100
    ref = reward_normalize_reference(reward, np.zeros((1, N), bool), 0.99, 10.0, 1e-8, [0.0, 1.0, 1e-4], carry)
    assert np.array_equal(ref["discounted"][0].view(np.int32), two.view(np.int32))


# ------------------------------------------------------------------------------------------------------- the C surface
def test_symbols_declared_bound_exported(lib):
    from gym_dockauv_amd import _capi
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(dockauv_[a-z0-9_]+)\s*\(", text))
    for name in NEW:
        assert name in declared, f"{name} not declared in include/dockauv.h"
        assert name in {s[0] for s in _capi.SYMBOLS}, f"{name} not in _capi.SYMBOLS"
        assert hasattr(lib, name), f"{name} not exported by libdockauv.so"
    assert re.search(r"typedef\s+struct\s+dockauv_rewnorm_io\b", text)
    # the change only adds a struct and functions: the ABI version stays
    assert re.search(r"#define\s+DOCKAUV_ABI_VERSION\s+3\b", text) and lib.dockauv_abi_version() == 3 and _capi.ABI_VERSION == 3


def test_rewnorm_io_layout_matches_c(tmp_path):
    from gym_dockauv_amd import _capi
    fields = [f[0] for f in _capi.RewnormIO._fields_]
    assert fields == ["struct_size", "n_steps", "training", "reserved", "rows_out", "reward_norm", "discounted", "step_stats"]
    src = tmp_path / "layout.c"
    src.write_text(f'''
#include <stdio.h>
#include <stddef.h>
#include "{HEADER}"
int main(void) {{
  printf("%zu", sizeof(dockauv_rewnorm_io));
''' + "".join(f'  printf(" %zu", offsetof(dockauv_rewnorm_io, {f}));\n' for f in fields) + '''  printf("\\n");
  return 0;
}''')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-o", str(exe), str(src)])
    out = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    got = [C.sizeof(_capi.RewnormIO)] + [getattr(_capi.RewnormIO, f).offset for f in fields]
    assert out == got


def ios(_capi, K=4):
    """a dockauv_rewnorm_io, dockauv_collect_io and dockauv_truncation_io that agree, every pointer a small fake address that is
    never dereferenced: the calls below are refused first"""
    fake = lambda i: 64 * (i + 1)
    nio = _capi.RewnormIO()
    nio.struct_size, nio.n_steps, nio.training = C.sizeof(_capi.RewnormIO), K, 1
    nio.rows_out, nio.reward_norm, nio.discounted, nio.step_stats = fake(1), fake(10), fake(11), fake(12)
    cio = _capi.CollectIO()
    cio.struct_size, cio.n_steps = C.sizeof(_capi.CollectIO), K
    cio.rows_in, cio.rows_out, cio.actions_out, cio.terminal_obs = fake(0), fake(1), fake(2), fake(3)
    cio.values, cio.advantages, cio.returns = fake(4), fake(5), fake(6)
    cio.gamma, cio.gae_lambda = 0.99, 0.95
    tio = _capi.TruncationIO()
    tio.struct_size, tio.n_steps, tio.n_slots = C.sizeof(_capi.TruncationIO), K, 1
    tio.gamma, tio.gae_lambda = 0.99, 0.95
    tio.rows_out, tio.terminal_obs, tio.values, tio.advantages, tio.returns = fake(1), fake(3), fake(4), fake(5), fake(6)
    tio.length_carry, tio.trunc_step, tio.trunc_row, tio.v_terminal = fake(7), fake(8), fake(9), fake(13)
    return nio, cio, tio


def test_refusals_without_a_device(lib):
    """Every new entry point hands back DOCKAUV_E_INVALID for a NULL handle or object (destroy of NULL: 0), and everything that can
    be seen on the arguments alone is refused by name before the handle is looked at -- so without a device."""
    from gym_dockauv_amd import _capi
    fake = C.c_void_p(8)   # never dereferenced
    err = lambda: lib.dockauv_last_error(None)
    out = C.c_void_p()
    P = lambda x: C.c_void_p(x)

    # create / destroy / state / reset
    assert lib.dockauv_rewnorm_destroy(None) == 0
    assert lib.dockauv_rewnorm_create(None, 0.99, 10.0, 1e-8, C.byref(out)) == -1 and b"dockauv_rewnorm_create: null handle" in err()
    assert not out.value
    assert lib.dockauv_rewnorm_create(None, 0.99, 10.0, 1e-8, None) == -1 and b"out is NULL" in err()
    for gamma in (-0.1, 1.5, float("nan")):
        assert lib.dockauv_rewnorm_create(None, gamma, 10.0, 1e-8, C.byref(out)) == -1 and b"gamma" in err() and b"outside [0, 1]" in err()
    for clip in (0.0, -1.0, float("nan")):
        assert lib.dockauv_rewnorm_create(None, 0.99, clip, 1e-8, C.byref(out)) == -1 and b"clip_reward" in err()
    assert lib.dockauv_rewnorm_create(None, 0.99, 10.0, -1e-8, C.byref(out)) == -1 and b"epsilon" in err()
    s, c = C.c_void_p(), C.c_void_p()
    assert lib.dockauv_rewnorm_state(None, C.byref(s), C.byref(c)) == -1 and b"dockauv_rewnorm_state: null normaliser" in err()
    assert lib.dockauv_rewnorm_reset(None, None) == -1 and b"dockauv_rewnorm_reset: null normaliser" in err()

    # scan
    nio, cio, tio = ios(_capi)
    assert lib.dockauv_rewnorm_scan(None, fake, C.byref(nio), None) == -1 and b"dockauv_rewnorm_scan: null handle" in err()
    assert lib.dockauv_rewnorm_scan(None, None, None, None) == -1 and b"dockauv_rewnorm_io is NULL" in err()
    for field, value, needle in (("struct_size", 8, b"dockauv_rewnorm_io.struct_size"), ("n_steps", 0, b"dockauv_rewnorm_io.n_steps"),
                                 ("rows_out", None, b"dockauv_rewnorm_io.rows_out is NULL"),
                                 ("reward_norm", None, b"dockauv_rewnorm_io.reward_norm is NULL"),
                                 ("discounted", None, b"dockauv_rewnorm_io.discounted is NULL"),
                                 ("step_stats", None, b"dockauv_rewnorm_io.step_stats is NULL")):
        bad, _, _ = ios(_capi)
        setattr(bad, field, value)
        assert lib.dockauv_rewnorm_scan(None, fake, C.byref(bad), None) == -1 and needle in err(), (field, err())
    frozen, _, _ = ios(_capi)
    frozen.training, frozen.discounted, frozen.step_stats = 0, None, None     # both nullable when frozen: only the handle is missing
    assert lib.dockauv_rewnorm_scan(None, fake, C.byref(frozen), None) == -1 and b"null handle" in err()

    # GAE on the column
    gae = lambda rn=64, rows=128, val=256, K=4, g=0.99, lam=0.95, adv=320, ret=384, t=None: lib.dockauv_gae_normalized(
        None, fake, P(rn), t, P(rows), P(val), K, g, lam, P(adv), P(ret), None)
    assert gae() == -1 and b"dockauv_gae_normalized: null handle" in err()
    assert gae(rn=None) == -1 and b"reward_norm is NULL" in err()
    assert gae(val=None) == -1 and b"must not be NULL" in err()
    assert gae(K=0) == -1 and b"n_steps 0 must be >= 1" in err()
    assert gae(g=1.01) == -1 and b"gamma" in err()
    assert gae(lam=-0.5) == -1 and b"gae_lambda" in err()
    assert gae(t=C.byref(tio)) == -1 and b"null handle" in err()

    # the whole collection
    col = lambda c=cio, t=None, n=nio: lib.dockauv_collect_normalized(None, fake, fake, None if c is None else C.byref(c),
                                                                     None if t is None else C.byref(t), fake,
                                                                     None if n is None else C.byref(n), None)
    assert col() == -1 and b"dockauv_collect_normalized: null handle" in err()
    assert col(t=tio) == -1 and b"dockauv_collect_normalized: null handle" in err()
    assert col(c=None) == -1 and b"cio is NULL" in err()
    assert col(n=None) == -1 and b"dockauv_rewnorm_io is NULL" in err()
    bad = ios(_capi)[1]
    bad.values = None
    assert col(c=bad) == -1 and b"values/advantages/returns must not be NULL" in err()
    bad = ios(_capi)[1]
    bad.terminal_obs = None
    assert col(c=bad, t=tio) == -1 and b"dockauv_collect_io.terminal_obs is NULL" in err()
    assert col(c=bad) == -1 and b"null handle" in err()                       # (without a truncation block it is optional)
    bad = ios(_capi)[1]
    bad.gamma = 1.25
    assert col(c=bad) == -1 and b"gamma" in err()
    bad = ios(_capi, K=5)[0]
    assert col(n=bad) == -1 and b"dockauv_rewnorm_io.n_steps: 5, dockauv_collect_io's is 4" in err()
    bad = ios(_capi)[0]
    bad.rows_out = 4096
    assert col(n=bad) == -1 and b"dockauv_rewnorm_io.rows_out is not dockauv_collect_io's" in err()


def test_python_surface():
    from gym_dockauv_amd.envs.batched import BatchedDocking3d
    from gym_dockauv_amd.envs.torch_env import Collected, TorchDocking3d
    from gym_dockauv_amd.normalize import RewardNormalizer
    sig = inspect.signature(TorchDocking3d.collect)
    names = list(sig.parameters)
    assert names[-2:] == ["bootstrap_truncated", "reward_norm"] and sig.parameters["reward_norm"].default is None
    assert sig.parameters["bootstrap_truncated"].default is False and sig.parameters["monitor"].default is None
    assert Collected._fields == ("obs", "actions", "reward", "done", "log_prob", "values", "advantages", "returns")
    sig = inspect.signature(TorchDocking3d.make_reward_normalizer)
    assert [sig.parameters[n].default for n in ("clip_reward", "epsilon")] == [10.0, 1e-8]
    for name in ("make_reward_normalizer", "reward_normalizer_state", "reward_normalizer_reset", "reward_normalizer_scan_device",
                 "gae_normalized_device", "collect_normalized_device"):
        assert callable(getattr(BatchedDocking3d, name)), name
    for name in ("mean", "var", "count", "state_dict", "load_state_dict", "reset", "scan"):
        assert hasattr(RewardNormalizer, name), name


def test_documented():
    """the header states the order of the arithmetic and of the sums and the launch count; INTEGRATION.md, the README, DESIGN.md
    and the kernel coverage list know the new calls"""
    text = " ".join(open(HEADER).read().replace("\n *", "\n").split())
    for phrase in ("ret = carry * gamma + reward[k]", "never a fused multiply-add", "M2 = (var * count + batch_var * N) + (((delta * delta) * count) * N) / tot",
                   "den_k = sqrt(var + epsilon)", "lane t adds the elements t, t + 1 024", "four when training", "one otherwise",
                   "rb = fmaf(gamma, v_terminal[s][env], reward_norm[k][env])"):
        assert phrase in text, phrase
    kern = open(os.path.join(ROOT, "gym_dockauv_amd", "csrc", "dockauv_rewnorm.hip")).read()
    assert "FOUR launches" in kern and "__fmul_rn" in kern and "__fadd_rn" in kern and "atomic" not in kern.replace("no atomics", "")
    integration = " ".join(open(os.path.join(ROOT, "INTEGRATION.md")).read().split())
    for name in ("dockauv_collect_normalized", "dockauv_gae_normalized", "dockauv_rewnorm_scan", "reward_norm="):
        assert name in integration, name
    assert "dockauv_collect_normalized" in open(os.path.join(ROOT, "README.md")).read()
    assert "dockauv_rewnorm_scan" in open(os.path.join(ROOT, "DESIGN.md")).read()
    cov = open(os.path.join(ROOT, "profiles", "coverage", "kernels.txt")).read()
    for k in ("rewnorm_scan_kernel", "rewnorm_moments_kernel", "rewnorm_merge_kernel", "rewnorm_apply_kernel<false>", "rewnorm_apply_kernel<true>",
              "rewnorm_reset_kernel", "gae_kernel<GaeArgsCol>", "gae_kernel<GaeArgsTruncCol>", "test_gpu_rewnorm"):
        assert k in cov, k
