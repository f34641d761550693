"""
Policy evaluation with an episode quota per env, host side (no GPU): SB3's ``episode_count_targets`` rule, the NumPy statement of
dockauv_eval_scan (gym_dockauv_amd/evaluate.py: evaluation_scan_reference) -- chunking, its slots against
``episode_scan_reference`` read in step order, the length bias of a fixed window on crafted data --, and the C surface: symbols
declared, bound and exported, the ctypes mirror of dockauv_eval_io, refusals by name before any device call, the Python surface,
the documents.  `crafted` below is also what tests/test_gpu_eval.py feeds the kernels.
"""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dockauv.h")
NEW = ["dockauv_eval_create", "dockauv_eval_destroy", "dockauv_eval_begin", "dockauv_eval_scan", "dockauv_eval_state"]
STATE_KEYS = ("carry_return", "carry_length", "count", "target", "ep_return", "ep_length", "ep_outcome")


@pytest.fixture(scope="module")
def lib():
    from gym_dockauv_amd.csrc import build
    build.build()
    from gym_dockauv_amd import _capi
    return _capi.load_library()


def crafted(K, N, n_obs, seed, p_done=0.3):
    """(rows float32 [K, N, n_obs + 2], reward, done, terminal rows): reward U(-1, 1); done with p = 0.3 -- so that envs finish
    more episodes than a quota of 3 in 57 steps and others fewer -- plus dones at k = 0 (envs 0-3) and k = K - 1 (envs 4-7) and
    none at all for env 8 (N > 8); observation columns NaN (never read).  Terminal rows: NaN except columns 0, 6, 7 where done,
    which cycle through goal, out of range, obs[6] = +1, -1, obs[7] = +1, -1 and two rows off every threshold (time limit or
    collision by length)."""
    rng = np.random.default_rng(seed)
    reward = rng.uniform(-1, 1, (K, N)).astype(np.float32)
    done = rng.random((K, N)) < p_done
    done[0, 0:4] = True
    done[K - 1, 4:8] = True
    if N > 8:
        done[:, 8] = False
    rows = np.full((K, N, n_obs + 2), np.nan, dtype=np.float32)
    rows[:, :, n_obs] = reward
    rows[:, :, n_obs + 1] = done
    term = np.full((K, N, n_obs), np.nan, dtype=np.float32)
    ks, es = np.nonzero(done)
    pat = (np.arange(ks.size) + seed) % 8
    term[ks, es, 0] = np.where(pat == 0, 0.0, np.where(pat == 1, 1.0, 0.5))
    term[ks, es, 6] = np.where(pat == 2, 1.0, np.where(pat == 3, -1.0, 0.3))
    term[ks, es, 7] = np.where(pat == 4, 1.0, np.where(pat == 5, -1.0, -0.2))
    return rows, reward, done, term


def same_state(a, b):
    for k in STATE_KEYS:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.dtype == y.dtype and x.shape == y.shape, k
        assert np.array_equal(x.view(np.int32) if x.dtype == np.float32 else x, y.view(np.int32) if y.dtype == np.float32 else y), k


# ------------------------------------------------------------------------------------------------------- the NumPy statement
@pytest.mark.parametrize("n_eval,N", [(1000, 64), (100, 129), (129, 129), (5, 1)])
def test_evaluation_targets_are_sb3s(n_eval, N):
    from gym_dockauv_amd.evaluate import evaluation_targets
    got = evaluation_targets(n_eval, N)
    want = np.array([(n_eval + i) // N for i in range(N)], dtype="int")      # (evaluate_policy's line, verbatim)
    assert got.dtype == np.int32 and got.shape == (N,) and np.array_equal(got, want)
    assert int(got.sum()) == n_eval
    if (n_eval, N) == (100, 129):
        assert (got[:29] == 0).all() and (got[29:] == 1).all()
    with pytest.raises(ValueError):
        evaluation_targets(0, N)


def test_one_scan_of_57_is_three_of_19():
    from gym_dockauv_amd.evaluate import evaluation_scan_reference, evaluation_state, evaluation_targets
    N, S, T = 129, 3, 3
    _, reward, done, term = crafted(57, N, 20, seed=11)
    s0 = evaluation_state(evaluation_targets(300, N), S)
    keep = {k: v.copy() for k, v in s0.items()}
    one, st_one = evaluation_scan_reference(reward, done, s0, T, terminal_obs=term)
    same_state(s0, keep)                                    # (the input state is not modified)
    st, stats = s0, None
    for i in range(3):
        sl = slice(19 * i, 19 * i + 19)
        st, stats = evaluation_scan_reference(reward[sl], done[sl], st, T, terminal_obs=term[sl])
    same_state(one, st)
    assert np.array_equal(st_one.view(np.int64), stats.view(np.int64))
    # the quota bites for some envs and not for others
    n_done = done.sum(axis=0)
    assert (n_done > one["target"]).any() and (n_done < one["target"]).any()
    assert np.array_equal(one["count"], np.minimum(n_done, one["target"]))
    assert st_one[15] == (one["target"] - one["count"]).sum() > 0
    # slots nothing reached keep 0 / 0 / 255
    free = np.arange(S)[:, None] >= one["count"][None, :]
    assert not one["ep_return"][free].any() and not one["ep_length"][free].any() and (one["ep_outcome"][free] == 255).all()
    assert (one["ep_outcome"][~free] < 5).all()


def test_with_every_target_at_k_the_slots_are_the_monitors_rows():
    """target = S = K: nothing is cut, so env i's slots are ``episode_scan_reference``'s per-row outputs where done, in step order"""
    from gym_dockauv_amd.evaluate import evaluation_scan_reference, evaluation_state
    from gym_dockauv_amd.monitor import episode_scan_reference
    K, N, T = 19, 70, 3
    _, reward, done, term = crafted(K, N, 20, seed=5)
    rng = np.random.default_rng(1)
    c_ret, c_len = rng.uniform(-2, 2, N).astype(np.float32), rng.integers(0, T + 1, N).astype(np.int32)   # mid-trajectory carries
    ref = episode_scan_reference(reward, done, c_ret, c_len, T, terminal_obs=term)
    st, stats = evaluation_scan_reference(reward, done, evaluation_state(np.full(N, K), K, c_ret, c_len), T, terminal_obs=term)
    for env in range(N):
        ks = np.flatnonzero(done[:, env])
        assert st["count"][env] == ks.size
        assert np.array_equal(st["ep_return"][: ks.size, env].view(np.int32), ref["ep_return"][ks, env].view(np.int32))
        assert np.array_equal(st["ep_length"][: ks.size, env], ref["ep_length"][ks, env])
        assert np.array_equal(st["ep_outcome"][: ks.size, env], ref["ep_outcome"][ks, env])
    assert np.array_equal(st["carry_return"].view(np.int32), ref["carry_return"].view(np.int32))
    assert np.array_equal(st["carry_length"], ref["carry_length"])
    # the same episodes: the monitor's stats, entry 15 aside (fsum is exact, so the order of the terms does not show)
    assert np.array_equal(stats[:14], ref["stats"][:14]) and np.isnan(stats[14]) and stats[15] == N * K - done.sum()
    # without terminal observations: outcome 255, nothing classified
    st_nt, stats_nt = evaluation_scan_reference(reward, done, evaluation_state(np.full(N, K), K, c_ret, c_len), T)
    rec = np.arange(K)[:, None] < st_nt["count"][None, :]
    assert (st_nt["ep_outcome"] == 255).all() and rec.sum() == done.sum() and not stats_nt[8:14].any()
    assert np.array_equal(stats_nt[:8], stats[:8])


def length_bias_data(K):
    """64 envs, reward 1 per step: envs 0-31 finish every 2 steps on a collision-coded terminal observation, envs 32-63 every 10
    steps on the goal (t[0] == 0)"""
    N, n_obs = 64, 9
    reward = np.ones((K, N), dtype=np.float32)
    done = np.zeros((K, N), dtype=bool)
    done[1::2, :32] = True
    done[9::10, 32:] = True
    term = np.full((K, N, n_obs), 0.5, dtype=np.float32)      # off every threshold; lengths 2 <= max_timesteps: collision
    term[:, 32:, 0] = 0.0
    return reward, done, term


def test_length_bias_on_crafted_data():
    from gym_dockauv_amd.evaluate import evaluation_scan_reference, evaluation_state
    from gym_dockauv_amd.monitor import episode_scan_reference, summary_from_stats
    N, T = 64, 50
    reward, done, term = length_bias_data(20)
    window = summary_from_stats(episode_scan_reference(reward, done, np.zeros(N, np.float32), np.zeros(N, np.int32), T,
                                                       terminal_obs=term)["stats"])
    assert window["n_episodes"] == 384 and window["goal_rate"] == 64 / 384 == 1 / 6 and window["collision_rate"] == 320 / 384
    st, stats = evaluation_scan_reference(reward, done, evaluation_state(np.ones(N, np.int32), 1), T, terminal_obs=term)
    quota = summary_from_stats(stats)
    assert quota["goal_rate"] == 0.5 and quota["collision_rate"] == 0.5 and quota["n_episodes"] == 64
    assert quota["rollout/ep_rew_mean"] == 6.0 and quota["rollout/ep_len_mean"] == 6.0 and stats[15] == 0
    assert (st["ep_outcome"][0, :32] == 4).all() and (st["ep_outcome"][0, 32:] == 0).all()
    # target 2 after only 10 steps: the slow envs have one episode each
    st2, stats2 = evaluation_scan_reference(reward[:10], done[:10], evaluation_state(np.full(N, 2), 2), T, terminal_obs=term[:10])
    assert stats2[15] == 32 and stats2[0] == 96 and (st2["count"][:32] == 2).all() and (st2["count"][32:] == 1).all()


# ------------------------------------------------------------------------------------------------------- the C surface
def test_symbols_declared_bound_exported(lib):
    from gym_dockauv_amd import _capi
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(dockauv_[a-z0-9_]+)\s*\(", text))
    for name in NEW:
        assert name in declared, f"{name} not declared in include/dockauv.h"
        assert name in {s[0] for s in _capi.SYMBOLS}, f"{name} not in _capi.SYMBOLS"
        assert hasattr(lib, name), f"{name} not exported by libdockauv.so"
    assert re.search(r"typedef\s+struct\s+dockauv_eval_io\b", text) and re.search(r"typedef\s+struct\s+dockauv_eval_s\s*\*\s*dockauv_eval\s*;", text)
    # the change only adds a struct and functions: the ABI version stays
    assert re.search(r"#define\s+DOCKAUV_ABI_VERSION\s+3\b", text) and lib.dockauv_abi_version() == 3 and _capi.ABI_VERSION == 3


def test_eval_io_layout_matches_c(tmp_path):
    from gym_dockauv_amd import _capi
    fields = [f[0] for f in _capi.EvalIO._fields_]
    assert fields == ["struct_size", "n_steps", "rows_out", "terminal_obs", "stats"]
    src = tmp_path / "layout.c"
    src.write_text(f'''
#include <stdio.h>
#include <stddef.h>
#include "{HEADER}"
int main(void) {{
  printf("%zu", sizeof(dockauv_eval_io));
''' + "".join(f'  printf(" %zu", offsetof(dockauv_eval_io, {f}));\n' for f in fields) + '''  printf("\\n");
  return 0;
}''')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-o", str(exe), str(src)])
    out = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    got = [C.sizeof(_capi.EvalIO)] + [getattr(_capi.EvalIO, f).offset for f in fields]
    assert out == got


def eval_io(_capi, K=4):
    """a dockauv_eval_io whose pointers are small fake addresses, never dereferenced: the calls below are refused first"""
    io = _capi.EvalIO()
    io.struct_size, io.n_steps = C.sizeof(_capi.EvalIO), K
    io.rows_out, io.terminal_obs, io.stats = 64, 128, 192
    return io


def test_refusals_without_a_device(lib):
    """Every entry point hands back DOCKAUV_E_INVALID for a NULL handle or object (destroy of NULL: 0), and everything that can
    be seen on the arguments alone is refused by name before the handle is looked at -- so without a device.  (A float64 handle,
    DOCKAUV_RESET_NONE, an evaluator of another handle, the 2^31 limit and a uniform target outside [0, S] need a live handle or
    evaluator: tests/test_gpu_eval.py.)"""
    from gym_dockauv_amd import _capi
    fake = C.c_void_p(8)   # never dereferenced
    err = lambda: lib.dockauv_last_error(None)
    out = C.c_void_p()

    assert lib.dockauv_eval_destroy(None) == 0
    assert lib.dockauv_eval_create(None, 2, C.byref(out)) == -1 and b"dockauv_eval_create: null handle" in err()
    assert not out.value
    assert lib.dockauv_eval_create(None, 2, None) == -1 and b"out is NULL" in err()
    for S in (0, -3):
        assert lib.dockauv_eval_create(None, S, C.byref(out)) == -1 and b"max_episodes_per_env" in err() and b"must be >= 1" in err()
    assert lib.dockauv_eval_begin(None, None, 1, None) == -1 and b"dockauv_eval_begin: null evaluator" in err()
    ptrs = [C.c_void_p() for _ in range(7)]
    assert lib.dockauv_eval_state(None, *[C.byref(p) for p in ptrs]) == -1 and b"dockauv_eval_state: null evaluator" in err()
    assert lib.dockauv_eval_state(None, *[None] * 7) == -1

    io = eval_io(_capi)
    assert lib.dockauv_eval_scan(None, fake, C.byref(io), None) == -1 and b"dockauv_eval_scan: null handle" in err()
    assert lib.dockauv_eval_scan(None, None, None, None) == -1 and b"dockauv_eval_scan: io is NULL" in err()
    for field, value, needle in (("struct_size", 8, b"dockauv_eval_io.struct_size"), ("n_steps", 0, b"dockauv_eval_io.n_steps"),
                                 ("n_steps", -1, b"dockauv_eval_io.n_steps"),
                                 ("rows_out", None, b"dockauv_eval_io.rows_out is NULL"),
                                 ("stats", None, b"dockauv_eval_io.stats is NULL")):
        bad = eval_io(_capi)
        setattr(bad, field, value)
        assert lib.dockauv_eval_scan(None, fake, C.byref(bad), None) == -1 and needle in err(), (field, err())
    ok = eval_io(_capi)
    ok.terminal_obs = None                                   # nullable: only the handle is missing
    assert lib.dockauv_eval_scan(None, fake, C.byref(ok), None) == -1 and b"null handle" in err()


def test_python_surface():
    from gym_dockauv_amd.envs.batched import BatchedDocking3d
    from gym_dockauv_amd.envs.torch_env import Collected, TorchDocking3d
    from gym_dockauv_amd.evaluate import Evaluator
    for name in ("make_evaluator", "evaluator_begin", "evaluator_scan_device", "evaluator_state"):
        assert callable(getattr(BatchedDocking3d, name)), name
    for name in ("begin", "scan", "missing", "episodes", "summary"):
        assert callable(getattr(Evaluator, name)), name
    sig = inspect.signature(Evaluator.begin)
    assert sig.parameters["targets"].default is None and sig.parameters["uniform"].default == 1
    assert inspect.signature(Evaluator.scan).parameters["terminal_obs"].default is None
    assert list(inspect.signature(TorchDocking3d.make_evaluator).parameters) == ["self", "max_episodes_per_env"]
    sig = inspect.signature(TorchDocking3d.evaluate)
    assert list(sig.parameters) == ["self", "policy", "n_eval_episodes", "deterministic", "seed", "n_steps", "return_episode_rewards",
                                    "evaluator"]
    assert [sig.parameters[n].default for n in ("deterministic", "seed", "n_steps", "return_episode_rewards", "evaluator")] == \
        [True, None, None, False, None]
    # collect is what it was
    sig = inspect.signature(TorchDocking3d.collect)
    assert list(sig.parameters) == ["self", "policy", "value", "n_steps", "gamma", "gae_lambda", "stochastic", "want_terminal_obs",
                                    "monitor", "bootstrap_truncated", "reward_norm"]
    assert Collected._fields == ("obs", "actions", "reward", "done", "log_prob", "values", "advantages", "returns")
    sig = inspect.signature(TorchDocking3d.rollout)
    assert list(sig.parameters) == ["self", "policy", "n_steps", "stochastic", "want_terminal_obs", "monitor"]


def test_documented():
    """the header states the arithmetic, the order of the sums and the launch count; INTEGRATION.md names the interfaces
    replaced; the README, DESIGN.md and the kernel coverage list know the new calls"""
    text = " ".join(open(HEADER).read().replace("\n *", "\n").split())
    for phrase in ("ret = carry_return + reward[k]", "if count < target: slot[count][env] = (ret, len, code); count += 1",
                   "clamped in the kernel", "a lane adds its own slots j = 0 .. count - 1 in order", "lane t the groups t, t + 1 024",
                   "Launches: two a scan", "15 the episodes still missing", "(n_eval_episodes + i) / n_envs"):
        assert phrase in text, phrase
    kern = open(os.path.join(ROOT, "gym_dockauv_amd", "csrc", "dockauv_eval.hip")).read()
    assert "TWO launches" in kern and "asm" not in kern and "atomic" not in kern.lower().replace("no atomics", "")
    integration = " ".join(open(os.path.join(ROOT, "INTEGRATION.md")).read().split())
    for name in ("dockauv_eval_scan", "dockauv_eval_begin", "evaluate_policy", "predict(", "env.evaluate("):
        assert name in integration, name
    assert "dockauv_eval_scan" in open(os.path.join(ROOT, "README.md")).read()
    assert "dockauv_eval_scan" in open(os.path.join(ROOT, "DESIGN.md")).read()
    cov = open(os.path.join(ROOT, "profiles", "coverage", "kernels.txt")).read()
    for k in ("eval_begin_kernel", "eval_scan_kernel", "eval_final_kernel", "test_gpu_eval"):
        assert k in cov, k
