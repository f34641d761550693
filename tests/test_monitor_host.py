"""
Episode monitor, host side (no GPU): the NumPy statement of dockauv_monitor_scan (gym_dockauv_amd/monitor.py:
episode_scan_reference) against every finished episode of the committed golden trajectories -- lengths, returns and the outcome
rule against the reference's own condition bits --, and the C surface: symbols declared, bound and exported, ABI 3, the ctypes
mirror of dockauv_monitor_io, NULL arguments refused by name before any device call.
"""
import ctypes as C
import glob
import math
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dockauv.h")
GOLDEN = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "traj_*.npz")))
NEW = ["dockauv_monitor_create", "dockauv_monitor_destroy", "dockauv_monitor_sync", "dockauv_monitor_scan", "dockauv_monitor_carry"]


@pytest.fixture(scope="module")
def lib():
    from gym_dockauv_amd import _capi
    return _capi.load_library()


@pytest.fixture(scope="module")
def scans():
    """every golden trajectory as one env of K steps through the restatement, computed once: (name, npz, result)"""
    from gym_dockauv_amd.monitor import episode_scan_reference
    out = []
    for path in GOLDEN:
        g = np.load(path)
        K = g["done"].shape[0]
        res = episode_scan_reference(g["reward"].reshape(K, 1), g["done"].reshape(K, 1), np.zeros(1, np.float32), np.zeros(1, np.int32),
                                     int(g["meta_max_timesteps"]), terminal_obs=g["obs"].reshape(K, 1, -1))
        out.append((os.path.basename(path), g, res))
    return out


def test_golden_set_is_the_one_the_rule_was_checked_on(scans):
    assert len(scans) == 25
    n = sum(int(g["done"].sum()) for _, g, _ in scans)
    assert n == 73, n
    counts = np.zeros(5, dtype=int)
    for _, g, res in scans:
        counts += np.bincount(res["ep_outcome"][g["done"].reshape(-1, 1)], minlength=5)
    # goal, out of range, attitude, time limit, collision
    assert counts.tolist() == [8, 3, 20, 24, 18], counts.tolist()


def test_lengths_from_done_alone_are_the_episode_starts(scans):
    for name, g, res in scans:
        done = g["done"]
        ends = np.flatnonzero(done)
        starts = np.asarray(g["ep_start"], dtype=np.int64)
        bounds = np.concatenate([starts, [done.shape[0]]])
        want = np.diff(bounds)[: len(ends)]
        got = res["ep_length"][ends, 0]
        assert got.tolist() == want.tolist(), name
        assert np.array_equal(ends + 1, bounds[1: len(ends) + 1]), name
        # the running length of the unfinished tail
        tail = done.shape[0] - (ends[-1] + 1 if len(ends) else 0)
        assert int(res["carry_length"][0]) == tail, name
        assert res["stats"][0] == len(ends) and res["stats"][3] == want.sum(), name


def test_returns_within_the_float32_accumulation_bound(scans):
    checked = 0
    for name, g, res in scans:
        ends = np.flatnonzero(g["done"])
        start = 0
        for e in ends:
            r = g["reward"][start: e + 1]
            n = e + 1 - start
            # the restatement adds the float32 of each reward: the conversions cost 2^-24 sum |r| together, each of the n - 1
            # inexact adds (the first, to a zero carry, is exact) at most 2^-24 of a partial sum, which never exceeds sum |r|
            bound = n * 2.0 ** -24 * math.fsum(np.abs(r))
            got = float(res["ep_return"][e, 0])
            assert abs(got - math.fsum(r)) <= bound, (name, int(e), got, math.fsum(r), bound)
            start = e + 1
            checked += 1
    assert checked == 73


def test_outcome_bits_and_code_are_the_references(scans):
    checked = 0
    for name, g, res in scans:
        for e in np.flatnonzero(g["done"]):
            cond = g["conditions"][e]
            assert cond.any(), (name, int(e))
            bits = int(res["ep_bits"][e, 0])
            assert [bool(bits >> i & 1) for i in range(4)] == cond[:4].tolist(), (name, int(e), bits, cond.tolist())
            assert int(res["ep_outcome"][e, 0]) == int(np.flatnonzero(cond)[0]), (name, int(e))
            if cond[3]:
                assert int(res["ep_length"][e, 0]) == int(g["meta_max_timesteps"]) + 1, (name, int(e))
            checked += 1
        # rows that are not done hold nothing
        nd = ~g["done"]
        assert not res["ep_outcome"][nd].any() and not res["ep_bits"][nd].any() and not res["ep_length"][nd].any()
    assert checked == 73


def test_restatement_carries_across_calls_and_without_terminal_obs():
    from gym_dockauv_amd.monitor import episode_scan_reference, explained_variance_reference, summary_from_stats
    rng = np.random.default_rng(3)
    K, N = 23, 7
    r = rng.normal(size=(K, N)).astype(np.float32)
    d = rng.random((K, N)) < 0.2
    whole = episode_scan_reference(r, d, np.zeros(N, np.float32), np.zeros(N, np.int32), 5)
    a = episode_scan_reference(r[:9], d[:9], np.zeros(N, np.float32), np.zeros(N, np.int32), 5)
    b = episode_scan_reference(r[9:], d[9:], a["carry_return"], a["carry_length"], 5)
    assert np.array_equal(np.concatenate([a["ep_return"], b["ep_return"]]).view(np.int32), whole["ep_return"].view(np.int32))
    assert np.array_equal(np.concatenate([a["ep_length"], b["ep_length"]]), whole["ep_length"])
    assert np.array_equal(b["carry_return"].view(np.int32), whole["carry_return"].view(np.int32))
    assert whole["stats"][0] == d.sum() and not whole["stats"][8:14].any() and np.isnan(whole["stats"][14])
    s = summary_from_stats(whole["stats"])
    rets = whole["ep_return"][d].astype(np.float64)
    assert s["n_episodes"] == d.sum() and abs(s["rollout/ep_rew_mean"] - rets.mean()) < 1e-12
    assert abs(s["ep_rew_std"] - rets.std()) < 1e-9 and abs(s["rollout/ep_len_mean"] - whole["ep_length"][d].mean()) < 1e-12
    assert math.isnan(s["goal_rate"]) and math.isnan(s["train/explained_variance"])
    empty = episode_scan_reference(r[:2], np.zeros((2, N), bool), np.zeros(N, np.float32), np.zeros(N, np.int32), 5)
    assert empty["stats"][0] == 0 and np.isnan(empty["stats"][4:8]).all()
    v = rng.normal(size=(K + 1, N)).astype(np.float32)
    y = rng.normal(size=(K, N)).astype(np.float32)
    want = 1.0 - np.var((y - v[:K]).astype(np.float64)) / np.var(y.astype(np.float64))
    assert abs(explained_variance_reference(v, y) - want) < 1e-12
    assert math.isnan(explained_variance_reference(v, np.full((K, N), 2.5, np.float32)))
    with pytest.raises(ValueError):
        episode_scan_reference(r, d[:3], np.zeros(N, np.float32), np.zeros(N, np.int32), 5)


def test_symbols_declared_bound_exported(lib):
    from gym_dockauv_amd import _capi
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(dockauv_[a-z0-9_]+)\s*\(", text))
    for name in NEW:
        assert name in declared, f"{name} not declared in include/dockauv.h"
        assert name in {s[0] for s in _capi.SYMBOLS}, f"{name} not in _capi.SYMBOLS"
        assert hasattr(lib, name), f"{name} not exported by libdockauv.so"
    assert re.search(r"typedef\s+struct\s+dockauv_monitor_io\b", text)
    assert re.search(r"typedef\s+struct\s+dockauv_monitor_s\s*\*\s*dockauv_monitor\s*;", text)
    # the change only adds a struct and functions: the ABI version stays
    assert re.search(r"#define\s+DOCKAUV_ABI_VERSION\s+3\b", text) and lib.dockauv_abi_version() == 3 and _capi.ABI_VERSION == 3


def test_monitor_io_layout_matches_c(tmp_path):
    from gym_dockauv_amd import _capi
    fields = [f[0] for f in _capi.MonitorIO._fields_]
    assert fields == ["struct_size", "n_steps", "rows_out", "terminal_obs", "values", "returns", "ep_return", "ep_length",
                      "ep_outcome", "stats"]
    src = tmp_path / "layout.c"
    src.write_text(f'''
#include <stdio.h>
#include <stddef.h>
#include "{HEADER}"
int main(void) {{
  printf("%zu", sizeof(dockauv_monitor_io));
''' + "".join(f'  printf(" %zu", offsetof(dockauv_monitor_io, {f}));\n' for f in fields) + '''  printf("\\n");
  return 0;
}''')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-o", str(exe), str(src)])
    out = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    got = [C.sizeof(_capi.MonitorIO)] + [getattr(_capi.MonitorIO, f).offset for f in fields]
    assert out == got


def test_null_arguments_refused_without_a_device(lib):
    from gym_dockauv_amd import _capi
    io = _capi.MonitorIO()
    io.struct_size = C.sizeof(_capi.MonitorIO)
    fake = C.c_void_p(8)   # never dereferenced: the calls are refused first
    out = C.c_void_p()
    err = lambda: lib.dockauv_last_error(None)
    assert lib.dockauv_monitor_create(None, C.byref(out)) == -1 and b"dockauv_monitor_create: null handle" in err()
    assert not out.value
    assert lib.dockauv_monitor_scan(None, fake, C.byref(io), None) == -1 and b"dockauv_monitor_scan: null handle" in err()
    assert lib.dockauv_monitor_scan(None, None, None, None) == -1 and b"dockauv_monitor_scan: null handle" in err()
    assert lib.dockauv_monitor_sync(None, None) == -1 and b"dockauv_monitor_sync: null monitor" in err()
    assert lib.dockauv_monitor_carry(None, None, None) == -1 and b"dockauv_monitor_carry: null monitor" in err()
    assert lib.dockauv_monitor_destroy(None) == 0


def test_documented(lib):
    """the header states the scan's order and the rule's two limits; INTEGRATION.md, the README and the kernel coverage list
    know the monitor"""
    text = " ".join(open(HEADER).read().replace("\n *", "\n").split())
    for phrase in ("ret = carry_return + reward[k]", "within one float32 rounding of a threshold", "reported under the lower index",
                   "last 100 episodes"):
        assert phrase in text, phrase
    for path in ("INTEGRATION.md", "README.md"):
        assert "dockauv_monitor_scan" in open(os.path.join(ROOT, path)).read(), path
    cov = open(os.path.join(ROOT, "profiles", "coverage", "kernels.txt")).read()
    for k in ("monitor_scan_kernel", "monitor_ev_kernel", "monitor_final_kernel"):
        assert k in cov, k
