"""CPU: the replay buffer's surface and its NumPy statements (include/dockauv.h: dockauv_replay_*; gym_dockauv_amd/replay.py).
The new symbols are declared, bound and exported and the ABI is still 3; the two io structs have the layout of their ctypes
mirrors; every entry point refuses a NULL handle or buffer before it touches a device; one push of K steps leaves what K pushes
of one step leave (with a wrap inside the push and K = capacity); the sample indices are in range, advance with ``draws``,
depend on the seed and are uniform over the step slots; and the 64-bit record offset, compiled for the host, is exact beyond
2^39 bytes."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dockauv.h")
CSRC = os.path.join(ROOT, "gym_dockauv_amd", "csrc")

REPLAY_SYMBOLS = ["dockauv_replay_counts", "dockauv_replay_create", "dockauv_replay_destroy", "dockauv_replay_push",
                  "dockauv_replay_sample", "dockauv_replay_set_counts", "dockauv_replay_state", "dockauv_replay_sync"]


@pytest.fixture(scope="module")
def lib():
    from gym_dockauv_amd.csrc import build
    build.build()
    from gym_dockauv_amd import _capi
    return _capi.load_library()


def test_symbols_declared_bound_and_exported(lib):
    from gym_dockauv_amd import _capi
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = sorted(n for n in set(re.findall(r"\b(dockauv_[a-z0-9_]+)\s*\(", text)) if n.startswith("dockauv_replay_"))
    bound = sorted(s[0] for s in _capi.SYMBOLS if s[0].startswith("dockauv_replay_"))
    assert declared == REPLAY_SYMBOLS and bound == REPLAY_SYMBOLS
    assert sorted(s[0] for s in _capi.SYMBOLS[-len(REPLAY_SYMBOLS):]) == REPLAY_SYMBOLS, "the new entries of SYMBOLS are the last"
    for n in REPLAY_SYMBOLS:
        assert hasattr(lib, n), f"{n} not exported by libdockauv.so"
    assert _capi.ABI_VERSION == 3 and lib.dockauv_abi_version() == 3
    assert re.search(r"#define\s+DOCKAUV_ABI_VERSION\s+3\b", text)


def test_io_struct_layouts_match_c(tmp_path):
    from gym_dockauv_amd import _capi
    push = ["struct_size", "n_steps", "rows_in", "rows_out", "actions", "terminal_obs", "ep_outcome"]
    samp = ["struct_size", "n_batches", "batch_size", "obs", "actions", "next_obs", "rewards", "dones", "index"]
    items = (["sizeof(dockauv_replay_push_io)"] + [f"offsetof(dockauv_replay_push_io, {f})" for f in push]
             + ["sizeof(dockauv_replay_sample_io)"] + [f"offsetof(dockauv_replay_sample_io, {f})" for f in samp])
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(void) {\n%s  return 0;\n}\n'
                   % (HEADER, "".join(f'  printf("%zu\\n", (size_t){it});\n' for it in items)))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-o", str(exe), str(src)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    want = ([C.sizeof(_capi.ReplayPushIO)] + [getattr(_capi.ReplayPushIO, f).offset for f in push]
            + [C.sizeof(_capi.ReplaySampleIO)] + [getattr(_capi.ReplaySampleIO, f).offset for f in samp])
    assert got == want
    assert [f[0] for f in _capi.ReplayPushIO._fields_] == push and [f[0] for f in _capi.ReplaySampleIO._fields_] == samp


def test_entry_points_refuse_null_without_a_device(lib):
    from gym_dockauv_amd import _capi
    pio, sio = _capi.ReplayPushIO(), _capi.ReplaySampleIO()
    pio.struct_size, sio.struct_size = C.sizeof(pio), C.sizeof(sio)
    out = C.c_void_p()
    ll, u64, vp, ci = C.c_longlong(), C.c_uint64(), C.c_void_p(), C.c_int()
    invalid = {
        "create (null handle)": lambda: lib.dockauv_replay_create(None, 1000, 0, C.byref(out)),
        "sync (null handle)": lambda: lib.dockauv_replay_sync(None, None, None, None),
        "push (null handle)": lambda: lib.dockauv_replay_push(None, None, C.byref(pio), None),
        "push (null handle, null io)": lambda: lib.dockauv_replay_push(None, None, None, None),
        "sample (null handle)": lambda: lib.dockauv_replay_sample(None, None, C.byref(sio), None),
        "counts (null rb)": lambda: lib.dockauv_replay_counts(None, C.byref(ll), C.byref(ll), C.byref(u64)),
        "set_counts (null rb)": lambda: lib.dockauv_replay_set_counts(None, 0, 0, 0),
        "state (null rb)": lambda: lib.dockauv_replay_state(None, C.byref(vp), C.byref(vp), C.byref(ll), C.byref(ci)),
    }
    for name, call in invalid.items():
        assert call() == -1, name
        assert b"null" in lib.dockauv_last_error(None), name
    assert not out.value
    assert lib.dockauv_replay_destroy(None) == 0


# ------------------------------------------------------------------------------------------------- the push statement
def synthetic(rng, K, N, n_obs, n_u):
    rows = rng.standard_normal((K, N, n_obs + 2)).astype(np.float32)
    done = rng.random((K, N)) < 0.3
    rows[:, :, n_obs + 1] = done
    rows[rng.random(rows.shape) < 0.02] = np.float32(-0.0)
    rows[:, :, n_obs + 1] = done
    acts = rng.uniform(-1, 1, (K, N, n_u)).astype(np.float32)
    term = np.where(done[:, :, None], rng.standard_normal((K, N, n_obs)), np.nan).astype(np.float32)
    out = np.where(done, rng.integers(0, 5, (K, N)), 255).astype(np.uint8)
    return rows, acts, term, out


@pytest.mark.parametrize("n_obs,n_u", [(20, 6), (36, 3)])
def test_push_reference_one_push_of_k_is_k_pushes_of_one(n_obs, n_u):
    from gym_dockauv_amd.replay import record_floats, replay_push_reference
    rng = np.random.default_rng(11)
    cap, N = 5, 37
    R = record_floats(n_obs, n_u)
    assert R % 4 == 0 and 0 <= R - (2 * n_obs + n_u + 3) < 4
    a = (np.zeros((cap, N, R), np.float32), rng.standard_normal((N, n_obs)).astype(np.float32), 0, 0)
    b = a
    want_pos = [3, 1, 2, 2]
    for i, K in enumerate((3, 3, 1, 5)):        # a wrap inside the second push, K = capacity in the last
        rows, acts, term, out = synthetic(rng, K, N, n_obs, n_u)
        rows_in = rng.standard_normal((N, n_obs + 2)).astype(np.float32) if i == 0 else None
        a = replay_push_reference(*a, rows_in, rows, acts, term, out)
        for k in range(K):
            b = replay_push_reference(*b, rows_in if k == 0 else None, rows[k:k + 1], acts[k:k + 1], term[k:k + 1], out[k:k + 1])
        assert a[2] == b[2] == want_pos[i] and a[3] == b[3] == min(sum((3, 3, 1, 5)[:i + 1]), cap)
        assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
        assert not np.isnan(a[0]).any(), "a terminal observation was read where not done"
        # the fields of the newest step slot, read back
        s = (a[2] - 1) % cap
        d = rows[K - 1, :, n_obs + 1] > 0.5
        o3 = 2 * n_obs + n_u
        assert np.array_equal(a[0][s, :, o3 + 1], d.astype(np.float32))
        assert np.array_equal(a[0][s, :, o3 + 2], (d & (out[K - 1] == 3)).astype(np.float32))
        assert np.array_equal(a[0][s, :, o3].view(np.uint32), rows[K - 1, :, n_obs].view(np.uint32))
        assert np.array_equal(a[0][s, d, n_obs:2 * n_obs].view(np.uint32), term[K - 1, d].view(np.uint32))
        assert (a[0][s, :, o3 + 3:] == 0).all()
    # without ep_outcome no timeout anywhere
    c = replay_push_reference(np.zeros((cap, N, R), np.float32), a[1], 0, 0, None, rows, acts, term, None)
    assert (c[0][:, :, 2 * n_obs + n_u + 2] == 0).all()


# ------------------------------------------------------------------------------------------------- the index statement
def test_indices_reference():
    from gym_dockauv_amd.replay import replay_indices_reference as ref
    seed, size, N = 0x1234_5678_9ABC_DEF0, 5, 200
    two = ref(seed, 7, 333, 2, size, N)
    assert two.shape == (2, 333) and two.dtype == np.int64
    assert two.min() >= 0 and two.max() < size * N
    assert np.array_equal(two[0], ref(seed, 7, 333, 1, size, N)[0]) and np.array_equal(two[1], ref(seed, 8, 333, 1, size, N)[0])
    assert not np.array_equal(two[0], two[1])
    assert not np.array_equal(two, ref(seed + 1, 7, 333, 2, size, N)), "the seed's low word is not in the key"
    assert not np.array_equal(two, ref(seed + (1 << 32), 7, 333, 2, size, N)), "the seed's high word is not in the key"
    # draws beyond 2^32 reach the counter's third word
    assert not np.array_equal(ref(seed, 7, 333, 1, size, N), ref(seed, 7 + (1 << 32), 333, 1, size, N))
    # a partly filled ring: nothing beyond size
    assert ref(seed, 0, 4096, 1, 3, N).max() < 3 * N
    assert (ref(seed, 0, 64, 1, 1, 1) == 0).all()


def test_indices_reference_is_uniform_over_the_step_slots():
    from gym_dockauv_amd.replay import replay_indices_reference as ref
    B, size, N = 100_000, 5, 200
    idx = ref(2024, 0, B, 1, size, N)[0]
    counts = np.bincount(idx // N, minlength=size)
    sd = math.sqrt(B * (1 / size) * (1 - 1 / size))
    print("step-slot counts", counts.tolist(), "5 sd =", 5 * sd)
    assert counts.sum() == B and (np.abs(counts - B / size) <= 5 * sd).all(), counts
    env_counts = np.bincount(idx % N, minlength=N)
    sd_e = math.sqrt(B * (1 / N) * (1 - 1 / N))
    assert (np.abs(env_counts - B / N) <= 5 * sd_e).all()


# ------------------------------------------------------------------------------------------------- 64-bit offsets on the host
@pytest.fixture(scope="module")
def offset_exe(tmp_path_factory):
    exe = tmp_path_factory.mktemp("replay") / "replay_offset_host"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC,
                           os.path.join(ROOT, "tests", "replay_offset_host.cpp"), "-o", str(exe)])
    return str(exe)


def test_record_offsets_are_64_bit(offset_exe):
    from gym_dockauv_amd.replay import record_floats
    run = lambda *a: [int(x) for x in subprocess.check_output([offset_exe, *map(str, a)]).decode().split()]
    slot = 2 ** 31 + 5
    floats, nbytes = run(slot, 84)
    assert floats == slot * 84 and nbytes == slot * 84 * 4 and nbytes > 2 ** 39
    # step slot x n_envs + env beyond 2^32 records: 40 000 steps of 131 072 envs
    assert run("index", 40_000, 131_072, 131_071) == [40_000 * 131_072 + 131_071]
    for n_obs, n_u in ((20, 6), (36, 3), (36, 6), (36, 8), (16, 1)):
        assert run("floats", n_obs, n_u) == [record_floats(n_obs, n_u)]
    for x, n in ((0xFFFFFFFF, 5), (0x80000000, 5), (0x33333333, 5), (0x33333334, 5), (0xFFFFFFFF, 2 ** 31 - 1), (12345, 1)):
        assert run("mulshift", x, n) == [(x * n) >> 32]
