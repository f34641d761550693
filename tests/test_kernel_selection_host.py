"""CPU: which step kernel serves a call is decided by plain host functions (gym_dockauv_amd/csrc/dockauv_device.h: select_step,
select_sequence, choose_threads).  tests/kernel_selection_host.cpp prints their answers over a grid -- both precisions, both
kinetics paths, the four vehicle kinds, with and without obstacles, 64 / 128 / 256 / 512 threads, 262 144 and 262 208 envs,
fans padded to 16 / 32 / 64 lanes, ten kinds of request; for the group shape every batch-size boundary and the value above
it -- and the table must equal tests/golden/kernel_selection.txt line for line.  The golden table was printed by the
launchers as they stood before the selection became one function (their text compiled with stub kernels), so a changed
line is a call that now gets another kernel."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gym_dockauv_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "kernel_selection.txt")


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    exe = tmp_path_factory.mktemp("selection") / "kernel_selection_host"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC,
                           os.path.join(ROOT, "tests", "kernel_selection_host.cpp"), "-o", str(exe)])
    return subprocess.check_output([str(exe)]).decode().splitlines()


def test_selection_table_is_the_golden_one(table):
    golden = open(GOLDEN).read().splitlines()
    assert len(golden) > 400 and os.path.getsize(GOLDEN) < 100_000
    changed = [(g, t) for g, t in zip(golden, table) if g != t]
    assert not changed and len(golden) == len(table), (len(golden), len(table), changed[:5])


def test_group_shapes_of_the_baseline_configs(table):
    """The expectations of tests/test_gpu_fullsize.py::test_group_shape_the_library_picks, through choose_threads."""
    expect = {(2, 4096): 256, (2, 131072): 128, (2, 262144): 64,
              (3, 65536): 256, (3, 262144): 64,
              (4, 32768): 512, (4, 65536): 256, (4, 196608): 256, (4, 262144): 64,
              (5, 65536): 256, (5, 262144): 256, (5, 524288): 64}
    got = {}
    for line in table:
        w = line.split()
        if w[0] == "config":
            got[(int(w[1]), w[2], int(w[3]))] = int(w[5])
    assert len(got) == 13
    for (cid, n), threads in expect.items():
        assert got[(cid, "f32", n)] == threads, (cid, n, got[(cid, "f32", n)], threads)
    # float64 has no register-resident records: the one-wave shape of a heavy fan starts where it did before
    assert got[(4, "f64", 262144)] == 256
