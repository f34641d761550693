"""CPU: the packed tail part of the parameter block (gym_dockauv_amd/csrc/dockauv_device.h: TailP, pack_tail) holds bit-for-bit
copies of the EnvP values the wave roles read behind the integrator, for both vehicles and a sensor-free, a 16-ray and a 63-ray
config, in float32 and float64; it is appended to the block on whole 64-byte lines and moves no older field.
tests/tail_params_host.cpp fills every field element with a value of its own, packs and compares; built with g++ like
tests/test_hot_params_host.py, and once more as a stand-alone program with the address and undefined-behaviour sanitizers."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gym_dockauv_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "tail_params_host.cpp")
SLOTS = 40   # 9 integers and 31 reals


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    out = tmp_path_factory.mktemp("tail_params_host")
    exes = {}
    for name, extra in (("plain", []), ("sanitized", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exes[name] = str(out / name)
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", *extra, "-I", CSRC, SRC, "-o", exes[name]])
    return exes


@pytest.mark.parametrize("build", ["plain", "sanitized"])
def test_tail_block_is_a_copy_of_its_sources(built, build):
    r = subprocess.run([built[build]], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert not r.stderr.strip(), r.stderr   # (a sanitizer report)
    lines = r.stdout.splitlines()
    assert lines[-1] == f"ok {2 * 3 * 2 * SLOTS}", r.stdout
    assert not [ln for ln in lines if ln.startswith("FAIL")]
    # float32: 40 scalars in three lines, appended behind the two hot blocks
    assert "TailP 192 bytes" in lines[0] and "TailP 320 bytes" in lines[1], r.stdout
