"""CPU: the packed hot block of the parameter block (gym_dockauv_amd/csrc/dockauv_device.h: HotP, pack_hot) holds bit-for-bit
copies of the EnvP / VehicleP values the integrating wave reads in front of stage 2, for a six-input diagonal-B vehicle and a
LAUV, in float32 and float64, and lies on whole 64-byte lines of the block.  tests/hot_params_host.cpp fills every field
element with a value of its own, packs and compares; built with g++ like tests/test_kernel_selection_host.py."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gym_dockauv_amd", "csrc")


def test_hot_block_is_a_copy_of_its_sources(tmp_path):
    exe = tmp_path / "hot_params_host"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC,
                           os.path.join(ROOT, "tests", "hot_params_host.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert lines[-1] == f"ok {4 * 2 * 87}", r.stdout
    assert not [ln for ln in lines if ln.startswith("FAIL")]
    # float32: 87 scalars in six lines, the block behind EnvP and both VehicleP
    assert "HotP 384 bytes" in lines[0] and "HotP 704 bytes" in lines[2], r.stdout
