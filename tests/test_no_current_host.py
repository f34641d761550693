"""CPU: the "handle without a water current" property and the choice of the lean (NOCUR) step kernels
(gym_dockauv_amd/csrc/dockauv_device.h: scenario_without_current, no_current_after_write, nocur_shape, select_step,
select_sequence).  tests/no_current_host.cpp walks the property through its transitions -- which scenarios start with it, that a
write of exact +0.0 zeros keeps it, that any other value in any column of any written row (-0.0, NaN and a denormal included)
clears it, that nothing brings it back -- and select_step / select_sequence over a grid of requests with the property set and
cleared: NOCUR is set exactly for the product kernels (plain, TERM, riding, resident sequence) of the three group shapes that
have a lean twin, the property changes no other field of the choice, and every request BASELINE configs 2, 3 and 4 make at their
batch sizes gets a lean kernel.  Built with g++ like tests/test_tail_params_host.py, and once more as a stand-alone program with
the address and undefined-behaviour sanitizers."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gym_dockauv_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "no_current_host.cpp")


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    out = tmp_path_factory.mktemp("no_current_host")
    exes = {}
    for name, extra in (("plain", []), ("sanitized", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exes[name] = str(out / name)
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", *extra, "-I", CSRC, SRC, "-o", exes[name]])
    return exes


@pytest.mark.parametrize("build", ["plain", "sanitized"])
def test_property_transitions_and_kernel_choice(built, build):
    r = subprocess.run([built[build]], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert not r.stderr.strip(), r.stderr   # (a sanitizer report)
    lines = r.stdout.splitlines()
    assert not [ln for ln in lines if ln.startswith("FAIL")]
    assert lines[-1].startswith("ok ") and int(lines[-1].split()[1]) > 1_000_000, lines[-1]
