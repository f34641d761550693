"""GPU: the float32 step kernels reproduce the recorded bits of tests/golden/step_bits_<case>.npz -- 24 single launches at 66
envs (one full group and a partial one) with in-kernel episode resets, for the BlueROV2 with the 16-beam fan and 8 spheres
(256 / 64 threads per group), the LAUV with 63 rays and 5 capsules (512 / 256 / 64), the interleaved BlueROV2 / LAUV batch
with current (256) and the sensor-free BlueROV2 (256 / 128 / 64): the state field and the packed rows after the step that
follows the reset and after the last step, compared as int32.

The fixtures pin the output of ONE toolchain: they were recorded with scripts/record_step_bits.py from the library of the
commit before the parameter block got its hot part (a change that only moves loads; with -ffp-contract=on what a step
computes is a property of the source expressions).  A change that is meant to alter results, or a new compiler whose code
rounds differently, needs new fixtures: build the library whose results are to be kept and run
`python scripts/record_step_bits.py` on the GPU (it writes tests/golden/).  tests/test_gpu_reset.py::
test_step_sequence_equals_single_steps ties the resident kernels to the single launches checked here."""
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("record_step_bits", os.path.join(ROOT, "scripts", "record_step_bits.py"))
rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rec)


def test_every_case_has_a_small_fixture():
    assert len(rec.CASES) == 9
    for case in rec.CASES:
        path = rec.golden_path(case)
        assert os.path.exists(path), path
        assert os.path.getsize(path) <= 100_000, path


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(rec.CASES))
def test_step_bits_are_the_recorded_ones(case):
    golden = np.load(rec.golden_path(case))
    got = rec.run_case(case)
    assert sorted(golden.files) == sorted(got) and len(got) == 4
    for name in sorted(got):
        a, b = golden[name], got[name]
        assert a.dtype == np.int32 and a.shape == b.shape, (name, a.dtype, a.shape, b.shape)
        bad = np.argwhere(a != b)
        assert bad.size == 0, (f"{case}: {name}: {len(bad)} words differ; first: env {bad[0][0]} column {bad[0][1]}: "
                               f"recorded {a.view(np.float32)[tuple(bad[0])]!r} now {b.view(np.float32)[tuple(bad[0])]!r}")
