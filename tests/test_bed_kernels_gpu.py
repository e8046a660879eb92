"""GPU (-m gpu): cbx_wave_duck_f32 on the device against the NumPy oracle of bed_common.py -- the cases, tolerances and properties of tests/test_bed_host.py
(which runs the same .hip on the SIMT emulator), here on the compiled gfx950 kernels: every length, lead and seam position at the four misalignments, the rows
with g == 1 bit for bit, no gain vector, a NaN sample, what ducking does, determinism.  R = 64, the level launch and the refusals of the entries on device
pointers are in test_turbo_stream_bed_kernels_gpu.py, beside the other wave kernels' entry-level tests."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import bed_common as C  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = C.cases()


@pytest.fixture(scope="module")
def run(dev):
    from chatterbox_amd import ops
    with torch.cuda.device(dev):
        yield dict(ops=ops, device=dev, sync=torch.cuda.synchronize)


@pytest.mark.parametrize("mis", range(4))
@pytest.mark.parametrize("name", sorted(CASES))
def test_a_case_against_the_oracle(run, name, mis):
    C.run_case(run["ops"], name, CASES[name], mis, run["device"], run["sync"])


@pytest.mark.parametrize("check", ["check_nan_row", "check_determinism", "check_gain_null", "check_ducking"])
def test_a_property_of_the_definition(run, check):
    getattr(C, check)(**run)
