"""GPU (-m gpu): cbx_wave_mix_f32 on the device against the NumPy oracle of wave_mix_common.py, BITWISE -- the cases and properties of tests/test_wave_mix_host.py
(which runs the same .hip on the SIMT emulator), here on the compiled gfx950 kernel: one row over a tile edge, rows that meet at a tile edge, the order of
summation, rows of 0 .. 5 samples with every flag value, uncovered samples with and without accumulate, 64 stacked rows with gains through gain_idx, NULL gain and
gain_idx, rows split over three launches, a NaN sample, the join's bits for non-negative gaps, and the refusals of the entry on device pointers."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import wave_mix_common as C  # noqa: E402

pytestmark = pytest.mark.gpu

T = 4096
CASES = C.cases(T)


@pytest.fixture(scope="module")
def run(dev):
    from chatterbox_amd import ops
    assert ops.WAVE_MIX_TILE == T
    with torch.cuda.device(dev):
        yield dict(ops=ops, device=dev, sync=torch.cuda.synchronize)


@pytest.mark.parametrize("mis", range(4))
@pytest.mark.parametrize("name", sorted(CASES))
def test_a_case_against_the_oracle(run, name, mis):
    C.run_case(run["ops"], name, CASES[name], mis, run["device"], run["sync"])


@pytest.mark.parametrize("check", ["order", "gap", "gain_null", "split", "nan"])
def test_a_property_of_the_definition(run, check):
    getattr(C, f"check_{check}")(run["ops"], T, run["device"], run["sync"])


def test_non_negative_gaps_give_the_joins_bits(run):
    C.check_join(run["ops"], run["device"], run["sync"])


def test_the_entry_refuses_bad_descriptors_on_device_pointers_and_runs_the_good_one(run):
    from chatterbox_amd import _lib
    C.check_refusals(_lib.lib, run["ops"], run["device"], None, run["sync"])
