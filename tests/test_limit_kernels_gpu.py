"""GPU (-m gpu): cbx_wave_limit_f32 on the device against the NumPy oracle of limit_common.py -- the cases, tolerances and properties of tests/test_limit_host.py
(which runs the same .hip on the SIMT emulator), here on the compiled gfx950 kernels: every length and peak position at the four misalignments, the inter-sample
peak, rows under the ceiling and rows that are not limited bit for bit, H = 3 and 480, no gain vector, measure only, a NaN sample, determinism.  R = 64 and the refusals of
the entry on device pointers are in test_turbo_stream_limit_kernels_gpu.py, beside the other wave kernels' entry-level tests."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import limit_common as C  # noqa: E402

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


def test_the_inter_sample_peak_is_limited(run):
    C.check_inter_sample(**run)


def test_no_gain_vector_is_a_gain_of_ones(run):
    C.check_gain_null(**run)


def test_measure_only_reads_the_same_true_peak_and_writes_nothing(run):
    C.check_measure_only(**run)


def test_a_row_with_a_nan_sample(run):
    C.check_nan_row(**run)


def test_the_result_does_not_depend_on_alignment_or_batch(run):
    C.check_determinism(**run)
