"""GPU (-m gpu), kernel level: cbx_wave_format_f32 (ops.wave_format, ops.WaveFormatStream), the resample + encode launch of the output formats, against the oracle
of wave_format_common.py: (a) the fp32 form within the derived bound of scipy.signal.resample_poly in fp64, per element; (b) lengths ceil(n U / D) and a prefilled
output untouched outside the rows; (c) s16 / mulaw / alaw exactly the NumPy quantisation (G.711: the tables of tests/golden/g711_tables.npz) of the same launch's
fp32 form, identity-rate s16 exactly the quantisation of the input with the tie and clip cases constructed; (d) the concatenated pushes of any split of the rows
torch.equal to the one-shot launch, and positions past 2^32 the bits of the same launch at small ones; (e) refused descriptors return -22 and write nothing.  Shapes: the six resampled rates and the identity; R = 1 and R = 5 rows as
views of one padded tensor whose padding holds NaN, 16-byte aligned and at every 4-byte misalignment; lengths 0, 1, 7, 479, 480, 1931 and 70 000 (several
workgroups per row); uniform input, a full-scale square wave whose overshoot clips, a row of zeros.

WHY THIS FILE NAME: test_host_logic.py::test_every_kernel_entry_point_is_named_by_a_kernel_level_test finds the kernel-level modules by a fixed list of patterns of which
`test_turbo_stream_*` is the only glob, and existing test files are not edited when a feature is added (test_turbo_stream_wave_join_kernels_gpu.py is the precedent).  Do
not rename this file without extending _KERNEL_LEVEL_MODULES there."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import wave_format_common as C  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("rate", C.RATES)
@pytest.mark.parametrize("name,aligned", [("A", False), ("A", True), ("B", False), ("B", True)])
def test_wave_format_meets_the_bound_and_its_encodings_are_the_numpy_quantisation(dev, name, aligned, rate):
    from chatterbox_amd import ops
    with torch.cuda.device(dev):
        worst, _ = C.check_one_shot(ops, dev, name, rate, aligned, sync=torch.cuda.synchronize)
    print(f"set {name}, {rate} Hz: worst |y - y64| / bound = {worst:.3f}")


def test_the_cases_the_shapes_are_chosen_for_are_what_they_claim():
    C.what_the_sets_cover()


def test_identity_rate_s16_rounds_ties_to_even_and_clips(dev):
    from chatterbox_amd import ops
    x, expect = C.tie_cases()
    assert np.array_equal(C.quantise(x, "s16"), expect), "the constructed cases are what they claim"
    with torch.cuda.device(dev):
        big = torch.full((len(x) + 2,), float("nan"), device=dev)
        big[1:-1] = torch.from_numpy(x).to(dev)
        got = {enc: ops.wave_format([big[1:-1]], dict(sample_rate=24000, encoding=enc))[0].cpu().numpy() for enc in C.ENCODINGS}
    assert np.array_equal(got["s16"], expect)
    assert np.array_equal(got["f32"].view(np.uint32), x.view(np.uint32)), "24000 -> 24000 fp32 stores the input's bits"
    for enc in ("mulaw", "alaw"):
        assert np.array_equal(got[enc], C.quantise(x, enc))


@pytest.mark.parametrize("rate", [8000, 22050, 48000])
@pytest.mark.parametrize("k", range(len(C.SPLITS)))
def test_any_split_concatenates_to_the_one_shot_output(dev, k, rate):
    from chatterbox_amd import ops
    with torch.cuda.device(dev):
        for enc in ("f32", "mulaw"):
            C.check_split(ops, dev, k, rate, enc, sync=torch.cuda.synchronize)


@pytest.mark.parametrize("rate", [8000, 22050, 48000])
def test_positions_past_two_to_the_32_give_the_bits_of_the_same_launch_at_small_ones(dev, rate):
    from chatterbox_amd import ops
    with torch.cuda.device(dev):
        C.check_large_positions(ops, dev, rate, sync=torch.cuda.synchronize)


@pytest.mark.parametrize("rate,encoding", [(8000, "mulaw"), (48000, "s16"), (22050, "f32"), (24000, "alaw")])
def test_nothing_is_written_outside_the_rows(dev, rate, encoding):
    from chatterbox_amd import ops
    with torch.cuda.device(dev):
        C.check_sentinels(ops, dev, rate, encoding, sync=torch.cuda.synchronize)


def test_refused_descriptors_launch_nothing(dev):
    """A null pointer, R outside [1, 64], a negative length / offset / n0 / m0, an unknown rate or encoding, a table that is not the rate's, a continued row without
    a history, an output that is too small: -22 with the entry's name (cbx_wave_format_f32), nothing written."""
    from chatterbox_amd import _lib, ops
    with torch.cuda.device(dev):
        C.check_refusals(_lib.lib, ops, dev, torch.cuda.current_stream().cuda_stream, sync=torch.cuda.synchronize)
