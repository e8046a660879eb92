"""GPU (-m gpu), kernel level: cbx_wave_ingest (ops.wave_ingest), the decode + mixdown + resample launch of the audio inputs, and cbx_wave_trim_edges_f32
(ops.wave_trim_edges), against the oracle of wave_ingest_common.py: (a) decode and mixdown bit for bit the NumPy restatement at the decode-only pair, for all seven
encodings with both extremes and every G.711 code, at 1, 2, 3 and 8 channels; (b) the resampled form within the derived per-element bound of
scipy.signal.resample_poly in fp64 of that decoded signal, lengths ceil(n U / D); (c) identical bits with the rows at every byte misalignment the encoding allows
and 16-byte aligned, and with different padding bytes around them (NaN padding for f32); (d) a prefilled output untouched outside the rows; (e) refused descriptors
return -22 and write nothing; (f) the trim edges equal the host rule's exactly.  Shapes: frame counts 0, 1, 7, 479, 480, 1931 (R = 5) and 3101 (R = 1: at least four
workgroups per row at every pair); the pairs of C.PAIRS (U = 1, D = 1, LDS-staged and global-memory tables, no table).

WHY THIS FILE NAME: test_host_logic.py::test_every_kernel_entry_point_is_named_by_a_kernel_level_test finds the kernel-level modules by a fixed list of patterns of which
`test_turbo_stream_*` is the only glob, and existing test files are not edited when a feature is added (test_turbo_stream_wave_format_kernels_gpu.py is the
precedent).  Do not rename this file without extending _KERNEL_LEVEL_MODULES there."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import wave_ingest_common as C  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("rate_in,rate_out", C.PAIRS)
@pytest.mark.parametrize("enc", C.ENCODINGS)
def test_wave_ingest_decodes_exactly_and_meets_the_bound_at_every_alignment(dev, enc, rate_in, rate_out):
    from chatterbox_amd import ops
    with torch.cuda.device(dev):
        worst = C.check_ingest(ops, dev, "A", enc, rate_in, rate_out, sync=torch.cuda.synchronize)
        worst = max(worst, C.check_ingest(ops, dev, "B", enc, rate_in, rate_out, alignments=("aligned", 5), channels=(1, 3), sync=torch.cuda.synchronize))
        worst = max(worst, C.check_ingest(ops, dev, "b", enc, rate_in, rate_out, alignments=(15,), channels=(1, 8), sync=torch.cuda.synchronize))
    print(f"{enc}, {rate_in} -> {rate_out}: worst |y - y64| / bound = {worst:.3f}")


@pytest.mark.parametrize("rate_in", [r for r in C.IN_RATES if r != 16000])
def test_every_source_rate_converts_to_both_analysis_rates(dev, rate_in):
    from chatterbox_amd import ops
    with torch.cuda.device(dev):
        for rate_out in (16000, 24000):
            if rate_in != rate_out:
                C.check_ingest(ops, dev, "A", "s16", rate_in, rate_out, alignments=(5,), channels=(2,), sync=torch.cuda.synchronize)
                C.check_ingest(ops, dev, "B", "mulaw", rate_in, rate_out, alignments=(5,), channels=(1,), sync=torch.cuda.synchronize)


def test_the_cases_the_shapes_are_chosen_for_are_what_they_claim():
    C.what_the_sets_cover()
    C.check_g711_expansion_is_pinned()


@pytest.mark.parametrize("enc,channels,rate_in,rate_out", [("mulaw", 1, 8000, 24000), ("s24", 3, 44100, 16000), ("f32", 8, 16000, 16000), ("s16", 2, 48000, 16000)])
def test_nothing_is_written_outside_the_rows(dev, enc, channels, rate_in, rate_out):
    from chatterbox_amd import ops
    with torch.cuda.device(dev):
        C.check_sentinels(ops, dev, enc, channels, rate_in, rate_out, sync=torch.cuda.synchronize)


def test_refused_descriptors_launch_nothing(dev):
    """A null pointer, R outside [1, 64], a negative frame count or offset, an offset that is not a multiple of the sample size, channels outside [1, 8], an unknown
    encoding, U / D not reduced, a T that is not theirs, a span or table over the caps, an output that is too small: -22 with the entry's name (cbx_wave_ingest),
    nothing written."""
    from chatterbox_amd import _lib, ops
    with torch.cuda.device(dev):
        C.check_refusals(_lib.lib, ops, dev, torch.cuda.current_stream().cuda_stream, sync=torch.cuda.synchronize)


def test_trim_edges_equal_the_host_rule_exactly(dev):
    """cbx_wave_trim_edges_f32 through ops.wave_trim_edges: bursts with a silent head and tail, all silent, all loud, shorter than one frame, as rows of one
    launch at two alignments"""
    from chatterbox_amd import ops
    with torch.cuda.device(dev):
        C.check_trim(ops, dev, sync=torch.cuda.synchronize)
        assert ops.wave_trim_edges([torch.zeros(3000, device=dev)], 0.0).cpu().tolist() == [[0, 0]]


@pytest.mark.parametrize("lengths", C.TRIM_SEAMS, ids=lambda t: "-".join(map(str, t)))
def test_trim_edges_at_the_block_seams(dev, lengths):
    """rows of 0 .. 1025 samples on either side of the 480- and 512-sample block lengths, two of the three off the 16-byte grid: the host rule's edges"""
    from chatterbox_amd import ops
    with torch.cuda.device(dev):
        C.check_trim_seams(ops, dev, lengths, sync=torch.cuda.synchronize)
