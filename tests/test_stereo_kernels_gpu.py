"""GPU (-m gpu): the three entries of wave_stereo.hip on the device against the restatements of stereo_common.py -- the checks tests/test_stereo_host.py runs on
the SIMT emulator, here on the compiled gfx950 kernels, at the smallest shapes that can still go wrong.
Pan mix: R = 3 rows of 1, 4097 and 5000 samples at 0, 3 and 4090 (they overlap and cross the 4096-output tile), out 0, 1 and 2 floats above a 16-byte boundary
(the right plane then sits at another offset), fades of 240, a device balance gain through gain_idx, a second accumulating launch: BIT FOR BIT the restatement,
plus the {1, 1}, L == R and zero-gain properties.
Meter, hop = 2400: n = 4 hop (one block), 4 hop - 1 (none: L = -inf, gain 1), 5 hop + 1203; C = 1 bitwise ops.wave_loudness; L == R reads the mono loudness plus
10 log10 2; swapped channels identical bits; unequal channels within loudness_common's TOL_L = 1e-6 LU of the fp64 restatement (no wider constant was needed:
the worst |dL| printed on the MI355X is 7.6e-13 LU).
Limiter: signals of 1, 1025 and 2300 samples; C = 1 bitwise ops.wave_limit; L == R the mono output in both planes; a burst in L at 1020 .. 1027 with R quiet:
out_R = u_R g of the restatement within limit_common's TOL_OUT, the ceiling held at the samples and between them, a NaN ceiling passes through.
The refusals on device pointers and R = 64 are in test_turbo_stream_stereo_kernels_gpu.py, beside the other wave kernels' entry-level tests."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import stereo_common as S  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def run(dev):
    from chatterbox_amd import ops
    with torch.cuda.device(dev):
        yield dict(ops=ops, device=dev, sync=torch.cuda.synchronize)


def test_the_pan_mix_is_the_restatement_bit_for_bit(run):
    S.check_pan_mix(**run)


def test_the_meter_sums_the_channels_energies(run):
    S.check_loudness_ch(**run)


def test_the_limiter_links_the_channels(run):
    S.check_limit_ch(**run)

