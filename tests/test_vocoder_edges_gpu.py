"""GPU (-m gpu), kernel level: the HiFT tail kernels and the convolution forms of the vocoder at the shapes and values that can break them; the bodies, references
and bounds are in vocoder_edges_common.py, which tests/test_simt_kernels.py drives on the SIMT emulator at the small shapes.

  * iSTFT (cbx_hift_istft_f32, cbx_hift_istft_rows_f32): frames {2, 3, 17, 65, 66, 121, 361} x B {1, 3} x ldx {18, 32} x fade_n {0, 480} against fp64 torch.istft
    within c 2^-24 S / env + 2^-24 |ref| (c = twice torch's own fp32 ratio, measured 4.713 on the CPU) and within the older 1e-5 (1 + |ref|); the ragged batch
    (rows torch.equal to solo launches on the cut rows, 0 beyond); clip, expf overflow and phases of +-50; refusals.
    Worst ratio of the kernel to the first term: emulator 1.73 (frames 361), 1.69 (ragged), 0.96 (values); MI355X: MI355X_RATIO below.
  * source: f0 at 10.0 / 0.0 / just above 10; the grid-stride second lap (1 152 000 samples, excluded share asserted <= 1e-5, measured 1.7e-6).
  * STFT: L = 16 and 20; second lap (1 050 005 frames) at ld = 18.
  * act / axpby / cfm_euler: second laps.  (The front-end kernels cap their grids at 65 535 x 256 items, which no production shape reaches: left alone.)
  * conv: the table of vocoder_edges_common.CONV_CASES at precision 0, 3, 6 and 16.
"""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import vocoder_edges_common as V  # noqa: E402

pytestmark = pytest.mark.gpu

MI355X_RATIO = "geometry 1.741 (frames 361, B 3), ragged 1.694, value case 1.017"  # first run on the MI355X, as printed by the tests below (allowed: 9.44)


@pytest.mark.parametrize("ldx", [18, 32])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("frames", V.ISTFT_FRAMES)
def test_istft_geometry(dev, frames, B, ldx):
    from chatterbox_amd import ops
    with torch.cuda.device(dev):
        worst = V.check_istft_geometry(ops, dev, frames, B, ldx)
    print(f"iSTFT frames {frames} B {B} ldx {ldx}: worst (|err| - eps |ref|) / (eps S / env) = {worst:.3f} (allowed {V.ISTFT_C:.2f})")


def test_istft_ragged_rows_equal_solo_launches_and_end_in_zeros(dev):
    from chatterbox_amd import ops
    with torch.cuda.device(dev):
        worst = V.check_istft_ragged(ops, dev)
    print(f"ragged iSTFT: worst ratio {worst:.3f} (allowed {V.ISTFT_C:.2f})")


def test_istft_clip_overflow_and_large_phases(dev):
    from chatterbox_amd import ops
    with torch.cuda.device(dev):
        worst = V.check_istft_values(ops, dev)
    print(f"iSTFT value case: worst ratio {worst:.3f} (allowed {V.ISTFT_C:.2f})")


def test_istft_refusals_and_defined_frame_lens(dev):
    from chatterbox_amd import ops
    with torch.cuda.device(dev):
        V.check_istft_refusals(ops, dev)


def test_source_f0_thresholds(dev):
    from chatterbox_amd import ops
    with torch.cuda.device(dev):
        V.check_source_thresholds(ops, dev)


def test_source_second_lap(dev):
    from chatterbox_amd import ops
    with torch.cuda.device(dev):
        share = V.check_source_second_lap(ops, dev)
    print(f"source second lap: excluded share {share:.2e}")


@pytest.mark.parametrize("B,L,ld", [(2, 16, 18), (2, 16, 32), (2, 20, 18), (2, 20, 32), (5, 840000, 18)])
def test_stft_minimum_lengths_and_second_lap(dev, B, L, ld):
    from chatterbox_amd import ops
    with torch.cuda.device(dev):
        V.check_stft(ops, dev, B, L, ld)


def test_act_second_lap(dev):
    from chatterbox_amd import ops
    with torch.cuda.device(dev):
        V.check_act_second_lap(ops, dev)


def test_axpby_second_lap(dev):
    from chatterbox_amd import ops
    with torch.cuda.device(dev):
        V.check_axpby_second_lap(ops, dev)


def test_cfm_euler_second_lap(dev):
    from chatterbox_amd import ops
    with torch.cuda.device(dev):
        V.check_cfm_euler_second_lap(ops, dev)


@pytest.mark.parametrize("name,precision", [(c["name"], p) for c in V.CONV_CASES for p in c["precisions"]])
def test_conv_geometry_and_dispatch_form(dev, name, precision):
    from chatterbox_amd import ops
    with torch.cuda.device(dev):
        V.check_conv_case(ops, dev, name, precision)
