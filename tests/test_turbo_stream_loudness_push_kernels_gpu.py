"""GPU (-m gpu), kernel level: cbx_wave_loudness_push_f32 (ops.wave_loudness_push, ops.WaveLoudnessStream), the running BS.1770-4 meter of generate_long_stream.
The contract is BITWISE: after every push stats and gain are the bit patterns ops.wave_loudness gives for each row's concatenated pieces on the same device, and at
the end the E table is the one-shot kernel's; the final numbers also meet the SciPy oracle within loudness_common.py's tolerances.  The cases of
loudness_push_common.py (their reasons there) at every 4-byte misalignment, the refusals with device buffers, a non-default stream.  The signals are at most 72 007
samples: a few seconds in all.

WHY THIS FILE NAME: test_host_logic.py::test_every_kernel_entry_point_is_named_by_a_kernel_level_test finds the kernel-level modules by a fixed list of patterns of which
`test_turbo_stream_*` is the only glob, and existing test files are not edited when a feature is added (test_turbo_stream_loudness_kernels_gpu.py is the precedent).
Do not rename this file without extending _KERNEL_LEVEL_MODULES there."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import loudness_common as C  # noqa: E402
import loudness_push_common as P  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("mis", range(4))
def test_one_row_in_pieces_is_the_one_shot_meter_bit_for_bit(dev, mis):
    from chatterbox_amd import ops
    with torch.cuda.device(dev):
        for k, name in enumerate(sorted(P.SPLITS_ONE)):
            P.run_split(ops, [P.short()], [P.SPLITS_ONE[name]], [(-23.0, None, -30.0)[(mis + k) % 3]], mis, dev, torch.cuda.synchronize)


@pytest.mark.parametrize("mis", range(4))
def test_three_rows_with_their_own_pieces(dev, mis):
    from chatterbox_amd import ops
    with torch.cuda.device(dev):
        out = P.run_split(ops, [P.long(), P.short(), P.short()], P.SPLITS_THREE, P.TARGETS_THREE, mis, dev, torch.cuda.synchronize)
    assert all(g[1] == 1.0 and st[1, 2] == 1.0 for st, g in out), "a target of None: measure only"
    assert out[-1][1][0] != 1.0 and out[-1][1][2] != 1.0


def test_a_nan_in_the_second_piece_makes_the_peak_nan_and_the_gain_one_from_then_on(dev):
    from chatterbox_amd import ops
    x = P.short()
    x[3000] = np.nan
    with torch.cuda.device(dev):
        out = P.run_split(ops, [x, P.short()], [[2500, 2500, 7000, P.REST]] * 2, [-23.0, -23.0], 1, dev, torch.cuda.synchronize, oracle=False)
    assert not np.isnan(out[0][0][0, 1]) and all(np.isnan(st[0, 1]) and st[0, 2] == 1.0 and g[0] == 1.0 for st, g in out[1:])
    assert not np.isnan(out[-1][0][1]).any() and out[-1][1][1] != 1.0


def test_growing_the_record_keeps_the_bits_and_the_entry_refuses_what_would_pass_seg_cap(dev):
    from chatterbox_amd import ops
    with torch.cuda.device(dev):
        a = P.run_split(ops, [P.short()], [P.SPLITS_ONE["ragged"]], [-23.0], 3, dev, torch.cuda.synchronize, seg_cap=2)
        b = P.run_split(ops, [P.short()], [P.SPLITS_ONE["ragged"]], [-23.0], 3, dev, torch.cuda.synchronize)
        assert all(np.array_equal(x[0].view(np.int64), y[0].view(np.int64)) and np.array_equal(x[1].view(np.int32), y[1].view(np.int32)) for x, y in zip(a, b))
        meter = ops.WaveLoudnessStream(1, dev, seg_cap=3)
        with pytest.raises(RuntimeError, match="wave_loudness_push"):
            ops.wave_loudness_push(meter, [torch.from_numpy(C.bursts(4 * P.HOP, 1)).to(dev)], -20.0)
        torch.cuda.synchronize()
        assert meter.n0 == [0] and float(meter.rec.abs().max()) == 0.0, "-22: nothing written, the meter not advanced"


def test_refused_descriptors_launch_nothing_and_the_good_one_runs(dev):
    from chatterbox_amd import _lib, ops
    with torch.cuda.device(dev):
        P.check_push_refusals(_lib.lib, ops, dev, torch.cuda.current_stream().cuda_stream, torch.cuda.synchronize)


def test_on_a_non_default_stream(dev):
    from chatterbox_amd import _lib, ops
    with torch.cuda.device(dev):
        want = P.run_split(ops, [P.short()], [P.SPLITS_ONE["ragged"]], [-23.0], 2, dev, torch.cuda.synchronize)
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            got = P.run_split(ops, [P.short()], [P.SPLITS_ONE["ragged"]], [-23.0], 2, dev, torch.cuda.synchronize)
            P.check_push_refusals(_lib.lib, ops, dev, side.cuda_stream, torch.cuda.synchronize)
        assert all(np.array_equal(x[0].view(np.int64), y[0].view(np.int64)) and np.array_equal(x[1].view(np.int32), y[1].view(np.int32)) for x, y in zip(want, got))
