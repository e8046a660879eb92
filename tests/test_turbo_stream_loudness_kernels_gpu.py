"""GPU (-m gpu), kernel level: cbx_wave_loudness_f32 and cbx_wave_gain_f32 (ops.wave_loudness, ops.wave_gain, ops.wave_normalize), the BS.1770-4 meter and the gain
launch of loudness=, against the NumPy / SciPy oracle of loudness_common.py: |dL| <= 1e-6 LU, peak and blocks used exact, gain within 1e-6 relative, the rows bit for
bit x * float32(gain) and the NaN padding around them untouched.  The cases of test_loudness_host.py -- the sine anchor, lengths 0, 1, 9599, 9600, 9601, 12 000 and
25 234 as R = 1 and R = 3 rows of one padded buffer at every 4-byte misalignment, the degenerate rows, the ceiling, the refusals -- plus R = 64 short rows, one row
of 300 007 samples (a carry chain over 125 segments, 32 workgroups per pass) and a second run of one case whose stats must be bitwise those of the first.

WHY THIS FILE NAME: test_host_logic.py::test_every_kernel_entry_point_is_named_by_a_kernel_level_test finds the kernel-level modules by a fixed list of patterns of which
`test_turbo_stream_*` is the only glob, and existing test files are not edited when a feature is added (test_turbo_stream_wave_format_kernels_gpu.py is the precedent).
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

pytestmark = pytest.mark.gpu


def test_the_kernels_read_the_sine_anchor(dev):
    from chatterbox_amd import ops
    with torch.cuda.device(dev):
        st, _ = C.run_case(ops, [C.sine(5 * C.FS), C.sine(5 * C.FS, amp=0.1)], [None, None], 1, dev, torch.cuda.synchronize)
    assert abs(st[0, 0] + 3.01) <= 0.1 and abs((st[0, 0] - st[1, 0]) - 20.0) <= C.TOL_L and st[0, 3] == 47


@pytest.mark.parametrize("mis", range(4))
def test_one_row_of_every_length_against_the_oracle(dev, mis):
    from chatterbox_amd import ops
    with torch.cuda.device(dev):
        for k, n in enumerate(C.LENGTHS):
            C.run_case(ops, [C.bursts(n, 10 + n)], [C.TARGETS[k % 3]], mis, dev, torch.cuda.synchronize)


@pytest.mark.parametrize("mis", range(4))
def test_three_rows_against_the_oracle(dev, mis):
    from chatterbox_amd import ops
    with torch.cuda.device(dev):
        for g in range(len(C.GROUPS)):
            C.run_case(ops, [C.bursts(n, 10 + n) for n in C.GROUPS[g]], [C.TARGETS[(g + r) % 3] for r in range(3)], mis, dev, torch.cuda.synchronize)


def test_degenerate_rows_get_gain_one(dev):
    from chatterbox_amd import ops
    bad = C.bursts(12000, 5)
    bad[5000] = np.nan
    sig = [np.zeros(12000, np.float32), C.bursts(9599, 6), bad, C.bursts(12000, 7)]
    with torch.cuda.device(dev):
        st, g = C.run_case(ops, sig, [-20.0, -20.0, -20.0, None], 2, dev, torch.cuda.synchronize)
    assert np.array_equal(g, np.ones(4, np.float32)) and np.array_equal(st[:, 2], np.ones(4))
    assert st[0, 0] == -np.inf and st[0, 1] == 0.0 and st[1, 0] == -np.inf and st[1, 3] == 0 and np.isnan(st[2, 1]) and np.isfinite(st[3, 0])


def test_the_ceiling_limits_the_gain_to_one_over_the_peak(dev):
    from chatterbox_amd import ops
    x = C.bursts(25234, 10 + 25234)
    ref = C.oracle(x, -10.0)
    assert 10.0 ** ((-10.0 - ref["L"]) / 20.0) * ref["peak"] > 1.0
    with torch.cuda.device(dev):
        st, g = C.run_case(ops, [x, x], [-10.0, -30.0], 3, dev, torch.cuda.synchronize)
        assert g[0] == np.float32(1.0 / ref["peak"])
        st, g = C.run_case(ops, [x], [-10.0], 0, dev, torch.cuda.synchronize, ceiling=None)
        assert st[0, 2] * ref["peak"] > 1.0


def test_sixty_four_short_rows(dev):
    """the most rows a launch takes: lengths 9600 .. 12 120 in steps of 40 (4 or 5 whole segments, ragged tails), every alignment"""
    from chatterbox_amd import ops
    sig = [C.bursts(9600 + 40 * r, 100 + r) for r in range(64)]
    with torch.cuda.device(dev):
        C.run_case(ops, sig, [C.TARGETS[r % 3] for r in range(64)], 1, dev, torch.cuda.synchronize)
        with pytest.raises(ValueError, match="rows"):
            ops.wave_loudness([torch.zeros(8, device=dev)] * 65)


def test_a_long_row_carries_its_state_over_125_segments_and_a_second_run_gives_the_same_bits(dev):
    from chatterbox_amd import ops
    x = C.bursts(300007, 77)
    with torch.cuda.device(dev):
        st, g = C.run_case(ops, [x], [-23.0], 3, dev, torch.cuda.synchronize)
        assert st[0, 3] > 20
        buf, rows, _ = C.padded_rows([x, C.bursts(25234, 10 + 25234)], 2, dev)
        a, ga = ops.wave_loudness(rows, [-23.0, -16.0])
        b, gb = ops.wave_loudness(rows, [-23.0, -16.0])
        torch.cuda.synchronize()
        assert torch.equal(a.view(torch.int64), b.view(torch.int64)) and torch.equal(ga.view(torch.int32), gb.view(torch.int32)), "reproducible run to run"
        assert a[0, 0].item() == st[0, 0], "and whatever the row's alignment and the rows beside it"


def test_refused_descriptors_launch_nothing_and_the_good_one_runs(dev):
    """cbx_wave_loudness_f32: a null pointer, R outside [1, 64], a negative length or offset, hop < 1, a coefficient that is not finite, a workspace that is too small;
    cbx_wave_gain_f32: a null pointer, R, a negative length or offset -- -22 with the entry's name, nothing written"""
    from chatterbox_amd import _lib, ops
    with torch.cuda.device(dev):
        C.check_refusals(_lib.lib, ops, dev, torch.cuda.current_stream().cuda_stream, torch.cuda.synchronize)
