"""GPU (-m gpu), kernel level: cbx_mel_time_scale_win_f32 (ops.mel_time_scale_window), the window of the speed-control map a streaming round at a speaking rate
launches, through the C ABI on the MI355X: against the frames of one cbx_mel_time_scale_f32 launch over the whole rows bit for bit, against the NumPy fp64
restatement (stream_speed_common.py), with NaN around the window and sentinels around the output, at a long stream's offset, and its descriptor errors.  The same
checks run on the SIMT emulator in test_stream_speed_host.py; the engine- and API-level tests of the stream at a rate are in test_stream_speed_gpu.py.

WHY THIS FILE NAME: test_host_logic.py::test_every_kernel_entry_point_is_named_by_a_kernel_level_test finds the kernel-level modules by a fixed list of patterns of which
`test_turbo_stream_*` is the only glob, and existing test files are not edited when a feature is added (test_turbo_stream_batch_kernels_gpu.py is the precedent).  Do not
rename this file without extending _KERNEL_LEVEL_MODULES there."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import stream_speed_common as C  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("strided", [False, True], ids=["contiguous_float4", "row_stride_83_scalar"])
@pytest.mark.parametrize("rate", [0.5, 0.9, 1.0, 1.25, 2.0])
def test_window_launch_equals_the_whole_launch_and_the_restatement(dev, rate, strided):
    """(a) - (d) of stream_speed_common.check_window_launch for windows that start at unscaled frame 0, 6, 7 and 40: B = 3 ragged rows, C = 80, T_in = 61."""
    from chatterbox_amd import ops
    with torch.cuda.device(dev):
        for i_org in (0, 6, 7, 40):
            C.check_window_launch(ops, dev, rate, i_org, strided, sync=torch.cuda.synchronize)


def test_far_window_keeps_the_fp64_position(dev):
    """(e): output frame 2^20 + 3 over an 8-frame input, every rate of the set"""
    from chatterbox_amd import ops
    with torch.cuda.device(dev):
        for rate in (0.5, 0.9, 1.0, 1.25, 2.0):
            C.check_far_window(ops, dev, rate, sync=torch.cuda.synchronize)


def test_descriptor_errors_return_before_a_launch(dev):
    """(f): null pointers, strides below C, negative shapes, a bad rate or origin -> -22 and a message; the buffers are HOST memory, so a launch would fault"""
    from chatterbox_amd import _lib
    C.descriptor_errors(_lib.lib)
    assert _lib.lib.cbx_abi_version() == 16
