"""GPU (-m gpu), kernel level: cbx_mel_time_warp_f32 (ops.mel_time_warp), the piecewise-linear time map of the mel behind `duration=` / `timing=`, against the NumPy
fp64 restatement of its definition (mel_warp_common.py) and, for one-segment tables, against ops.mel_time_scale bit for bit -- ragged rows, four different tables in
one launch, a row whose 250 segments span many workgroups, the float4 form on contiguous tensors and the scalar form on views with row stride 83 whose padding holds
NaN.

WHY THIS FILE NAME: test_host_logic.py::test_every_kernel_entry_point_is_named_by_a_kernel_level_test finds the kernel-level modules by a fixed list of patterns of which
`test_turbo_stream_*` is the only glob, and existing test files are not edited when a feature is added (test_turbo_stream_mel_speed_kernels_gpu.py is the precedent).
The new entry is named here through `ops.mel_time_warp(`.  Do not rename this file without extending _KERNEL_LEVEL_MODULES there."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import mel_speed_common as S  # noqa: E402
import mel_warp_common as W  # noqa: E402

pytestmark = pytest.mark.gpu

IN_LENS, T_IN = (1, 2, 7, 61), 64
RATES = (0.5, 0.75, 0.9, 1.1, 1.25, 1.5, 2.0)
FORMS = pytest.mark.parametrize("strided", [False, True], ids=["contiguous_float4", "row_stride_83_scalar"])


@FORMS
@pytest.mark.parametrize("s", RATES)
def test_one_segment_equals_mel_time_scale_bit_for_bit(dev, s, strided, C=80):
    """The table (0, 0.0, s) is the plain stretch: the same contracted fp64 multiply-add, the same taps, the same blend -- torch.equal on the device, in both forms,
    and the fp64 restatement of the warp agrees with what both produce."""
    from chatterbox_amd import ops
    O = [S.out_len(m, s) for m in IN_LENS]
    with torch.cuda.device(dev):
        got, _ = W.check_launch(ops, dev, IN_LENS, [[(0, 0.0, s)]] * 4, O, T_IN, strided, sync=torch.cuda.synchronize)
        mel = S.log_mel((4, T_IN, C), 0)
        if strided:
            big = torch.full((4, T_IN, C + 3), float("nan"))
            big[:, :, :C] = mel
            src = big.to(dev)[:, :, :C]
            dst = torch.full((4, max(O) + 3, C + 3), W.SENT, device=dev)[:, :, :C]
            want, ol = ops.mel_time_scale(src, [s] * 4, in_lens=list(IN_LENS), out=dst)
        else:
            want, ol = ops.mel_time_scale(mel.to(dev), [s] * 4, in_lens=list(IN_LENS))
        torch.cuda.synchronize()
    assert ol.cpu().tolist() == O and torch.equal(got, want.cpu()), f"s = {s}: a one-segment warp must reproduce the stretch's bits"


def _four_tables():
    """1 segment; 2 at (0.5, 2.0); one per output frame; 61 segments of alternating 0.5 / 2.0 (its tail runs beyond the row: clamped taps)"""
    t1, o1 = [(0, 0.0, 0.9)], 1                       # M = 1
    t2, o2 = [(0, 0.0, 0.5), (2, 1.0, 2.0)], 3        # M = 2: frame 0 over two output frames, frame 1 (and half a frame beyond) in one
    t3, o3 = W.per_output_frame(7, 0.75)              # M = 7: 9 segments of one frame
    t4, o4, end = W.alternating(61)                   # M = 61
    assert o3 == 9 and len(t3) == 9 and len(t4) == 61 and o4 == 92 and end == 91.0
    return [t1, t2, t3, t4], [o1, o2, o3, o4]


@FORMS
def test_four_different_tables_in_one_launch(dev, strided):
    from chatterbox_amd import ops
    tables, O = _four_tables()
    with torch.cuda.device(dev):
        W.check_launch(ops, dev, IN_LENS, tables, O, T_IN, strided, sync=torch.cuda.synchronize)


@FORMS
def test_a_row_whose_segments_span_many_workgroups(dev, strided):
    """500 frames, 250 segments of two input frames each over 2, 1, 3 and 4 output frames in turn (rates 1, 2, 2 / 3 and 0.5), the last at rate 1.  A workgroup
    of 256 threads covers 12.8 output frames in the float4 form and 3.2 in the scalar form, so the segment edges (every 1 to 4 frames) fall on and off workgroup
    edges in both; a second row of 3 frames rides along so that blocks beyond a short row only write zeros."""
    from chatterbox_amd import ops
    anchors, o = [], 0
    for i in range(1, 250):
        o += (4, 2, 1, 3)[i % 4]
        anchors.append((2 * i, o))
    table, frames, achieved, clamped = W.plan(500, anchors)
    assert len(table) == 250 and clamped == [] and achieved[-1] == o and frames > 500
    with torch.cuda.device(dev):
        W.check_launch(ops, dev, (500, 3), [table, [(0, 0.0, 1.5)]], [frames, 2], 500, strided, seed=2, sync=torch.cuda.synchronize)


def test_out_lens_beyond_t_out_and_refused_descriptors(dev):
    """An out_lens[b] above T_out (which the host entry cannot see) is cut to T_out by the kernel: the buffer behind the output stays untouched.  A refused
    descriptor launches nothing."""
    import ctypes
    from chatterbox_amd import _lib
    f = _lib.lib.cbx_mel_time_warp_f32
    with torch.cuda.device(dev):
        mel = S.log_mel((1, 8, 80), seed=5).to(dev)
        buf = torch.full((2, 4, 80), 777.0, device=dev)      # the launch owns buf[0]; buf[1] lies right behind it
        tab = torch.tensor([0.0, 1.25], dtype=torch.float64, device=dev)     # seg_a, seg_s
        ints = torch.tensor([0, 8, 6], dtype=torch.int32, device=dev)        # seg_o, in_lens 8, out_lens 6 > T_out = 4
        off = (ctypes.c_int * 2)(0, 1)
        p = lambda t: t.data_ptr()
        st = torch.cuda.current_stream().cuda_stream
        good = [p(mel), 640, 80, 8, p(ints) + 4, ctypes.addressof(off), 1, p(ints), p(tab), p(tab) + 8, p(buf), 320, 80, 4, p(ints) + 8, 1, 80, st]
        bad_off = (ctypes.c_int * 2)(0, 0)
        for i, bad in ((0, None), (5, None), (7, None), (8, None), (9, None), (10, None), (14, None), (16, 0), (1, 79), (2, 79), (11, 79), (12, 79), (15, 65), (15, -1),
                       (3, -1), (13, -1), (6, 0), (5, ctypes.addressof(bad_off))):
            args = list(good)
            args[i] = bad
            assert f(*args) == -22 and b"mel_time_warp" in _lib.lib.cbx_last_error(), (i, bad)
        torch.cuda.synchronize()
        assert bool((buf == 777.0).all()), "a refused call launches nothing"
        assert f(*good) == 0
        torch.cuda.synchronize()
    import numpy as np
    want = W.reference(mel[0].cpu().numpy(), 8, 4, [(0, 0.0, 1.25)])
    assert np.abs(buf[0].double().cpu().numpy() - want).max() <= 4 * S.U * float(mel.abs().max())
    assert bool((buf[1] == 777.0).all()), "out_lens > T_out must not overrun the output"
