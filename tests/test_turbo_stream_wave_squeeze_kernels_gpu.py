"""GPU (-m gpu), kernel level: cbx_wave_squeeze_f32 (ops.wave_squeeze, ops.wave_join(squeeze=)), the pause control, against the NumPy restatement of its definition
(wave_squeeze_common.py): the shortened samples equal BITWISE, the stats and the mapped edge table equal as integers, the tail [n', n) zeros, nothing written outside
the rows.  Shapes: R = 1, 5, 6 and 64 rows as views of one NaN-filled buffer at misalignments 0 .. 3 floats; lengths 0, 137, 480, 2879, 7680 and three rows of 2100
frames (1 M samples) whose pauses end at, start at and straddle every multiple of the plan kernel's tile; pauses of exactly K and K + 1 frames, K odd, K = 2, leading
and trailing silence, two pauses one frame apart, zeros, no silence, keep = 0, a frame ON the threshold, a NaN frame; fade 0, 240 and 480; the edge table at 0, n,
c0, c1, inside a cut and beyond n.

WHY THIS FILE NAME: test_host_logic.py::test_every_kernel_entry_point_is_named_by_a_kernel_level_test finds the kernel-level modules by a fixed list of patterns of which
`test_turbo_stream_*` is the only glob, and existing test files are not edited when a feature is added.  Do not rename this file without extending
_KERNEL_LEVEL_MODULES there."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import wave_squeeze_common as S  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name,fade,db", S.CASES, ids=S.CASE_IDS)
def test_wave_squeeze_equals_the_restatement_bitwise(dev, name, fade, db):
    from chatterbox_amd import ops
    with torch.cuda.device(dev):
        stats, host = S.check_launch(ops, dev, name, fade, db, sync=torch.cuda.synchronize)
        again, host2 = S.check_launch(ops, dev, name, fade, db, sync=torch.cuda.synchronize)
    assert stats == again and (host.view("int32") == host2.view("int32")).all(), "two launches give identical results"


def test_the_cases_are_what_they_claim():
    S.what_the_sets_cover()


@pytest.mark.parametrize("trim_db", [None, 40.0], ids=["notrim", "trim40"])
@pytest.mark.parametrize("first,last", [(True, True), (True, False), (False, True), (False, False)], ids=["first-last", "first", "last", "inner"])
def test_edges_squeeze_join_equals_the_numpy_composition(dev, trim_db, first, last):
    """The long-form order: edges on the original rows, squeeze (maps the table), join over the shortened rows with the host-side lengths.  The last row of "pauses"
    is shortened and keeps its trailing silence without a trim, so with last=True its stop is no longer n and the end of the text gets the fade-out."""
    from chatterbox_amd import ops
    with torch.cuda.device(dev):
        for name in ("pauses", "edges"):
            total, frames = S.check_composition(ops, dev, name, trim_db, first, last, sync=torch.cuda.synchronize)
            assert frames > 0 and total > 0


def test_refused_descriptors_launch_nothing(dev):
    """Every refusal of the header returns -22 with the entry's name, and nothing is written; the good descriptor then runs."""
    import ctypes
    from chatterbox_amd import _lib
    lib = _lib.lib
    with torch.cuda.device(dev):
        wav = torch.zeros(2400, device=dev)
        wav[:480] = 0.5
        wav[960:1200] = 0.5
        out = torch.full((2400,), 7.0, device=dev)
        edges = torch.tensor([5, 6, 7, 8], dtype=torch.int32, device=dev)
        stats = torch.full((8,), -5, dtype=torch.int32, device=dev)
        ws = torch.full((12,), -1.0, dtype=torch.float64, device=dev)
        ramp = torch.ones(480, device=dev)
        off, n, keep = (ctypes.c_long * 2)(0, 1200), (ctypes.c_int * 2)(1200, 1200), (ctypes.c_int * 2)(2, 0)
        neg, noff, k1, kneg = (ctypes.c_int * 2)(1200, -1), (ctypes.c_long * 2)(0, -4), (ctypes.c_int * 2)(2, 1), (ctypes.c_int * 2)(-2, 2)
        a = ctypes.addressof
        st = torch.cuda.current_stream().cuda_stream
        need = 16 * 2 * 3
        good = [wav.data_ptr(), a(off), a(n), a(keep), 2, 1e-4, ramp.data_ptr(), 240, out.data_ptr(), 2400, edges.data_ptr(), stats.data_ptr(), ws.data_ptr(), need, st]
        for i, bad in ((0, None), (1, None), (2, None), (3, None), (8, None), (11, None), (12, None), (4, 0), (4, -1), (4, 65), (2, a(neg)), (1, a(noff)), (3, a(k1)),
                       (3, a(kneg)), (5, -1.0), (5, float("nan")), (5, float("inf")), (7, -1), (7, 481), (6, None), (8, wav.data_ptr()), (8, wav.data_ptr() + 4 * 2399),
                       (9, 2399), (9, 0), (13, need - 1), (13, 0), (12, ws.data_ptr() + 4)):
            args = list(good)
            args[i] = bad
            assert lib.cbx_wave_squeeze_f32(*args) == -22 and b"wave_squeeze" in lib.cbx_last_error(), (i, bad)
        torch.cuda.synchronize()
        assert bool((out == 7.0).all()) and edges.tolist() == [5, 6, 7, 8] and bool((stats == -5).all()) and bool((ws == -1.0).all()), "a refused call launches nothing"
        assert lib.cbx_wave_squeeze_f32(*good) == 0
        torch.cuda.synchronize()
    # row 0: frames S Z S(half): no pause longer than 2; row 1: zeros, keep 0
    assert stats.tolist() == [1200, 0, 0, 1200] * 2 and edges.tolist() == [5, 6, 7, 8] and torch.equal(out, wav)
