"""GPU (-m gpu), kernel level: cbx_wave_edges_f32 and cbx_wave_join_f32 (ops.wave_edges, ops.wave_join), the trim + join of long-form synthesis, against the NumPy
restatement of their definition (wave_join_common.py): the edge table and the layout record equal as integers, the joined samples equal BITWISE, nothing written at
or beyond `total`.  Shapes: R = 1 and R = 5 rows as views of one padded (R, L) tensor whose padding holds NaN; lengths 0, 137 (less than a frame), 480, 2879 (partial
last frame), 7680 and 70 000 (several workgroups per row); a row of zeros, a row that needs no trim, a row whose live part is one frame (fade > L / 2); pad 0 and 2;
fade 0, 240 and 1000; trim_db=None; the four first / last combinations; gaps including 0; 16-byte and 4-byte access.

WHY THIS FILE NAME: test_host_logic.py::test_every_kernel_entry_point_is_named_by_a_kernel_level_test finds the kernel-level modules by a fixed list of patterns of which
`test_turbo_stream_*` is the only glob, and existing test files are not edited when a feature is added (test_turbo_stream_mel_speed_kernels_gpu.py is the precedent).  Do
not rename this file without extending _KERNEL_LEVEL_MODULES there."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import wave_join_common as W  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name,cfg", W.CASES, ids=W.CASE_IDS)
def test_wave_join_equals_the_restatement_bitwise(dev, name, cfg):
    from chatterbox_amd import ops
    with torch.cuda.device(dev):
        W.check_launch(ops, dev, name, cfg, sync=torch.cuda.synchronize)


@pytest.mark.parametrize("lengths", W.SEAMS, ids=lambda t: "-".join(map(str, t)))
def test_wave_edges_at_the_block_seams(dev, lengths):
    """rows of 0 .. 1025 samples on either side of the 480- and 512-sample block lengths, two of the three off the 16-byte grid: the table is the restatement's"""
    from chatterbox_amd import ops
    with torch.cuda.device(dev):
        W.check_seams(ops, dev, lengths, sync=torch.cuda.synchronize)


def test_the_cases_the_shapes_are_chosen_for_are_what_they_claim():
    W.what_the_sets_cover()


def test_wave_edges_alone_is_reproducible_and_equals_the_table_inside_the_join(dev):
    """ops.wave_edges on its own: the same integers from two launches (fixed reduction order, no floating-point atomics) and from the launch inside ops.wave_join."""
    from chatterbox_amd import ops
    with torch.cuda.device(dev):
        rows, views = W.build("B", True, dev)
        a = ops.wave_edges(views, 40.0, 2).cpu().tolist()
        b = ops.wave_edges(views, 40.0, 2).cpu().tolist()
        piece = ops.wave_join(views, W.GAPS, trim_db=40.0, pad_frames=2, fade=240, first=True, last=True)
        torch.cuda.synchronize()
    assert a == b == piece["edges"].cpu().tolist() == [list(W.edges(r, 40.0, 2)) for r in rows]


def test_refused_descriptors_launch_nothing(dev):
    """Null pointers, R outside [1, 64], a negative gap / fade / length and an `out` that is too small return -22 with the entry's name, and nothing is written."""
    import ctypes
    from chatterbox_amd import _lib
    lib = _lib.lib
    with torch.cuda.device(dev):
        wav = torch.ones(2, 960, device=dev)
        out = torch.full((4000,), 7.0, device=dev)
        rec = torch.full((7,), -5, dtype=torch.int32, device=dev)
        ws = torch.zeros(8, dtype=torch.float64, device=dev)
        ramp = torch.ones(8, device=dev)
        off, n, gaps, neg = (ctypes.c_long * 2)(0, 960), (ctypes.c_int * 2)(960, 960), (ctypes.c_int * 2)(10, 10), (ctypes.c_int * 2)(960, -1)
        a = ctypes.addressof
        st = torch.cuda.current_stream().cuda_stream
        good_e = [wav.data_ptr(), a(off), a(n), 2, 1e-4, 2, rec.data_ptr() + 12, ws.data_ptr(), 8, st]
        for i, bad in ((0, None), (1, None), (2, None), (6, None), (7, None), (3, 0), (3, 65), (2, a(neg)), (4, -1.0), (4, float("nan")), (5, -1), (8, 3)):
            args = list(good_e)
            args[i] = bad
            assert lib.cbx_wave_edges_f32(*args) == -22 and b"wave_edges" in lib.cbx_last_error(), (i, bad)
        good_j = [wav.data_ptr(), a(off), a(n), a(gaps), 2, rec.data_ptr() + 12, ramp.data_ptr(), 8, 1, 1, out.data_ptr(), 4000, rec.data_ptr(), st]
        for i, bad in ((0, None), (1, None), (2, None), (3, None), (5, None), (10, None), (12, None), (4, 0), (4, 65), (2, a(neg)), (3, a(neg)), (7, -1), (6, None),
                       (11, 1939)):
            args = list(good_j)
            args[i] = bad
            assert lib.cbx_wave_join_f32(*args) == -22 and b"wave_join" in lib.cbx_last_error(), (i, bad)
        torch.cuda.synchronize()
        assert bool((out == 7.0).all()) and bool((rec == -5).all()), "a refused call launches nothing"
        args = list(good_j)
        args[11] = 1940  # exactly sum n + sum gaps
        assert lib.cbx_wave_edges_f32(*good_e) == 0 and lib.cbx_wave_join_f32(*args) == 0
        torch.cuda.synchronize()
    assert rec.cpu().tolist() == [0, 970, 1930, 0, 960, 0, 960] and bool((out[1930:] == 7.0).all())
