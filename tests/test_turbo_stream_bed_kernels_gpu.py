"""GPU (-m gpu): the entry-level tests of cbx_wave_duck_f32 and cbx_wave_duck_level_f32 (include/cbx.h; ops.wave_duck, ops.wave_duck_level), in a module of the
kernel-level family that test_host_logic.py lists, beside test_turbo_stream_limit_kernels_gpu.py: the most rows a call takes, the level launch, calls without
speech or without any output, and every refusal of the two entries on device pointers -- each -22 with the entry's name in cbx_last_error and nothing written --,
after which the good descriptor runs.  The cases against the oracle are in test_bed_kernels_gpu.py; both share tests/bed_common.py with the host tests, which run
the same .hip on the SIMT emulator."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import bed_common as C  # noqa: E402

pytestmark = pytest.mark.gpu


def test_sixty_four_rows(dev):
    from chatterbox_amd import ops
    with torch.cuda.device(dev):
        C.check_many_rows(ops, dev, torch.cuda.synchronize)


def test_the_level_launch(dev):
    from chatterbox_amd import ops
    with torch.cuda.device(dev):
        C.check_level(ops, dev, torch.cuda.synchronize)


def test_descriptor_errors_write_nothing_and_the_good_descriptor_runs(dev):
    from chatterbox_amd import _lib, ops
    with torch.cuda.device(dev):
        C.check_refusals(_lib.lib, ops, dev, torch.cuda.current_stream().cuda_stream, torch.cuda.synchronize)


def test_every_output_row_empty_is_no_launch_and_no_speech_is_the_bed_alone(dev):
    from chatterbox_amd import ops
    with torch.cuda.device(dev):
        out, st = ops.wave_duck([torch.zeros(0, device=dev)] * 2, None, C.plan(), gain=torch.tensor([0.5, 0.25], device=dev))
        assert [o.numel() for o in out] == [0, 0] and st.cpu().tolist() == [[0.5, 0.0, 0.0, 0.0], [0.25, 0.0, 0.0, 0.0]]
        b = torch.from_numpy(C.bed(700, 1)).to(dev)
        out, st = ops.wave_duck([None], [b], C.plan(lead=300, tail=200, fi=0, fo=0))
        torch.cuda.synchronize()
        assert torch.equal(out[0], b[:500]) and st.cpu().tolist() == [[1.0, 0.0, 3.0, float(b[:500].abs().max())]]
