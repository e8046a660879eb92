"""GPU (-m gpu): the entry-level tests of cbx_wave_limit_f32 (include/cbx.h; ops.wave_limit, ops.wave_true_peak), in a module of the kernel-level family that
test_host_logic.py lists, beside test_turbo_stream_loudness_kernels_gpu.py: the most rows a call takes, a table other than the product's (the general tap loop), and every refusal of the entry on device pointers --
each -22 with the entry's name in cbx_last_error and nothing written --, after which the good descriptor runs.  The cases against the oracle are in
test_limit_kernels_gpu.py; both share tests/limit_common.py with the host tests, which run the same .hip on the SIMT emulator."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import limit_common as C  # noqa: E402

pytestmark = pytest.mark.gpu


def test_sixty_four_rows(dev):
    from chatterbox_amd import ops
    with torch.cuda.device(dev):
        C.check_many_rows(ops, dev, torch.cuda.synchronize)


def test_a_table_that_is_not_the_products_takes_the_general_tap_loop(dev):
    from chatterbox_amd import _lib, ops
    with torch.cuda.device(dev):
        C.check_other_table(_lib.lib, ops, dev, torch.cuda.current_stream().cuda_stream, torch.cuda.synchronize)


def test_descriptor_errors_write_nothing_and_the_good_descriptor_runs(dev):
    from chatterbox_amd import _lib, ops
    with torch.cuda.device(dev):
        C.check_refusals(_lib.lib, ops, dev, torch.cuda.current_stream().cuda_stream, torch.cuda.synchronize)
