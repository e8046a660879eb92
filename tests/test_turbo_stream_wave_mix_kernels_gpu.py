"""GPU (-m gpu): the entry-level tests of cbx_wave_mix_f32, beside the other wave kernels': the refusals of the entry on device pointers with the good descriptor
run afterwards, and ops.wave_mix over R = 64 stacked rows -- the most a call takes -- into an out at each misalignment, bitwise against the NumPy oracle of
wave_mix_common.py.  The cases and properties of the definition are in test_wave_mix_kernels_gpu.py."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import loudness_common as L  # noqa: E402
import wave_mix_common as C  # noqa: E402

pytestmark = pytest.mark.gpu


def test_cbx_wave_mix_f32_refuses_bad_descriptors_on_device_pointers_and_runs_the_good_one(dev):
    from chatterbox_amd import _lib, ops
    with torch.cuda.device(dev):
        C.check_refusals(_lib.lib, ops, dev, None, torch.cuda.synchronize)


@pytest.mark.parametrize("mis", range(4))
def test_sixty_four_rows_in_one_call(dev, mis):
    from chatterbox_amd import ops
    c = C.cases(ops.WAVE_MIX_TILE)["stack64"]
    with torch.cuda.device(dev):
        buf, rows, _ = L.padded_rows(c["rows"], mis, dev)
        obuf = torch.full((c["out_len"] + 16,), float("nan"), dtype=torch.float32, device=dev)
        out = obuf[4 + mis: 4 + mis + c["out_len"]]
        ops.wave_mix(rows, c["starts"], c["flags"], out, gain=torch.tensor(c["gain"], dtype=torch.float32, device=dev), gain_idx=c["gain_idx"], fade=c["fade"])
        torch.cuda.synchronize()
        got = obuf.cpu().numpy()
    ref = C.oracle(c["rows"], c["starts"], c["flags"], c["out_len"], c["gain"], c["gain_idx"], c["fade"])
    assert C.same_bits(got[4 + mis: 4 + mis + c["out_len"]], ref) and np.isnan(got[: 4 + mis]).all() and np.isnan(got[4 + mis + c["out_len"]:]).all()
