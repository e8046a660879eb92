"""GPU (-m gpu): the entry-level tests of cbx_wave_pan_mix_f32, cbx_wave_loudness_ch_f32 and cbx_wave_limit_ch_f32, beside the other wave kernels': the refusals
of each entry on device pointers with the good descriptor run afterwards, and R = 64 rows -- the most a call takes --: ops.wave_pan_mix over 64 stacked rows
bitwise against the restatement, ops.wave_loudness_ch and ops.wave_limit_ch over 32 two-channel signals bitwise against launches over one signal each (a signal's
numbers do not depend on its neighbours).  The cases and properties of the definitions are in test_stereo_kernels_gpu.py."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import stereo_common as S  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("entry,check", [("cbx_wave_pan_mix_f32", "pan"), ("cbx_wave_loudness_ch_f32", "loud"), ("cbx_wave_limit_ch_f32", "limit")])
def test_the_entry_refuses_bad_descriptors_on_device_pointers_and_runs_the_good_one(dev, entry, check):
    from chatterbox_amd import _lib, ops
    assert hasattr(_lib.lib, entry)
    with torch.cuda.device(dev):
        getattr(S, f"check_{check}_refusals")(_lib.lib, ops, dev, torch.cuda.current_stream().cuda_stream, torch.cuda.synchronize)


def test_sixty_four_rows_in_one_pan_mix(dev):
    from chatterbox_amd import ops
    c = S.M.cases(ops.WAVE_MIX_TILE)["stack64"]
    pan = [ops.pan_gains(-1.0 + 2.0 * r / 63.0) for r in range(64)]
    with torch.cuda.device(dev):
        buf, rows, _ = S.L.padded_rows(c["rows"], 1, dev)
        obuf = torch.full((2 * c["out_len"] + 16,), float("nan"), dtype=torch.float32, device=dev)
        out = obuf[5: 5 + 2 * c["out_len"]].view(2, c["out_len"])
        ops.wave_pan_mix(rows, c["starts"], c["flags"], pan, out, gain=torch.tensor(c["gain"], dtype=torch.float32, device=dev), gain_idx=c["gain_idx"], fade=c["fade"])
        torch.cuda.synchronize()
        got = obuf.cpu().numpy()
    ref = S.pan_oracle(c["rows"], c["starts"], c["flags"], pan, c["out_len"], c["gain"], c["gain_idx"], c["fade"])
    assert S.M.same_bits(got[5: 5 + 2 * c["out_len"]].reshape(2, -1), ref) and np.isnan(got[:5]).all() and np.isnan(got[5 + 2 * c["out_len"]:]).all()


def test_thirty_two_signals_in_one_meter_and_one_limiter_call(dev):
    from chatterbox_amd import ops
    n = 4 * S.HOP + 77
    sig = [S.K.bursts(n, 100 + r) * np.float32(3.0) for r in range(64)]
    with torch.cuda.device(dev):
        buf, rows, _ = S.L.padded_rows(sig, 1, dev)
        st, g = ops.wave_loudness_ch(rows, [-5.0] * 32, None)
        out, ls = ops.wave_limit_ch(rows, [-1.0] * 32, gain=g)
        torch.cuda.synchronize()
        st, g, ls, out = st.cpu().numpy(), g.cpu().numpy(), ls.cpu().numpy(), [o.cpu().numpy() for o in out]
        assert st.shape == (32, 4) and g.shape == (32,) and ls.shape == (32, 4) and len(out) == 64
        for s in (0, 17, 31):
            b1, r1, _ = S.L.padded_rows(sig[2 * s: 2 * s + 2], 2, dev)
            st1, g1 = ops.wave_loudness_ch(r1, [-5.0], None)
            o1, ls1 = ops.wave_limit_ch(r1, [-1.0], gain=g1)
            torch.cuda.synchronize()
            assert st1.cpu().numpy().tobytes() == st[s: s + 1].tobytes() and g1.cpu().numpy().tobytes() == g[s: s + 1].tobytes() and ls1.cpu().numpy().tobytes() == ls[s: s + 1].tobytes()
            assert all(S.M.same_bits(o1[c].cpu().numpy(), out[2 * s + c]) for c in range(2)), f"signal {s}: the same bits alone and among 32"
    assert np.isfinite(st[:, 0]).all() and (ls[:, 2] > 0).all(), "every signal is measured, and every signal is limited"
