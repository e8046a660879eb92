"""GPU (-m gpu), kernel level: cbx_mel_time_scale_f32 (ops.mel_time_scale), the mel interpolation behind `speed=`, against the NumPy fp64 restatement of its
definition (mel_speed_common.py) and against F.interpolate on the CPU -- ragged rows, every rate of the set, four rates in one launch, the float4 form on
contiguous tensors and the scalar form on views with row stride 83 whose padding holds NaN.

WHY THIS FILE NAME: test_host_logic.py::test_every_kernel_entry_point_is_named_by_a_kernel_level_test finds the kernel-level modules by a fixed list of patterns of which
`test_turbo_stream_*` is the only glob, and existing test files are not edited when a feature is added (test_turbo_stream_batch_kernels_gpu.py is the precedent).  Do not
rename this file without extending _KERNEL_LEVEL_MODULES there."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import mel_speed_common as S  # noqa: E402

pytestmark = pytest.mark.gpu

IN_LENS, T_IN = (1, 2, 7, 61), 64   # M = 1: both taps clamp; M = 7 at s = 0.9: O == M must still interpolate; the last frame at s = 0.5: i1 clamps
RATES = (0.5, 0.75, 0.9, 1.1, 1.25, 1.5, 2.0)
MIXED = (2.0, 0.75, 0.9, 1.25)


@pytest.mark.parametrize("strided", [False, True], ids=["contiguous_float4", "row_stride_83_scalar"])
@pytest.mark.parametrize("rates", [(s,) * 4 for s in RATES] + [MIXED], ids=[f"s{s}" for s in RATES] + ["four_rates"])
def test_mel_time_scale_equals_the_fp64_restatement(dev, rates, strided):
    from chatterbox_amd import ops
    with torch.cuda.device(dev):
        S.check_launch(ops, dev, IN_LENS, rates, T_IN, strided, sync=torch.cuda.synchronize)


def test_the_cases_the_shapes_are_chosen_for_are_what_they_claim():
    """Host arithmetic on the restatement: M = 7 at s = 0.9 keeps its length and is NOT a copy (torch would copy), at s < 1 frame 0 clamps x to 0, at s = 0.5 the last
    frame clamps i1, at M = 1 both taps are frame 0."""
    assert S.out_len(7, 0.9) == 7
    i0, i1, lam = S.taps(7, 7, 0.9)
    assert i0.tolist() == [0, 0, 1, 2, 3, 4, 5] and float(lam[1:].min()) > 0.05 and float(lam[0]) == 0.0
    for s in (0.5, 0.75, 0.9):
        assert S.taps(S.out_len(61, s), 61, s)[2][0] == 0.0, s
    for M in (2, 7, 61):   # s = 0.5: the last output frame lies beyond the last input frame
        i0, i1, lam = S.taps(S.out_len(M, 0.5), M, 0.5)
        assert i0[-1] == i1[-1] == M - 1 and lam[-1] == 0.25, M
    i0, i1, _ = S.taps(S.out_len(1, 0.5), 1, 0.5)
    assert i0.tolist() == i1.tolist() == [0, 0]


@pytest.mark.parametrize("s", [0.5, 0.75, 1.25, 1.5, 2.0])
def test_mel_time_scale_agrees_with_torch_interpolate(dev, s, C=80):
    """One launch over rows of M = 2, 7, 61, 500 frames against F.interpolate(mode="linear", align_corners=False, scale_factor=1 / s,
    recompute_scale_factor=False) on the CPU: the same length and the bound of the restatement test (torch's fp32 position is accurate enough at these lengths).
    Pairs with O == M, where torch copies, are skipped: of these twenty that is (M, s) = (2, 0.75) alone."""
    from chatterbox_amd import ops
    Ms = (2, 7, 61, 500)
    mel = S.log_mel((len(Ms), max(Ms), C), seed=3)
    with torch.cuda.device(dev):
        out, out_lens = ops.mel_time_scale(mel.to(dev), [s] * len(Ms), in_lens=list(Ms))
        torch.cuda.synchronize()
    got, O = out.cpu(), out_lens.cpu().tolist()
    compared = 0
    for b, M in enumerate(Ms):
        if O[b] == M:
            continue
        want = F.interpolate(mel[b, :M].t()[None], scale_factor=1.0 / s, mode="linear", align_corners=False, recompute_scale_factor=False)[0].t()
        assert want.shape[0] == O[b] == S.out_len(M, s), (M, s, want.shape, O[b])
        bound = 4 * S.U * float(mel[b, :M].abs().max())
        err = float((got[b, : O[b]].double() - want.double()).abs().max())
        print(f"M={M} s={s} O={O[b]}: max |kernel - F.interpolate| {err:.3e} (bound {bound:.3e})")
        assert err <= bound, (M, s, err, bound)
        compared += 1
    assert compared == sum(S.out_len(M, s) != M for M in Ms) == (3 if s == 0.75 else 4)


def test_descriptor_errors_and_an_out_lens_beyond_t_out(dev):
    """Null pointers, C <= 0 and a stride below C are refused before any launch; an out_lens[b] above T_out (which the host entry cannot see) is cut to T_out by
    the kernel: the frames behind the output stay untouched."""
    from chatterbox_amd import _lib
    f = _lib.lib.cbx_mel_time_scale_f32
    with torch.cuda.device(dev):
        mel = S.log_mel((1, 8, 80), seed=5).to(dev)
        buf = torch.full((2, 4, 80), 777.0, device=dev)      # the launch owns buf[0]; buf[1] lies right behind it
        rate = torch.tensor([1.25], dtype=torch.float64, device=dev)
        lens = torch.tensor([8, 6], dtype=torch.int32, device=dev)  # in_lens 8, out_lens 6 > T_out = 4
        p = lambda t: t.data_ptr()
        st = torch.cuda.current_stream().cuda_stream
        good = [p(mel), 640, 80, 8, p(lens), p(rate), p(buf), 320, 80, 4, p(lens) + 4, 1, 80, st]
        for i, bad in ((0, None), (5, None), (6, None), (10, None), (12, 0), (12, -1), (1, 79), (2, 79), (7, 79), (8, 79)):
            args = list(good)
            args[i] = bad
            assert f(*args) != 0 and b"mel_time_scale" in _lib.lib.cbx_last_error(), (i, bad)
        torch.cuda.synchronize()
        assert bool((buf == 777.0).all()), "a refused call launches nothing"
        assert f(*good) == 0
        torch.cuda.synchronize()
    want = S.reference(mel[0].cpu().numpy(), 8, 1.25)[:4]
    assert np.abs(buf[0].double().cpu().numpy() - want).max() <= 4 * S.U * float(mel.abs().max())
    assert bool((buf[1] == 777.0).all()), "out_lens > T_out must not overrun the output"
