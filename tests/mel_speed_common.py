"""Shared by tests/test_mel_speed_host.py (SIMT emulator, CPU tensors) and tests/test_turbo_stream_mel_speed_kernels_gpu.py: the NumPy fp64 restatement of the
speed-control definition (include/cbx.h cbx_mel_time_scale_f32) and the check of one launch against it.  Not a test module."""
import math

import numpy as np
import torch

U = 2.0 ** -24  # half an ulp of a fp32 in [1, 2): the unit of the rounding budget


def out_len(M, s):
    """max(1, floor(M / s)) in Python floats -- restated here, NOT imported from ops"""
    return max(1, int(math.floor(M / s)))


def taps(O, M, s):
    """Output frames 0 .. O - 1 of a row of M frames at rate s -> (i0, i1, lambda), the position in fp64"""
    j = np.arange(O, dtype=np.float64)
    x = np.maximum(0.0, (j + 0.5) * np.float64(s) - 0.5)
    i0 = np.minimum(np.floor(x).astype(np.int64), M - 1)
    i1 = np.minimum(i0 + 1, M - 1)
    return i0, i1, x - i0


def reference(row, M, s):
    """row (>= M, C) array -> (out_len(M, s), C) float64: (1 - l) row[i0] + l row[i1]"""
    row = np.asarray(row, dtype=np.float64)
    i0, i1, lam = taps(out_len(M, s), M, s)
    return (1.0 - lam)[:, None] * row[i0] + lam[:, None] * row[i1]


def log_mel(shape, seed):
    """seeded normal * 3 - 5: the scale of a log-mel"""
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * 3 - 5


def check_launch(ops, dev, in_lens, rates, T_in, strided, C=80, seed=0, extra_out=3, sync=lambda: None):
    """One ops.mel_time_scale launch over B = len(in_lens) ragged rows against the restatement.  strided=False: contiguous tensors, out allocated by the wrapper
    (T_out = the longest row).  strided=True: input and output are the first C columns of tensors with row stride C + 3 (no 16-byte access: the scalar form); the
    input's pad columns and its frames from in_lens[b] on hold NaN, the output has `extra_out` frames more than the longest row and a sentinel everywhere.
    Conditions: every valid element within 4 * 2^-24 * max|mel| of the reference (1 - l, l * b and the fma round once each: 3 roundings of a convex combination of
    values <= max|mel|, plus one of slack for l itself), no NaN there, frames [out_lens[b], T_out) exactly 0, pad columns keep the sentinel, out_lens as defined.
    Returns the largest error in units of the bound."""
    B = len(in_lens)
    mel = log_mel((B, T_in, C), seed)
    O = [out_len(m, s) for m, s in zip(in_lens, rates)]
    valid_max = max(float(mel[b, :m].abs().max()) for b, m in enumerate(in_lens))
    bound = 4 * U * valid_max
    if strided:
        big = torch.full((B, T_in, C + 3), float("nan"))
        for b, m in enumerate(in_lens):
            big[b, :m, :C] = mel[b, :m]
        big = big.to(dev)
        SENT = 12345.0
        obig = torch.full((B, max(O) + extra_out, C + 3), SENT, device=dev)
        src, dst = big[:, :, :C], obig[:, :, :C]
        assert src.stride(1) == C + 3 and not src.is_contiguous()
        out, out_lens = ops.mel_time_scale(src, rates, in_lens=list(in_lens), out=dst)
        sync()
        assert out.data_ptr() == obig.data_ptr() and bool((obig[:, :, C:] == SENT).all()), "the output's pad columns must keep their sentinel"
    else:
        out, out_lens = ops.mel_time_scale(mel.to(dev), rates, in_lens=list(in_lens))
        sync()
        assert out.shape == (B, max(O), C) and out.is_contiguous()
    assert out_lens.dtype == torch.int32 and out_lens.cpu().tolist() == O
    got = out.detach().cpu()
    worst = 0.0
    for b, (m, s) in enumerate(zip(in_lens, rates)):
        g = got[b, : O[b]].double().numpy()
        assert np.isfinite(g).all(), f"row {b}: NaN / inf in the valid region (a read beyond in_lens, or of a pad column)"
        err = float(np.abs(g - reference(mel[b].numpy(), m, s)).max())
        worst = max(worst, err / bound)
        print(f"row {b}: M={m} s={s} O={O[b]} max |err| {err:.3e} (bound {bound:.3e})")
        assert err <= bound, f"row {b} (M={m}, s={s}): max |err| {err:.3e} > {bound:.3e}"
        assert bool((got[b, O[b]:] == 0).all()), f"row {b}: frames [out_lens, T_out) must be exactly 0"
        if s < 1:
            assert torch.equal(got[b, 0], mel[b, 0]), f"row {b}: at s < 1 frame 0 samples x = 0 (lambda = 0): the first input frame itself"
    return worst
