"""Shared by tests/test_mel_warp_host.py (SIMT emulator, CPU tensors), tests/test_turbo_stream_mel_warp_kernels_gpu.py and tests/test_timing_api_gpu.py: the NumPy
fp64 restatement of the timing-control definition (include/cbx.h cbx_mel_time_warp_f32), of the plan (ops.warp_plan) and of its inverse
(ops.warp_place) -- written out here, NOT imported from ops -- and the check of one launch against it.  Not a test module."""
import math

import numpy as np
import torch

from mel_speed_common import U, log_mel

SENT = 12345.0


def positions(O, table):
    """Output frames 0 .. O - 1 under table [(o, a, s), ...] -> their input positions in fp64: frame j belongs to the last segment k with o_k <= j (the first when
    there is none) and sits at x = max(0, a_k + (((j - o_k) + 0.5) s_k - 0.5)); a NaN counts as 0."""
    o = np.array([t[0] for t in table], dtype=np.int64)
    a = np.array([t[1] for t in table], dtype=np.float64)
    s = np.array([t[2] for t in table], dtype=np.float64)
    j = np.arange(O, dtype=np.int64)
    k = np.zeros(O, dtype=np.int64)
    for i in range(len(table)):  # "the last k with o_k <= j" for an increasing o
        k[j >= o[i]] = i
    with np.errstate(invalid="ignore", over="ignore"):
        x = a[k] + (((j - o[k]).astype(np.float64) + 0.5) * s[k] - 0.5)
    x = np.where(np.isnan(x), 0.0, x)
    return np.maximum(0.0, x)


def taps(O, M, table):
    x = positions(O, table)
    i0 = np.minimum(np.floor(np.minimum(x, 1e15)).astype(np.int64), M - 1)
    i1 = np.minimum(i0 + 1, M - 1)
    return i0, i1, np.clip(x - i0, 0.0, 1.0)


def reference(row, M, O, table):
    """row (>= M, C) array -> (O, C) float64: (1 - l) row[i0] + l row[i1]"""
    row = np.asarray(row, dtype=np.float64)
    i0, i1, lam = taps(O, M, table)
    return (1.0 - lam)[:, None] * row[i0] + lam[:, None] * row[i1]


def plan(K, anchors, end=None, lo=0.5, hi=2.0):
    """The plan of the feature, restated: start at (x, o) = (0, 0); anchor (x, t) with L = x - x_prev > 0 gets n = min(max(t - o_prev, ceil(L / hi), 1),
    floor(L / lo)) frames; one with L = 0 is dropped; the last segment runs to K with target `end` (None: rate 1).
    -> (table, frames, achieved, clamped anchors)"""
    table, achieved, clamped, x0, o0 = [], [], [], 0, 0
    for k, (x, t) in enumerate(anchors):
        L = x - x0
        if L > 0:
            n = min(max(t - o0, math.ceil(L / hi), 1), math.floor(L / lo))
            table.append((o0, float(x0), L / n))
            x0, o0 = x, o0 + n
        achieved.append(o0)
        if o0 != t:
            clamped.append(k)
    L = K - x0
    if L > 0:
        n = min(max((L if end is None else end - o0), math.ceil(L / hi), 1), math.floor(L / lo))
        table.append((o0, float(x0), L / n))
        o0 += n
    return table, o0, achieved, clamped


def place(table, x):
    """Input position x -> output position o_k + (x - a_k) / s_k, k the last segment with a_k <= x"""
    k = max([i for i, t in enumerate(table) if t[1] <= x], default=0)
    o, a, s = table[k]
    return o + (x - a) / s


def alternating(n_seg):
    """n_seg segments, continuous, the rates alternating 0.5 (one input frame over two output frames) and 2.0 (two input frames in one output frame)
    -> (table, frames, the input position its end maps to: where that lies beyond the row the taps clamp to the last frame)"""
    table, o, a = [], 0, 0.0
    for i in range(n_seg):
        s, n = (0.5, 2) if i % 2 == 0 else (2.0, 1)
        table.append((o, a, s))
        o, a = o + n, a + n * s
    return table, o, a


def per_output_frame(M, s=0.75):
    """One segment per OUTPUT frame at rate s, continuous: floor(M / s) segments of one frame each -> (table, frames)"""
    O = max(1, int(math.floor(M / s)))
    return [(j, j * s, s) for j in range(O)], O


def check_launch(ops, dev, in_lens, tables, out_lens, T_in, strided, C=80, seed=0, extra_out=3, sync=lambda: None, finite_only=False):
    """One ops.mel_time_warp launch over B = len(in_lens) ragged rows against the restatement; the layout, the poison and the conditions are those of
    mel_speed_common.check_launch: strided=False contiguous tensors (the float4 form), out allocated by the wrapper; strided=True the first C columns of tensors
    with row stride C + 3 (the scalar form), NaN in the input's pad columns and in its frames from in_lens[b] on, `extra_out` frames more than the longest row and
    a sentinel everywhere in the output.  Every valid element within 4 * 2^-24 * max|mel| of the reference (1 - l, l * b and the fma round once each: 3 roundings
    of a convex combination of values <= max|mel|, plus one of slack for l itself; the extra fp64 add moves x by ~1e-13 frames, far below that), no NaN there,
    frames [out_lens[b], T_out) exactly 0, pad columns and the frames of other buffers keep the sentinel.  finite_only (a MALFORMED table, whose map the
    restatement does not define): every valid element is finite and within max|mel| instead.  Returns (out on the CPU, the largest error in units of the bound)."""
    B = len(in_lens)
    mel = log_mel((B, T_in, C), seed)
    O = list(out_lens)
    valid_max = max(float(mel[b, :m].abs().max()) for b, m in enumerate(in_lens))
    bound = 4 * U * valid_max
    poisoned = torch.full((B, T_in, C + 3 if strided else C), float("nan"))
    for b, m in enumerate(in_lens):
        poisoned[b, :m, :C] = mel[b, :m]
    if strided:
        big = poisoned.to(dev)
        obig = torch.full((B, max(O) + extra_out, C + 3), SENT, device=dev)
        src, dst = big[:, :, :C], obig[:, :, :C]
        assert src.stride(1) == C + 3 and not src.is_contiguous()
        out, ol = ops.mel_time_warp(src, tables, in_lens=list(in_lens), out=dst, out_lens=O)
        sync()
        assert out.data_ptr() == obig.data_ptr() and bool((obig[:, :, C:] == SENT).all()), "the output's pad columns must keep their sentinel"
    else:
        out, ol = ops.mel_time_warp(poisoned.to(dev), tables, in_lens=list(in_lens), out_lens=O)
        sync()
        assert out.shape == (B, max(O), C) and out.is_contiguous()
    assert ol.dtype == torch.int32 and ol.cpu().tolist() == O
    got = out.detach().cpu()
    worst = 0.0
    for b, m in enumerate(in_lens):
        g = got[b, : O[b]].double().numpy()
        assert np.isfinite(g).all(), f"row {b}: NaN / inf in the valid region (a read beyond in_lens, or of a pad column)"
        assert bool((got[b, O[b]:] == 0).all()), f"row {b}: frames [out_lens, T_out) must be exactly 0"
        if finite_only:
            assert float(np.abs(g).max()) <= valid_max * (1 + 4 * U), f"row {b}: a blend of valid frames cannot exceed max|mel|"
            continue
        err = float(np.abs(g - reference(mel[b].numpy(), m, O[b], tables[b])).max())
        worst = max(worst, err / bound)
        print(f"row {b}: M={m} segments={len(tables[b])} O={O[b]} max |err| {err:.3e} (bound {bound:.3e})")
        assert err <= bound, f"row {b} (M={m}, {len(tables[b])} segments): max |err| {err:.3e} > {bound:.3e}"
    return got, worst
