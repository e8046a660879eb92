"""Shared by tests/test_stream_speed_host.py (SIMT emulator, CPU tensors), tests/test_turbo_stream_speed_window_kernels_gpu.py and tests/test_stream_speed_gpu.py
(MI355X): the NumPy fp64 restatement of a WINDOW of the speed-control map (cbx_mel_time_scale_win_f32; built on mel_speed_common.taps, nothing imported from
chatterbox_amd.ops or .engine), the host rules of a stream at a speaking rate restated on it, the checks of one window launch, and the windowed schedule at a rate
restated on the CPU oracle.  Not a test module."""
import ctypes
import math

import numpy as np
import torch

import mel_speed_common as S

FAR = 1 << 62  # "no clamp": a row longer than any index


# ----------------------------------------------------------------------------------------------------------------- the map, restated
def abs_taps(j0, n, s, M_abs=FAR):
    """Absolute stretched frames [j0, j0 + n) at rate s over a row of M_abs unscaled frames -> (i0, i1, lambda), absolute indices (S.taps: position in fp64)"""
    i0, i1, lam = S.taps(j0 + n, M_abs, s)
    return i0[j0:], i1[j0:], lam[j0:]


def position(j, s):
    return max(0.0, (j + 0.5) * s - 0.5)


def first_frame_at(x0, s):
    j = 0
    while position(j, s) < x0:
        j += 1
    return j


def ready_frames(M_abs, s):
    """frames [0, R) whose right tap exists without a clamp: floor(x_j) + 1 <= M_abs - 1"""
    j = 0
    while M_abs >= 2 and math.floor(position(j, s)) + 1 <= M_abs - 1:
        j += 1
    return j


def origin_frame(i_org, s):
    """the first frame all of whose taps lie at or right of unscaled frame i_org, with the quarter-frame margin; 0 at the start"""
    return 0 if i_org == 0 else first_frame_at(i_org + 0.25, s)


def window_origin(E, W, s):
    """tokens: je = E // 480, ie = floor(x_je + max(0, s - 1)), a = max(0, ie // 2 - W)"""
    return max(0, int(math.floor(position(E // 480, s) + max(0.0, s - 1.0) + 1e-9)) // 2 - W)


def stretch_window(mel, i_org, j0, n, s, M_abs):
    """mel (C, T) float tensor = unscaled frames [i_org, i_org + T) of a row of M_abs frames -> (C, n) float32: absolute stretched frames [j0, j0 + n), the blend
    in fp64"""
    i0, i1, lam = abs_taps(j0, n, s, M_abs)
    assert n == 0 or (i0.min() >= i_org and i1.max() < i_org + mel.shape[1]), "a tap outside the window"
    m = mel.double().numpy()
    return torch.from_numpy((1.0 - lam)[None] * m[:, i0 - i_org] + lam[None] * m[:, i1 - i_org]).float()


# ----------------------------------------------------------------------------------------------------------------- one window launch
LENS = (61, 52, 45)  # ragged rows inside T_in = 61, all longer than the largest i_org
SENT = 12345.0


def check_window_launch(ops, dev, rate, i_org, strided, T_in=61, C=80, seed=0, sync=lambda: None):
    """B = 3 rows of LENS valid frames; the window holds unscaled frames [i_org, T_in) and its output starts at j0 = origin_frame(i_org, rate).  Row 0 asks for every
    frame up to out_len(M, rate) (the last taps clamp to the row's end, as a final round's do), rows 1 and 2 for their ready frames only.
      (a) == frames [j0, j0 + n) of ONE ops.mel_time_scale launch over the whole rows, bit for bit;
      (b) within 4 * 2^-24 * max|mel| of the fp64 restatement (mel_speed_common.check_launch derives the bound);
      (c) i_org = 0 (so j0 = 0) is the whole launch itself;
      (d) frames [out_lens, T_out) are exactly 0; the sentinel in the output's pad columns and in the frames behind T_out survives; NaN in the input frames beyond
          in_lens, in its pad columns and in the frame LEFT of the window reaches nothing.
    strided: views with row stride C + 3 (the scalar form); else contiguous, 16-byte aligned (the float4 form).  Returns the largest error in units of the bound."""
    B = len(LENS)
    mel = S.log_mel((B, T_in, C), seed)
    j0 = origin_frame(i_org, rate)
    O_abs = [S.out_len(LENS[0], rate)] + [ready_frames(m, rate) for m in LENS[1:]]
    n = [max(0, o - j0) for o in O_abs]
    assert min(n) > 0, "every row has frames in the window"
    in_lens = [m - i_org for m in LENS]
    whole, whole_lens = ops.mel_time_scale(mel.to(dev), [rate] * B, in_lens=list(LENS))
    sync()
    assert whole_lens.tolist() == [S.out_len(m, rate) for m in LENS]
    whole = whole.cpu()
    Tw, T_out, ld = T_in - i_org, max(n) + 3, C + 3 if strided else C
    big = torch.full((B, 1 + Tw, ld), float("nan"))       # frame 0: the frame left of the window
    for b, m in enumerate(LENS):
        big[b, 1: 1 + in_lens[b], :C] = mel[b, i_org:m]
    big = big.to(dev)
    obig = torch.full((B, T_out + 2, ld), SENT, device=dev)
    src, dst = big[:, 1:, :C], obig[:, :T_out, :C]
    assert src.stride(1) == ld and (strided or (src.data_ptr() % 16 == 0 and dst.data_ptr() % 16 == 0))
    out, out_lens = ops.mel_time_scale_window(src, rate, j0, i_org, in_lens, n, out=dst)
    sync()
    assert out.data_ptr() == obig.data_ptr() and out_lens.dtype == torch.int32 and out_lens.cpu().tolist() == n
    got_all = obig.cpu()
    assert bool((got_all[:, T_out:] == SENT).all()), "frames behind T_out must keep their sentinel"
    assert bool((got_all[:, :, C:] == SENT).all()), "the output's pad columns must keep their sentinel"
    got = got_all[:, :T_out, :C]
    bound = 4 * S.U * max(float(mel[b, :m].abs().max()) for b, m in enumerate(LENS))
    worst = 0.0
    for b, m in enumerate(LENS):
        g = got[b, : n[b]]
        assert torch.isfinite(g).all(), f"row {b}: NaN / inf in the valid region (a read left of the window, beyond in_lens, or of a pad column)"
        assert torch.equal(g, whole[b, j0: j0 + n[b]]), f"row {b}: window launch != the whole launch's frames [{j0}, {j0 + n[b]}), max |diff| {(g - whole[b, j0: j0 + n[b]]).abs().max().item():.3e}"
        ref = S.reference(mel[b].numpy(), m, rate)[j0: j0 + n[b]]
        err = float(np.abs(g.double().numpy() - ref).max())
        worst = max(worst, err / bound)
        print(f"rate {rate} i_org {i_org} j0 {j0} row {b}: M={m} frames {n[b]} max |err| {err:.3e} (bound {bound:.3e})")
        assert err <= bound, f"row {b}: max |err| {err:.3e} > {bound:.3e}"
        assert bool((got[b, n[b]:] == 0).all()), f"row {b}: frames [out_lens, T_out) must be exactly 0"
    if i_org == 0:
        assert j0 == 0 and torch.equal(got[0, : n[0]], whole[0, : whole_lens[0]]), "j0 = i_org = 0 is cbx_mel_time_scale_f32 itself"
    return worst


def check_far_window(ops, dev, rate, sync=lambda: None, C=80):
    """(e) the fp64 position at a long stream's offset: j0 ~ 2^20 over an 8-frame input, against the restatement within the same bound"""
    j0 = (1 << 20) + 3
    i_org = int(math.floor(position(j0, rate) - 0.25))
    assert position(j0, rate) >= i_org + 0.25
    n = 0
    while math.floor(position(j0 + n, rate)) + 1 <= i_org + 7:
        n += 1
    assert n >= 3
    mel = S.log_mel((1, 8, C), 9)
    out, _ = ops.mel_time_scale_window(mel.to(dev), rate, j0, i_org, [8], [n])
    sync()
    want = stretch_window(mel[0].t(), i_org, j0, n, rate, FAR).t().double().numpy()
    i0, i1, lam = abs_taps(j0, n, rate)
    ref = (1.0 - lam)[:, None] * mel[0].double().numpy()[i0 - i_org] + lam[:, None] * mel[0].double().numpy()[i1 - i_org]
    assert np.abs(want - ref).max() <= 1e-6
    err, bound = float(np.abs(out[0].cpu().double().numpy() - ref).max()), 4 * S.U * float(mel.abs().max())
    print(f"far window rate {rate}: j0 {j0} i_org {i_org} frames {n} max |err| {err:.3e} (bound {bound:.3e})")
    assert out.shape == (1, n, C) and err <= bound
    return err / bound


def descriptor_errors(lib):
    """(f) every refused descriptor returns -22 with a message before any launch (host buffers: a launch of the product library on them would fault)"""
    f = lib.cbx_mel_time_scale_win_f32
    buf, lens = (ctypes.c_float * 64)(), (ctypes.c_int * 2)(4, 3)
    a = ctypes.addressof
    #        in     sb  ld T_in in_lens  rate  j0 i_org out        sb  ld T_out out_lens    B  C  stream
    good = [a(buf), 32, 8, 4, a(lens), 1.25, 2, 2, a(buf) + 128, 32, 8, 4, a(lens) + 4, 1, 8, None]
    bads = ((0, None), (8, None), (12, None), (14, 0), (14, -3), (1, 7), (2, 7), (9, 7), (10, 7), (3, -1), (11, -1), (13, -1), (5, 0.0), (5, float("nan")),
            (5, float("inf")), (5, -1.25), (6, -1), (7, -1))
    for i, bad in bads:
        args = list(good)
        args[i] = bad
        assert f(*args) == -22 and b"mel_time_scale_win" in lib.cbx_last_error(), (i, bad)
    for i in (13, 11):   # B = 0, T_out = 0: nothing to do, no launch
        args = list(good)
        args[i] = 0
        assert f(*args) == 0


# ----------------------------------------------------------------------------------------------------------------- the windowed schedule at a rate, on the CPU oracle
def oracle_window_stream(O, s3_sd, tokens, ref, z, phase, noise, first, chunk, lookahead, fade, window, n_steps, rate, meanflow=False, sil=None, drop_last=True):
    """stream_window_common.oracle_window_stream with a speaking rate: after O.flow_inference the window's mel is stretched by the fp64 restatement over ABSOLUTE
    stretched frames [j0, R) (R: the ready frames, or all out_len(M_abs, rate) of the final round), and everything after it -- the noise columns, the phase carry
    and the cached source of the previous round (offset j0 - j0_prev), trim_fade (j0 == 0), emitted / end / avail and the tail -- is indexed in stretched frames and
    samples.  noise (1, 9, >= 480 * out_len(2 N, rate)).  -> the pieces."""
    N, P = tokens.numel(), ref["prompt_token"].shape[1]
    pieces, emitted, tail, n = [], 0, None, min(N, first + lookahead)
    prev = None  # (j0, cum (1, 9, T) float64 exclusive per-frame cumulative cycles incl. carry, source (1, 1, L))
    ramp = torch.linspace(0.0, 1.0, fade + 2)[1:-1]
    mult = torch.arange(1, 10, dtype=torch.float32)[None, :, None]
    while True:
        final = n >= N
        hold = 0 if final else 2 * lookahead
        a = 0 if window is None else window_origin(emitted, window, rate)
        j0 = origin_frame(2 * a, rate)
        toks = tokens[:n] if not (final and sil is not None) else torch.cat([tokens[:n], sil])
        m = toks.numel()
        zz = torch.cat([z[:, :, : 2 * P], z[:, :, 2 * (P + a): 2 * (P + m)]], 2)
        mel = O.flow_inference(s3_sd, toks[a:][None], torch.tensor([m - a]), ref, zz, n_steps, meanflow=meanflow, hold_back=torch.tensor([hold]))
        M_abs = 2 * m - hold
        R = S.out_len(M_abs, rate) if final else ready_frames(M_abs, rate)
        nv = R - j0
        assert nv > 0
        vmel = stretch_window(mel[0, :, : M_abs - 2 * a], 2 * a, j0, nv, rate, M_abs)[None]
        f0 = O.f0_predict(s3_sd, vmel)
        carry = torch.zeros(1, 9, dtype=torch.float64)
        cache = None
        if prev is not None:
            d = j0 - prev[0]
            carry = prev[1][:, :, d]
            cache = prev[2][:, :, 480 * d:]
        ph = phase.double() + 2 * math.pi * (carry - carry.floor())[:, :, None]
        o = 480 * j0
        assert noise.shape[2] >= o + 480 * nv
        src = O.source_module(s3_sd, f0, ph.float(), noise[:, :, o: o + 480 * nv])
        if cache is not None and cache.shape[2]:
            src = src.clone()
            src[:, :, : cache.shape[2]] = cache
        wav = O.hift_decode(s3_sd, vmel, src)
        wav = (O.trim_fade(wav) if j0 == 0 else wav)[0]
        inc = 480.0 * ((f0[:, None, :] * mult) / 24000.0).double()
        cum = carry[:, :, None] + torch.cumsum(inc, 2) - inc
        prev = (j0, cum, src[:, :, : 480 * nv])
        keep = 480 * S.out_len(2 * (max(1, m - 1) if drop_last else m), rate)
        avail = min(o + 480 * nv, keep) if final else o + 480 * nv
        end = avail if final else max(emitted, avail - fade)
        new = wav[emitted - o: end - o].clone()
        if tail is not None and new.numel():
            k = min(tail.numel(), new.numel())
            new[:k] = tail[:k] * (1 - ramp[:k]) + new[:k] * ramp[:k]
        tail = None if final else wav[end - o: min(avail, end + fade) - o].clone()
        emitted = end
        pieces.append(new)
        if final:
            return pieces
        n = min(N, n + max(1, int(round(chunk))))
