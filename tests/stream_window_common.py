"""Shared by tests/test_stream_window_host.py (SIMT emulator, CPU tensors), tests/test_turbo_stream_window_kernels_gpu.py and tests/test_stream_window_gpu.py
(MI355X): the inputs and the bit-for-bit checks of the two kernels behind windowed streaming -- the HiFT source with a phase carry-in
(cbx_hift_source_carry_f32) and the end-of-round emission (cbx_stream_emit_f32) -- and the windowed schedule restated on the CPU oracle.  Not a test module."""
import math

import torch


# ----------------------------------------------------------------------------------------------------------------- source with a phase carry-in
def source_inputs(dev, B=3, T=60, seed=0):
    """f0 tracks (Hz per mel frame) with unvoiced frames (0 and below the 10 Hz voicing threshold), long constant runs and jumps, so that the cumulative
    phase is hundreds of cycles away from 0 where a window starts; SineGen phases, noise and the 9 -> 1 linear of the source module."""
    g = torch.Generator().manual_seed(900 + seed)
    f0 = 80.0 + 320.0 * torch.rand(B, T, generator=g)
    f0[:, 5:25] = f0[:, 5:6]                                   # a long run of one pitch
    f0[:, 30:36] = 0.0                                         # unvoiced
    f0[0, 40:44] = 7.5                                         # below the voicing threshold, but not zero: still integrates
    f0[-1, : T // 2] = 391.995                                 # a row that starts with a long high run
    phase = (torch.rand(B, 9, generator=g) * 2 - 1) * math.pi
    phase[:, 0] = 0
    noise = torch.randn(B, 9, 480 * T, generator=g)
    lin_w = torch.randn(9, generator=g) * 0.3
    return f0.to(dev), phase.to(dev), noise.to(dev), lin_w.to(dev), 0.05


def run_source(ops, f0, phase, noise, lin_w, lin_b, cum_in=None):
    B, T = f0.shape
    s = torch.full((B, 480 * T), float("nan"), device=f0.device)
    cum = torch.full((B, 9, T), float("nan"), dtype=torch.float64, device=f0.device)
    ops.hift_source(f0.contiguous(), phase.contiguous(), noise.contiguous(), lin_w, lin_b, s, cum, cum_in=cum_in)
    return s, cum


def check_source_carry(ops, dev, w0s=(1, 17, 31, 33, 47, 59), B=3, T=60, sync=lambda: None):
    """Frames [w0, T) with cum_in = frame_cum_full[:, :, w0] and the matching slices of f0 and noise == samples [480 w0, 480 T) of the full-length source, bit
    for bit (and the window's own scan == the tail of the full one); NULL and all-zero cum_in == the entry without a carry."""
    f0, phase, noise, lin_w, lin_b = source_inputs(dev, B, T)
    full, cum = run_source(ops, f0, phase, noise, lin_w, lin_b)
    sync()
    assert torch.isfinite(full).all() and float(cum[:, 0, -1].min()) > 50.0, "the cumulative phase is far from 0 at the end"
    for w0 in w0s:
        s, c = run_source(ops, f0[:, w0:], phase, noise[:, :, 480 * w0:], lin_w, lin_b, cum_in=cum[:, :, w0].contiguous())
        sync()
        assert torch.equal(s, full[:, 480 * w0:]), f"w0={w0}: max |diff| {(s - full[:, 480 * w0:]).abs().max().item():.3e}"
        assert torch.equal(c, cum[:, :, w0:]), f"w0={w0}: the window's frame scan is not the tail of the full one"
    zeros, _ = run_source(ops, f0, phase, noise, lin_w, lin_b, cum_in=torch.zeros(B, 9, dtype=torch.float64, device=dev))
    s_null = torch.empty_like(full)
    c_null = torch.empty_like(cum)
    from chatterbox_amd._lib import check
    check(ops.lib.cbx_hift_source_carry_f32(f0.data_ptr(), phase.data_ptr(), noise.data_ptr(), lin_w.data_ptr(), lin_b, s_null.data_ptr(), c_null.data_ptr(), None,
                                            B, T, 480, 24000.0, ops._stream()), "cbx_hift_source_carry_f32")
    sync()
    assert torch.equal(zeros, full) and torch.equal(s_null, full) and torch.equal(c_null, cum)
    # a carry that is NOT the full run's moves the phase: the check above is not vacuous
    moved, _ = run_source(ops, f0[:, 17:], phase, noise[:, :, 480 * 17:], lin_w, lin_b, cum_in=(cum[:, :, 17] + 0.25).contiguous())
    sync()
    assert not torch.equal(moved, full[:, 480 * 17:])


# ----------------------------------------------------------------------------------------------------------------- end-of-round emission
def torch_emit(wav, origin, emitted, end, avail, tails, ramp):
    """The host loop at the end of a round of engine.synthesize_stream, on a window that starts at absolute sample `origin`: per utterance -> (new samples,
    next tail).  tails[b]: a 1-D tensor or None."""
    news, nxt = [], []
    fade = ramp.numel()
    for b in range(wav.shape[0]):
        new = wav[b, max(0, emitted[b] - origin): max(0, end[b] - origin)].clone() if end[b] > emitted[b] else wav[b, :0].clone()
        if tails[b] is not None and new.numel() > 0:
            k = min(tails[b].numel(), new.numel())
            new[:k] = tails[b][:k] * (1.0 - ramp[:k]) + new[:k] * ramp[:k]
        news.append(new)
        nxt.append(wav[b, end[b] - origin: min(avail[b], end[b] + fade) - origin].clone() if avail[b] > end[b] else None)
    return news, nxt


EMIT_CASES = {
    # name: (origin, L, fade, rows of (emitted, end, avail, tail length or None)); a row with emitted == end == avail is closed
    "first_round_no_tails": (0, 5280, 240, [(0, 5040, 5280, None), (0, 5040, 5280, None), (0, 4000, 4000, None)]),
    "steady_window": (9600, 20000, 480, [(14000, 29120, 29600, 480), (14000, 29120, 29600, 480), (14000, 29120, 29600, 480)]),
    "short_tails_finals_closed": (960, 9000, 480, [(3000, 7000, 7300, 300), (3000, 9960, 9960, 480), (5000, 5000, 5000, None), (3000, 3100, 3580, 480),
                                                  (3000, 3000, 3200, 7)]),
    "no_fade": (0, 3000, 0, [(0, 2880, 2880, None), (100, 3000, 3000, None)]),
}


def check_stream_emit(ops, dev, name, sync=lambda: None):
    """One cbx_stream_emit_f32 launch == torch_emit for every row: the new samples, the cross-fade (tail * (1 - ramp) + new * ramp, product by product), the
    next tails; rows beyond their valid lengths are left as they were."""
    origin, L, fade, rows = EMIT_CASES[name]
    B = len(rows)
    g = torch.Generator().manual_seed(77)
    wav = (torch.randn(B, L, generator=g) * 0.3).to(dev)
    ramp = torch.linspace(0.0, 1.0, fade + 2)[1:-1].contiguous().to(dev)
    tail_buf = (torch.randn(B, max(fade, 1), generator=g) * 0.3)[:, :fade].contiguous().to(dev)
    tails = [None if r[3] is None else tail_buf[b, : r[3]] for b, r in enumerate(rows)]
    emitted, end, avail = ([r[k] for r in rows] for k in range(3))
    want_new, want_tail = torch_emit(wav, origin, emitted, end, avail, tails, ramp)
    meta = torch.tensor([emitted, end, avail, [r[3] or 0 for r in rows]], dtype=torch.int32).to(dev)
    max_new = max(max(0, e - s) for s, e in zip(emitted, end))
    out = torch.full((B, max_new), 7.0, device=dev)
    tail_out = torch.full((B, fade), 9.0, device=dev)
    ops.stream_emit(wav, origin, meta, tail_buf if fade else None, ramp if fade else None, out, tail_out if fade else None)
    sync()
    faded = 0
    for b in range(B):
        n = want_new[b].numel()
        assert torch.equal(out[b, :n], want_new[b]), f"{name} row {b}: new samples differ, max |diff| {(out[b, :n] - want_new[b]).abs().max().item():.3e}"
        assert bool((out[b, n:] == 7.0).all()), f"{name} row {b}: wrote beyond its {n} new samples"
        k = 0 if want_tail[b] is None else want_tail[b].numel()
        if fade:
            assert k == 0 or torch.equal(tail_out[b, :k], want_tail[b]), f"{name} row {b}: next tail differs"
            assert bool((tail_out[b, k:] == 9.0).all()), f"{name} row {b}: wrote beyond its {k} tail samples"
        faded += 0 if tails[b] is None else min(n, tails[b].numel())
    return faded


# ----------------------------------------------------------------------------------------------------------------- the windowed schedule on the CPU oracle
def oracle_window_stream(O, s3_sd, tokens, ref, z, phase, noise, first, chunk, lookahead, fade, window, n_steps, meanflow=False, sil=None, drop_last=True):
    """engine._stream_rounds(window=W) for ONE utterance that never ends early, restated on the oracle's stage functions.  Round r: O.flow_inference on tokens
    [a, n) behind the full prompt with the noise of the absolute frames, O.f0_predict + O.source_module with the noise of the absolute samples and the carry
    taken as phase + 2 pi frac(cum_in) -- cum_in = the double-precision cumsum of the PREVIOUS round's f0 track up to the frame this window starts (plus that
    round's own carry); the kernel carries it in fp64 through the scan, which is the same angle up to fp32 rounding --, the previous round's source from this
    window's first sample on as the cache, O.hift_decode, trim_fade while a == 0.  sil: tokens the final round appends (Turbo); drop_last: the final round
    drops the last token's 960 samples.  z (1, 80, 2 (P + N)), phase (1, 9, 1), noise (1, 9, 960 N).  -> the pieces."""
    N, P = tokens.numel(), ref["prompt_token"].shape[1]
    pieces, emitted, tail, n = [], 0, None, min(N, first + lookahead)
    prev = None  # (a, cum (1, 9, T) float64 exclusive per-frame cumulative cycles incl. carry, source (1, 1, L) of the rows' reusable part)
    ramp = torch.linspace(0.0, 1.0, fade + 2)[1:-1]
    mult = torch.arange(1, 10, dtype=torch.float32)[None, :, None]
    while True:
        final = n >= N
        hold = 0 if final else 2 * lookahead
        a = 0 if window is None else max(0, emitted // 960 - window)
        toks = tokens[:n] if not (final and sil is not None) else torch.cat([tokens[:n], sil])
        m = toks.numel()
        win = toks[a:]
        zz = torch.cat([z[:, :, : 2 * P], z[:, :, 2 * (P + a): 2 * (P + m)]], 2)
        mel = O.flow_inference(s3_sd, win[None], torch.tensor([m - a]), ref, zz, n_steps, meanflow=meanflow, hold_back=torch.tensor([hold]))
        frames = 2 * (m - a) - hold
        mel = mel[:, :, :frames]
        f0 = O.f0_predict(s3_sd, mel)
        carry = torch.zeros(1, 9, dtype=torch.float64)
        cache = None
        if prev is not None:
            d = a - prev[0]
            carry = prev[1][:, :, 2 * d]
            cache = prev[2][:, :, 960 * d:]
        ph = phase.double() + 2 * math.pi * (carry - carry.floor())[:, :, None]
        src = O.source_module(s3_sd, f0, ph.float(), noise[:, :, 960 * a: 960 * a + 480 * frames])
        if cache is not None and cache.shape[2]:
            src = src.clone()
            src[:, :, : cache.shape[2]] = cache
        wav = O.hift_decode(s3_sd, mel, src)
        wav = (O.trim_fade(wav) if a == 0 else wav)[0]
        inc = 480.0 * ((f0[:, None, :] * mult) / 24000.0).double()       # cycles per frame, the fp32 F_mat of source_module summed in double
        cum = carry[:, :, None] + torch.cumsum(inc, 2) - inc              # exclusive
        prev = (a, cum, src[:, :, : 480 * frames])
        o = 960 * a
        keep = (max(1, m - 1) if drop_last else m) * 960
        avail = min(o + 480 * frames, keep) if final else o + 480 * frames
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
