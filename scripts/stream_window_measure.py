"""What bounded-cost ("windowed") streaming costs and what it changes, on one MI355X, one process:

  tts   engine.synthesize_stream at the bench shape (250 tokens, 10 s) and at 1000 tokens (40 s), B = 1 and B = 8, window=None (the schedule before windows;
        the same code path) and window=200: first-audio and whole-stream wall time (default overlapped form, median of 3), and the flow + vocoder time of
        EVERY round (serial form, synchronised around each stage);
  vc    ChatterboxEngine.vocode_stream at 1500 tokens (60 s), B = 1, on the T3-less engine ChatterboxVC builds: one-shot vocode() against the stream with
        window in {None, 50, 100, 200, 400};
  sens  for the same tokens and noise: mel L1 and waveform RMSE of the windowed stream against the one-shot synthesis per window size, over samples at least
        8000 away from every seam.  The weights are SEEDED RANDOM-INIT: this measures how far a truncated left context moves the output of such a model, it
        says nothing about perceptual quality.

    python scripts/stream_window_measure.py [tts] [vc] [sens]        (default: all three; one JSON line per row)"""
import json
import statistics
import sys
import time

import torch

sys.path.insert(0, ".")
from chatterbox_amd import synth  # noqa: E402
from chatterbox_amd.api import ChatterboxVC  # noqa: E402
from chatterbox_amd.engine import ChatterboxEngine, stream_window_schedule  # noqa: E402

dev = torch.device("cuda", 0)
what = set(sys.argv[1:]) or {"tts", "vc", "sens"}
say = lambda **kw: print(json.dumps(kw), flush=True)
ms = lambda s: round(1e3 * s, 1)


def timed_stages(eng):
    """Wrap flow.inference / hift.inference with a synchronised wall clock -> (per-call lists, restore())."""
    t = {"flow": [], "hift": []}
    saved = eng.flow.inference, eng.hift.inference

    def wrap(fn, key):
        def run(*a, **k):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn(*a, **k)
            torch.cuda.synchronize()
            t[key].append(time.perf_counter() - t0)
            return out
        return run
    eng.flow.inference, eng.hift.inference = wrap(saved[0], "flow"), wrap(saved[1], "hift")

    def restore():
        eng.flow.inference, eng.hift.inference = saved
    return t, restore


def wall(make_stream, reps=4):
    """(median first-yield s, median total s, rounds) over reps - 1 runs (the first one warms graphs and kernel forms)."""
    first, total, n = [], [], 0
    for rep in range(reps):
        torch.cuda.synchronize()
        t0, f, n = time.perf_counter(), None, 0
        for _ in make_stream(rep):
            n += 1
            f = f if f is not None else time.perf_counter() - t0
        torch.cuda.synchronize()
        if rep:
            first.append(f), total.append(time.perf_counter() - t0)
    return statistics.median(first), statistics.median(total), n


if "tts" in what:
    L = 30
    eng = ChatterboxEngine(synth.t3_state_dict(L, 0), synth.s3gen_state_dict(0), dev, n_t3_layers=L)
    t3c, gen = synth.t3_cond(prompt_len=150), synth.s3gen_ref()
    for N in (250, 1000):
        for B in (1, 8):
            texts = [synth.text_tokens(64, seed=b) for b in range(B)]
            for window in (None, 200):
                def stream(rep, **kw):
                    us = torch.rand(B, N, generator=torch.Generator(device=dev).manual_seed(99 + rep), device=dev)
                    return eng.synthesize_stream(texts, t3c, gen, max_new_tokens=N, uniforms=us, ban_eos=True, ban_from=6561, window=window, **kw)
                f, tot, n = wall(stream)
                t, restore = timed_stages(eng)
                list(stream(0, overlap=False))
                restore()
                say(part="tts", tokens=N, B=B, window=window, rounds=n, first_audio_ms=ms(f), stream_ms=ms(tot), audio_s_per_wall_s=round(B * (N - 1) / 25.0 / tot, 1),
                    tokens_per_round=[n_r - a for a, n_r in stream_window_schedule(N, window=window)],
                    round_flow_ms=[ms(x) for x in t["flow"]], round_vocoder_ms=[ms(x) for x in t["hift"]])
    del eng
    torch.cuda.empty_cache()

if what & {"vc", "sens"}:
    eng = ChatterboxVC._engine(synth.s3gen_state_dict(0), dev)
    gen = synth.s3gen_ref()
    P = gen["prompt_token"].shape[-1]

if "vc" in what:
    N = 1500
    toks = [synth.speech_tokens(N, seed=1)]
    eng.vocode(toks, gen)
    one = []
    for _ in range(4):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        w, _ = eng.vocode(toks, gen, sync=False)
        w[0].cpu()
        one.append(time.perf_counter() - t0)
    say(part="vc", tokens=N, mode="one-shot vocode", ms=ms(statistics.median(one[1:])), audio_s_per_wall_s=round(N / 25.0 / statistics.median(one[1:]), 1))
    for window in (200, 50, 100, 400, None):
        f, tot, n = wall(lambda rep: eng.vocode_stream(toks, gen, window=window))
        t, restore = timed_stages(eng)
        list(eng.vocode_stream(toks, gen, window=window))
        restore()
        per = [a + b for a, b in zip(t["flow"], t["hift"])]
        say(part="vc", tokens=N, mode="vocode_stream", window=window, rounds=n, first_audio_ms=ms(f), stream_ms=ms(tot), audio_s_per_wall_s=round(N / 25.0 / tot, 1),
            round_ms_first=ms(per[0]), round_ms_median=ms(statistics.median(per)), round_ms_last=ms(per[-1]), round_ms_max=ms(max(per)))

if "sens" in what:
    print("# sensitivity to the window: SEEDED RANDOM-INIT weights -- how far a truncated left context moves THIS model's output; not a measure of perceptual quality",
          flush=True)
    N, fade, look = 500, 480, 3
    toks = [synth.speech_tokens(N, seed=2)]
    z, noise = synth.randn((1, 2 * (P + N), 80), seed=5).to(dev), synth.randn((1, 9, 960 * N), seed=6).to(dev)
    phase = ((synth.rand((1, 9), seed=6) * 2 - 1) * 3.141592653589793).to(dev)
    phase[:, 0] = 0
    kw = dict(z=z, phase=phase, noise=noise)
    full, mel_full = eng.vocode(toks, gen, **kw)
    full, mel_full = full[0].cpu(), mel_full[0].cpu()
    for window in (None, 400, 200, 100, 50, 20, 10):
        sched = stream_window_schedule(N, window=window, fade=fade, lookahead=look)
        mels, hift = [], eng.hift.inference
        eng.hift.inference = lambda mel, *a, **k: (mels.append(mel[0].cpu()), hift(mel, *a, **k))[1]
        pieces = [r["wavs"][0] for r in eng.vocode_stream(toks, gen, window=window, fade=fade, lookahead=look, **kw)]
        eng.hift.inference = hift
        wav = torch.cat(pieces)
        seams = torch.tensor([0] + list(torch.tensor([p.numel() for p in pieces]).cumsum(0)[:-1]))
        pos = torch.arange(wav.numel())
        away = ((pos[:, None] - seams[None, :]).abs().min(1).values >= 8000)
        rmse_all = (wav - full).pow(2).mean().sqrt().item()
        rmse_away = (wav - full)[away].pow(2).mean().sqrt().item()
        # the mel frames a round was the LAST to emit from: frames [E_r / 480, E_{r+1} / 480) of round r's window (origin 2 a_r)
        l1, e = [], 0
        for (a, _), m, p in zip(sched, mels, pieces):
            f0, f1 = e // 480, (e + p.numel()) // 480
            l1.append((m[f0 - 2 * a: f1 - 2 * a] - mel_full[f0:f1]).abs().mean(1))
            e += p.numel()
        say(part="sens", tokens=N, window=window, rounds=len(pieces), mel_l1_emitted_frames=float(f"{torch.cat(l1).mean().item():.3e}"),
            wav_rmse=float(f"{rmse_all:.3e}"), wav_rmse_8000_from_seams=float(f"{rmse_away:.3e}"), samples_compared=int(away.sum()),
            one_shot_wav_rms=float(f"{full.pow(2).mean().sqrt().item():.3e}"))
