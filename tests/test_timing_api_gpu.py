"""GPU (-m gpu): timing control -- `warp=` on the engine, `duration=` on the three TTS classes and on voice conversion, `timing=` on ChatterboxTTS -- on the
synthetic 2-layer models of test_loudness_api_gpu.py (token budget 20, EOS banned) with the stand-in tokenizer of test_word_times_api_gpu.py that has pieces().
The kernel-level tests are in test_turbo_stream_mel_warp_kernels_gpu.py, the host arithmetic in test_mel_warp_host.py."""
import math
import os
import sys
import warnings

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

from test_baseline_shapes_gpu import TOL_WAV_E2E_8S  # noqa: E402  (read-only import: the stated batch-against-single tolerance)
from test_loudness_api_gpu import _model, _rmse  # noqa: E402  (read-only import: the synthetic models of that module, token budget 20, EOS banned)
from test_seeded_api_gpu import SEEDS, TEXTS  # noqa: E402  (read-only import: the requests)
from test_word_times_api_gpu import HEADS, _PiecesTok  # noqa: E402  (read-only import: the tokenizer with pieces, the heads on layers 0 and 1)

pytestmark = pytest.mark.gpu

r = lambda v: int(math.floor(v + 0.5))


@pytest.fixture()
def tts(dev):
    m, _ = _model(dev, "ChatterboxTTS")
    saved = m.tokenizer, m.align_heads
    m.tokenizer, m.align_heads = _PiecesTok(type(m)._TEXT_VOCAB), HEADS
    yield m
    m.tokenizer, m.align_heads = saved


# ----------------------------------------------------------------------------- engine level
def test_vocode_warp_is_the_vocoder_on_the_warped_mel_and_leaves_a_plain_row_alone(dev):
    """vocode(warp=) returns hift.inference(ops.mel_time_warp(returned mel, the same tables), lens = frames, the same seeded phase / noise) cut to frames * 480,
    and a plain row beside a warped one equals the same call without warp.  Bit for bit when the unwarped vocode is run-to-run bitwise at this shape (checked
    first, and printed); otherwise within the project's batch-against-single tolerance TOL_WAV_E2E_8S."""
    from chatterbox_amd import ops, synth
    m, _ = _model(dev, "ChatterboxTTS")
    eng, ref = m.engine, m.conds.gen
    st = [synth.speech_tokens(12, seed=1), synth.speech_tokens(9, seed=2)]
    seeds = [5, 6]
    with torch.cuda.device(dev):
        a, mel_a = eng.vocode(st, ref, seeds=seeds)
        b, mel_b = eng.vocode(st, ref, seeds=seeds)
        exact = all(torch.equal(x, y) for x, y in zip(a, b)) and torch.equal(mel_a, mel_b)
        print(f"unwarped vocode run-to-run bitwise at (2, 24, 80): {exact}")
        same = (lambda x, y: torch.equal(x, y)) if exact else (lambda x, y: x.shape == y.shape and _rmse(x[None].cpu(), y[None].cpu()) <= TOL_WAV_E2E_8S)
        K = [w.numel() // 480 for w in a]
        assert K == [24, 18]
        wavs, mel = eng.vocode(st, ref, seeds=seeds, warp=[dict(frames=30), None])
        assert same(mel, mel_a), "the returned mel stays the flow's"
        assert eng.last_fit[1] is None and eng.last_fit[0]["frames"] == 30 and eng.last_fit[0]["clamped"] == [] and eng.last_fit[0]["rate"] == (0.8, 0.8)
        vmel, lens = ops.mel_time_warp(mel, [[(0, 0.0, 24 / 30)], [(0, 0.0, 1.0)]], in_lens=[24, 18], out_lens=[30, 18])
        want, _ = eng.hift.inference(vmel, lens=lens, fade=True, seeds=seeds)
        torch.cuda.synchronize()
        assert [w.numel() for w in wavs] == [30 * 480, 18 * 480]
        assert same(wavs[0], want[0, : 30 * 480]) and same(wavs[1], want[1, : 18 * 480])
        assert torch.equal(vmel[1, :18], mel[1, :18]), "the rate-1 table copies a plain row"
        assert same(wavs[1], a[1]), "a plain row beside a warped one is the row of the call without warp"
        # anchors: mel frame 8 on output frame 12, the end at 30
        wavs, mel = eng.vocode(st, ref, seeds=seeds, warp=[dict(anchors=[(8, 12)], end=30), dict(frames=12)])
        fit = eng.last_fit
        assert fit[0]["table"] == [(0, 0.0, 8 / 12), (12, 8.0, 16 / 18)] and fit[0]["achieved"] == [12] and fit[0]["frames"] == 30 and fit[1]["table"] == [(0, 0.0, 1.5)]
        vmel, lens = ops.mel_time_warp(mel, [fit[0]["table"], fit[1]["table"]], in_lens=[24, 18], out_lens=[30, 12])
        want, _ = eng.hift.inference(vmel, lens=lens, fade=True, seeds=seeds)
        torch.cuda.synchronize()
        assert [w.numel() for w in wavs] == [30 * 480, 12 * 480] and same(wavs[0], want[0, : 30 * 480]) and same(wavs[1], want[1, : 12 * 480])


# ----------------------------------------------------------------------------- duration=
@pytest.mark.parametrize("name", ["ChatterboxTTS", "ChatterboxMultilingualTTS", "ChatterboxTurboTTS", "ChatterboxVC"])
def test_duration_gives_exactly_the_frames_asked_for_or_says_what_it_gave(dev, name):
    from chatterbox_amd import ops, synth
    m, lang = _model(dev, name)
    if name == "ChatterboxVC":
        src = synth.speech_tokens(20, seed=4)
        gen = lambda **kw: m.generate(s3_tokens=src, seed=7, **kw)
    else:
        gen = lambda **kw: m.generate(TEXTS[0], *lang, seed=7, **kw)
    m.seen.clear()
    plain = gen()
    K = plain.shape[-1] // 480
    assert plain.shape[-1] == K * 480 and K >= 20
    for c in (1.25, 0.8):
        d = c * K / 50
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            wav = gen(duration=d)
        assert wav.shape[-1] == r(50 * d) * 480, (name, c, wav.shape, K)
        assert m.last_fit[0]["frames"] == r(50 * d) == m.last_fit[0]["target"] and m.last_fit[0]["clamped"] == []
        assert torch.isfinite(wav).all() and float(wav.abs().max()) > 0
    with pytest.warns(UserWarning, match="request"):
        wav = gen(duration=0.3 * K / 50)
    assert wav.shape[-1] == math.ceil(K / 2) * 480 and m.last_fit[0]["clamped"] == ["end"] and m.last_fit[0]["rate"] == (K / math.ceil(K / 2),) * 2
    d = 1.25 * K / 50
    wav16 = gen(duration=d, sample_rate=16000)
    assert wav16.shape[-1] == ops.formatted_len(r(50 * d) * 480, 16000)
    assert all(s == m.seen[0] for s in m.seen), "the speech tokens do not depend on the duration"
    with pytest.raises(ValueError, match="duration together with speed"):
        gen(duration=d, speed=1.25)


@pytest.mark.parametrize("max_batch", [None, 2])
def test_generate_batch_takes_a_duration_per_request(dev, max_batch):
    """three requests as one device batch and as sub-batches of two (the throughput schedule, where the fit reports travel with their jobs): rows 0 and 2 have the
    lengths asked for, row 1 (None) is the plain seeded request within the batch-against-single statement the seeded tests make"""
    m, lang = _model(dev, "ChatterboxTTS")
    m.max_batch = max_batch
    try:
        base = m.generate_batch(TEXTS[:3], seeds=SEEDS[:3])
        K = [w.shape[-1] // 480 for w in base]
        d = [1.25 * K[0] / 50, None, 0.3 * K[2] / 50]
        with pytest.warns(UserWarning, match="request"):
            got = m.generate_batch(TEXTS[:3], seeds=SEEDS[:3], duration=d)
    finally:
        m.max_batch = None
    assert [w.shape[-1] for w in got] == [r(50 * d[0]) * 480, K[1] * 480, math.ceil(K[2] / 2) * 480]
    assert m.last_fit[1] is None and m.last_fit[0]["clamped"] == [] and m.last_fit[0]["target"] == r(50 * d[0]) and m.last_fit[2]["clamped"] == ["end"], "in the caller's order"
    single = m.generate(TEXTS[1], seed=SEEDS[1])
    err = _rmse(got[1], single)
    print(f"max_batch={max_batch}: row 1 against generate(seed=): RMSE {err:.3e} (tolerance {TOL_WAV_E2E_8S:.1e})")
    assert err <= TOL_WAV_E2E_8S


# ----------------------------------------------------------------------------- timing=
def test_timing_puts_every_word_on_its_target_frame(dev, tts):
    """word_times=True gives the natural starts; with timing = floor(c * 2 x_i + 0.5) / 50 (2 x_i the mel frame of word i, None for a word at frame 0) and the end at
    floor(c K + 0.5) frames nothing clamps (test_mel_warp_host.py proves and enumerates it), so every returned start is its target * 24000 exactly."""
    m = tts
    text = TEXTS[3]
    m.seen.clear()
    wav0, base = m.generate(text, seed=7, word_times=True)
    K = wav0.shape[-1] // 480
    x = [2 * w["frames"][0] for w in base]
    assert m.words(text) == [w["text"] for w in base] == text.split() and [w["start"] for w in base] == [480 * v for v in x]
    assert x == sorted(x) and len(set(x)) > 1, f"the natural starts {x}"
    # a word that starts where an earlier one does (or at 0) has no input in front of it: it is asked for where it will be
    for c in (1.25, 1.5):
        timing = [None if v == 0 else r(c * v) / 50 for v in x]
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            wav, words = m.generate(text, seed=7, timing=timing, duration=r(c * K) / 50, word_times=True)
        fit = m.last_fit[0]
        assert fit["clamped"] == [], f"precondition (proved in test_mel_warp_host.py): no clamp at c = {c}: {fit}"
        assert wav.shape[-1] == r(c * K) * 480 == fit["frames"] * 480
        assert [w["frames"] for w in words] == [w["frames"] for w in base], "the tokens and their alignment do not depend on the timing"
        for w, v, t in zip(words, x, timing):
            assert w["start"] == (0 if t is None else int(round(t * 24000))) == r(c * v) * 480, (c, w, v, t)
        assert all(all(0.5 <= s <= 2.0 for _, _, s in fit["table"]) for _ in (0,))
    assert all(s == m.seen[0] for s in m.seen), "the speech tokens are identical"


def test_targets_that_cannot_be_met_are_clamped_and_reported(dev, tts):
    m = tts
    text = TEXTS[3]
    wav0, base = m.generate(text, seed=7, word_times=True)
    x = [2 * w["frames"][0] for w in base]
    with pytest.warns(UserWarning, match="clamped"):
        wav, words = m.generate(text, seed=7, timing=[0.1 * v / 50 for v in x], word_times=True)
    fit = m.last_fit[0]
    starts = [w["start"] for w in words]
    assert fit["clamped"] and starts == sorted(starts) and wav.shape[-1] == fit["frames"] * 480
    assert all(0.5 <= s <= 2.0 for _, _, s in fit["table"]) and 0.5 <= fit["rate"][0] <= fit["rate"][1] <= 2.0
    with pytest.raises(ValueError, match="entries for"):
        m.generate(text, timing=[0.1])
    turbo, _ = _model(dev, "ChatterboxTurboTTS")
    with pytest.raises(TypeError, match="timing"):
        turbo.generate(text, timing=[0.1])
    jobs = [dict(text_tokens=[m._engine_tokens(m._text_ids(text))], t3_conds=m.conds.t3.as_dict(), gen_ref=m.conds.gen, warp=[dict(anchors=[(4, 6)], end=None)])]
    with pytest.raises(ValueError, match="anchors"):
        next(iter(m.engine.synthesize_pipelined(jobs)))
