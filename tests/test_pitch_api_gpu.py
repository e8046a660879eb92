"""GPU (-m gpu): pitch= through the engines and the public API on synthetic 2-layer models with a token budget of 20 (0.8 s, 40 frames).  For a seeded request
the SOURCE is what the same method returns with speed = s / r and no pitch (r = 2^(p / 12)): the flow, the stretch and the vocoder of the pitched call are exactly
that call's.  The result with pitch=p, speed=s must have the length of the call with speed=s alone and lie, element for element, within the bound of the fp64
restatement (wave_pitch_common.py) applied to that source.
generate of the four classes at one positive and one negative p (the negative one with s != 1), generate_batch with a mixed list over two sub-batches (ChatterboxTTS:
the throughput schedule, synthesize_pipelined), loudness= / max_pause= / a delivery format behind the pitch (each bitwise the existing ops step applied to the pitched
call's plain result), generate_long and generate_long_stream, pitch=None and 0 bitwise and call for call the method without the argument, and the ValueErrors before
any launch.  The kernel-level tests are in test_turbo_stream_wave_pitch_kernels_gpu.py."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import wave_pitch_common as P  # noqa: E402
from test_loudness_api_gpu import TTS, _model  # noqa: E402  (read-only import: the synthetic models of the module, token budget 20, EOS banned)
from test_seeded_api_gpu import SEEDS, TEXTS  # noqa: E402  (read-only import: the requests)

pytestmark = pytest.mark.gpu

CASES = [(3.0, 1.0), (-2.0, 0.8)]   # (semitones, speed)


def _within(got, source, p, plain, what):
    """got = the pitched call's (1, N) result, source = the (1, n_src) result at speed s / r, plain = the (1, N) result at speed s"""
    assert got.dtype == torch.float32 and got.shape == plain.shape, f"{what}: {tuple(got.shape)}, the call without pitch returns {tuple(plain.shape)}"
    worst = P.check_bound(got[0].numpy(), source[0].numpy(), P.ratio(p), what)
    print(f"{what}: {source.shape[1]} source samples -> {got.shape[1]}, worst error / bound = {worst:.3f}")


@pytest.mark.parametrize("name", TTS + ["ChatterboxVC"])
def test_generate_is_the_restatement_of_its_source_and_none_is_the_call_without_it(dev, name, monkeypatch):
    from chatterbox_amd import ops, synth
    m, lang = _model(dev, name)
    src = synth.speech_tokens(20, seed=3)
    call = (lambda **kw: m.generate(s3_tokens=src, seed=77, **kw)) if name == "ChatterboxVC" else (lambda **kw: m.generate(TEXTS[0], *lang, seed=77, **kw))
    real, calls = ops.lib, []
    call(), call(speed=1.0 / P.ratio(CASES[0][0]))  # (what a shape's first call does once -- plans, captures -- stays out of the comparison)

    class Spy:
        def __getattr__(self, entry):
            calls.append(entry)
            return getattr(real, entry)

    monkeypatch.setattr(ops, "lib", Spy())
    base = call()
    plain_calls = list(calls)
    calls.clear()
    none = call(pitch=None)
    calls_none = list(calls)
    calls.clear()
    zero = call(pitch=0)
    calls_zero = list(calls)
    calls.clear()
    up = call(pitch=CASES[0][0])
    calls_on = list(calls)
    calls.clear()
    up_source = call(speed=1.0 / P.ratio(CASES[0][0]))
    calls_source = list(calls)
    monkeypatch.setattr(ops, "lib", real)
    assert torch.equal(base, none) and torch.equal(base, zero), "pitch=None / 0: bitwise the seeded call without the argument"
    assert calls_none == plain_calls and calls_zero == plain_calls and "cbx_wave_pitch_f32" not in plain_calls, "and the same calls into the library, one for one"
    assert calls_on.count("cbx_wave_pitch_f32") == 1 and calls_on.count("cbx_mel_time_scale_f32") == 1
    assert [c for c in calls_on if c != "cbx_wave_pitch_f32"] == calls_source, "with it: the calls of the source (ONE stretch) and ONE more entry"
    for p, s in CASES:
        r = P.ratio(p)
        plain = base if s == 1.0 else call(speed=s)
        source = up_source if (p, s) == CASES[0] else call(speed=s / r)
        got = up if (p, s) == CASES[0] else call(pitch=p, speed=s)
        assert source.shape[1] != plain.shape[1], "the case is what it claims: the source has another length"
        _within(got, source, p, plain, f"{name}.generate(pitch={p}, speed={s})")
    # behind the pitch: loudness, pauses and the delivery format are the existing steps on the pitched call's plain result
    p, s = CASES[1]
    got = call(pitch=p, speed=s)
    with torch.cuda.device(dev):
        row = got[0].to(dev)
        want = row.clone()
        ops.wave_normalize([want], [-23.0])
        loud = call(pitch=p, speed=s, loudness=-23)
        assert torch.equal(loud[0], want.cpu()) and not torch.equal(loud, got), "loudness= measures and gains the pitched rows"
        sq = ops.wave_squeeze([row], [2], 3.0, 240)
        want = ops.cut_pauses(sq["rows"], sq["stats"].cpu())[0].cpu()
        short = call(pitch=p, speed=s, max_pause=0.04, pause_db=3.0)
        print(f"{name}: max_pause behind the pitch: {got.shape[1]} -> {short.shape[1]} samples")
        assert torch.equal(short[0], want), "max_pause= shortens the pitched rows"
        fmt = dict(sample_rate=16000, encoding="s16")
        want = ops.wave_format([row], fmt)[0].cpu()
        enc = call(pitch=p, speed=s, **fmt)
        assert enc.dtype == torch.int16 and torch.equal(enc[0], want), "the format launch converts the pitched rows"
        chain = row.clone()
        ops.wave_normalize([chain], [-23.0])
        sq = ops.wave_squeeze([chain], [2], 3.0, 240)
        n_new = int(sq["stats"].cpu()[0, 0])
        want = ops.wave_format(sq["rows"], fmt)[0].cpu()[: ops.formatted_len(n_new, 16000)]
        allof = call(pitch=p, speed=s, loudness=-23, max_pause=0.04, pause_db=3.0, **fmt)
        assert torch.equal(allof[0], want), "pitch, loudness, pauses, format: in that order"


@pytest.mark.parametrize("name", ["ChatterboxTTS", "ChatterboxTurboTTS"])
def test_generate_batch_takes_a_pitch_per_request_over_two_sub_batches(dev, name):
    """three requests as sub-batches of two and one (ChatterboxTTS: synthesize_pipelined): every row lies within the bound of the restatement on the row of the
    batch at speed / r; the None row, read at a step of 1, keeps that batch's samples"""
    m, lang = _model(dev, name)
    pitch, speed = [4.0, None, -5.0], [1.0, 1.25, 0.9]
    eff = [s / P.ratio(p or 0.0) if p else s for s, p in zip(speed, pitch)]
    m.max_batch = 2
    try:
        plain = m.generate_batch(TEXTS[:3], *lang, seeds=SEEDS[:3], speed=speed)
        source = m.generate_batch(TEXTS[:3], *lang, seeds=SEEDS[:3], speed=eff)
        got = m.generate_batch(TEXTS[:3], *lang, seeds=SEEDS[:3], speed=speed, pitch=pitch)
        same = m.generate_batch(TEXTS[:3], *lang, seeds=SEEDS[:3], speed=speed, pitch=[None, 0, None])
    finally:
        m.max_batch = None
    assert all(torch.equal(a, b) for a, b in zip(plain, same)), "no request with a pitch: the call without the argument"
    for k in range(3):
        _within(got[k], source[k], pitch[k] or 0.0, plain[k], f"{name} row {k}")
    assert torch.equal(got[1], source[1]), "a None row, read at a step of 1, keeps its samples"


@pytest.mark.parametrize("name", TTS)
def test_generate_long_transposes_its_chunks_and_the_stream_concatenates_to_it(dev, name):
    m, lang = _model(dev, name)
    text = "The first sentence is here. A second one follows it! Is the third a question?"
    base, seg0 = m.generate_long(text, *lang, seed=5, max_chars=30, return_segments=True, trim_db=None)
    got, seg = m.generate_long(text, *lang, seed=5, max_chars=30, return_segments=True, trim_db=None, pitch=-3)
    assert len(seg) == len(seg0) == 3 and got.shape == base.shape, "without a trim every chunk keeps its length, so the whole text does"
    assert [(s["start"], s["stop"]) for s in seg] == [(s["start"], s["stop"]) for s in seg0] and not torch.equal(got, base)
    assert all(s["tokens"].tolist() == s0["tokens"].tolist() for s, s0 in zip(seg, seg0))
    got, seg = m.generate_long(text, *lang, seed=5, max_chars=30, return_segments=True, pitch=-3)
    gaps = [b["start"] - a["stop"] for a, b in zip(seg0, seg0[1:])]
    assert seg[0]["start"] == 0 and seg[-1]["stop"] == got.shape[1] and [b["start"] - a["stop"] for a, b in zip(seg, seg[1:])] == gaps, "the segments add up"
    assert all(s["stop"] - s["start"] == s["src_stop"] - s["src_start"] for s in seg)
    pieces = list(m.generate_long_stream(text, *lang, seed=5, max_chars=30, pitch=-3, first_batch=None))
    assert torch.equal(torch.cat(pieces, dim=1), got), "first_batch=None concatenates to generate_long bit for bit"
    none = m.generate_long(text, *lang, seed=5, max_chars=30, trim_db=None, pitch=None)
    assert torch.equal(none, base)


def test_bad_values_raise_before_anything_is_launched(dev, monkeypatch):
    from chatterbox_amd import ops, synth
    m, lang = _model(dev, "ChatterboxTTS")
    vc, _ = _model(dev, "ChatterboxVC")
    real, calls = ops.lib, []

    class Spy:
        def __getattr__(self, entry):
            calls.append(entry)
            return getattr(real, entry)

    monkeypatch.setattr(ops, "lib", Spy())
    m.seen.clear()
    tok = synth.speech_tokens(8, seed=1)
    for call, match in ((lambda: m.generate(TEXTS[0], pitch=12.5), "pitch"), (lambda: m.generate(TEXTS[0], pitch=12, speed=0.9), r"speed.*pitch"),
                        (lambda: m.generate_batch(TEXTS[:2], pitch=[1]), "pitch"), (lambda: m.generate_batch(TEXTS[:2], pitch=[0, -12], speed=[1.0, 1.1]), r"speed.*pitch"),
                        (lambda: m.generate_long("One. Two.", pitch=float("nan")), "pitch"), (lambda: list(m.generate_long_stream("One. Two.", pitch=-7, speed=1.5)), r"speed.*pitch"),
                        (lambda: vc.generate(s3_tokens=tok, pitch=-12.5), "pitch"), (lambda: vc.generate_batch(s3_tokens=[tok, tok], pitch=7, speed=0.7), r"speed.*pitch"),
                        (lambda: m.engine.synthesize([torch.arange(5)], m.conds.t3.as_dict(), m.conds.gen, pitch=12, speed=0.9), r"speed.*pitch"),
                        (lambda: m.engine.vocode([tok], m.conds.gen, pitch=13), "pitch")):
        with pytest.raises(ValueError, match=match):
            call()
    with pytest.raises(TypeError, match="pitch"):
        m.generate_stream(TEXTS[0], pitch=2)
    monkeypatch.setattr(ops, "lib", real)
    assert calls == [], "no entry of the library was called"
    assert m.seen == [[tok.tolist()]], "only the engine call itself was seen, and it raised before its first launch"
