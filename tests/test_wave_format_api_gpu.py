"""GPU (-m gpu): sample_rate= / encoding= through the engines and the public API on synthetic 2-layer models (built as test_speed_api_gpu.py builds them, with a
bounded token budget).  A seeded call is repeatable bit for bit, so every formatted call is compared EXACTLY with ops.wave_format of the same call without a format:
generate of the four classes (whose fp32 form also meets the kernel tests' bound (a) against scipy.signal.resample_poly), generate_batch through the serial and
the throughput schedule, vocode(format=) with a join, and the streams -- generate_stream without and with a window, ChatterboxVC.generate_stream, a ragged
two-row vocode_stream, and the watermarker path whose converter state the API holds.  Default arguments return what the call without them returns; bad arguments
raise before anything is launched.  The kernel-level tests are in test_turbo_stream_wave_format_kernels_gpu.py."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import test_seeded_api_gpu as A  # noqa: E402  (read-only import: the recording wrapper, the stand-in tokenizer, TEXTS / SEEDS)
import wave_format_common as C  # noqa: E402

pytestmark = pytest.mark.gpu

TTS = ["ChatterboxTTS", "ChatterboxMultilingualTTS", "ChatterboxTurboTTS"]
S16_16K = dict(sample_rate=16000, encoding="s16")
MULAW_8K = dict(sample_rate=8000, encoding="mulaw")


@pytest.fixture(scope="module")
def models(dev):
    """name -> (model, extra positional arguments of its text methods); built on first use, token budget bounded (A._bound_and_record), shared by the tests"""
    from chatterbox_amd import api
    built = {}

    def get(name):
        if name not in built:
            if name == "ChatterboxVC":
                m = api.ChatterboxVC.from_synthetic(dev, tokenizer_layers=1)
                A._bound_and_record(m.engine, None)
            else:
                turbo = name == "ChatterboxTurboTTS"
                cls = getattr(api, name)
                m = cls.from_synthetic(dev, t3_layers=2)
                m.tokenizer = A._Tok(50000 if turbo else cls._TEXT_VOCAB)
                A._bound_and_record(m.engine, "max_gen_len" if turbo else "max_new_tokens")
            m.watermarker = None
            built[name] = (m, ("en",) if name == "ChatterboxMultilingualTTS" else ())
        return built[name]
    return get


def _convert(dev, wav, fmt):
    """ops.wave_format of a (1, n) CPU waveform -> (1, m) on the host"""
    from chatterbox_amd import ops
    with torch.cuda.device(dev):
        return ops.wave_format([wav[0].to(dev)], fmt)[0].cpu().unsqueeze(0)


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b)


@pytest.mark.parametrize("name", TTS + ["ChatterboxVC"])
def test_generate_in_a_format_is_the_conversion_of_generate(dev, models, name):
    from chatterbox_amd import ops, synth
    m, lang = models(name)
    src = synth.speech_tokens(20, seed=3)
    call = (lambda **kw: m.generate(s3_tokens=src, seed=77, **kw)) if name == "ChatterboxVC" else (lambda **kw: m.generate(A.TEXTS[0], *lang, seed=77, **kw))
    base = call()
    assert base.dtype == torch.float32 and base.dim() == 2 and base.shape[1] >= 480 * 8
    for kw in (dict(), dict(sample_rate=None, encoding=None), dict(sample_rate=24000, encoding="f32")):
        assert _same(call(**kw), base), f"default arguments {kw} return the call without them"
    s16 = call(**S16_16K)
    assert s16.dtype == torch.int16 and s16.shape == (1, ops.formatted_len(base.shape[1], 16000)) == (1, -(-base.shape[1] * 2 // 3)) and s16.device.type == "cpu"
    assert _same(s16, _convert(dev, base, S16_16K)) and m.sr == 24000
    f32 = call(sample_rate=16000)
    assert f32.dtype == torch.float32 and _same(f32, _convert(dev, base, dict(sample_rate=16000)))
    worst = C.check_bound(f32[0].numpy(), base[0].numpy(), 16000, name)
    print(f"{name}: generate(sample_rate=16000) against resample_poly in fp64: worst |y - y64| / bound = {worst:.3f}")
    assert torch.equal(s16[0], torch.from_numpy(C.quantise(f32[0].numpy(), "s16")))
    for fmt in (dict(sample_rate=48000, encoding="alaw"), dict(encoding="mulaw")):
        assert _same(call(**fmt), _convert(dev, base, fmt)), fmt


@pytest.mark.parametrize("name,max_batch", [("ChatterboxTTS", 2), ("ChatterboxTTS", None), ("ChatterboxTurboTTS", 2), ("ChatterboxVC", 2)])
def test_generate_batch_in_a_format_is_the_conversion_of_generate_batch(dev, models, name, max_batch):
    """three requests, as one device batch and as sub-batches of two (ChatterboxTTS: the throughput schedule, whose pinned copies then carry the encoded audio)"""
    from chatterbox_amd import synth
    m, lang = models(name)
    if name == "ChatterboxVC":
        toks = [synth.speech_tokens(n, seed=k) for k, n in enumerate((20, 12, 16))]
        m.MAX_BATCH = max_batch or 8
        call = lambda **kw: m.generate_batch(s3_tokens=toks, seeds=A.SEEDS[:3], **kw)
    else:
        m.max_batch = max_batch
        call = lambda **kw: m.generate_batch(A.TEXTS[:3], *([["en", "fr", "de"]] if lang else []), seeds=A.SEEDS[:3], **kw)
    try:
        base, got = call(), call(sample_rate=8000, encoding="alaw")
        same = call(sample_rate=24000)
    finally:
        if name == "ChatterboxVC":
            m.MAX_BATCH = 8
        else:
            m.max_batch = None
    assert len(base) == len(got) == 3 and (name != "ChatterboxVC" or len({w.shape[1] for w in base}) == 3), "the conversions are ragged"
    for k in range(3):
        assert _same(same[k], base[k]) and got[k].dtype == torch.uint8 and _same(got[k], _convert(dev, base[k], dict(sample_rate=8000, encoding="alaw"))), k


def test_vocode_with_a_join_converts_the_joined_piece(dev, models):
    from chatterbox_amd import ops, synth
    m, _ = models("ChatterboxTTS")
    eng, ref = m.engine, m.conds.gen
    st = [synth.speech_tokens(n, seed=k) for k, n in enumerate((12, 20, 16))]
    kw = dict(seeds=[5, 6, 7], n_cfm_timesteps=2, join=dict(gaps=[100, 0, 50], trim_db=40.0, last=False))
    with torch.cuda.device(dev):
        plain, _ = eng.vocode(st, ref, **kw)
        piece, _ = eng.vocode(st, ref, format=MULAW_8K, **kw)
        torch.cuda.synchronize()
        total = int(plain["layout"][3])
        assert total > 0 and plain["rec"].tolist() == piece["rec"].tolist() and torch.equal(piece["out"][:total], plain["out"][:total])
        assert bool((piece["out"][total:] == 0).all()), "the join wrote into a zeroed buffer"
        want = ops.wave_format([plain["out"][:total]], MULAW_8K)[0]
        n = ops.formatted_len(total, 8000)
        assert piece["format"] == MULAW_8K and piece["formatted"].dtype == torch.uint8 and torch.equal(piece["formatted"][:n], want)
        host = ops.piece_on_host(piece["formatted"].cpu(), piece["rec"].cpu(), piece["n"], MULAW_8K)
    assert torch.equal(host["wav"], want.cpu()) and host["total"] == total and host["format"] == MULAW_8K


def _cat(pieces):
    assert pieces and all(p.dim() == 2 and p.shape[0] == 1 and p.numel() and p.device.type == "cpu" for p in pieces)
    return torch.cat(pieces, 1)


@pytest.mark.parametrize("window", [None, 9])
@pytest.mark.parametrize("name", ["ChatterboxTTS", "ChatterboxTurboTTS"])
def test_generate_stream_in_a_format_is_the_conversion_of_the_stream(dev, models, name, window, monkeypatch):
    """40 tokens in rounds of 10: with window=9 the window slides; the formatted stream has the rounds of the plain one, and its concatenation is the conversion of
    the plain stream's"""
    monkeypatch.setattr(A, "N_TOK", 40)
    m, lang = models(name)
    call = lambda **kw: list(m.generate_stream(A.TEXTS[1], *lang, seed=31, first_chunk=10, chunk=10, window=window, overlap=False, **kw))   # (the bounded budget of A._bound_and_record needs the serial schedule)
    plain, got = call(), call(**MULAW_8K)
    assert len(plain) >= 3 and all(p.dtype == torch.float32 for p in plain) and all(p.dtype == torch.uint8 for p in got)
    assert _same(_cat(call(sample_rate=24000, encoding="f32")), _cat(plain))
    assert _same(_cat(got), _convert(dev, _cat(plain), MULAW_8K))
    f32 = _cat(call(sample_rate=48000))
    assert _same(f32, _convert(dev, _cat(plain), dict(sample_rate=48000)))


class _Half:
    """a stand-in watermarker: halves what it is given, and counts"""
    calls = 0

    def apply_watermark(self, wav, sample_rate):
        assert sample_rate == 24000 and wav.dtype.name == "float32"
        self.calls += 1
        return wav * 0.5


@pytest.mark.parametrize("marked", [False, True])
def test_vc_generate_stream_in_a_format(dev, models, marked):
    """130 source tokens, window 20 / chunks of 25 (the window slides).  marked: a watermarker is loaded, so the engine streams 24 kHz fp32 and the API converts the
    watermarked pieces through its own ops.WaveFormatStream -- the concatenation is still the conversion of the whole"""
    from chatterbox_amd import synth
    m, _ = models("ChatterboxVC")
    src = synth.speech_tokens(130, seed=3)
    m.watermarker = _Half() if marked else None
    try:
        call = lambda **kw: list(m.generate_stream(s3_tokens=src, first_chunk=10, chunk=25, window=20, seed=9, **kw))
        plain, got = call(), call(**MULAW_8K)
    finally:
        m.watermarker = None
    assert len(plain) >= 4 and sum(p.shape[1] for p in plain) == 960 * 130
    assert _same(_cat(got), _convert(dev, _cat(plain), MULAW_8K))


@pytest.mark.parametrize("window", [None, 20])
def test_a_ragged_two_row_stream_converts_every_row(dev, models, window):
    """S3GenEngine.vocode_stream over 70 and 30 tokens: the short row goes final rounds before the long one; one push per round serves both"""
    from chatterbox_amd import ops, synth
    m, _ = models("ChatterboxVC")
    toks = [synth.speech_tokens(70, seed=1), synth.speech_tokens(30, seed=2)]
    pushes, push = [], ops.WaveFormatStream.push

    def counted(self, rows, final):
        pushes.append(list(final))
        return push(self, rows, final)

    def run(**kw):
        rounds = list(m.engine.vocode_stream(toks, m.ref_dict, first_chunk=10, chunk=25, window=window, seeds=[4, 5], **kw))
        return rounds, [torch.cat([r["wavs"][b] for r in rounds if r["wavs"][b].numel()]) for b in range(2)]

    plain_rounds, plain = run()
    ops.WaveFormatStream.push = counted
    try:
        rounds, got = run(format=S16_16K)
    finally:
        ops.WaveFormatStream.push = push
    assert len(pushes) == len(rounds) == len(plain_rounds) and [r["final"] for r in rounds] == [r["final"] for r in plain_rounds]
    assert [n.numel() for n in plain] == [960 * 70, 960 * 30]
    for b in range(2):
        assert got[b].dtype == torch.int16 and got[b].numel() == ops.formatted_len(plain[b].numel(), 16000)
        assert torch.equal(got[b], _convert(dev, plain[b][None], S16_16K)[0]), f"row {b}"


def test_bad_formats_raise_before_anything_is_launched(dev, models, monkeypatch):
    """Every call into the library goes through ops.lib: a counting proxy in its place sees none while the bad values are refused, and sees the conversion's entry
    for a good one."""
    from chatterbox_amd import ops, synth
    m, _ = models("ChatterboxTTS")
    vc, _ = models("ChatterboxVC")
    real, calls = ops.lib, []

    class Spy:
        def __getattr__(self, name):
            calls.append(name)
            return getattr(real, name)

    st = [synth.speech_tokens(12, seed=1)]
    monkeypatch.setattr(ops, "lib", Spy())
    bad = ((dict(sample_rate=11025), ValueError), (dict(sample_rate=8000.0), TypeError), (dict(sample_rate=True), TypeError), (dict(encoding="pcm16"), ValueError),
           (dict(encoding=1), TypeError))
    for kw, err in bad:
        for call in (lambda: m.generate("One.", **kw), lambda: m.generate_batch(["One.", "Two."], **kw), lambda: m.generate_stream("One.", **kw),
                     lambda: m.generate_long("One. Two.", **kw), lambda: vc.generate(s3_tokens=st[0], **kw), lambda: vc.generate_batch(s3_tokens=st, **kw),
                     lambda: vc.generate_stream(s3_tokens=st[0], **kw), lambda: m.engine.vocode(st, m.conds.gen, format=kw),
                     lambda: m.engine.synthesize([synth.text_tokens(12)], synth.t3_cond(), m.conds.gen, max_new_tokens=4, format=kw),
                     lambda: next(m.engine.vocode_stream(st, m.conds.gen, format=kw))):
            with pytest.raises(err, match="sample_rate|encoding"):
                call()
    with pytest.raises(TypeError, match="format"):
        m.engine.vocode(st, m.conds.gen, format="s16")
    assert calls == [], f"refused calls reached the library: {calls[:5]}"
    m.engine.vocode(st, m.conds.gen, n_cfm_timesteps=2, format=S16_16K)
    assert calls.count("cbx_wave_format_f32") == 1
