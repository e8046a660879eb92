"""What the public classes hand to their engines, as data: record() runs generate / generate_batch / generate_stream / generate_long of the three TTS classes and
generate / generate_batch / generate_stream of ChatterboxVC over recording engines (the stand-ins of the host tests, read-only imports; nothing is launched) and
returns the ordered list of engine calls in a JSON form.  tests/golden/api_calls.json is that list as the code gave it before the request path was folded into one
copy; tests/test_api_calls_host.py compares the two for equality.  Rewrite the fixture (python tests/api_calls_common.py) only for a change that is MEANT to alter
what reaches the engines.

An entry is dict(scenario, call, kw): every positional and keyword argument of the call by name.  Tensors are written as dict(tensor=nested list, dtype=...); a voice
(a T3 cond dict or an S3Gen reference dict) as dict(voice=k), k = the position of its first occurrence in the scenario -- two dicts are the same voice when they
hold the same tensors (by identity; the one-element emotion tensor by value, since the classes rebuild it).

record_delivery() does the same for the delivery options (format, loudness, pauses, pitch, word_times, guard): scenarios of their own, recorded before those
options were folded into one record, in a file of their own (tests/golden/api_calls_delivery.json, packed as delivery_chain_common.py writes its own; test_delivery_chain_host.py compares), so
the older fixture stays byte for byte what it was.  Its entries are compact: a tensor is dict(n=its element count), and the voices, sampling and round-schedule
arguments (NOT_DELIVERY), which the older fixture pins, are left out.  The recording engines return an alignment for words= and leave a last_guard for guard=,
and the ops the classes call on the host side of a result (_host_ops) are stand-ins: nothing is launched."""
import contextlib
import json
import os
import sys
import warnings

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (HERE, os.path.join(HERE, "simt")):
    if p not in sys.path:
        sys.path.insert(0, p)

from test_wave_join_host import _LongEngine, _LongSerial, _tts  # noqa: E402  (read-only import: the recording engines of the host tests)

FIXTURE = os.path.join(HERE, "golden", "api_calls.json")
FIXTURE_DELIVERY = os.path.join(HERE, "golden", "api_calls_delivery.json")
CPU = torch.device("cpu")
LENS = [9, 2, 5, 7, 30]   # characters; the texts end in punctuation, so the normalisers add nothing
TEXTS = ["x" * (n - 1) + "." for n in LENS]
SEEDS = [101, 2 ** 64 - 1, 0, 104, 2 ** 33]
SPEEDS = [1.25, None, 0.5, 2.0, 1.0]
LOUDS = [-16, None, None, -23, None]
PAUSES = [None, 0.3, None, None, 0.1]
PITCHES = [2, None, 0, None, -3]
NOT_DELIVERY = ("t3_conds", "gen_ref", "max_new_tokens", "max_gen_len", "drop_last_token", "temperature", "cfg_weight", "repetition_penalty", "min_p", "top_p", "top_k", "first_chunk",
                "chunk", "chunk_growth", "lookahead", "fade", "overlap")
LONG_TEXT = "Aaaa bbbb cc. Dd eeee! Ffffff gg hh?\n\nIiii jj. Kk llll mmmm."   # two paragraphs; max_chars=14 gives five chunks


class _Log:
    """The ordered calls of one scenario and the voices seen in it"""

    def __init__(self, scenario, out, compact=False):
        self.scenario, self.out, self.voices, self.compact = scenario, out, [], compact

    def voice(self, d):
        key = tuple(sorted((k, (v.reshape(-1).tolist() if v.numel() <= 4 else id(v)) if torch.is_tensor(v) else repr(v)) for k, v in d.items()))
        for k, (seen, _) in enumerate(self.voices):
            if seen == key:
                return k
        self.voices.append((key, d))   # (the dict is kept: its tensors' ids stay taken for the scenario)
        return len(self.voices) - 1

    def enc(self, v):
        if torch.is_tensor(v):
            return dict(n=v.numel()) if self.compact else dict(tensor=v.tolist(), dtype=str(v.dtype))
        if isinstance(v, dict) and ("speaker_emb" in v or "prompt_token" in v):
            return dict(voice=self.voice(v))
        if isinstance(v, dict):
            return {k: self.enc(x) for k, x in v.items()}
        if isinstance(v, (list, tuple)):
            return [self.enc(x) for x in v]
        if v is None or isinstance(v, (bool, int, float, str)):
            return v
        raise TypeError(f"api_calls: no JSON form for a {type(v).__name__}")

    def add(self, call, **kw):
        if self.compact:   # (voices, sampling and round-schedule arguments are the older fixture's matter)
            kw = {k: v for k, v in kw.items() if k not in NOT_DELIVERY}
            if "jobs" in kw:
                kw["jobs"] = [{k: v for k, v in job.items() if k not in NOT_DELIVERY} for job in kw["jobs"]]
        self.out.append(dict(scenario=self.scenario, call=call, kw=self.enc(kw)))


def _reports(text_tokens):
    """last_guard of a guarded call, as the stand-in of test_guard_host.py leaves it: "tail" for an odd count of text tokens"""
    return [dict(reason="tail" if t.numel() % 2 else "eos", tokens=int(t.numel()), fired_at=None, completed_at=None, position=0, text_tokens=int(t.numel())) for t in text_tokens]


class _RecSerial(_LongSerial):
    """An engine without a throughput schedule (as TurboEngine)"""
    log = last_guard = None

    def synthesize(self, text_tokens, t3_conds, gen_ref, **kw):
        self.log.add("synthesize", text_tokens=text_tokens, t3_conds=t3_conds, gen_ref=gen_ref, **kw)
        res = super().synthesize(text_tokens, t3_conds, gen_ref, **kw)
        self.last_guard = _reports(text_tokens) if kw.get("guard") is not None else None
        if kw.get("words") is None:
            return res
        sp = kw.get("speed")   # (the alignment of test_word_times_host.py's stand-in: every text token owns two frames)
        return (*res, [dict(frames=[(2 * i, 2 * i + 2) for i in range(t.numel())], n_frames=2 * t.numel(), speed=None if sp is None else sp[b], pitch=None)
                       for b, t in enumerate(text_tokens)])

    def synthesize_stream(self, text_tokens, t3_conds, gen_ref, **kw):
        self.log.add("synthesize_stream", text_tokens=text_tokens, t3_conds=t3_conds, gen_ref=gen_ref, **kw)
        yield dict(wavs=[torch.zeros(0)], final=[False])
        yield dict(wavs=[torch.ones(5)], final=[True])


class _RecEngine(_RecSerial, _LongEngine):
    def synthesize_pipelined(self, jobs, **kw):
        self.log.add("synthesize_pipelined", jobs=jobs, **kw)
        for job, res in zip(jobs, _LongEngine.synthesize_pipelined(self, jobs, **kw)):
            self.last_guard = _reports(job["text_tokens"]) if job.get("guard") is not None else None
            yield res


class _RecVoc:
    dev = CPU

    def __init__(self, log):
        self.log = log

    def vocode(self, speech_tokens, gen_ref, **kw):
        self.log.add("vocode", speech_tokens=speech_tokens, gen_ref=gen_ref, **kw)
        return [torch.full((2,), float(t.numel())) for t in speech_tokens], None

    def vocode_stream(self, speech_tokens, gen_ref, **kw):
        self.log.add("vocode_stream", speech_tokens=speech_tokens, gen_ref=gen_ref, **kw)
        yield dict(wavs=[torch.zeros(0)], final=[False])
        yield dict(wavs=[torch.ones(7)], final=[True])


def _model(api, cls_name, log):
    eng = _RecSerial() if cls_name == "ChatterboxTurboTTS" else _RecEngine()
    eng.log = log
    return _tts(getattr(api, cls_name), eng)


def _tts_scenarios(api, synth, cls_name, out):
    lang = ("en",) if cls_name == "ChatterboxMultilingualTTS" else ()
    turbo = cls_name == "ChatterboxTurboTTS"

    def scenario(name):
        log = _Log(f"{cls_name}/{name}", out)
        return _model(api, cls_name, log), log

    m, _ = scenario("defaults")
    m.generate("aaaa.", *lang)
    m.generate_batch(TEXTS, *lang)
    list(m.generate_stream("aaaa.", *lang))
    m.generate_long(LONG_TEXT, *lang, max_chars=14)
    m.generate_long("Aaaa bbbb cc. Dd eeee!", *lang, max_chars=14)   # one device batch: the serial schedule

    m, _ = scenario("seed_speed_window")
    m.generate("aaaa.", *lang, seed=3, speed=1.25)
    m.generate_batch(TEXTS, *lang, seeds=SEEDS, speed=SPEEDS, temperature=[0.1, 0.2, 0.3, 0.4, 0.5], top_p=0.9)
    list(m.generate_stream("aaaa.", *lang, seed=3, speed=1.25, window=20, first_chunk=10, chunk=25, fade=240, overlap=False))
    m.generate_long(LONG_TEXT, *lang, max_chars=14, seed=11, speed=1.25, temperature=0.7, top_p=0.9, trim_db=None, pause=0.1, return_segments=True)

    m, _ = scenario("max_batch_2")
    m.max_batch = 2
    m.generate_batch(TEXTS, *lang, seeds=SEEDS, speed=SPEEDS)
    m.generate_batch(TEXTS, *lang)
    m.generate_long(LONG_TEXT, *lang, max_chars=14, seed=11, speed=0.8)
    m.generate_long(LONG_TEXT, *lang, max_chars=14)

    m, _ = scenario("mixed_voices")
    own, other = m.conds, api.Conditionals(api.T3Cond(**synth.t3_cond(seed=5)), synth.s3gen_ref(seed=6, n_prompt_tokens=8))
    m.generate_batch(TEXTS, *lang, conds=[own, other, own, other, own], exaggeration=[0.5, 0.5, 0.9, 0.5, 0.5])
    m.generate_batch(TEXTS[:2], *lang, conds=other)
    m.generate("aaaa.", *lang, exaggeration=0.7)
    list(m.generate_stream("aaaa.", *lang, exaggeration=0.3))
    m.generate_long(LONG_TEXT, *lang, max_chars=14, exaggeration=0.6)

    # a voice given as a path: the analysis is a stand-in that records what it was asked for and returns a voice of its own
    m, log = scenario("voice_from_a_path")
    made = {}

    def analyse(analyzer, wav, exaggeration, prompt_len, device, **kw):
        log.add("prepare_conditionals", wav=wav, exaggeration=exaggeration, prompt_len=prompt_len, **kw)
        k = len(made)
        made[k] = api.Conditionals(api.T3Cond(**dict(synth.t3_cond(seed=20 + k), emotion_adv=exaggeration * torch.ones(1, 1, 1))), synth.s3gen_ref(seed=30 + k, n_prompt_tokens=8))
        return made[k]
    real, api._prepare_conditionals = api._prepare_conditionals, analyse
    try:
        extra = dict(norm_loudness=False) if turbo else {}
        m.generate("aaaa.", *lang, audio_prompt_path="a.wav", exaggeration=0.7, **extra)
        list(m.generate_stream("aaaa.", *lang, audio_prompt_path="b.wav"))
        m.generate_long(LONG_TEXT, *lang, max_chars=14, audio_prompt_path="c.wav", **extra)
        m.generate_batch(TEXTS, *lang, audio_prompt_paths=["a.wav", "b.wav", "a.wav", "b.wav", "a.wav"], exaggeration=[0.5, 0.5, 0.5, 0.5, 0.9], **extra)
        m.prepare_conditionals("d.wav")
        m.generate("aaaa.", *lang)
    finally:
        api._prepare_conditionals = real


def _tts_delivery_scenarios(api, synth, cls_name, out):
    """the delivery options: format, loudness, pauses, pitch (and, on the Llama classes, word_times and guard)"""
    lang = ("en",) if cls_name == "ChatterboxMultilingualTTS" else ()
    turbo = cls_name == "ChatterboxTurboTTS"

    def scenario(name):
        log = _Log(f"{cls_name}/{name}", out, compact=True)
        return _model(api, cls_name, log), log

    every = dict(sample_rate=16000, encoding="s16", loudness=-16, max_pause=0.3, pause_db=35, pitch=2)
    m, _ = scenario("delivery_generate")
    m.generate("aaaa.", *lang, seed=3, speed=1.25, **every)
    for off in (dict(seed=None), dict(speed=1.0), dict(speed=None), dict(sample_rate=24000, encoding="f32"), dict(sample_rate=None, encoding=None), dict(loudness=None),
                dict(max_pause=None, pause_db=12), dict(pitch=0), dict(pitch=None)):
        m.generate("aaaa.", *lang, **off)

    m, _ = scenario("delivery_batch")
    m.max_batch = 2
    m.generate_batch(TEXTS, *lang, seeds=SEEDS, speed=SPEEDS, loudness=LOUDS, max_pause=PAUSES, pause_db=30, pitch=PITCHES, sample_rate=8000, encoding="alaw")
    m.generate_batch(TEXTS, *lang, loudness=[None] * 5, max_pause=[None] * 5, pitch=[0, None, 0, None, 0], sample_rate=24000)

    m, _ = scenario("delivery_long")
    m.max_batch = 2
    with _host_ops():
        long_kw = dict(max_chars=14, seed=11, speed=1.25, return_segments=True, max_pause=0.3, pitch=2, loudness=-16, sample_rate=16000, encoding="s16")
        m.generate_long(LONG_TEXT, *lang, **long_kw)
        list(m.generate_long_stream(LONG_TEXT, *lang, first_batch=None, **long_kw))
        list(m.generate_long_stream(LONG_TEXT, *lang, **long_kw))
        m.generate_long(LONG_TEXT, *lang, max_chars=14, max_pause=None, pitch=0, loudness=None, sample_rate=24000)
        list(m.generate_long_stream(LONG_TEXT, *lang, max_chars=14, max_pause=None, pitch=0, loudness=None, sample_rate=24000))

    m, _ = scenario("delivery_stream")
    list(m.generate_stream("aaaa.", *lang, sample_rate=8000, encoding="mulaw", speed=0.8))
    list(m.generate_stream("aaaa.", *lang, sample_rate=24000, encoding="f32", speed=1.0))

    # a watermarker works on the 24 kHz fp32 waveform: the engine then receives no format, and the conversion follows the watermark on the host side
    if cls_name == "ChatterboxTTS":   # (one class serves: the rule is _Finish's)
        m, _ = scenario("watermarked")
        m.watermarker = type("Mark", (), {"apply_watermark": staticmethod(lambda x, sample_rate: x)})()
        with _host_ops():
            m.generate("aaaa.", *lang, **every)
            m.generate_batch(TEXTS[:3], *lang, sample_rate=8000, loudness=[-16, None, -23])
            list(m.generate_stream("aaaa.", *lang, sample_rate=8000, encoding="mulaw", speed=0.8))
            m.generate_long(LONG_TEXT, *lang, max_chars=14, sample_rate=16000, loudness=-16)
    if turbo:
        return

    m, _ = scenario("words_guard")
    m.tokenizer = _Pieces()
    m.max_batch = 2
    for words in (True, "tokens"):
        m.generate("aa bb.", *lang, seed=3, speed=1.25, word_times=words)
        m.generate_batch(TEXTS, *lang, seeds=SEEDS, pitch=PITCHES, word_times=words)
        m.generate_long(LONG_TEXT, *lang, max_chars=14, seed=11, return_segments=True, word_times=words)
    m.align_heads = ((0, 1), (1, 0))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")   # (the guard's UserWarning names the requests the stand-in ended by "tail")
        for guard in (True, dict(tail=2.0)):
            m.generate("aa bb.", *lang, seed=3, guard=guard)
            m.generate_batch(TEXTS, *lang, seeds=SEEDS, loudness=LOUDS, guard=guard)
            m.generate_long(LONG_TEXT, *lang, max_chars=14, seed=11, return_segments=True, guard=guard)
        m.generate_long(LONG_TEXT, *lang, max_chars=14, return_segments=True, word_times=True, guard=True, pitch=1)
    m.generate("aa bb.", *lang, word_times=False, guard=None)
    m.generate_batch(TEXTS, *lang, word_times=None, guard=False)


class _Pieces:
    """A tokenizer with pieces(ids), which word_times="words" needs (the stand-in of test_word_times_host.py)"""
    SPACE = "_"

    def text_to_tokens(self, text, language_id=None):
        return torch.tensor([ord(c) for c in text], dtype=torch.int32).unsqueeze(0)

    def pieces(self, ids):
        return ["[START]" if i == 255 else "[STOP]" if i == 0 else "_" if chr(i) == " " else chr(i) for i in ids]


@contextlib.contextmanager
def _host_ops():
    """ops.wave_format, wave_normalize, wave_gain and the two stream converters as stand-ins of the right structure, for what the public classes do to a result on
    the host side of the engine call (the conversion behind a watermark; long-form loudness and format): nothing is launched and nothing of it is recorded"""
    from chatterbox_amd import ops

    class Meter:
        def __init__(self, B, dev):
            pass

        def push(self, rows, targets, ceiling):
            return "stats", [1.0] * len(rows)

    class Conv:
        def __init__(self, B, fmt, dev):
            self.rate = fmt["sample_rate"]

        def push(self, rows, final):
            return [r[: ops.formatted_len(int(r.numel()), self.rate)] for r in rows]

    stand_ins = dict(wave_format=lambda rows, fmt: [r[: ops.formatted_len(int(r.numel()), fmt["sample_rate"])] for r in rows], wave_normalize=lambda rows, target, **kw: "stats",
                     wave_gain=lambda rows, gain: None, WaveLoudnessStream=Meter, WaveFormatStream=Conv)
    real = {k: getattr(ops, k) for k in stand_ins}
    for k, v in stand_ins.items():
        setattr(ops, k, v)
    try:
        yield
    finally:
        for k, v in real.items():
            setattr(ops, k, v)


def _vc_scenarios(api, synth, out):
    def scenario(name):
        log = _Log(f"ChatterboxVC/{name}", out)
        vc = api.ChatterboxVC.__new__(api.ChatterboxVC)
        vc.engine, vc.device, vc.ref_dict, vc.analyzer, vc.watermarker = _RecVoc(log), CPU, synth.s3gen_ref(n_prompt_tokens=8), None, None
        return vc

    toks = [synth.speech_tokens(n, seed=n) for n in (30, 10, 20)]
    refs = [synth.s3gen_ref(seed=s, n_prompt_tokens=8) for s in (1, 2, 3)]
    vc = scenario("defaults")
    vc.generate(s3_tokens=toks[0])
    vc.generate_batch(s3_tokens=toks)
    list(vc.generate_stream(s3_tokens=toks[0]))

    vc = scenario("seed_speed_window")
    vc.generate(s3_tokens=toks[1], seed=8, speed=1.25)
    vc.generate_batch(s3_tokens=toks, seeds=[7, 8, 9], speed=[1.25, None, 0.5])
    list(vc.generate_stream(s3_tokens=toks[0], seed=8, speed=1.25, window=20, first_chunk=10, chunk=25))

    vc = scenario("max_batch_2")
    vc.MAX_BATCH = 2
    vc.generate_batch(s3_tokens=toks, ref_dicts=refs, seeds=[7, 8, 9], speed=[1.25, None, 0.5])
    vc.generate_batch(s3_tokens=toks, ref_dicts=refs[0])
    vc.generate_batch(s3_tokens=toks)


def _vc_delivery_scenarios(api, synth, out):
    def scenario(name):
        log = _Log(f"ChatterboxVC/{name}", out, compact=True)
        vc = api.ChatterboxVC.__new__(api.ChatterboxVC)
        vc.engine, vc.device, vc.ref_dict, vc.analyzer, vc.watermarker = _RecVoc(log), CPU, synth.s3gen_ref(n_prompt_tokens=8), None, None
        return vc

    toks = [synth.speech_tokens(n, seed=n) for n in (30, 10, 20)]
    every = dict(sample_rate=16000, encoding="s16", loudness=-16, max_pause=0.3, pause_db=35, pitch=2)
    vc = scenario("delivery_generate")
    vc.generate(s3_tokens=toks[0], seed=8, speed=1.25, **every)
    for off in (dict(seed=None), dict(speed=1.0), dict(sample_rate=24000, encoding="f32"), dict(loudness=None), dict(max_pause=None, pause_db=12), dict(pitch=0), dict(pitch=None)):
        vc.generate(s3_tokens=toks[0], **off)

    five = toks + [synth.speech_tokens(n, seed=n) for n in (15, 25)]
    vc = scenario("delivery_batch")
    vc.MAX_BATCH = 2
    vc.generate_batch(s3_tokens=five, seeds=SEEDS, speed=SPEEDS, loudness=LOUDS, max_pause=PAUSES, pause_db=30, pitch=PITCHES, sample_rate=8000, encoding="alaw")
    vc.generate_batch(s3_tokens=five, loudness=[None] * 5, max_pause=[None] * 5, pitch=[0, None, 0, None, 0], sample_rate=24000)

    vc = scenario("delivery_stream")
    list(vc.generate_stream(s3_tokens=toks[0], sample_rate=8000, encoding="mulaw", speed=0.8))
    list(vc.generate_stream(s3_tokens=toks[0], sample_rate=24000, encoding="f32", speed=1.0))


def record():
    from chatterbox_amd import api, synth
    out = []
    for cls_name in ("ChatterboxTTS", "ChatterboxMultilingualTTS", "ChatterboxTurboTTS"):
        _tts_scenarios(api, synth, cls_name, out)
    _vc_scenarios(api, synth, out)
    return out


def record_delivery():
    from chatterbox_amd import api, synth
    out = []
    for cls_name in ("ChatterboxTTS", "ChatterboxMultilingualTTS", "ChatterboxTurboTTS"):
        _tts_delivery_scenarios(api, synth, cls_name, out)
    _vc_delivery_scenarios(api, synth, out)
    return out


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(HERE))
    calls = record()
    with open(FIXTURE, "w") as f:
        json.dump(calls, f, separators=(",", ":"))
        f.write("\n")
    print(f"{len(calls)} calls -> {FIXTURE} ({os.path.getsize(FIXTURE)} bytes)")
    from delivery_chain_common import write   # (packed, one entry per line)
    write(record_delivery(), FIXTURE_DELIVERY)
