"""What the public classes hand to their engines, as data: record() runs generate / generate_batch / generate_stream / generate_long of the three TTS classes and
generate / generate_batch / generate_stream of ChatterboxVC over recording engines (the stand-ins of the host tests, read-only imports; nothing is launched) and
returns the ordered list of engine calls in a JSON form.  tests/golden/api_calls.json is that list as the code gave it before the request path was folded into one
copy; tests/test_api_calls_host.py compares the two for equality.  Rewrite the fixture (python tests/api_calls_common.py) only for a change that is MEANT to alter
what reaches the engines.

An entry is dict(scenario, call, kw): every positional and keyword argument of the call by name.  Tensors are written as dict(tensor=nested list, dtype=...); a voice
(a T3 cond dict or an S3Gen reference dict) as dict(voice=k), k = the position of its first occurrence in the scenario -- two dicts are the same voice when they
hold the same tensors (by identity; the one-element emotion tensor by value, since the classes rebuild it)."""
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (HERE, os.path.join(HERE, "simt")):
    if p not in sys.path:
        sys.path.insert(0, p)

from test_wave_join_host import _LongEngine, _LongSerial, _tts  # noqa: E402  (read-only import: the recording engines of the host tests)

FIXTURE = os.path.join(HERE, "golden", "api_calls.json")
CPU = torch.device("cpu")
LENS = [9, 2, 5, 7, 30]   # characters; the texts end in punctuation, so the normalisers add nothing
TEXTS = ["x" * (n - 1) + "." for n in LENS]
SEEDS = [101, 2 ** 64 - 1, 0, 104, 2 ** 33]
SPEEDS = [1.25, None, 0.5, 2.0, 1.0]
LONG_TEXT = "Aaaa bbbb cc. Dd eeee! Ffffff gg hh?\n\nIiii jj. Kk llll mmmm."   # two paragraphs; max_chars=14 gives five chunks


class _Log:
    """The ordered calls of one scenario and the voices seen in it"""

    def __init__(self, scenario, out):
        self.scenario, self.out, self.voices = scenario, out, []

    def voice(self, d):
        key = tuple(sorted((k, (v.reshape(-1).tolist() if v.numel() <= 4 else id(v)) if torch.is_tensor(v) else repr(v)) for k, v in d.items()))
        for k, (seen, _) in enumerate(self.voices):
            if seen == key:
                return k
        self.voices.append((key, d))   # (the dict is kept: its tensors' ids stay taken for the scenario)
        return len(self.voices) - 1

    def enc(self, v):
        if torch.is_tensor(v):
            return dict(tensor=v.tolist(), dtype=str(v.dtype))
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
        self.out.append(dict(scenario=self.scenario, call=call, kw=self.enc(kw)))


class _RecSerial(_LongSerial):
    """An engine without a throughput schedule (as TurboEngine)"""
    log = None

    def synthesize(self, text_tokens, t3_conds, gen_ref, **kw):
        self.log.add("synthesize", text_tokens=text_tokens, t3_conds=t3_conds, gen_ref=gen_ref, **kw)
        return super().synthesize(text_tokens, t3_conds, gen_ref, **kw)

    def synthesize_stream(self, text_tokens, t3_conds, gen_ref, **kw):
        self.log.add("synthesize_stream", text_tokens=text_tokens, t3_conds=t3_conds, gen_ref=gen_ref, **kw)
        yield dict(wavs=[torch.zeros(0)])
        yield dict(wavs=[torch.ones(5)])


class _RecEngine(_RecSerial, _LongEngine):
    def synthesize_pipelined(self, jobs, **kw):
        self.log.add("synthesize_pipelined", jobs=jobs, **kw)
        yield from _LongEngine.synthesize_pipelined(self, jobs, **kw)


class _RecVoc:
    dev = CPU

    def __init__(self, log):
        self.log = log

    def vocode(self, speech_tokens, gen_ref, **kw):
        self.log.add("vocode", speech_tokens=speech_tokens, gen_ref=gen_ref, **kw)
        return [torch.full((2,), float(t.numel())) for t in speech_tokens], None

    def vocode_stream(self, speech_tokens, gen_ref, **kw):
        self.log.add("vocode_stream", speech_tokens=speech_tokens, gen_ref=gen_ref, **kw)
        yield dict(wavs=[torch.zeros(0)])
        yield dict(wavs=[torch.ones(7)])


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


def record():
    from chatterbox_amd import api, synth
    out = []
    for cls_name in ("ChatterboxTTS", "ChatterboxMultilingualTTS", "ChatterboxTurboTTS"):
        _tts_scenarios(api, synth, cls_name, out)
    _vc_scenarios(api, synth, out)
    return out


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(HERE))
    calls = record()
    with open(FIXTURE, "w") as f:
        json.dump(calls, f, separators=(",", ":"))
        f.write("\n")
    print(f"{len(calls)} calls -> {FIXTURE} ({os.path.getsize(FIXTURE)} bytes)")
