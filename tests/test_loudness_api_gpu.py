"""GPU (-m gpu): loudness= through the engines and the public API on synthetic 2-layer models with a token budget of 20 (0.8 s: five whole 400 ms blocks).  The
oracle of loudness_common.py (SciPy, fp64) reads every returned waveform: a call with a target reads the target within 0.01 LU -- the applied gain is one fp32
multiply per sample of a gain known to 1e-6 LU, far inside it -- or, where the ceiling held the gain back, its peak is 1.0 and it reads below the target.
generate of the four classes, generate_batch with a list (a None row equals the plain seeded call within the batch-against-single tolerance), s16 without a
saturated sample, generate_long measured over the whole piece, Turbo's norm_loudness="device", and loudness=None bitwise the call without the keyword.
The kernel-level tests are in test_turbo_stream_loudness_kernels_gpu.py."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import loudness_common as C  # noqa: E402
from test_baseline_shapes_gpu import TOL_WAV_E2E_8S  # noqa: E402  (read-only import: the stated batch-against-single tolerance)
from test_seeded_api_gpu import SEEDS, TEXTS, _rmse, _Tok  # noqa: E402  (read-only import: the stand-in tokenizer, the requests)

pytestmark = pytest.mark.gpu

N_TOK = 20
TOL_API = 0.01
TTS = ["ChatterboxTTS", "ChatterboxMultilingualTTS", "ChatterboxTurboTTS"]
_MODELS = {}


def _model(dev, name):
    """One synthetic model per class for the module: the token budget is N_TOK, EOS is banned (synthetic weights rarely sample it); the speech tokens every vocode
    call gets are recorded in m.seen"""
    if name not in _MODELS:
        from chatterbox_amd import api
        if name == "ChatterboxVC":
            m = api.ChatterboxVC.from_synthetic(dev, tokenizer_layers=1)
        else:
            turbo = name == "ChatterboxTurboTTS"
            cls = getattr(api, name)
            m = cls.from_synthetic(dev, t3_layers=2)
            m.tokenizer = _Tok(50000 if turbo else cls._TEXT_VOCAB)
            key = "max_gen_len" if turbo else "max_new_tokens"
            syn = m.engine.synthesize
            m.engine.synthesize = lambda *a, **kw: syn(*a, **{**kw, key: N_TOK, "ban_eos": True})
            if hasattr(m.engine, "synthesize_pipelined"):
                pip = m.engine.synthesize_pipelined
                m.engine.synthesize_pipelined = lambda jobs, **kw: pip(jobs, **{**kw, key: N_TOK, "ban_eos": True})
        m.watermarker, m.seen = None, []
        voc = m.engine.vocode

        def vocode(speech_tokens, gen_ref, **kw):
            m.seen.append([t.tolist() for t in speech_tokens])
            return voc(speech_tokens, gen_ref, **kw)
        m.engine.vocode = vocode
        _MODELS[name] = (m, ("en",) if name == "ChatterboxMultilingualTTS" else ())
    return _MODELS[name]


def _reads(wav, target, what):
    """the oracle on a returned (1, n) fp32 waveform: the target within TOL_API, or the ceiling held the gain back: peak 1.0 (to fp32 rounding) and below the target"""
    x = wav[0].numpy()
    ref = C.oracle(x)
    print(f"{what}: {len(x)} samples read {ref['L']:.4f} LUFS (target {target}), peak {ref['peak']:.6f}, {ref['blocks']} blocks")
    assert np.isfinite(ref["L"]) and ref["blocks"] >= 1, "the request is long enough to be measured"
    assert ref["peak"] <= 1.0 + 2.0 ** -23
    if abs(ref["L"] - target) > TOL_API:
        assert abs(ref["peak"] - 1.0) <= 2.0 ** -23 and ref["L"] < target, f"{what}: reads {ref['L']}, target {target}, peak {ref['peak']}"
    return ref


@pytest.mark.parametrize("name", TTS + ["ChatterboxVC"])
def test_generate_reads_its_target_and_none_is_the_call_without_the_keyword(dev, name):
    from chatterbox_amd import synth
    m, lang = _model(dev, name)
    src = synth.speech_tokens(N_TOK, seed=3)
    call = (lambda **kw: m.generate(s3_tokens=src, seed=77, **kw)) if name == "ChatterboxVC" else (lambda **kw: m.generate(TEXTS[0], *lang, seed=77, **kw))
    m.seen.clear()
    base, none = call(), call(loudness=None)
    assert base.dtype == torch.float32 and base.shape == none.shape and torch.equal(base, none), "loudness=None: bitwise the seeded call without the keyword"
    before = C.oracle(base[0].numpy())
    got = call(loudness=-20)
    assert m.seen[0] == m.seen[1] == m.seen[2], "the same tokens"
    _reads(got, -20.0, f"{name}.generate(loudness=-20), {before['L']:.2f} LUFS without")
    stats = m.engine.last_loudness.cpu().numpy()
    assert stats.shape == (1, 4) and abs(stats[0, 0] - before["L"]) <= C.TOL_L and stats[0, 1] == before["peak"], "engine.last_loudness: what the meter read"
    assert torch.equal(got[0], base[0] * float(np.float32(stats[0, 2]))), "one fp32 multiply per sample"
    s16 = call(loudness=-20, encoding="s16")
    want = np.clip(np.rint(got[0].numpy().astype(np.float64) * 32768.0), -32768, 32767).astype(np.int16)
    assert s16.dtype == torch.int16 and np.array_equal(s16[0].numpy(), want), "the store sees the normalised signal"
    assert float(got.abs().max()) * 32768.0 <= 32768.0, "and clamps nothing by more than the one step between 1.0 and 32767 / 32768"
    _reads(call(loudness=-5), -5.0, f"{name}.generate(loudness=-5)")


@pytest.mark.parametrize("name,max_batch", [("ChatterboxTTS", None), ("ChatterboxTTS", 2), ("ChatterboxTurboTTS", 2)])
def test_generate_batch_takes_a_target_per_request(dev, name, max_batch):
    """three requests as one device batch and as sub-batches of two (ChatterboxTTS: the throughput schedule): rows 0 and 2 read their targets, row 1 (None) is the
    seeded call without the keyword"""
    m, lang = _model(dev, name)
    m.max_batch = max_batch
    try:
        base = m.generate_batch(TEXTS[:3], *lang, seeds=SEEDS[:3])
        got = m.generate_batch(TEXTS[:3], *lang, seeds=SEEDS[:3], loudness=[-16, None, -23])
    finally:
        m.max_batch = None
    single = m.generate(TEXTS[1], *lang, seed=SEEDS[1])
    _reads(got[0], -16.0, f"{name} row 0"), _reads(got[2], -23.0, f"{name} row 2")
    assert torch.equal(got[1], base[1]), "a None row keeps its samples"
    err = _rmse(got[1], single)
    print(f"{name} max_batch={max_batch}: row 1 against generate(seed=): RMSE {err:.3e} (tolerance {TOL_WAV_E2E_8S:.1e})")
    assert err <= TOL_WAV_E2E_8S
    for k in (0, 2):
        r = got[k][0].double() / base[k][0].double()
        r = r[base[k][0].abs() > 1e-3]
        assert float(r.max() - r.min()) <= 1e-6 * float(r.mean()), "one gain for the whole request"


@pytest.mark.parametrize("name", TTS)
def test_generate_long_reads_its_target_over_the_whole_piece(dev, name):
    m, lang = _model(dev, name)
    text = "The first sentence is here. A second one follows it! Is the third a question?"
    base, seg = m.generate_long(text, *lang, seed=5, max_chars=30, return_segments=True)
    got, seg2 = m.generate_long(text, *lang, seed=5, max_chars=30, return_segments=True, loudness=-24)
    assert len(seg) == 3 and [(s["start"], s["stop"]) for s in seg] == [(s["start"], s["stop"]) for s in seg2] and got.shape == base.shape
    _reads(got, -24.0, f"{name}.generate_long(loudness=-24)")
    g = np.float32(m.engine.last_loudness.cpu().numpy()[0, 2])
    assert torch.equal(got, base * float(g)), "ONE gain for the assembled waveform: the chunks keep their relative level"
    s16 = m.generate_long(text, *lang, seed=5, max_chars=30, loudness=-24, sample_rate=16000, encoding="s16")
    assert s16.dtype == torch.int16 and s16.shape[1] == -(-base.shape[1] * 2 // 3)


def test_turbo_norm_loudness_device_levels_the_analysed_prompt(dev, capsys):
    """prepare_conditionals(norm_loudness="device") hands the analysis a prompt at -27 LUFS; True (no pyloudnorm here: the reference's warning) and False hand it the
    prompt as it is"""
    from chatterbox_amd import synth
    m, _ = _model(dev, "ChatterboxTurboTTS")
    wav = np.asarray(synth.prompt_wav(6.0), np.float32)
    seen = []

    class _Stop(Exception):
        pass

    def embed_ref(w, sr):
        seen.append(np.array(w, copy=True))
        raise _Stop
    avail = type("Avail", (), {"available": True})
    m.analyzer = type("Analyzer", (), dict(tokenizer=avail, speaker_encoder=avail, ve=object(), DEC_COND_LEN=m.DEC_COND_LEN, embed_ref=staticmethod(embed_ref)))()
    conds = m.conds
    try:
        for value in ("device", False):
            with pytest.raises(_Stop):
                m.prepare_conditionals((wav, 24000), norm_loudness=value)
    finally:
        m.analyzer = None
    assert m.conds is conds
    before, after = C.oracle(wav), C.oracle(seen[0])
    print(f"the prompt reads {before['L']:.3f} LUFS; the analysis sees {after['L']:.4f} with norm_loudness='device'")
    assert abs(before["L"] + 27.0) > 1.0, "the case is what it claims: the prompt is not at the target already"
    assert abs(after["L"] + 27.0) <= TOL_API and np.array_equal(seen[1], wav)


def test_bad_targets_raise_before_anything_is_launched(dev):
    from chatterbox_amd import synth
    m, lang = _model(dev, "ChatterboxTTS")
    m.seen.clear()
    for call in (lambda: m.generate(TEXTS[0], loudness=-4), lambda: m.generate_batch(TEXTS[:2], loudness=[-20]), lambda: m.generate_long("One. Two.", loudness=float("nan"))):
        with pytest.raises(ValueError, match="loudness"):
            call()
    with pytest.raises(TypeError, match="loudness"):
        m.generate_stream(TEXTS[0], loudness=-20)
    with pytest.raises(ValueError, match="loudness together with join"):
        m.engine.vocode([synth.speech_tokens(8, seed=1)], m.conds.gen, join=dict(gaps=[0]), loudness=-20)
    assert m.seen == [[synth.speech_tokens(8, seed=1).tolist()]], "only the engine call itself was seen, and it raised before its first launch"
