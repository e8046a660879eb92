"""GPU (-m gpu): generate_dialogue on the three TTS classes, on the synthetic models of test_long_form_gpu.py (t3_layers=2, a budget of 30 tokens, a stub
tokenizer).  Everything is compared BITWISE:
  * a one-voice dialogue with one turn per sentence, turn_pause = pause and the paragraph's gap spelled out equals generate_long(text, seed=...) -- as one device
    batch and as batches of two;
  * two voices with turn 1 at gap=-0.2: the waveform equals the NumPy oracle's mix (wave_mix_common.py) of the waveforms engine.synthesize returns for the same
    rows, voices and derived seeds, at the reported src_start / src_stop, and the segments of turns 0 and 1 overlap by 4800 samples;
  * balance=-23 on two voices analysed from prompts that differ by a factor of 4 in amplitude: last_balance holds both readings and the output equals the oracle's
    mix with the gains ops.wave_loudness gives for the packed voice signals;
  * loudness, true_peak, sample_rate and encoding give the existing one-shot chain applied to the fp32 dialogue, and the segments follow formatted_len.
The kernel-level tests are in test_wave_mix_kernels_gpu.py."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import wave_mix_common as C  # noqa: E402
from test_batch_api_gpu import _Tok  # noqa: E402  (read-only import: the stub tokenizer)
from test_long_form_gpu import CLASSES, FIVE, N_TOK, SEED, _model  # noqa: E402  (read-only imports: the synthetic models with a budget of 30 tokens)

pytestmark = pytest.mark.gpu

SENTENCES = ["The first sentence is here.", "A second one follows it!", "Is the third a question?", "A new paragraph begins.", "And it ends here."]
FADE = 240


def _same(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, f"{what}: {got.dtype} {got.shape} against {want.dtype} {want.shape}"
    bad = np.nonzero(got.view(np.int32 if got.dtype == np.float32 else got.dtype) != want.view(np.int32 if want.dtype == np.float32 else want.dtype))[0]
    assert len(bad) == 0, f"{what}: {len(bad)} of {len(want)} samples differ bitwise ({int((got[bad] != want[bad]).sum())} of them in value), first at {bad[:5]}"


def _voice(seed, cls_name):
    """a second synthetic voice, shaped as the class's from_synthetic shapes its own"""
    from chatterbox_amd import api, synth
    if cls_name == "ChatterboxTurboTTS":
        c = synth.t3_cond(seed=seed, prompt_len=375)
        return api.Conditionals(api.T3Cond(speaker_emb=c["speaker_emb"], cond_prompt_speech_tokens=c["cond_prompt_speech_tokens"], emotion_adv=None), synth.s3gen_ref(seed=seed))
    return api.Conditionals(api.T3Cond(**synth.t3_cond(seed=seed)), synth.s3gen_ref(seed=seed))


def _layout(lengths, after):
    """the layout rule, restated: empty rows start at the front and change nothing"""
    starts, front, pending = [], 0, 0
    for n, g in zip(lengths, after):
        if n:
            starts.append(max(0, front + pending))
            front, pending = max(front, starts[-1] + n), g
        else:
            starts.append(front)
    return starts, front


def _engine_rows(m, cls_name, kw, texts, conds, ex, groups, seed):
    """the engine's own waveforms (no join) for the same consecutive groups, voices and derived seeds"""
    from chatterbox_amd import api
    from chatterbox_amd.text import punc_norm, punc_norm_en, punc_norm_turbo
    if cls_name == "ChatterboxTurboTTS":
        tok = lambda c: m.tokenizer(punc_norm_turbo(c)).input_ids[0].view(-1).long().cpu()
        samp = dict(temperature=0.8, top_k=1000, top_p=0.95, repetition_penalty=1.2)
    else:
        norm, lang = (punc_norm, dict(language_id="en")) if kw else (punc_norm_en, {})
        tok = lambda c: torch.cat([torch.tensor([255]), m.tokenizer.text_to_tokens(norm(c), **lang).view(-1).long().cpu(), torch.tensor([0])])
        samp = dict(max_new_tokens=1000, drop_last_token=bool(kw), temperature=0.8, cfg_weight=0.5, repetition_penalty=1.2, min_p=0.05, top_p=1.0)
    one = lambda items: items[0] if all(it is items[0] for it in items) else list(items)
    rows = []
    for idx in groups:
        wavs, _ = m.engine.synthesize([tok(texts[k]) for k in idx], one([api._t3_dict(conds[k].t3, ex) for k in idx]), one([conds[k].gen for k in idx]), **samp,
                                      seeds=[api.chunk_seed(seed, k) for k in idx])
        rows += [w.float().cpu().numpy() for w in wavs]
    return rows


def _oracle_mix(rows, seg, after, gain=None, gain_idx=None):
    kept = [r[s["src_start"]: s["src_stop"]] for r, s in zip(rows, seg)]
    starts, total = _layout([len(x) for x in kept], after)
    flags = [3] * len(kept)
    if seg[0]["src_start"] == 0:
        flags[0] &= ~1
    if seg[-1]["src_stop"] == len(rows[-1]):
        flags[-1] &= ~2
    assert [s["start"] for s in seg] == starts and [s["stop"] for s in seg] == [a + len(x) for a, x in zip(starts, kept)]
    return C.oracle(kept, starts, flags, total, gain, gain_idx, FADE), kept


@pytest.mark.parametrize("max_batch", [None, 2], ids=["one_batch", "batches_of_two"])
@pytest.mark.parametrize("cls_name", list(CLASSES))
def test_a_one_voice_dialogue_is_generate_long_bitwise(dev, cls_name, max_batch):
    m = _model(dev, cls_name)
    kw = CLASSES[cls_name][1]
    turns = [(None, SENTENCES[0]), (None, SENTENCES[1]), dict(text=SENTENCES[2]), dict(text=SENTENCES[3], gap=0.4), (None, SENTENCES[4])]
    m.max_batch = max_batch
    try:
        want, wseg = m.generate_long(FIVE, seed=SEED, max_chars=30, return_segments=True, **kw)
        got, seg = m.generate_dialogue(turns, seed=SEED, max_chars=30, turn_pause=0.15, return_segments=True, **kw)
    finally:
        m.max_batch = None
    assert [s["text"] for s in seg] == SENTENCES == [s["text"] for s in wseg] and [s["turn"] for s in seg] == list(range(5)) and all(s["voice"] is None for s in seg)
    assert [(s["start"], s["stop"], s["src_start"], s["src_stop"], s["truncated"]) for s in seg] == [(s["start"], s["stop"], s["src_start"], s["src_stop"], s["truncated"]) for s in wseg]
    assert got.dtype == torch.float32 and got.device.type == "cpu" and got.shape[1] > 5 * 4800
    print(f"{cls_name} max_batch={max_batch}: {got.shape[1]} samples, kept {[(s['src_start'], s['src_stop']) for s in seg]}")
    _same(got[0].numpy(), want[0].numpy(), "a one-voice dialogue against generate_long")


@pytest.mark.parametrize("cls_name", list(CLASSES))
def test_two_voices_with_an_overlap_equal_the_oracles_mix_of_the_engines_waveforms(dev, cls_name):
    m = _model(dev, cls_name)
    kw = CLASSES[cls_name][1]
    other = _voice(7, cls_name)
    turns = [("host", SENTENCES[0]), dict(voice="guest", text=SENTENCES[1], gap=-0.2), ("host", SENTENCES[2]), ("guest", SENTENCES[4])]
    conds = m.conds
    got, seg = m.generate_dialogue(turns, dict(host=m.conds, guest=other), seed=SEED, max_chars=30, return_segments=True, **kw)
    assert m.conds is conds and [s["voice"] for s in seg] == ["host", "guest", "host", "guest"] and m.last_balance is None
    ex = 0.0 if cls_name == "ChatterboxTurboTTS" else 0.5
    texts = [SENTENCES[0], SENTENCES[1], SENTENCES[2], SENTENCES[4]]
    rows = _engine_rows(m, cls_name, kw, texts, [m.conds, other, m.conds, other], ex, [[0, 1, 2, 3]], SEED)
    want, kept = _oracle_mix(rows, seg, [-4800, 7200, 7200, 0])
    print(f"{cls_name}: {got.shape[1]} samples, kept {[len(x) for x in kept]}, starts {[s['start'] for s in seg]}")
    _same(got[0].numpy(), want, "two voices against the oracle's mix")
    if min(len(kept[0]), len(kept[1])) > 4800:
        assert seg[0]["stop"] - seg[1]["start"] == 4800, "turn 1 comes in 0.2 s before turn 0 has finished"
        lo, hi = seg[1]["start"] + FADE, seg[0]["stop"] - FADE
        both = kept[0][lo - seg[0]["start"]: hi - seg[0]["start"]] + kept[1][lo - seg[1]["start"]: hi - seg[1]["start"]]
        _same(got[0].numpy()[lo:hi], both, "inside the overlap, clear of the fades, a sample is the float32 sum of the two voices")
    else:
        print(f"{cls_name}: the chunks of turns 0 and 1 keep {len(kept[0])} and {len(kept[1])} samples: the 4800-sample overlap is not asserted")


_PROMPT_MODEL = {}


def _prompt_model(dev):
    """ChatterboxTTS with the synthetic prompt networks, so that a voice can be analysed from a waveform; the budget of N_TOK tokens as _model sets it"""
    if not _PROMPT_MODEL:
        from chatterbox_amd import api
        m = api.ChatterboxTTS.from_synthetic(dev, t3_layers=2, with_prompt_nets=True, tokenizer_layers=1)
        m.tokenizer = _Tok(api.ChatterboxTTS._TEXT_VOCAB)
        syn, pip = m.engine.synthesize, m.engine.synthesize_pipelined
        m.engine.synthesize = lambda *a, **kw: syn(*a, **{**kw, "max_new_tokens": N_TOK, "ban_eos": True})
        m.engine.synthesize_pipelined = lambda jobs, **kw: pip(jobs, **{**kw, "max_new_tokens": N_TOK, "ban_eos": True})
        m.watermarker = None
        _PROMPT_MODEL["m"] = m
    return _PROMPT_MODEL["m"]


def test_balance_brings_two_voices_from_prompts_of_different_level_to_one_loudness(dev):
    from chatterbox_amd import ops, synth
    m = _prompt_model(dev)
    loud, quiet = synth.prompt_wav(6.5, 24000, seed=1).numpy().astype(np.float32), synth.prompt_wav(6.5, 24000, seed=2).numpy().astype(np.float32)
    scale = float(np.abs(loud).max()) / float(np.abs(quiet).max()) / 4.0
    quiet = (quiet * np.float32(scale)).astype(np.float32)
    assert abs(float(np.abs(loud).max()) / float(np.abs(quiet).max()) - 4.0) < 1e-3, "the prompts differ by a factor of 4 in amplitude"
    voices = dict(a=(loud, 24000), b=(quiet, 24000))
    turns = [("a", SENTENCES[0]), ("b", SENTENCES[1]), dict(voice="a", text=SENTENCES[2], gap=-0.1)]
    got, seg = m.generate_dialogue(turns, voices, seed=SEED, max_chars=30, balance=-23, return_segments=True)
    bal = m.last_balance
    assert [b["voice"] for b in bal] == ["a", "b"] and all(np.isfinite(b["lufs"]) and b["gain"] > 0 and b["blocks"] > 0 for b in bal), bal
    ca, cb = (m._analyse(voices[k], 0.5) for k in ("a", "b"))
    rows = _engine_rows(m, "ChatterboxTTS", {}, [SENTENCES[0], SENTENCES[1], SENTENCES[2]], [ca, cb, ca], 0.5, [[0, 1, 2]], SEED)
    kept = [r[s["src_start"]: s["src_stop"]] for r, s in zip(rows, seg)]
    with torch.cuda.device(dev):
        packed = torch.from_numpy(np.concatenate([kept[0], kept[2], kept[1]])).to(dev)
        na = len(kept[0]) + len(kept[2])
        stats, gain = ops.wave_loudness([packed[:na], packed[na:]], [-23.0, -23.0], 1.0)
        stats, gain = stats.cpu().numpy(), gain.cpu().numpy()
    assert [b["lufs"] for b in bal] == stats[:, 0].tolist() and [b["gain"] for b in bal] == stats[:, 2].tolist() and [b["peak"] for b in bal] == stats[:, 1].tolist()
    print(f"balance: voices at {stats[:, 0].tolist()} LUFS, gains {gain.tolist()}")
    want, _ = _oracle_mix(rows, seg, [7200, -2400, 0], [float(g) for g in gain], [0, 1, 0])
    _same(got[0].numpy(), want, "balance against the oracle's mix with the meter's gains")
    assert gain[0] != 1.0 and gain[1] != 1.0 and gain[0] != gain[1], "both voices are long enough to be measured, and are gained apart"


def test_the_finish_is_the_one_shot_chain_applied_to_the_fp32_dialogue(dev):
    from chatterbox_amd import ops
    m = _model(dev, "ChatterboxTTS")
    other = _voice(7, "ChatterboxTTS")
    turns = [("host", SENTENCES[0]), dict(voice="guest", text=SENTENCES[1], gap=-0.2), ("host", SENTENCES[3])]
    voices = dict(host=m.conds, guest=other)
    plain, pseg = m.generate_dialogue(turns, voices, seed=SEED, max_chars=30, return_segments=True)
    got, seg = m.generate_dialogue(turns, voices, seed=SEED, max_chars=30, return_segments=True, loudness=-16, true_peak=-1, sample_rate=16000, encoding="s16")
    want = m._finish(plain[0], ops.check_format(16000, "s16"), converted=False, loud=-16.0, peak=-1.0)
    assert got.dtype == torch.int16 and got.device.type == "cpu" and got.shape == (1, ops.formatted_len(plain.shape[1], 16000))
    _same(got[0].numpy(), want[0].numpy(), "loudness, true_peak and the format against the one-shot chain")
    assert [(s["start"], s["stop"]) for s in seg] == [(ops.formatted_len(s["start"], 16000), ops.formatted_len(s["stop"], 16000)) for s in pseg]
    assert [(s["src_start"], s["src_stop"]) for s in seg] == [(s["src_start"], s["src_stop"]) for s in pseg] and seg[-1]["stop"] == got.shape[1]
