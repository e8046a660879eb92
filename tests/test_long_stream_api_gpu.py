"""GPU (-m gpu): generate_long_stream on the three TTS classes, on the synthetic models of test_long_form_gpu.py (t3_layers=2, a 30-token budget, EOS banned, its texts
ONE and FIVE, max_chars=30; read-only import, so the modules share the models).  Everything is BITWISE:
  * first_batch=None, max_batch=2: three pieces whose concatenation is generate_long(seed=) and whose segments are its segments -- also as 16 kHz PCM16 and as
    8 kHz mu-law, where one ops.WaveFormatStream carries the resampler across the pieces;
  * the default ramp (groups [0], [1, 2], [3, 4]): every chunk's tokens are generate_long's and every piece is the restated join (wave_join_common.join) of
    engine.synthesize over its group with the chunk seeds, the way test_long_form_gpu.py checks generate_long;
  * loudness=-23: piece k is raw piece k times the fp32 gain ops.wave_loudness gives for raw pieces 0 .. k concatenated; the last stats' L is that call's over the
    whole raw signal; for ONE the stream is generate_long(loudness=-23); no sample exceeds 1.0;
  * closing the stream after one piece leaves the engines as they were: generate() and a full stream afterwards give their earlier bits;
  * ONE with trim_db=None is generate(seed=).
The kernel-level tests of the running meter are in test_turbo_stream_loudness_push_kernels_gpu.py."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import wave_join_common as W  # noqa: E402
from test_long_form_gpu import CLASSES, FIVE, ONE, SEED, _model  # noqa: E402  (read-only import: the models, texts and seed)

pytestmark = pytest.mark.gpu

FORMATS = {"f32_24k": {}, "s16_16k": dict(sample_rate=16000, encoding="s16"), "mulaw_8k": dict(sample_rate=8000, encoding="mulaw")}
DTYPES = {"f32_24k": torch.float32, "s16_16k": torch.int16, "mulaw_8k": torch.uint8}
_WHOLE = {}


def _bits_equal(a, b):
    a, b = a.contiguous(), b.contiguous()
    return a.shape == b.shape and a.dtype == b.dtype and (torch.equal(a.view(torch.int32), b.view(torch.int32)) if a.dtype == torch.float32 else torch.equal(a, b))


def _segments_equal(a, b):
    return len(a) == len(b) and all(x.keys() == y.keys() and all(torch.equal(x[k].cpu(), y[k].cpu()) if torch.is_tensor(x[k]) else x[k] == y[k] for k in x) for x, y in zip(a, b))


def _long(m, cls_name, fmt="f32_24k", max_batch=2, **kw):
    """generate_long(FIVE, seed=SEED, max_chars=30) with segments, computed once per (class, format) and left unchanged"""
    key = (cls_name, fmt, max_batch, tuple(sorted(kw.items())))
    if key not in _WHOLE:
        m.max_batch = max_batch
        try:
            _WHOLE[key] = m.generate_long(FIVE, seed=SEED, max_chars=30, return_segments=True, **FORMATS[fmt], **CLASSES[cls_name][1], **kw)
        finally:
            m.max_batch = None
    return _WHOLE[key]


def _stream(m, cls_name, text=FIVE, max_batch=2, **kw):
    m.max_batch = max_batch
    try:
        return list(m.generate_long_stream(text, seed=SEED, max_chars=30, **CLASSES[cls_name][1], **kw))
    finally:
        m.max_batch = None


@pytest.mark.parametrize("fmt", list(FORMATS))
@pytest.mark.parametrize("cls_name", list(CLASSES))
def test_generate_longs_own_plan_streams_its_bits_in_three_pieces(dev, cls_name, fmt):
    m = _model(dev, cls_name)
    want, seg = _long(m, cls_name, fmt)
    got = _stream(m, cls_name, first_batch=None, return_segments=True, **FORMATS[fmt])
    assert len(got) == 3 and all(w.dim() == 2 and w.shape[0] == 1 and w.dtype == DTYPES[fmt] and w.device.type == "cpu" for w, _ in got)
    cat = torch.cat([w for w, _ in got], dim=1)
    assert _bits_equal(cat, want), f"{cls_name} {fmt}: {int((cat != want).sum()) if cat.shape == want.shape else (cat.shape, want.shape)} samples differ"
    assert _segments_equal([s for _, ss in got for s in ss], seg) and [len(ss) for _, ss in got] == [2, 2, 1]
    assert seg[-1]["stop"] == cat.shape[1]


@pytest.mark.parametrize("cls_name", list(CLASSES))
def test_the_default_ramp_equals_the_restated_join_of_the_engines_waveforms(dev, cls_name):
    from chatterbox_amd import api
    from chatterbox_amd.text import punc_norm, punc_norm_en, punc_norm_turbo, split_text
    m = _model(dev, cls_name)
    kw = CLASSES[cls_name][1]
    _, ref_seg = _long(m, cls_name)
    got = _stream(m, cls_name, max_batch=None, return_segments=True)
    groups = [[0], [1, 2], [3, 4]]
    assert [[s["text"] for s in ss] for _, ss in got] == [[ref_seg[k]["text"] for k in idx] for idx in groups]
    seg = [s for _, ss in got for s in ss]
    chunks = split_text(FIVE, 30)
    gaps = [3600, 3600, 9600, 3600, 3600]
    if cls_name == "ChatterboxTurboTTS":
        tok = lambda c: m.tokenizer(punc_norm_turbo(c)).input_ids[0].view(-1).long().cpu()
        call = lambda tts, seeds: m.engine.synthesize(tts, m.conds.t3.as_dict(), m.conds.gen, temperature=0.8, top_k=1000, top_p=0.95, repetition_penalty=1.2, seeds=seeds)
    else:
        norm, lang = (punc_norm, dict(language_id="en")) if kw else (punc_norm_en, {})
        tok = lambda c: torch.cat([torch.tensor([255]), m.tokenizer.text_to_tokens(norm(c), **lang).view(-1).long().cpu(), torch.tensor([0])])
        call = lambda tts, seeds: m.engine.synthesize(tts, m.conds.t3.as_dict(), m.conds.gen, max_new_tokens=1000, drop_last_token=bool(kw), temperature=0.8,
                                                      cfg_weight=0.5, repetition_penalty=1.2, min_p=0.05, top_p=1.0, seeds=seeds)
    k0 = 0
    for g, idx in enumerate(groups):
        wavs, st = call([tok(chunks[k][0]) for k in idx], [api.chunk_seed(SEED, k) for k in idx])
        rows = [w.float().cpu().numpy() for w in wavs]
        for r, k in enumerate(idx):
            assert torch.equal(seg[k]["tokens"].cpu(), st[r].cpu()), f"chunk {k}: tokens differ from the engine's"
            assert torch.equal(seg[k]["tokens"].cpu(), ref_seg[k]["tokens"].cpu()), f"chunk {k}: tokens differ from generate_long's"
        table = [(seg[k]["src_start"], seg[k]["src_stop"]) for k in idx]
        want, offs, total = W.join(rows, table, [gaps[k] for k in idx], 240, g == 0, g == len(groups) - 1)
        for r, k in enumerate(idx):
            assert seg[k]["start"] == k0 + offs[r] and seg[k]["stop"] - seg[k]["start"] == table[r][1] - table[r][0], "start / stop count samples of the whole stream"
        piece = got[g][0][0].numpy()
        assert piece.shape == want.shape and np.array_equal(piece.view(np.int32), want.view(np.int32)), f"piece {g}: differs bitwise from the restated join"
        k0 += total
    assert seg[-1]["stop"] == k0 == sum(w.shape[1] for w, _ in got)


@pytest.mark.parametrize("cls_name", list(CLASSES))
def test_piece_k_carries_the_gain_of_the_signal_so_far(dev, cls_name):
    from chatterbox_amd import ops
    m = _model(dev, cls_name)
    mark, m.watermarker = m.watermarker, None
    try:
        raw = _stream(m, cls_name, first_batch=None)
        got = _stream(m, cls_name, first_batch=None, loudness=-23)
        last = m.engine.last_loudness.cpu().clone()
        assert len(raw) == len(got) == 3
        with torch.cuda.device(dev):
            for k in range(3):
                so_far = torch.cat([w[0] for w in raw[: k + 1]]).to(dev)
                stats, gain = ops.wave_loudness([so_far], [-23.0], 1.0)
                want = raw[k][0] * gain.cpu()
                print(f"{cls_name} piece {k}: {raw[k].shape[1]} samples, L so far {stats[0, 0].item():.3f} LUFS, gain {gain.item():.6f}")
                assert _bits_equal(got[k][0], want), f"piece {k}: {int((got[k][0] != want).sum())} samples are not raw * the gain of pieces 0 .. {k}"
        assert last.shape == (1, 4) and torch.equal(last.view(torch.int64), stats.cpu().view(torch.int64)), "last_loudness: the one-shot meter's numbers over the whole raw signal"
        assert float(last[0, 0]) > -70.0 and float(last[0, 2]) != 1.0, "the synthetic voice is neither silent nor at the target: the gain does something"
        assert max(float(w.abs().max()) for w in got) <= 1.0
        one = _stream(m, cls_name, text=ONE, first_batch=None, loudness=-23)
        want = m.generate_long(ONE, seed=SEED, max_chars=30, loudness=-23, **CLASSES[cls_name][1])
        assert len(one) == 1 and _bits_equal(one[0], want), "one piece: the running meter IS the whole-signal meter"
    finally:
        m.watermarker = mark


@pytest.mark.parametrize("cls_name", list(CLASSES))
def test_closing_early_leaves_the_engines_as_they_were(dev, cls_name):
    m = _model(dev, cls_name)
    kw = CLASSES[cls_name][1]
    full = _stream(m, cls_name, first_batch=None)
    w0 = m.generate(ONE, seed=SEED, **kw)
    m.max_batch = 2
    try:
        it = m.generate_long_stream(FIVE, seed=SEED, max_chars=30, first_batch=None, **kw)
        first = next(it)
        it.close()
    finally:
        m.max_batch = None
    assert _bits_equal(first, full[0])
    assert _bits_equal(m.generate(ONE, seed=SEED, **kw), w0)
    again = _stream(m, cls_name, first_batch=None)
    assert len(again) == len(full) and all(_bits_equal(a, b) for a, b in zip(again, full))
    want, _ = _long(m, cls_name)
    assert _bits_equal(torch.cat(again, dim=1), want)


@pytest.mark.parametrize("cls_name", list(CLASSES))
def test_one_chunk_without_trimming_is_generate_bitwise(dev, cls_name):
    m = _model(dev, cls_name)
    kw = CLASSES[cls_name][1]
    want = m.generate(ONE, seed=SEED, **kw)
    got = list(m.generate_long_stream(ONE, seed=SEED, trim_db=None, return_segments=True, **kw))
    assert len(got) == 1 and _bits_equal(got[0][0], want)
    (seg,) = got[0][1]
    assert (seg["start"], seg["stop"], seg["src_start"], seg["src_stop"]) == (0, want.shape[1], 0, want.shape[1])
