"""GPU (-m gpu): generate_long on the three TTS classes, on synthetic weights (t3_layers=2), the engines' token budget cut to 30 and a stub tokenizer.
  * a one-chunk text with trim_db=None equals generate() bitwise;
  * a five-chunk text -- as one device batch (synthesize) and as batches of two (synthesize_pipelined where the engine has it) -- equals, bitwise, the NumPy
    restatement's join (wave_join_common.py) of the waveforms engine.synthesize returns for the same consecutive groups with the same derived seeds, at the reported
    src_start / src_stop; the segments are contiguous up to the gaps and carry the engine's tokens;
  * with the budget spent and EOS banned every chunk reports truncated=True and ONE warning is logged.
The kernel-level tests of the two launches are in test_turbo_stream_wave_join_kernels_gpu.py."""
import logging
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import wave_join_common as W  # noqa: E402
from test_batch_api_gpu import _Tok  # noqa: E402  (read-only import: the stub tokenizer)

pytestmark = pytest.mark.gpu

N_TOK = 30
SEED = 2 ** 40 + 12345
ONE = "Hello there, this is one chunk."
FIVE = "The first sentence is here. A second one follows it! Is the third a question?\n\nA new paragraph begins. And it ends here."
CLASSES = {"ChatterboxTTS": ("max_new_tokens", {}), "ChatterboxMultilingualTTS": ("max_new_tokens", dict(language_id="en")), "ChatterboxTurboTTS": ("max_gen_len", {})}
_MODELS = {}


def _model(dev, cls_name):
    """One synthetic model per class for the module; its engine's token budget is N_TOK and EOS is banned (synthetic weights rarely sample it)."""
    if cls_name not in _MODELS:
        from chatterbox_amd import api
        cls = getattr(api, cls_name)
        m = cls.from_synthetic(dev, t3_layers=2)
        m.tokenizer = _Tok(50000 if cls_name == "ChatterboxTurboTTS" else cls._TEXT_VOCAB)
        key = CLASSES[cls_name][0]
        syn = m.engine.synthesize
        m.engine.synthesize = lambda *a, **kw: syn(*a, **{**kw, key: N_TOK, "ban_eos": True})
        if hasattr(m.engine, "synthesize_pipelined"):
            pip = m.engine.synthesize_pipelined
            m.engine.synthesize_pipelined = lambda jobs, **kw: pip(jobs, **{**kw, key: N_TOK, "ban_eos": True})
        _MODELS[cls_name] = m
    return _MODELS[cls_name]


@pytest.mark.parametrize("cls_name", list(CLASSES))
def test_one_chunk_without_trimming_equals_generate_bitwise(dev, cls_name):
    m = _model(dev, cls_name)
    kw = CLASSES[cls_name][1]
    want = m.generate(ONE, seed=SEED, **kw)
    got, seg = m.generate_long(ONE, seed=SEED, trim_db=None, return_segments=True, **kw)
    assert len(seg) == 1 and (seg[0]["start"], seg[0]["stop"], seg[0]["src_start"]) == (0, want.shape[1], 0) and seg[0]["src_stop"] == want.shape[1]
    assert got.shape == want.shape and got.dtype == torch.float32 and got.device.type == "cpu"
    assert torch.equal(got, want), f"{int((got != want).sum())} of {want.numel()} samples differ"


@pytest.mark.parametrize("max_batch", [None, 2], ids=["one_batch_serial", "batches_of_two"])
@pytest.mark.parametrize("cls_name", list(CLASSES))
def test_five_chunks_equal_the_restated_join_of_the_engines_waveforms(dev, cls_name, max_batch):
    from chatterbox_amd import api
    from chatterbox_amd.text import punc_norm, punc_norm_en, punc_norm_turbo, split_text
    m = _model(dev, cls_name)
    kw = CLASSES[cls_name][1]
    m.max_batch = max_batch
    try:
        got, seg = m.generate_long(FIVE, seed=SEED, max_chars=30, return_segments=True, **kw)
    finally:
        m.max_batch = None
    chunks = split_text(FIVE, 30)
    assert [c for c, _ in chunks] == ["The first sentence is here.", "A second one follows it!", "Is the third a question?", "A new paragraph begins.", "And it ends here."]
    assert [p for _, p in chunks] == [False, False, True, False, False] and [s["text"] for s in seg] == [c for c, _ in chunks]
    gaps = [3600, 3600, 9600, 3600, 3600]
    groups = [[0, 1, 2, 3, 4]] if max_batch is None else [[0, 1], [2, 3], [4]]
    # the engine's own waveforms for the same consecutive groups with the same derived seeds (no join)
    if cls_name == "ChatterboxTurboTTS":
        tok = lambda c: m.tokenizer(punc_norm_turbo(c)).input_ids[0].view(-1).long().cpu()
        call = lambda tts, seeds: m.engine.synthesize(tts, m.conds.t3.as_dict(), m.conds.gen, temperature=0.8, top_k=1000, top_p=0.95, repetition_penalty=1.2, seeds=seeds)
    else:
        norm, lang = (punc_norm, dict(language_id="en")) if kw else (punc_norm_en, {})
        tok = lambda c: torch.cat([torch.tensor([255]), m.tokenizer.text_to_tokens(norm(c), **lang).view(-1).long().cpu(), torch.tensor([0])])
        call = lambda tts, seeds: m.engine.synthesize(tts, m.conds.t3.as_dict(), m.conds.gen, max_new_tokens=1000, drop_last_token=bool(kw), temperature=0.8,
                                                      cfg_weight=0.5, repetition_penalty=1.2, min_p=0.05, top_p=1.0, seeds=seeds)
    pieces, k0 = [], 0
    for g, idx in enumerate(groups):
        wavs, st = call([tok(chunks[k][0]) for k in idx], [api.chunk_seed(SEED, k) for k in idx])
        rows = [w.float().cpu().numpy() for w in wavs]
        for r, k in enumerate(idx):
            assert torch.equal(seg[k]["tokens"].cpu(), st[r].cpu()), f"chunk {k}: tokens differ from the engine's"
            assert 0 <= seg[k]["src_start"] <= seg[k]["src_stop"] <= len(rows[r]) and seg[k]["src_start"] % 480 == 0
        table = [(seg[k]["src_start"], seg[k]["src_stop"]) for k in idx]
        want, offs, total = W.join(rows, table, [gaps[k] for k in idx], 240, g == 0, g == len(groups) - 1)
        for r, k in enumerate(idx):
            assert seg[k]["start"] == k0 + offs[r] and seg[k]["stop"] - seg[k]["start"] == table[r][1] - table[r][0]
        pieces.append(want)
        k0 += total
    for k in range(4):
        if seg[k]["stop"] > seg[k]["start"]:
            assert seg[k + 1]["start"] == seg[k]["stop"] + gaps[k], f"chunk {k}: the segments are contiguous up to the gap"
    want = np.concatenate(pieces)
    assert got.shape == (1, len(want)) and got.shape[1] == seg[-1]["stop"]
    bad = np.nonzero(got[0].numpy().view(np.int32) != want.view(np.int32))[0]
    print(f"{cls_name} max_batch={max_batch}: {len(want)} samples, kept {[(s['src_start'], s['src_stop']) for s in seg]}, {len(bad)} differ bitwise")
    assert len(bad) == 0, f"{len(bad)} of {len(want)} samples differ bitwise, first at {bad[:5]}"


@pytest.mark.parametrize("cls_name", list(CLASSES))
def test_chunks_that_spend_the_budget_are_reported_truncated_with_one_warning(dev, cls_name, caplog):
    m = _model(dev, cls_name)
    with caplog.at_level(logging.WARNING, logger="chatterbox_amd.api"):
        _, seg = m.generate_long(FIVE, seed=SEED, max_chars=30, return_segments=True, **CLASSES[cls_name][1])
    assert len(seg) == 5 and all(s["truncated"] for s in seg)
    msgs = [r.getMessage() for r in caplog.records if "generate_long" in r.getMessage()]
    assert len(msgs) == 1 and "max_chars" in msgs[0] and "[0, 1, 2, 3, 4]" in msgs[0]
