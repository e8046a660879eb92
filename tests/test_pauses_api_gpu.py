"""GPU (-m gpu): max_pause= / pause_db= through the engines and the public API on synthetic 2-layer models with a token budget of 20 (0.8 s, 40 frames).  The
oracle is the NumPy restatement of wave_squeeze_common.py applied to what the call WITHOUT the arguments returns (same seed): the shortened result equals it
bitwise.  Synthetic weights make no real pauses, so pause_db is small (PAUSE_DB = 3: frames under half the loudest frame's power count as silent; the one-request
test tries further seeds, and 2 and 1 dB, when the oracle finds nothing to remove in that request's plain result) and max_pause is 0.04 s (K = 2); every test asserts
FROM THE ORACLE that at least one frame is removed, so none passes empty.
generate of the four classes, generate_batch with a mixed list over two sub-batches (ChatterboxTTS: the throughput schedule, synthesize_pipelined), the delivery
format, loudness ahead of the squeeze, generate_long and generate_long_stream, and max_pause=None bitwise and call for call the method without the argument.
The kernel-level tests are in test_turbo_stream_wave_squeeze_kernels_gpu.py."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import wave_squeeze_common as S  # noqa: E402
from test_loudness_api_gpu import TTS, _model  # noqa: E402  (read-only import: the synthetic models of the module, token budget 20, EOS banned)
from test_seeded_api_gpu import SEEDS, TEXTS  # noqa: E402  (read-only import: the requests)

pytestmark = pytest.mark.gpu

PAUSE_DB = 3.0
MAX_PAUSE = 0.04   # K = 2 frames
FADE = 240         # api.PAUSE_FADE


def _oracle(wav, max_pause=MAX_PAUSE, db=PAUSE_DB, what=""):
    """(1, n) fp32 -> (the shortened (n',) array, stats) by the restatement; at least one frame must go"""
    x = wav[0].numpy()
    y, stats, _ = S.squeeze(x, int(round(max_pause * 50)), S.ratio_of(db), FADE, check_margin=True)
    print(f"{what}: {len(x)} samples -> {stats[0]}: {stats[1]} pauses cut, {stats[2]} frames removed")
    return y[: stats[0]], stats


def _pick_case(call, what):
    """The seed and the pause_db of a test whose text is fixed: the first seed of 77, SEEDS[0 .. 2], 78, 79 and, for it, the first pause_db of 3, 2, 1 at which the
    ORACLE removes a frame from the plain result -- a choice of the test's INPUT, made from the call without the arguments and the restatement alone (a synthetic
    result whose loud frames are contiguous has no pause at any threshold).  None of them: the test fails instead of passing empty.  -> (seed, db, plain result)"""
    for seed in (77, *SEEDS[:3], 78, 79):
        wav = call(seed)
        for db in (PAUSE_DB, 2.0, 1.0):
            if S.squeeze(wav[0].numpy(), 2, S.ratio_of(db), FADE)[1][2] >= 1:
                print(f"{what}: seed = {seed}, pause_db = {db}")
                return seed, db, wav
    raise AssertionError(f"{what}: the case is empty -- no frame of the synthetic result is removed for any of six seeds at pause_db 3, 2 or 1")


def _same(got, want, what):
    assert got.dtype == torch.float32 and got.shape == (1, len(want)), (what, got.shape, len(want))
    bad = np.nonzero(got[0].numpy().view(np.int32) != want.view(np.int32))[0]
    assert len(bad) == 0, f"{what}: {len(bad)} of {len(want)} samples differ bitwise, first at {bad[:5]}"


@pytest.mark.parametrize("name", TTS + ["ChatterboxVC"])
def test_generate_equals_the_oracle_on_the_plain_result_and_none_is_the_call_without_it(dev, name, monkeypatch):
    from chatterbox_amd import ops, synth
    m, lang = _model(dev, name)
    src = synth.speech_tokens(20, seed=3)
    gen = (lambda seed, **kw: m.generate(s3_tokens=src, seed=seed, **kw)) if name == "ChatterboxVC" else (lambda seed, **kw: m.generate(TEXTS[0], *lang, seed=seed, **kw))
    seed, db, base = _pick_case(gen, f"{name}.generate")
    call = lambda **kw: gen(seed, **kw)
    real, calls = ops.lib, []

    class Spy:
        def __getattr__(self, entry):
            calls.append(entry)
            return getattr(real, entry)

    monkeypatch.setattr(ops, "lib", Spy())
    again = call()
    plain = list(calls)
    calls.clear()
    none = call(max_pause=None, pause_db=db)
    calls_none = list(calls)
    calls.clear()
    got = call(max_pause=MAX_PAUSE, pause_db=db)
    calls_on = list(calls)
    monkeypatch.setattr(ops, "lib", real)
    assert torch.equal(base, again) and torch.equal(base, none), "max_pause=None: bitwise the seeded call without the argument"
    assert calls_none == plain and "cbx_wave_squeeze_f32" not in plain, "and the same calls into the library, one for one"
    assert calls_on.count("cbx_wave_squeeze_f32") == 1 and [c for c in calls_on if c != "cbx_wave_squeeze_f32"] == plain, "with it: ONE more entry"
    want, stats = _oracle(base, db=db, what=f"{name}.generate")
    assert stats[2] >= 1, "the case is empty: no frame of the synthetic result is removed at this pause_db"
    _same(got, want, f"{name}.generate(max_pause=)")
    assert m.engine.last_pauses.cpu().tolist() == [stats], "engine.last_pauses: the record of the call"
    # the delivery format: the conversion of the oracle's output
    fmt = dict(sample_rate=8000, encoding="mulaw")
    enc = call(max_pause=MAX_PAUSE, pause_db=db, **fmt)
    with torch.cuda.device(dev):
        ref = ops.wave_format([torch.from_numpy(want).to(dev)], fmt)[0].cpu()
    assert enc.dtype == torch.uint8 and enc.shape == (1, ops.formatted_len(len(want), 8000)) and torch.equal(enc[0], ref), "mu-law at 8 kHz of the shortened signal"
    # loudness runs ahead: the oracle applied to the loudness-only result
    loud = call(loudness=-23)
    both = call(loudness=-23, max_pause=MAX_PAUSE, pause_db=db)
    want_l, stats_l = _oracle(loud, db=db, what=f"{name}.generate(loudness=-23)")
    assert stats_l[2] >= 1
    _same(both, want_l, f"{name}.generate(loudness=-23, max_pause=)")


@pytest.mark.parametrize("name", ["ChatterboxTTS", "ChatterboxTurboTTS"])
def test_generate_batch_takes_a_max_pause_per_request_over_two_sub_batches(dev, name):
    """three requests as sub-batches of two and one (ChatterboxTTS: synthesize_pipelined, where the record travels as a pinned copy behind the event): rows 0 and 2 equal
    the oracle on the plain batch's rows with their own K, row 1 (None) keeps its samples"""
    m, lang = _model(dev, name)
    m.max_batch = 2
    try:
        base = m.generate_batch(TEXTS[:3], *lang, seeds=SEEDS[:3])
        got = m.generate_batch(TEXTS[:3], *lang, seeds=SEEDS[:3], max_pause=[MAX_PAUSE, None, 0.06], pause_db=PAUSE_DB)
        same = m.generate_batch(TEXTS[:3], *lang, seeds=SEEDS[:3], max_pause=[None, None, None])
    finally:
        m.max_batch = None
    assert all(torch.equal(a, b) for a, b in zip(base, same)) and torch.equal(got[1], base[1]), "a None row keeps its samples"
    removed = 0
    for k, mp in ((0, MAX_PAUSE), (2, 0.06)):
        want, stats = _oracle(base[k], mp, what=f"{name} row {k}")
        _same(got[k], want, f"{name} row {k}")
        removed += stats[2]
    assert removed >= 1, "the case is empty: no frame of either row is removed"


@pytest.mark.parametrize("name", TTS)
def test_generate_long_shortens_its_chunks_and_the_stream_concatenates_to_it(dev, name):
    m, lang = _model(dev, name)
    text = "The first sentence is here. A second one follows it! Is the third a question?"
    base, seg0 = m.generate_long(text, *lang, seed=5, max_chars=30, return_segments=True)
    got, seg = m.generate_long(text, *lang, seed=5, max_chars=30, return_segments=True, max_pause=MAX_PAUSE, pause_db=PAUSE_DB)
    stats = m.engine.last_pauses.cpu().tolist()
    print(f"{name}.generate_long: {base.shape[1]} -> {got.shape[1]} samples, stats {stats}")
    assert len(seg) == len(seg0) == 3 and len(stats) == 3, "three chunks in one device batch"
    frames = sum(s[2] for s in stats)
    assert frames >= 1, "the case is empty: no frame of any chunk is removed"
    assert got.shape[1] == base.shape[1] - 480 * frames, "the total shrinks by 480 samples per removed frame"
    gaps = [b["start"] - a["stop"] for a, b in zip(seg0, seg0[1:])]
    assert seg[0]["start"] == 0 and seg[-1]["stop"] == got.shape[1] and [b["start"] - a["stop"] for a, b in zip(seg, seg[1:])] == gaps, "the segments tile the result"
    for s, s0, st in zip(seg, seg0, stats):
        assert s["stop"] - s["start"] == s["src_stop"] - s["src_start"] == (s0["stop"] - s0["start"]) - 480 * st[2], "a segment holds its chunk's kept, shortened samples"
        assert s["tokens"].tolist() == s0["tokens"].tolist()
    pieces = list(m.generate_long_stream(text, *lang, seed=5, max_chars=30, max_pause=MAX_PAUSE, pause_db=PAUSE_DB, first_batch=None))
    assert torch.equal(torch.cat(pieces, dim=1), got), "first_batch=None concatenates to generate_long bit for bit"
    m.max_batch = 2
    try:
        ramped = list(m.generate_long_stream(text, *lang, seed=5, max_chars=30, max_pause=MAX_PAUSE, pause_db=PAUSE_DB, return_segments=True))
    finally:
        m.max_batch = None
    assert len(ramped) == 2 and [len(sg) for _, sg in ramped] == [1, 2], "two device batches (ChatterboxTTS: the throughput schedule, where the record is a pinned copy)"
    assert ramped[-1][1][-1]["stop"] == sum(w.shape[1] for w, _ in ramped), "the segments count samples of the shortened stream"
