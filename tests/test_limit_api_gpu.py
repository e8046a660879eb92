"""GPU (-m gpu): true_peak= through the engines and the public API on the synthetic 2-layer models of test_loudness_api_gpu.py (token budget 20, EOS banned).  The
oracle of limit_common.py (NumPy, fp64) restates every returned waveform from the plain seeded call: with loudness=-5 and true_peak=-1 the meter's gain is the
UNCAPPED one, the waveform is the oracle's limiter over base * float32(gain) within the kernel tolerance and reads under the ceiling, and engine.last_limit holds
the oracle's stats; true_peak alone limits without a gain; None is bitwise the call without the keyword; a batch mixes rows with a target, a ceiling, or both;
the s16 store sees the limited signal; generate_long limits the assembled piece once and leaves the segments alone."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import limit_common as C  # noqa: E402
import loudness_common as LC  # noqa: E402
from test_loudness_api_gpu import N_TOK, TTS, _model  # noqa: E402  (read-only import: the synthetic models, built once for both modules)
from test_seeded_api_gpu import SEEDS, TEXTS  # noqa: E402  (read-only import: the requests)

pytestmark = pytest.mark.gpu


def _full_gain(x, target, what):
    """the UNCAPPED gain 10^((target - L) / 20) of the loudness oracle over x, and a note when the sample-peak cap of the call without true_peak would have cut it"""
    ref = LC.oracle(x, target, ceiling=None)
    assert np.isfinite(ref["L"]) and ref["blocks"] >= 1, "the request is long enough to be measured"
    capped = LC.oracle(x, target)["gain"]
    print(f"{what}: {ref['L']:.3f} LUFS, peak {ref['peak']:.4f}: full gain {ref['gain']:.5f}, with the sample-peak cap {capped:.5f}")
    return ref


@pytest.mark.parametrize("name", TTS + ["ChatterboxVC"])
def test_generate_limits_behind_the_full_gain_and_none_is_the_call_without_the_keyword(dev, name):
    from chatterbox_amd import synth
    m, lang = _model(dev, name)
    src = synth.speech_tokens(N_TOK, seed=3)
    call = (lambda **kw: m.generate(s3_tokens=src, seed=77, **kw)) if name == "ChatterboxVC" else (lambda **kw: m.generate(TEXTS[0], *lang, seed=77, **kw))
    m.seen.clear()
    base, none = call(), call(true_peak=None)
    assert base.dtype == torch.float32 and torch.equal(base, none), "true_peak=None: bitwise the seeded call without the keyword"
    x = base[0].numpy()
    # a loud target and a ceiling: the full gain, then the limiter
    got = call(loudness=-5, true_peak=-1)
    assert m.seen[0] == m.seen[1] == m.seen[2] and got.shape == base.shape, "the same tokens, the same length"
    ref = _full_gain(x, -5.0, f"{name}.generate(loudness=-5, true_peak=-1)")
    loud, lim = m.engine.last_loudness.cpu().numpy(), m.engine.last_limit.cpu().numpy()
    assert loud.shape == (1, 4) and lim.shape == (1, 4) and abs(loud[0, 2] - ref["gain"]) <= LC.TOL_GAIN * ref["gain"], f"the UNCAPPED gain: {loud[0, 2]!r}, oracle {ref['gain']!r}"
    C.check_row(name, 0, x, -1.0, np.float32(loud[0, 2]), C.LOOK, got[0].numpy(), lim[0])
    # the s16 store sees the limited signal, and nothing saturates
    s16 = call(loudness=-5, true_peak=-1, encoding="s16")
    want = np.clip(np.rint(got[0].numpy().astype(np.float64) * 32768.0), -32768, 32767).astype(np.int16)
    assert s16.dtype == torch.int16 and np.array_equal(s16[0].numpy(), want), "the store equals rint(clip(. 32768)) of the limited fp32 result"
    assert int(np.abs(want.astype(np.int32)).max()) < 32767, "no sample saturates"
    # a ceiling alone: limited, no gain.  The ceiling is put under the signal's own true peak so that the limiter has work to do
    tp = C.true_peak(x)
    db = float(np.clip(np.floor(20.0 * np.log10(tp) - 3.0), -20.0, 0.0))
    alone = call(true_peak=db)
    lim = m.engine.last_limit.cpu().numpy()
    print(f"{name}.generate(true_peak={db}): the plain call reads a true peak of {tp:.5f} ({20 * np.log10(tp):.2f} dBTP)")
    C.check_row(name + " alone", 0, x, db, 1.0, C.LOOK, alone[0].numpy(), lim[0])
    if tp > C.linear(db):
        assert lim[0, 3] > 0 and not torch.equal(alone, base)


@pytest.mark.parametrize("name,max_batch", [("ChatterboxTTS", None), ("ChatterboxTTS", 2), ("ChatterboxTurboTTS", 2)])
def test_generate_batch_mixes_targets_and_ceilings(dev, name, max_batch):
    """three requests as one device batch and as sub-batches of two: row 0 has a target and a ceiling, row 1 a target alone (bitwise today's row), row 2 a ceiling
    alone"""
    m, lang = _model(dev, name)
    m.max_batch = max_batch
    try:
        base = m.generate_batch(TEXTS[:3], *lang, seeds=SEEDS[:3])
        today = m.generate_batch(TEXTS[:3], *lang, seeds=SEEDS[:3], loudness=[None, -16, None])
        got = m.generate_batch(TEXTS[:3], *lang, seeds=SEEDS[:3], loudness=[-5, -16, None], true_peak=[-1, None, -3])
    finally:
        m.max_batch = None
    assert torch.equal(got[1], today[1]), "a row with a target and no ceiling keeps the sample-peak cap, and so today's bits"
    assert [g.shape for g in got] == [b.shape for b in base], "the limiter changes no length"
    x0, x2 = base[0][0].numpy(), base[2][0].numpy()
    ref = _full_gain(x0, -5.0, f"{name} max_batch={max_batch} row 0")
    g0, lim = ref["gain32"], [None] * 3
    if max_batch is None:  # ONE device batch: the engine's stats cover the three requests -- in ITS row order, which the gains identify
        loud, rows = m.engine.last_loudness.cpu().numpy(), m.engine.last_limit.cpu().numpy()
        want = [ref["gain"], LC.oracle(base[1][0].numpy(), -16.0)["gain"], 1.0]
        at = [int(np.argmin(np.abs(loud[:, 2] - w))) for w in want]
        assert loud.shape == (3, 4) and rows.shape == (3, 4) and sorted(at) == [0, 1, 2], (loud, want)
        assert all(abs(loud[a, 2] - w) <= LC.TOL_GAIN * w for a, w in zip(at, want)), "row 0: the UNCAPPED gain; row 1: the capped gain of today; row 2: no gain"
        assert rows[at[1], 1] == 1.0 and rows[at[1], 2] == 0 and rows[at[1], 3] == 0, "row 1 is not limited"
        g0, lim = np.float32(loud[at[0], 2]), [rows[a] for a in at]
    C.check_row(f"{name} row 0", 0, x0, -1.0, g0, C.LOOK, got[0][0].numpy(), lim[0])
    C.check_row(f"{name} row 2", 2, x2, -3.0, 1.0, C.LOOK, got[2][0].numpy(), lim[2])


@pytest.mark.parametrize("name", TTS)
def test_generate_long_limits_the_whole_piece_once_and_keeps_its_segments(dev, name):
    m, lang = _model(dev, name)
    text = "The first sentence is here. A second one follows it! Is the third a question?"
    base, seg = m.generate_long(text, *lang, seed=5, max_chars=30, return_segments=True)
    plain, seg1 = m.generate_long(text, *lang, seed=5, max_chars=30, return_segments=True, loudness=-16)
    got, seg2 = m.generate_long(text, *lang, seed=5, max_chars=30, return_segments=True, loudness=-16, true_peak=-1)
    strip = lambda segs: [{k: (v.tolist() if torch.is_tensor(v) else v) for k, v in s.items()} for s in segs]
    assert len(seg) == 3 and strip(seg2) == strip(seg1) and got.shape == base.shape, "the segments equal those of the call without a peak"
    x = base[0].numpy()
    ref = _full_gain(x, -16.0, f"{name}.generate_long(loudness=-16, true_peak=-1)")
    loud, lim = m.engine.last_loudness.cpu().numpy(), m.engine.last_limit.cpu().numpy()
    assert abs(loud[0, 2] - ref["gain"]) <= LC.TOL_GAIN * ref["gain"], "ONE uncapped gain for the assembled waveform"
    C.check_row(name + " long", 0, x, -1.0, np.float32(loud[0, 2]), C.LOOK, got[0].numpy(), lim[0])


def test_bad_ceilings_raise_before_anything_is_launched(dev):
    from chatterbox_amd import synth
    m, lang = _model(dev, "ChatterboxTTS")
    m.seen.clear()
    for call in (lambda: m.generate(TEXTS[0], true_peak=1), lambda: m.generate_batch(TEXTS[:2], true_peak=[-1]), lambda: m.generate_long("One. Two.", true_peak=float("nan"))):
        with pytest.raises(ValueError, match="true_peak"):
            call()
    with pytest.raises(TypeError, match="true_peak"):
        m.generate_stream(TEXTS[0], true_peak=-1)
    with pytest.raises(ValueError, match="true_peak together with join"):
        m.engine.vocode([synth.speech_tokens(8, seed=1)], m.conds.gen, join=dict(gaps=[0]), true_peak=-1)
    assert m.seen == [[synth.speech_tokens(8, seed=1).tolist()]], "only the engine call itself was seen, and it raised before its first launch"
