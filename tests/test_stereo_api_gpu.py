"""GPU (-m gpu): generate_dialogue(pan=) on the tiny synthetic models of test_loudness_api_gpu.py (t3_layers=2, a budget of 20 tokens = 0.8 s per chunk, a stub
tokenizer).  Two voices, one chunk per turn:
  * non-negative gaps, no balance: the result is (2, n); both voices at 0 give L == R bitwise and each plane is fp32(mono * pan_gains(0)[0]) bitwise, because
    every sample is covered by one row; voice a at -1 leaves the right plane exactly zero over a's segments; pan=None is the call without the argument bitwise;
    the segments equal the mono call's -- on all three classes;
  * a negative gap=: two calls with one seed give the same bits;
  * loudness=-16, true_peak=-1: a measure-only wave_loudness_ch / wave_limit_ch reading of the returned planes, within the bounds the mono API tests use: the
    true peak under -1 dBTP within limit_common's bound (CEIL_PRE for the gain modulation between the samples, TOL_OUT of the signal's scale for the kernel); the
    loudness by test_loudness_api_gpu._reads' rule -- -16 LUFS within TOL_API = 0.01 LU, or the ceiling held the level back: the peak sits AT the ceiling and the
    reading is below the target (there the sample peak 1.0, here the true peak -1 dBTP, and the limiter reports samples with g < 1).  Measured on the MI355X: the
    synthetic voices' mix reads -29.05 LUFS with a sample peak of 0.437, the full gain 4.49 lifts its true peak to 1.965, the limiter pulls 2413 samples down
    (min g 0.4535), and the result reads -16.1748 LUFS at a true peak of 0.891252 (ceiling 0.891251): the second branch;
  * sample_rate=8000, encoding="mulaw": (2, m) uint8, each plane equal to ops.wave_format of that plane of the fp32 result."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import limit_common as K  # noqa: E402
from test_dialogue_api_gpu import SENTENCES, _voice  # noqa: E402  (read-only import: the sentences, a second synthetic voice)
from test_loudness_api_gpu import TOL_API, TTS, _model  # noqa: E402  (read-only import: the synthetic models with a budget of 20 tokens, built once)

pytestmark = pytest.mark.gpu

SEED = 31
TURNS = [("a", SENTENCES[0]), ("b", SENTENCES[1]), dict(voice="a", text=SENTENCES[2], gap=0.1)]


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def _setup(dev, name):
    m, lang = _model(dev, name)
    kw = dict(language_id=lang[0]) if lang else {}
    return m, dict(a=m.conds, b=_voice(7, name)), kw


@pytest.mark.parametrize("name", TTS)
def test_two_voices_placed_centre_and_hard_left(dev, name):
    from chatterbox_amd import ops
    m, voices, kw = _setup(dev, name)
    mono, mseg = m.generate_dialogue(TURNS, voices, seed=SEED, return_segments=True, **kw)
    none, nseg = m.generate_dialogue(TURNS, voices, seed=SEED, return_segments=True, pan=None, **kw)
    assert mono.shape[0] == 1 and torch.equal(_bits(mono), _bits(none)) and mseg == nseg and m.last_pan is None, "pan=None: the call without the argument, bit for bit"
    mid, seg = m.generate_dialogue(TURNS, voices, seed=SEED, return_segments=True, pan=dict(a=0, b=0.0), **kw)
    n = mono.shape[1]
    print(f"{name}: {n} samples, segments {[(s['voice'], s['start'], s['stop']) for s in seg]}")
    assert mid.shape == (2, n) and mid.dtype == torch.float32 and mid.device.type == "cpu" and seg == mseg, "planar (2, n); the segments are the mono call's"
    assert all(a["stop"] <= b["start"] for a, b in zip(seg, seg[1:])), "non-negative gaps: every sample is covered by at most one row"
    g0 = ops.pan_gains(0)[0]
    assert torch.equal(_bits(mid[0]), _bits(mid[1])), "both voices at 0: L == R bit for bit"
    assert torch.equal(_bits(mid[0]), _bits(mono[0] * torch.tensor(g0, dtype=torch.float32))), "each plane is fp32(mono * pan_gains(0)[0]): one rounded multiply per sample"
    assert m.last_pan == [dict(voice="a", position=0.0, left=g0, right=g0), dict(voice="b", position=0.0, left=g0, right=g0)]
    left, lseg = m.generate_dialogue(TURNS, voices, seed=SEED, return_segments=True, pan=dict(a=-1), **kw)
    assert left.shape == (2, n) and lseg == mseg
    for s in seg:
        a, b = s["start"], s["stop"]
        if s["voice"] == "a":
            assert not left[1, a:b].any() and torch.equal(_bits(left[0, a:b]), _bits(mono[0, a:b])), "voice a at -1: gains exactly (1, 0)"
        else:
            assert torch.equal(_bits(left[0, a:b]), _bits(left[1, a:b])) and left[1, a:b].any(), "voice b, not named, sits at 0"


def test_an_overlap_is_reproducible_bit_for_bit(dev):
    m, voices, kw = _setup(dev, "ChatterboxTTS")
    turns = [("a", SENTENCES[0]), dict(voice="b", text=SENTENCES[1], gap=-0.2), ("a", SENTENCES[2])]
    one, seg = m.generate_dialogue(turns, voices, seed=SEED, pan=True, balance=True, return_segments=True)
    two = m.generate_dialogue(turns, voices, seed=SEED, pan=True, balance=True)
    assert seg[1]["start"] < seg[0]["stop"], "turn 1 comes in before turn 0 has finished"
    assert one.shape[0] == 2 and torch.equal(_bits(one), _bits(two)) and not torch.equal(one[0], one[1]), "the same bits; the voices sit apart"
    assert [p["position"] for p in m.last_pan] == [-0.3, 0.3] and [b["voice"] for b in m.last_balance] == ["a", "b"]


def test_loudness_and_true_peak_hold_for_the_two_channel_signal(dev):
    from chatterbox_amd import ops
    m, voices, kw = _setup(dev, "ChatterboxTTS")
    plain = m.generate_dialogue(TURNS, voices, seed=SEED, pan=dict(a=-0.6, b=0.4))
    got = m.generate_dialogue(TURNS, voices, seed=SEED, pan=dict(a=-0.6, b=0.4), loudness=-16, true_peak=-1)
    assert got.shape == plain.shape and got.dtype == torch.float32
    loud, lim = m.engine.last_loudness.cpu().numpy(), m.engine.last_limit.cpu().numpy()
    with torch.cuda.device(dev):
        d = got.to(dev)
        stats, _ = ops.wave_loudness_ch([d[0], d[1]], None)
        _, tp = ops.wave_limit_ch([d[0], d[1]], None)
        stats, tp = stats.cpu().numpy(), tp.cpu().numpy()
    C = K.linear(-1.0)
    scale = float(loud[0, 1] * loud[0, 2])   # the sample peak of u = x gamma over both channels
    print(f"the plain mix reads {loud[0, 0]:.4f} LUFS, peak {loud[0, 1]:.5f}; gain {loud[0, 2]:.5f}; limiter: true peak of u {lim[0, 0]:.5f}, min g {lim[0, 1]:.6f}, "
          f"{int(lim[0, 2])} samples with g < 1")
    print(f"the result reads {stats[0, 0]:.5f} LUFS (target -16, allowed +- {TOL_API}) and a true peak of {tp[0, 0]:.6f} = {20 * np.log10(tp[0, 0]):.4f} dBTP (ceiling {C:.6f})")
    assert loud.shape == (1, 4) and lim.shape == (1, 4) and stats[0, 3] >= 1, "ONE reading and ONE envelope for the two-channel signal; long enough to be measured"
    assert tp[0, 0] <= C * (1.0 + K.CEIL_PRE) + K.TOL_OUT * max(scale, 1.0), "under -1 dBTP at the samples and between them, in both channels"
    if abs(stats[0, 0] + 16.0) > TOL_API:   # (test_loudness_api_gpu._reads' rule: the ceiling held the level back)
        assert lim[0, 2] > 0 and abs(tp[0, 0] - C) <= C * K.CEIL_PRE + K.TOL_OUT * max(scale, 1.0) and stats[0, 0] < -16.0, \
            f"the result reads {stats[0, 0]} LUFS, target -16, true peak {tp[0, 0]} against the ceiling {C}, {lim[0, 2]} samples limited"
    assert abs(loud[0, 2] - 10.0 ** ((-16.0 - loud[0, 0]) / 20.0)) <= 1e-6 * loud[0, 2], "the UNCAPPED gain to -16 LUFS is the limiter's pre-gain"


def test_the_format_converts_both_planes(dev):
    from chatterbox_amd import ops
    m, voices, kw = _setup(dev, "ChatterboxTTS")
    plain, pseg = m.generate_dialogue(TURNS, voices, seed=SEED, pan=True, return_segments=True)
    got, seg = m.generate_dialogue(TURNS, voices, seed=SEED, pan=True, return_segments=True, sample_rate=8000, encoding="mulaw")
    fmt = ops.check_format(8000, "mulaw")
    assert got.dtype == torch.uint8 and got.shape == (2, ops.formatted_len(plain.shape[1], 8000))
    with torch.cuda.device(dev):
        for c in range(2):
            want = ops.wave_format([plain[c].to(dev)], fmt)[0].cpu()
            assert torch.equal(got[c], want), f"plane {c} is ops.wave_format of that plane"
    assert [(s["start"], s["stop"]) for s in seg] == [(ops.formatted_len(s["start"], 8000), ops.formatted_len(s["stop"], 8000)) for s in pseg]
