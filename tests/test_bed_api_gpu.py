"""GPU (-m gpu): bed= through the public API on the synthetic 2-layer models of test_loudness_api_gpu.py (token budget 20, EOS banned).  The oracle of
bed_common.py (NumPy, fp64) restates every returned waveform from the plain seeded call: generate_long(bed=) and generate_dialogue(bed=) of each class equal the
oracle applied to the seeded call without a bed, with the gain model.last_bed reports -- itself checked against the two meter readings --, within the kernel
tolerance; with loudness=-16, true_peak=-1, encoding="s16" the result is bitwise the existing one-shot chain (ops.wave_loudness, ops.wave_limit, ops.wave_format)
applied to that sum; bed=None is bitwise the call without it; the segments shift by lead; a bed decoded on the device and on the host agree within the ingest
test's bound."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import bed_common as C  # noqa: E402
import loudness_common as LC  # noqa: E402
import wave_ingest_common as WI  # noqa: E402
from test_loudness_api_gpu import TTS, _model  # noqa: E402  (read-only import: the synthetic models, built once for the modules that use them)

pytestmark = pytest.mark.gpu

TEXT = "The first sentence is here. A second one follows it! Is the third a question?"
TURNS = [(None, "The first sentence is here."), (None, "A second one follows it!"), dict(text="Is the third a question?", gap=-0.1)]
SOURCE = C.bed(12000, 3)                               # 0.5 s: one whole 400 ms block for the meter; it loops under 2.5 s of speech
BED = dict(audio=(SOURCE, 24000), lead=0.05, tail=0.1, loop_fade=0.05, fade_out=0.2, pre=0.03, post=0.05, ramp=0.04, level=-6)


def _calls(m, lang, which):
    if which == "long":
        return lambda **kw: m.generate_long(TEXT, *lang, seed=5, max_chars=30, return_segments=True, **kw)
    return lambda **kw: m.generate_dialogue(TURNS, **(dict(language_id=lang[0]) if lang else {}), seed=5, max_chars=30, return_segments=True, **kw)


def _bed_for(base, **over):
    """BED with the threshold 12 dB under the sample peak of the seeded call: some frame is active whatever level the synthetic weights speak at"""
    peak = float(np.abs(base[0].numpy()).max())
    assert peak > 1e-4, "the synthetic model is not silent"
    return dict(BED, threshold=float(np.clip(np.floor(20.0 * np.log10(peak)) - 12.0, -100.0, 0.0)), **over)


def _strip(segs):
    return [{k: (v.tolist() if torch.is_tensor(v) else v) for k, v in s.items()} for s in segs]


def _check_against_the_oracle(what, m, base, got, source, plan):
    """`got` (the call with the bed) against the oracle over `base` (the call without) and the 24 kHz source; the gain against the two readings.  Returns the gain."""
    x, lb = base[0].numpy(), m.last_bed
    ls, lbed = LC.oracle(x)["L"], LC.oracle(source)["L"]
    print(f"{what}: last_bed {lb}; the loudness oracle reads speech {ls:.4f}, bed {lbed:.4f} LUFS")
    assert set(lb) == {"gain", "speech_lufs", "bed_lufs", "ducked", "frames", "peak"}
    assert abs(lb["speech_lufs"] - ls) <= LC.TOL_L and abs(lb["bed_lufs"] - lbed) <= LC.TOL_L, "the speech over the mix before the bed, the bed over its whole source"
    want = C.level_oracle(lb["speech_lufs"], lb["bed_lufs"], plan["level"])
    assert abs(lb["gain"] - float(want)) <= 2.0 * float(np.spacing(want)), f"{what}: gain {lb['gain']!r}, 10^((Ls + level - Lb) / 20) = {want!r}"
    ref = C.check_row(what, 0, x, source, plan, lb["gain"], got[0].numpy(), [lb["gain"], lb["ducked"], lb["frames"], lb["peak"]])
    assert 0 < lb["ducked"] < lb["frames"], f"{what}: the bed goes down for some frames and not for all ({lb['ducked']} of {lb['frames']})"
    assert got.shape == (1, ref["N"]) and got.dtype == torch.float32
    return lb["gain"]


@pytest.mark.parametrize("which", ["long", "dialogue"])
@pytest.mark.parametrize("name", TTS)
def test_the_bed_is_the_oracle_over_the_seeded_call_and_the_finish_sees_the_sum(dev, name, which):
    from chatterbox_amd import ops
    m, lang = _model(dev, name)
    call = _calls(m, lang, which)
    (base, seg0), (none, seg1) = call(), call(bed=None)
    bed = _bed_for(base)
    plan = ops.check_bed(bed)
    assert torch.equal(base, none) and _strip(seg0) == _strip(seg1) and m.last_bed is None, "bed=None: bitwise the seeded call without the keyword"
    got, seg = call(bed=bed)
    _check_against_the_oracle(f"{name} {which}", m, base, got, SOURCE, plan)
    lead = plan["lead"]
    assert lead == 1200 and [(s["start"], s["stop"]) for s in seg] == [(s["start"] + lead, s["stop"] + lead) for s in seg0] and got.shape[1] == base.shape[1] + lead + plan["tail"]
    assert [(s["src_start"], s["src_stop"]) for s in seg] == [(s["src_start"], s["src_stop"]) for s in seg0]
    # loudness, true_peak and the s16 store see speech plus bed: the existing one-shot chain over that sum, bit for bit
    s16, seg2 = call(bed=bed, loudness=-16, true_peak=-1, encoding="s16")
    with torch.cuda.device(dev):
        w = got[0].to(dev)
        _, gain = ops.wave_loudness([w], [-16.0], None)
        lim, _ = ops.wave_limit([w], [-1.0], gain=gain)
        want = ops.wave_format([lim[0]], ops.check_format(None, "s16"))[0].cpu()
    assert s16.dtype == torch.int16 and torch.equal(s16[0], want), "bed, then loudness, true_peak and the format over the sum"
    assert _strip(seg2) == _strip(seg) and int(want.abs().max()) < 32767
    call()
    assert m.last_bed is None


def test_a_bed_decoded_on_the_device_and_on_the_host_agree_within_the_ingest_bound(dev):
    from chatterbox_amd import ops
    m, lang = _model(dev, "ChatterboxTTS")
    call = _calls(m, lang, "long")
    src = C.bed(11500, 4)                                  # 22050 Hz: both modes resample, the host in fp64, the device in fp32
    base, _ = call()
    bed = _bed_for(base, audio=(src, 22050))
    plan = ops.check_bed(bed)
    y64, S = WI.oracle(src, 22050, 24000)
    bound = (WI.taps(22050, 24000) + 2) * WI.EPS * S + WI.EPS * np.abs(y64)
    outs, gains = {}, {}
    try:
        for mode in ("host", "device"):
            m.audio_in = mode
            source = m._bed_source(plan)
            source = source.cpu().numpy() if torch.is_tensor(source) else source
            assert source.dtype == np.float32 and source.shape == y64.shape
            if mode == "device":
                print(f"device ingest 22050 -> 24000: worst |y - y64| / bound = {WI.check_bound(source, src, 22050, 24000, 'bed'):.3f}")
            else:
                assert np.all(np.abs(source - y64) <= WI.EPS * np.abs(y64) + 1e-12), "host mode: the fp64 chain, stored as float32"
            got, _ = call(bed=bed)
            gains[mode] = _check_against_the_oracle(f"audio_in={mode}", m, base, got, source, plan)
            outs[mode] = got[0].numpy().astype(np.float64)
    finally:
        m.audio_in = "host"
    # the two outputs differ by the sources' difference times the gain, by the two gains' difference times the bed, and by each kernel's own tolerance
    scale = max(float(np.abs(base[0].numpy()).max()), float(np.abs(y64).max()) * gains["host"])
    allowed = gains["host"] * float((bound + WI.EPS * np.abs(y64)).max()) + abs(gains["device"] - gains["host"]) * float(np.abs(y64).max()) + 2 * C.TOL_OUT * scale
    err = float(np.abs(outs["device"] - outs["host"]).max())
    print(f"device against host bed: |dout| {err:.3g}, allowed {allowed:.3g} (gains {gains})")
    assert err <= allowed


def test_bad_beds_raise_before_anything_is_launched_and_the_stream_refuses(dev):
    m, lang = _model(dev, "ChatterboxTTS")
    m.seen.clear()
    for call, err in ((lambda: m.generate_long("One. Two.", bed=dict(audio=BED["audio"], duck=3)), ValueError), (lambda: m.generate_dialogue(TURNS, bed=5), TypeError),
                      (lambda: m.generate_dialogue(TURNS, bed=dict(audio=(np.zeros(100, np.float32), 24000))), ValueError),
                      (lambda: m.generate_long_stream("One. Two.", bed=BED), TypeError), (lambda: m.generate("One.", bed=BED), TypeError)):
        with pytest.raises(err, match="bed"):
            call()
    assert m.seen == []
