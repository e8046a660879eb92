"""Host tests (no GPU) of the music bed: the oracle's own anchors, cbx_wave_duck_f32 / cbx_wave_duck_level_f32 on the SIMT emulator against the NumPy oracle of
bed_common.py (tolerances and their reasons there), the C ABI and its refusals, ops.check_bed, and the bed= keyword of generate_dialogue / generate_long of every
TTS class over the recording engines of the existing host tests."""
import ctypes
import inspect
import os
import re
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, os.path.join(HERE, "simt")):
    if p not in sys.path:
        sys.path.insert(0, p)

import bed_common as C  # noqa: E402
from test_wave_join_host import KINDS, LONG_TEXT, _jobs  # noqa: E402  (read-only import: the engines that know a joined piece)
from test_wave_mix_host import SCRIPT, STARTS, TOTAL, _lang_kw, _Mark, _model, _norm, _record, _voices  # noqa: E402  (read-only import: the dialogue's stand-ins)

CPU = torch.device("cpu")
ENTRIES = {"cbx_wave_duck_f32": 28, "cbx_wave_duck_level_f32": 6}
CASES = C.cases()


# ----------------------------------------------------------------------------- the definition
def test_the_oracle_ducks_around_speech_and_is_one_elsewhere():
    p = C.plan(pre=1, post=3, S=2, fi=0, fo=0, lead=100)
    s = np.zeros(6000, np.float32)
    s[900:2400] = C.SPEECH_AMP                                  # output samples 1000 .. 2499: frames 4 .. 10
    ref = C.oracle(s, np.ones(700, np.float32), p)
    d = float(np.float32(C.linear(-9.0)))
    assert ref["N"] == 6100 and ref["F"] == 26 and list(np.flatnonzero(ref["act"])) == list(range(4, 11)) and list(np.flatnonzero(ref["A"])) == list(range(3, 14))
    assert ref["stats"][:3] == [1.0, 11, 26] and abs(ref["G"][7] - d) < 1e-7 and np.all(ref["G"][:1] == 1.0) and np.all(ref["G"][16:] == 1.0)
    assert np.all(np.diff(ref["G"][:8]) <= 0) and np.all(np.diff(ref["G"][8:]) >= 0) and ref["g"].min() >= d - 1e-7 and ref["g"].max() == 1.0
    assert np.array_equal(ref["out"][:100], np.ones(100)) and np.array_equal(ref["out"][5000:], np.ones(1100)), "lead and tail: the bed alone, g = 1 far from speech"
    for q in (dict(duck=0.0), dict(threshold=0.0)):
        assert np.all(C.oracle(s, np.ones(700, np.float32), dict(p, **q))["g"] == 1.0), "duck = 0 dB, or no active frame: g is exactly 1"
    once = C.oracle(s, C.bed(1000, 1), dict(p, loop=False, fo=100))
    assert once["e"][999] == 1.0 / 101.0 and np.all(once["e"][1000:] == 0) and np.array_equal(once["out"][1000:], once["sp"][1000:].astype(np.float64))
    loop = C.oracle(s, C.bed(1000, 1), dict(p, xf=48))
    b = C.bed(1000, 1).astype(np.float64)
    assert loop["bed"][951] == b[951] and loop["bed"][952 + 48] == b[48] and abs(loop["bed"][952] - (b[952] + (b[0] - b[952]) / 96.0)) < 1e-7, "P = nb - xf: the seam fades b[P + r] into b[r]"


def test_fma32_is_the_correctly_rounded_fused_multiply_add():
    rng = np.random.default_rng(0)
    a, b, c = (rng.standard_normal(20000).astype(np.float32) for _ in range(3))
    c[:5000] = (-a[:5000].astype(np.float64) * b[:5000]).astype(np.float32)              # heavy cancellation: the product's low bits decide
    from fractions import Fraction
    got = C.fma32(a, b, c)
    for i in list(range(0, 20000, 97)) + list(range(0, 5000, 41)):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        lo = np.float32(float(exact))  # (float(Fraction) rounds correctly to fp64; the candidates around it decide the fp32 rounding exactly)
        cands = [np.nextafter(lo, np.float32(-np.inf)), lo, np.nextafter(lo, np.float32(np.inf))]
        best = min(cands, key=lambda v: (abs(Fraction(float(v)) - exact), int(v.view(np.int32)) & 1))
        assert got[i] == best, (i, got[i], best)


def test_the_float32_restatement_stays_within_the_measured_figure():
    worst = C.measure()
    print(f"float32 restatement against the fp64 oracle: |dout| / max(|s|, |b L|) {worst:.4g} (REF_OUT {C.REF_OUT})")
    assert worst <= C.REF_OUT and C.TOL_OUT == 4 * C.REF_OUT


def test_the_cases_are_what_they_claim():
    lens = sorted({len(s) for c in CASES.values() for s in c["speech"]})
    assert set((0, 1, 239, 240, 241, 1023, 1024, 1025, 2051, 3333, 24000)) <= set(lens)
    assert {c["plan"]["lead"] for c in CASES.values()} >= {0, 1, 239, 241, 1000} and all(c["plan"]["S"] in (1, 2) and c["plan"]["pre"] in (0, 1, 3) and c["plan"]["post"] in (0, 1, 3)
                                                                                         for k, c in CASES.items() if k != "defaults")
    c = CASES["seam_tile_edge"]
    assert [len(b) - c["plan"]["xf"] for b in c["bed"]] == [1024 - 48, 1023, 1025] and len(CASES["seam_frame_edge"]["bed"][0]) - 48 == 4 * C.Q
    c = CASES["first_last_frames"]
    ref = C.oracle(c["speech"][0], c["bed"][0], c["plan"], 0.5)
    assert ref["act"][0] and ref["act"][-1] and not ref["act"].all()
    p = CASES["lengths0"]["plan"]
    x = C.speech(20000, 1, p)
    gaps = np.diff(np.flatnonzero(np.diff((x != 0).astype(int))))[0::2]   # (the row begins with a burst: the transitions are end, start, end, ..)
    hold, wide = (p["pre"] + p["post"]) * C.Q, (p["pre"] + p["post"] + 2 * p["S"]) * C.Q
    assert any(g < hold for g in gaps) and any(hold < g < wide for g in gaps) and any(g > wide for g in gaps), "the gaps straddle the hold and hold plus smoothing"
    from chatterbox_amd import ops
    d = ops.check_bed((np.zeros(8, np.float32), 24000))
    assert {k: d[k] for k in C.DEFAULT_PLAN} == C.DEFAULT_PLAN, "the `defaults` case is ops.BED_DEFAULTS in samples and frames"


# ----------------------------------------------------------------------------- C ABI
def test_the_entries_are_declared_exported_bound_and_emulated_without_a_version_step():
    from chatterbox_amd import _lib, ops
    import harness
    hdr = open(os.path.join(ROOT, "include", "cbx.h")).read()
    lib = ctypes.CDLL(os.path.join(ROOT, "chatterbox_amd", "libcbx_hip.so"))
    emu = harness.load_emu()
    for entry, nargs in ENTRIES.items():
        assert re.search(rf"^int {entry}\(", hdr, re.M) and hasattr(lib, entry) and entry in _lib._SIGS and hasattr(emu, entry)
        assert len(_lib._SIGS[entry][0]) == len(re.search(rf"^int {entry}\((.*?)\);", hdr, re.M | re.S).group(1).split(",")) == nargs
    assert "#define CBX_ABI_VERSION 16" in hdr and _lib.lib.cbx_abi_version() == 16 and _lib.ABI_VERSION == 16 and emu.cbx_abi_version() == 16, "new functions only: no version step"
    block = hdr[hdr.index("---- music bed"): hdr.index("int cbx_wave_duck_level_f32(")]
    assert "reference has no counterpart" in block and all(ref in block for ref in ("tts.py:272", "mtl_tts.py:352", "tts_turbo.py:320"))
    assert "-22 before any launch" in block and "fmaf((bed'(i) * e) * g[i], L, s'[i])" in block and "ceil(max_r N_r / 240) + 4 * ceil(max_r N_r / 1024)" in block
    src = open(os.path.join(ROOT, "chatterbox_amd", "csrc", "wave_duck.hip")).read()
    assert "tts.py:272" in src and f"DK_Q = {ops.BED_FRAME}" in src and f"DK_HOLD_MAX = {ops.BED_HOLD_MAX}" in src and f"DK_S_MAX = {ops.BED_S_MAX}" in src \
        and f"DK_FADE_MAX = {ops.BED_FADE_MAX}" in src
    assert all(callable(getattr(ops, n)) for n in ("check_bed", "bed_len", "wave_duck", "wave_duck_level"))


def test_descriptor_errors_return_a_status_and_a_message():
    """the product library on host buffers: every refusal comes before a launch"""
    from chatterbox_amd import _lib, ops
    C.check_refusals(_lib.lib, ops, CPU, None, run_good=False)


# ----------------------------------------------------------------------------- the kernels on the SIMT emulator
@pytest.fixture(scope="module")
def emu():
    import build_emu
    if not os.path.exists(build_emu.CLANG):
        pytest.skip("ROCm's clang++ (x86 host compiler of the emulator build) is not installed")
    import harness
    with harness.emulated() as lib:
        yield lib


@pytest.mark.parametrize("mis", range(4))
@pytest.mark.parametrize("name", sorted(CASES))
def test_a_case_against_the_oracle(emu, name, mis):
    from chatterbox_amd import ops
    C.run_case(ops, name, CASES[name], mis)


@pytest.mark.parametrize("check", ["check_nan_row", "check_determinism", "check_gain_null", "check_ducking", "check_many_rows", "check_level"])
def test_a_property_of_the_definition(emu, check):
    from chatterbox_amd import ops
    getattr(C, check)(ops)


def test_the_emulated_entries_refuse_the_same_descriptors_and_ops_checks_its_arguments(emu):
    from chatterbox_amd import ops
    C.check_refusals(emu, ops, CPU, None)
    p = C.plan()
    out, st = ops.wave_duck([torch.zeros(0), torch.zeros(0)], None, p, gain=torch.tensor([0.5, 0.25]))
    assert [o.numel() for o in out] == [0, 0] and st.tolist() == [[0.5, 0.0, 0.0, 0.0], [0.25, 0.0, 0.0, 0.0]], "every output row empty: no launch"
    b = torch.from_numpy(C.bed(700, 1))
    out, st = ops.wave_duck([None], [b], C.plan(lead=300, tail=200, fi=0, fo=0))
    assert out[0].numel() == 500 == ops.bed_len(0, C.plan(lead=300, tail=200)) and torch.equal(out[0], b[:500]) and st.tolist() == [[1.0, 0.0, 3.0, float(b[:500].abs().max())]], "no speech: the bed alone"
    x = torch.from_numpy(C.speech(1276, 3, p))
    out, st = ops.wave_duck([x[:600], x[600:]], [b[:300], b[300:]], p)
    assert out[0].untyped_storage().data_ptr() == out[1].untyped_storage().data_ptr() != x.untyped_storage().data_ptr() and out[1].data_ptr() - out[0].data_ptr() == 2400
    with pytest.raises(ValueError, match="different allocations"):
        ops.wave_duck([torch.zeros(8), torch.zeros(8)], None, p)
    with pytest.raises(ValueError, match="bed rows"):
        ops.wave_duck([x], [b, b], p)
    with pytest.raises(ValueError, match="lengths"):
        ops.wave_duck([x], [b], p, out=[torch.zeros(5)])
    with pytest.raises(ValueError, match="limit_window"):
        ops.wave_duck([x], [b], dict(p, S=0))
    with pytest.raises(Exception, match="wave_duck"):
        ops.wave_duck([x], [b[:90]], p)   # a looped source no longer than 2 xf: the entry's refusal
    with pytest.raises(ValueError, match="levels"):
        ops.wave_duck_level(torch.zeros(2, 4, dtype=torch.float64), torch.zeros(2, 4, dtype=torch.float64), [-12.0])


# ----------------------------------------------------------------------------- ops.check_bed
def test_check_bed():
    from chatterbox_amd import ops
    wav = (np.zeros(100, np.float32), 24000)
    assert ops.check_bed(None) is None
    assert ops.BED_DEFAULTS == dict(level=-12.0, duck=-9.0, threshold=-40.0, pre=0.10, post=0.30, ramp=0.25, lead=0.0, tail=0.0, fade_in=0.02, fade_out=0.5, loop=True, loop_fade=0.1)
    assert "UNMEASURED" in ops.check_bed.__doc__
    d = ops.check_bed(wav)
    assert d["audio"] is wav and {k: v for k, v in d.items() if k != "audio"} == dict(level=-12.0, duck=-9.0, threshold=-40.0, lead=0, tail=0, fi=480, fo=12000, xf=2400, pre=10, post=30, S=12, loop=True)
    assert ops.check_bed("music.wav")["audio"] == "music.wav" and ops.check_bed((b"\0\0" * 8, 8000, "s16", 2))["xf"] == 2400
    d = ops.check_bed(dict(audio=wav, level=-20, duck=0, threshold=-30.5, pre=0, post=2, ramp=0.02, lead=1.5, tail=0.25, fade_in=0, fade_out=1, loop=False, loop_fade=0))
    assert {k: v for k, v in d.items() if k != "audio"} == dict(level=-20.0, duck=0.0, threshold=-30.5, lead=36000, tail=6000, fi=0, fo=24000, xf=0, pre=0, post=200, S=1, loop=False)
    assert ops.check_bed(dict(audio=wav, ramp=2.0))["S"] == 100 == ops.BED_S_MAX and ops.bed_len(1000, d) == 43000
    for bad, err in ((5, TypeError), (True, TypeError), (dict(level=-12), TypeError), (dict(audio=wav, volume=3), TypeError), (dict(audio=None), TypeError),
                     (dict(audio=wav, level="loud"), TypeError), (dict(audio=wav, duck=True), TypeError), (dict(audio=wav, loop=1), TypeError), ((wav[0], 24000.0), TypeError),
                     (dict(audio=wav, duck=1), ValueError), (dict(audio=wav, duck=-61), ValueError), (dict(audio=wav, level=float("nan")), ValueError),
                     (dict(audio=wav, threshold=1), ValueError), (dict(audio=wav, pre=2.5), ValueError), (dict(audio=wav, post=-0.1), ValueError),
                     (dict(audio=wav, ramp=0), ValueError), (dict(audio=wav, ramp=3), ValueError), (dict(audio=wav, lead=-1), ValueError), (dict(audio=wav, tail=float("inf")), ValueError),
                     (dict(audio=wav, fade_in=1.5), ValueError), (dict(audio=wav, fade_out=-1), ValueError), (dict(audio=wav, loop_fade=2), ValueError),
                     ((wav[0], 0), ValueError), ((b"\0" * 3, 8000, "s16"), ValueError)):
        with pytest.raises(err, match="bed"):
            ops.check_bed(bad)


# ----------------------------------------------------------------------------- the public classes over the recording engines (nothing is launched)
BED = (np.full(5000, 0.25, np.float32), 24000)


def _record_bed(monkeypatch, log):
    """the two launches of the bed step as recorders; the stand-in lays `lead` / `tail` samples of 0.5 round the speech and adds 100 to it"""
    from chatterbox_amd import ops

    def level(stats_s, stats_b, lv):
        log.append(("level", stats_s.clone(), stats_b.clone(), lv))
        return torch.tensor([0.125])

    def duck(speech_rows, bed_rows, plan, gain=None, out=None):
        log.append(("bed", [r.clone() for r in speech_rows], [r.clone() for r in bed_rows], plan, gain))
        w = torch.cat([torch.full((plan["lead"],), 0.5), speech_rows[0] + 100.0, torch.full((plan["tail"],), 0.5)])
        return [w], torch.tensor([[0.125, 7.0, 9.0, 0.75]], dtype=torch.float64)
    monkeypatch.setattr(ops, "wave_duck_level", level)
    monkeypatch.setattr(ops, "wave_duck", duck)


@pytest.mark.parametrize("cls_name,extra,lang", KINDS)
def test_generate_dialogue_lays_the_bed_behind_the_mix_ahead_of_loudness_limit_watermark_and_format(cls_name, extra, lang, monkeypatch):
    m, eng = _model(cls_name)
    voices = _voices()
    log = []
    _record(monkeypatch, log)
    _record_bed(monkeypatch, log)
    base, seg0 = m.generate_dialogue(SCRIPT, voices, **_lang_kw(lang), max_chars=14, seed=11, return_segments=True)
    calls0 = _norm(eng.calls)
    assert [e[0] for e in log] == ["mix"] and m.last_bed is None
    log.clear(), eng.calls.clear()
    same, seg1 = m.generate_dialogue(SCRIPT, voices, **_lang_kw(lang), max_chars=14, seed=11, return_segments=True, bed=None)
    assert [e[0] for e in log] == ["mix"] and torch.equal(same, base) and seg1 == seg0 and m.last_bed is None
    assert _norm(eng.calls) == calls0, "bed=None records exactly the calls of today"
    log.clear(), eng.calls.clear()
    m.watermarker = _Mark(log)
    wav, seg = m.generate_dialogue(SCRIPT, voices, **_lang_kw(lang), max_chars=14, seed=11, return_segments=True, loudness=-19, true_peak=-1.5, sample_rate=16000, encoding="s16",
                                   bed=dict(audio=BED, lead=0.5, tail=0.25, level=-15))
    assert all("bed" not in j and not {"loudness", "true_peak", "format"} & set(j) for j in _jobs(eng.calls)), "the jobs never carry the bed"
    assert _norm(eng.calls) == calls0
    assert [e[0] for e in log] == ["mix", "loudness", "loudness", "level", "bed", "loudness", "limit", "watermark", "format"]
    assert log[1][2:4] == (None, None) and len(log[1][1]) == 1 and torch.equal(log[1][1][0], base[0]), "the speech is measured over the mix before the bed, measure only"
    assert log[2][2:4] == (None, None) and torch.equal(log[2][1][0], torch.from_numpy(BED[0])), "the bed over its whole source"
    assert log[3][3] == -15.0 and float(log[3][1][0, 0]) == -30.0
    assert torch.equal(log[4][1][0], base[0]) and torch.equal(log[4][2][0], torch.from_numpy(BED[0])) and log[4][3]["lead"] == 12000 and log[4][3]["tail"] == 6000 and log[4][4].tolist() == [0.125]
    summed = torch.cat([torch.full((12000,), 0.5), base[0] + 100.0, torch.full((6000,), 0.5)])
    assert log[5][2] == [-19.0] and log[5][3] is None and torch.equal(log[5][1][0], summed), "meter and limiter see speech plus bed"
    assert log[6][2] == [-1.5] and torch.equal(log[6][1][0], summed)
    assert np.array_equal(log[7][1], summed.numpy() * 0.5) and torch.equal(log[8][1][0], summed * 0.5 * 2.0) and wav.dtype == torch.int16
    assert m.last_bed == dict(gain=0.125, speech_lufs=-30.0, bed_lufs=-30.0, ducked=7, frames=9, peak=0.75)
    fl = lambda v: -(-v * 2 // 3)
    assert [(s["start"], s["stop"]) for s in seg] == [(fl(a + 12000), fl(a + 12000 + 3840)) for a in STARTS], "the segments shift by lead, ahead of the format's mapping"
    assert [(s["src_start"], s["src_stop"]) for s in seg] == [(s["src_start"], s["src_stop"]) for s in seg0]
    log.clear()
    m.watermarker = None
    wav = m.generate_dialogue(SCRIPT, voices, **_lang_kw(lang), max_chars=14, seed=11, bed=BED)
    assert [e[0] for e in log] == ["mix", "loudness", "loudness", "level", "bed"] and torch.equal(wav[0], base[0] + 100.0) and wav.shape == (1, TOTAL)
    m.generate_dialogue(SCRIPT, voices, **_lang_kw(lang), max_chars=14, seed=11)
    assert m.last_bed is None, "a call without a bed clears the record"


@pytest.mark.parametrize("cls_name,extra,lang", KINDS)
def test_generate_long_lays_the_bed_in_the_visit_of_the_loudness_step_and_shifts_segments(cls_name, extra, lang, monkeypatch):
    m, eng = _model(cls_name)
    log = []
    _record(monkeypatch, log)
    _record_bed(monkeypatch, log)
    base, seg0 = m.generate_long(LONG_TEXT, *lang, max_chars=14, seed=11, return_segments=True)
    calls0 = _norm(eng.calls)
    assert log == []
    eng.calls.clear()
    same = m.generate_long(LONG_TEXT, *lang, max_chars=14, seed=11, bed=None)
    assert log == [] and torch.equal(same, base) and _norm(eng.calls) == calls0, "bed=None is the call without it"
    eng.calls.clear()
    m.watermarker = _Mark(log)
    wav, seg = m.generate_long(LONG_TEXT, *lang, max_chars=14, seed=11, return_segments=True, loudness=-19, true_peak=-1.5, encoding="s16", bed=dict(audio=BED, lead=0.1))
    assert all("bed" not in j for j in _jobs(eng.calls)) and _norm(eng.calls) == calls0
    assert [e[0] for e in log] == ["loudness", "loudness", "level", "bed", "loudness", "limit", "watermark", "format"]
    summed = torch.cat([torch.full((2400,), 0.5), base[0] + 100.0])
    assert torch.equal(log[0][1][0], base[0]) and torch.equal(log[3][1][0], base[0]) and torch.equal(log[4][1][0], summed) and torch.equal(log[5][1][0], summed)
    assert [(s["start"], s["stop"]) for s in seg] == [(s["start"] + 2400, s["stop"] + 2400) for s in seg0] and m.last_bed["ducked"] == 7
    log.clear()
    m.watermarker = None
    wav = m.generate_long(LONG_TEXT, *lang, max_chars=14, seed=11, bed=BED)
    assert [e[0] for e in log] == ["loudness", "loudness", "level", "bed"] and torch.equal(wav[0], base[0] + 100.0)
    log.clear()
    wav = m.generate_long(LONG_TEXT, *lang, max_chars=14, seed=11, bed=BED, loudness=-20)
    assert [e[0] for e in log] == ["loudness", "loudness", "level", "bed", "normalize"] and torch.equal(log[4][1][0], base[0] + 100.0)


def test_bad_beds_raise_at_the_call_before_the_engine_or_the_voice_analysis_is_touched_and_the_stream_does_not_take_one(monkeypatch, tmp_path):
    from chatterbox_amd import api
    touched = []
    for cls_name, extra, lang in KINDS:
        m, eng = _model(cls_name)
        monkeypatch.setattr(m, "prepare_conditionals", lambda *a, **k: touched.append("voice"))
        monkeypatch.setattr(m, "_analyse", lambda *a, **k: touched.append("voice"))
        voices = dict(_voices(), c="voice.wav")
        for value, err in ((5, TypeError), (dict(audio=BED, loud=1), TypeError), (dict(audio=BED, duck=3), ValueError), (dict(audio=BED, ramp=float("nan")), ValueError),
                           ((BED[0], "fast"), TypeError), (dict(level=-3), TypeError)):
            for call in (lambda: m.generate_dialogue(SCRIPT + [("c", "Hi.")], voices, **_lang_kw(lang), bed=value),
                         lambda: m.generate_long("a. b.", *lang, audio_prompt_path="voice.wav", bed=value)):
                with pytest.raises(err, match="bed"):
                    call()
        for value in ((np.zeros(0, np.float32), 24000), dict(audio=(np.zeros(4800, np.float32), 24000), loop_fade=0.1), str(tmp_path / "missing.wav")):
            for call in (lambda: m.generate_dialogue(SCRIPT + [("c", "Hi.")], voices, **_lang_kw(lang), bed=value),
                         lambda: m.generate_long("a. b.", *lang, audio_prompt_path="voice.wav", bed=value)):
                with pytest.raises((ValueError, OSError), match="bed|missing"):
                    call()
        with pytest.raises(ValueError, match="loudness"):
            m.generate_long("a. b.", *lang, loudness=-3, bed=5)   # the order of validation: loudness first
        with pytest.raises(TypeError, match="does not take bed"):
            m.generate_long_stream("a.", *lang, bed=BED)
        assert inspect.signature(m.generate_long_stream).parameters["bed"].default is None
        for name in ("generate_long", "generate_dialogue"):
            assert inspect.signature(getattr(m, name)).parameters["bed"].default is None
        assert inspect.signature(m.generate_dialogue).parameters["bed"].kind is inspect.Parameter.KEYWORD_ONLY
        for name in ("generate", "generate_batch", "generate_stream"):
            assert "bed" not in inspect.signature(getattr(m, name)).parameters
            with pytest.raises(TypeError, match="bed"):
                getattr(m, name)(["a."] if name == "generate_batch" else "a.", *([list(lang)] if name == "generate_batch" and lang else lang), bed=BED)
        assert eng.calls == [] and touched == []
    assert all("bed" not in inspect.signature(getattr(api.ChatterboxVC, n)).parameters for n in ("generate", "generate_batch", "generate_stream"))
    doc = api.ChatterboxTTS.generate_dialogue.__doc__
    assert "NOT\n        bounded" in doc and "true_peak=-1 is recommended" in doc and "UNMEASURED" in doc and "last_bed" in doc
