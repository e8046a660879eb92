"""CPU (-m "not gpu"): the output formats -- the NumPy filter design against scipy.signal.firwin, the fp64 restatement of the definition against
scipy.signal.resample_poly, cbx_wave_format_f32 on the SIMT emulator against the oracle (wave_format_common.py: bound, lengths, encodings, splits, sentinels), its C ABI
and descriptor errors, ops.check_format, and the plumbing of sample_rate= / encoding= on the public classes over the recording engines of test_seeded_rng_host.py
and test_wave_join_host.py (read-only imports; nothing is launched there)."""
import ctypes
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

import wave_format_common as C  # noqa: E402
from test_seeded_rng_host import _FakeEngine, _FakeSerialEngine, _tts  # noqa: E402  (read-only import: the recording engines)
from test_wave_join_host import CHUNKS, LONG_TEXT, _LongEngine, _LongSerial  # noqa: E402  (read-only import: the engines that know a joined piece)

CPU = torch.device("cpu")
LENGTHS = (1, 7, 479, 480, 1931)


# ----------------------------------------------------------------------------- the definition
@pytest.mark.parametrize("rate", C.RESAMPLED)
def test_the_numpy_design_is_scipys_and_the_table_is_its_phases(rate):
    """fp64: both evaluate the same closed form (sinc, Kaiser window through a Bessel I0 series, unit gain at 0) with a few hundred roundings of 2^-53 each, on
    values of at most U / max(U, D) <= 1.84: 1e-13 of the largest tap is three orders above that and six below the fp32 rounding of the table."""
    from chatterbox_amd import ops
    U, D, hl, h = C.scipy_design(rate)
    f = ops.wave_filter(rate)
    assert (f["U"], f["D"], f["hl"]) == (U, D, hl) and f["T"] == -(-(2 * hl + 1) // U) == C.taps(rate) and f["H"] == -(-2 * hl // U)
    assert f["h"].dtype == np.float64 and f["h"].shape == h.shape and np.abs(f["h"] - h).max() <= 1e-13 * np.abs(h).max()
    tab = f["tab"]
    assert tab.dtype == np.float32 and tab.shape == (U, f["T"]) and 21 <= f["T"] <= 61 and tab.size <= 3234 and tab.flags["C_CONTIGUOUS"]
    for p in range(U):
        for j in range(f["T"]):
            i = p + j * U
            assert tab[p, j] == (np.float32(f["h"][i]) if i <= 2 * hl else 0.0)
    assert ops.formatted_len(1931, rate) == C.out_len(1931, rate) and ops.formatted_len(0, rate) == 0


def test_the_identity_rate_has_no_filter():
    from chatterbox_amd import ops
    f = ops.wave_filter(24000)
    assert (f["U"], f["D"], f["hl"], f["T"], f["H"]) == (1, 1, 0, 1, 0) and ops.formatted_len(777, 24000) == ops.formatted_len(777, None) == 777
    assert ops.WAVE_RATES == (8000, 16000, 22050, 24000, 32000, 44100, 48000)
    with pytest.raises(ValueError, match="sample_rate"):
        ops.wave_filter(11025)


@pytest.mark.parametrize("rate", C.RESAMPLED)
def test_the_restatement_is_resample_poly(rate):
    from scipy.signal import resample_poly
    from chatterbox_amd import ops
    U, D = C.ratio(rate)
    for n in LENGTHS:
        x = C.signal("uniform", n, n).astype(np.float64)
        y64 = resample_poly(x, U, D)
        for h in (None, ops.wave_filter(rate)["h"]):   # scipy's design, and the product's
            y, S = C.restate(x, rate, h)
            assert y.shape == y64.shape == (C.out_len(n, rate),) and np.abs(y - y64).max() <= 1e-12, (rate, n)
            assert np.all(S >= np.abs(y) - 1e-12)


def test_the_g711_tables_are_the_codecs():
    """spot values of ITU-T G.711 (mu-law: 0 -> 0xFF, full scale -> 0x80 / 0x00; A-law: 0 -> 0xD5, -1 -> 0x55, full scale -> 0xAA / 0x2A) and the
    symmetries of both tables; where the interpreter still has audioop, the whole tables"""
    t = C.g711_tables()
    mu, al = t["mulaw"], t["alaw"]
    assert mu.shape == al.shape == (65536,) and mu.dtype == al.dtype == np.uint8
    at = lambda tab, s: int(tab[s + 32768])
    assert [at(mu, s) for s in (0, 32767, -32768)] == [0xFF, 0x80, 0x00] and [at(al, s) for s in (0, -1, 32767, -32768)] == [0xD5, 0x55, 0xAA, 0x2A]
    s = np.arange(0, 32768)
    assert np.array_equal(al[s + 32768] ^ 0x80, al[-s - 1 + 32768]), "A-law: s and -s - 1 differ in the sign bit alone"
    assert len(set(mu.tolist())) == 255 and len(set(al.tolist())) == 256, "every code is used (mu-law has no negative zero from a two's-complement sample)"
    try:
        import audioop
    except ImportError:
        return
    pcm = np.arange(-32768, 32768).astype("<i2").tobytes()
    assert audioop.lin2ulaw(pcm, 2) == mu.tobytes() and audioop.lin2alaw(pcm, 2) == al.tobytes()


# ----------------------------------------------------------------------------- C ABI
def test_entry_point_is_declared_exported_and_bound():
    from chatterbox_amd import _lib, ops
    hdr = open(os.path.join(ROOT, "include", "cbx.h")).read()
    lib = ctypes.CDLL(os.path.join(ROOT, "chatterbox_amd", "libcbx_hip.so"))
    assert re.search(r"^int cbx_wave_format_f32\(", hdr, re.M) and hasattr(lib, "cbx_wave_format_f32") and "cbx_wave_format_f32" in _lib._SIGS
    assert len(_lib._SIGS["cbx_wave_format_f32"][0]) == len(re.search(r"^int cbx_wave_format_f32\((.*?)\);", hdr, re.M | re.S).group(1).split(","))
    assert "#define CBX_ABI_VERSION 16" in hdr and _lib.lib.cbx_abi_version() == 16 and _lib.ABI_VERSION == 16, "a new function only: no version step"
    assert "leaves this to its caller" in hdr and "vc.py:104" in open(os.path.join(ROOT, "chatterbox_amd", "csrc", "wave_format.hip")).read()
    assert callable(ops.wave_format) and callable(ops.WaveFormatStream) and callable(ops.formatted_len) and callable(ops.check_format)


def test_descriptor_errors_return_a_status_and_a_message():
    """the product library on host buffers: every refusal comes before a launch"""
    from chatterbox_amd import _lib, ops
    C.check_refusals(_lib.lib, ops, CPU, None, run_good=False)


# ----------------------------------------------------------------------------- the kernel on the SIMT emulator
@pytest.fixture(scope="module")
def emu():
    import build_emu
    if not os.path.exists(build_emu.CLANG):
        pytest.skip("ROCm's clang++ (x86 host compiler of the emulator build) is not installed")
    import harness
    with harness.emulated() as lib:
        yield lib


@pytest.mark.parametrize("rate", C.RATES)
@pytest.mark.parametrize("name,aligned", [("A", False), ("A", True), ("b", False), ("C", False)])
def test_wave_format_on_the_emulator(emu, name, aligned, rate):
    """checks (a), (b: lengths) and (c) at n <= 5000; set C (4097 samples) spans several workgroups per row at every rate"""
    from chatterbox_amd import ops
    assert max(n for n, _ in C.SETS[name]) <= 5000
    C.check_one_shot(ops, CPU, name, rate, aligned)


def test_the_cases_the_shapes_are_chosen_for_are_what_they_claim():
    C.what_the_sets_cover()
    for rate in C.RATES:
        assert C.out_len(4097, rate) > 2 * 256


def test_identity_rate_s16_on_the_emulator(emu):
    from chatterbox_amd import ops
    x, expect = C.tie_cases()
    assert np.array_equal(C.quantise(x, "s16"), expect)
    got = ops.wave_format([torch.from_numpy(x)], dict(sample_rate=24000, encoding="s16"))[0]
    assert got.dtype == torch.int16 and np.array_equal(got.numpy(), expect)
    same = ops.wave_format([torch.from_numpy(x)], None)[0]
    assert same.dtype == torch.float32 and np.array_equal(same.numpy().view(np.uint32), x.view(np.uint32))


@pytest.mark.parametrize("rate", [8000, 22050, 48000, 24000])
@pytest.mark.parametrize("k", range(len(C.SPLITS)))
def test_any_split_concatenates_to_the_one_shot_output_on_the_emulator(emu, k, rate):
    from chatterbox_amd import ops
    for enc in ("f32", "mulaw"):
        got = C.check_split(ops, CPU, k, rate, enc)
    if k == 0:
        assert all(o.numel() == 0 for o in got[1][5:]) and all(o.numel() == 0 for o in got[2]), "a row gives nothing after its final push; an empty row nothing at all"


def test_a_stream_that_is_never_final_holds_back_the_outputs_whose_taps_are_missing(emu):
    """not final: exactly the outputs floor(((N - 1) U - hl) / D) + 1 of include/cbx.h, each equal to the one-shot output of the longer signal"""
    from chatterbox_amd import ops
    x = torch.from_numpy(C.signal("uniform", 2000, 5))
    for rate in (8000, 44100):
        f, fmt = ops.wave_filter(rate), dict(sample_rate=rate, encoding="f32")
        st = ops.WaveFormatStream(1, fmt, CPU)
        a = st.push([x[:700]], [False])[0].clone()
        b = st.push([x[700:1500]], [False])[0].clone()
        count = lambda N: max(0, ((N - 1) * f["U"] - f["hl"]) // f["D"] + 1)
        assert a.numel() == count(700) and a.numel() + b.numel() == count(1500) and (st.n0, st.m0) == ([1500], [count(1500)])
        whole = ops.wave_format([x], fmt)[0]
        assert torch.equal(torch.cat([a, b]), whole[: count(1500)])


@pytest.mark.parametrize("rate", [8000, 22050, 48000])
def test_positions_past_two_to_the_32_on_the_emulator(emu, rate):
    from chatterbox_amd import ops
    C.check_large_positions(ops, CPU, rate)


def test_nothing_is_written_outside_the_rows_on_the_emulator(emu):
    from chatterbox_amd import ops
    for rate, enc in ((8000, "mulaw"), (48000, "s16"), (22050, "f32"), (24000, "alaw")):
        C.check_sentinels(ops, CPU, rate, enc)


def test_emulated_entry_refuses_the_same_descriptors_and_runs_the_good_one(emu):
    from chatterbox_amd import ops
    C.check_refusals(emu, ops, CPU, None)


def test_wrapper_refuses_bad_rows(emu):
    from chatterbox_amd import ops
    big, fmt = torch.zeros(2, 960), dict(sample_rate=8000, encoding="s16")
    with pytest.raises(ValueError, match="different allocations"):
        ops.wave_format([big[0], torch.zeros(960)], fmt)
    with pytest.raises(ValueError, match="unit stride"):
        ops.wave_format([big[0, ::2]], fmt)
    with pytest.raises(ValueError, match="rows"):
        ops.wave_format([], fmt)
    with pytest.raises(ValueError, match="sample_rate"):
        ops.wave_format([big[0]], dict(sample_rate=8001))
    with pytest.raises(ValueError, match="push"):
        ops.WaveFormatStream(2, fmt, CPU).push([big[0]], [True])


# ----------------------------------------------------------------------------- check_format
def test_check_format():
    from chatterbox_amd import ops
    for rate, enc in ((None, None), (24000, None), (None, "f32"), (24000, "f32")):
        assert ops.check_format(rate, enc) is None, "the default format is no format"
    assert ops.check_format(8000, None) == dict(sample_rate=8000, encoding="f32") and ops.check_format(None, "mulaw") == dict(sample_rate=24000, encoding="mulaw")
    for rate in ops.WAVE_RATES:
        for enc in ops.WAVE_ENCODINGS:
            fmt = ops.check_format(rate, enc)
            assert fmt == (None if (rate, enc) == (24000, "f32") else dict(sample_rate=rate, encoding=enc)) and ops.check_format_arg(fmt) == fmt
    for rate, err in ((True, TypeError), (8000.0, TypeError), ("8000", TypeError), (11025, ValueError), (0, ValueError), (-8000, ValueError)):
        with pytest.raises(err, match="sample_rate"):
            ops.check_format(rate, "s16")
    for enc, err in ((1, TypeError), (b"s16", TypeError), ("pcm16", ValueError), ("S16", ValueError), ("", ValueError)):
        with pytest.raises(err, match="encoding"):
            ops.check_format(8000, enc)
    assert ops.check_format_arg(None) is None and ops.check_format_arg(dict(encoding="f32")) is None and ops.check_format_arg(dict(sample_rate=16000)) == dict(sample_rate=16000, encoding="f32")
    for bad, err in (("s16", TypeError), ((8000, "s16"), TypeError), (dict(rate=8000), ValueError), (dict(sample_rate=8000, encoding="s16", dither=True), ValueError)):
        with pytest.raises(err, match="format"):
            ops.check_format_arg(bad)


# ----------------------------------------------------------------------------- the public classes over the recording engines (nothing is launched)
KINDS = [("ChatterboxTTS", ()), ("ChatterboxMultilingualTTS", ("en",)), ("ChatterboxTurboTTS", ())]
FMT = dict(sample_rate=16000, encoding="s16")


def _jobs(calls):
    return [j for kind, kw in calls for j in (kw["jobs"] if kind == "pipelined" else [kw])]


class _Mark:
    """a stand-in watermarker: doubles the waveform, and records that it saw 24 kHz float32"""

    def __init__(self, log):
        self.log = log

    def apply_watermark(self, wav, sample_rate):
        assert wav.dtype == np.float32 and sample_rate == 24000
        self.log.append(("watermark", wav.copy()))
        return wav * 2.0


@pytest.mark.parametrize("cls_name,lang", KINDS)
def test_the_default_call_passes_no_new_key(cls_name, lang):
    from chatterbox_amd import api
    eng = _FakeEngine() if cls_name != "ChatterboxTurboTTS" else _FakeSerialEngine()
    m = _tts(getattr(api, cls_name), eng)
    m.max_batch = 2
    outs = [m.generate("aaaa.", *lang), m.generate("aaaa.", *lang, sample_rate=None, encoding=None), m.generate("aaaa.", *lang, sample_rate=24000, encoding="f32")]
    outs += m.generate_batch(["x.", "yy.", "zzz."], *lang, sample_rate=24000)
    assert all("format" not in j for j in _jobs(eng.calls)) and len(eng.calls) >= 4
    assert all(w.dtype == torch.float32 and w.dim() == 2 and w.shape[0] == 1 for w in outs)
    a, b = eng.calls[0][1], eng.calls[1][1]
    assert {k: v for k, v in a.items() if k != "text_tokens"} == {k: v for k, v in b.items() if k != "text_tokens"}


@pytest.mark.parametrize("cls_name,lang", KINDS)
def test_a_format_reaches_the_engine_once_per_job_and_the_result_is_what_the_engine_returned(cls_name, lang):
    from chatterbox_amd import api
    eng = _FakeEngine() if cls_name != "ChatterboxTurboTTS" else _FakeSerialEngine()
    m = _tts(getattr(api, cls_name), eng)
    m.max_batch = 2
    w = m.generate("aaaa.", *lang, sample_rate=16000, encoding="s16")
    (kind, kw), = eng.calls
    assert kind == "synthesize" and kw["format"] == FMT and w.shape == (1, 3)
    eng.calls.clear()
    out = m.generate_batch(["x.", "yy.", "zzz.", "wwww.", "v" * 9 + "."], *lang, sample_rate=16000, encoding="s16", seeds=[1, 2, 3, 4, 5])
    jobs = _jobs(eng.calls)
    assert len(jobs) == 3 and all(j["format"] == FMT for j in jobs) and len(out) == 5 and m.sr == 24000
    eng.calls.clear()
    m.generate_batch(["x.", "yy."], *lang, encoding="alaw")
    assert [j["format"] for j in _jobs(eng.calls)] == [dict(sample_rate=24000, encoding="alaw")]


@pytest.mark.parametrize("cls_name,lang", KINDS)
def test_with_a_watermarker_the_engine_gets_no_format_and_the_conversion_follows_the_watermark(cls_name, lang, monkeypatch):
    from chatterbox_amd import api, ops
    eng = _FakeEngine() if cls_name != "ChatterboxTurboTTS" else _FakeSerialEngine()
    m = _tts(getattr(api, cls_name), eng)
    log = []
    m.watermarker = _Mark(log)
    monkeypatch.setattr(ops, "wave_format", lambda rows, fmt: log.append(("format", [r.clone() for r in rows], fmt)) or [torch.arange(2, dtype=torch.int16)])
    w = m.generate("aaaa.", *lang, sample_rate=16000, encoding="s16")
    assert all("format" not in j for j in _jobs(eng.calls))
    assert [e[0] for e in log] == ["watermark", "format"] and log[1][2] == FMT and len(log[1][1]) == 1
    assert torch.equal(log[1][1][0], torch.from_numpy(log[0][1] * 2.0)), "the conversion takes the watermarked 24 kHz waveform"
    assert w.dtype == torch.int16 and w.tolist() == [[0, 1]]
    log.clear(), eng.calls.clear()
    out = m.generate_batch(["x.", "yy.", "zzz."], *lang, sample_rate=16000, encoding="s16")
    assert all("format" not in j for j in _jobs(eng.calls)) and [e[0] for e in log] == ["watermark", "format"] * 3 and all(o.dtype == torch.int16 for o in out)
    log.clear()
    assert m.generate("aaaa.", *lang).dtype == torch.float32 and [e[0] for e in log] == ["watermark"], "the default format converts nothing"


@pytest.mark.parametrize("cls_name,lang", KINDS)
@pytest.mark.parametrize("marked", [False, True])
def test_generate_long_converts_the_whole_once_and_counts_segments_in_output_samples(cls_name, lang, marked, monkeypatch):
    from chatterbox_amd import api, ops
    eng = _LongEngine() if cls_name != "ChatterboxTurboTTS" else _LongSerial()
    m = _tts(getattr(api, cls_name), eng)
    base_wav, base = m.generate_long(LONG_TEXT, *lang, max_chars=14, seed=11, return_segments=True)
    eng.calls.clear()
    log = []
    if marked:
        m.watermarker = _Mark(log)
    monkeypatch.setattr(ops, "wave_format", lambda rows, fmt: log.append(("format", [r.clone() for r in rows], fmt)) or
                        [torch.zeros(ops.formatted_len(rows[0].numel(), fmt["sample_rate"]), dtype=torch.uint8)])
    wav, seg = m.generate_long(LONG_TEXT, *lang, max_chars=14, seed=11, return_segments=True, sample_rate=8000, encoding="mulaw")
    assert all("format" not in j for j in _jobs(eng.calls)), "the jobs of generate_long never carry the format"
    assert [e[0] for e in log] == (["watermark", "format"] if marked else ["format"])
    rows = log[-1][1]
    assert len(rows) == 1 and torch.equal(rows[0], base_wav[0] * (2.0 if marked else 1.0)) and log[-1][2] == dict(sample_rate=8000, encoding="mulaw")
    up = lambda s: -(-s // 3)   # 8000 / 24000: ceil(s / 3)
    assert wav.dtype == torch.uint8 and wav.shape == (1, up(base_wav.shape[1])) == (1, seg[-1]["stop"]), "the last stop is the length"
    assert [s["text"] for s in seg] == CHUNKS
    for s, b in zip(seg, base):
        assert (s["start"], s["stop"]) == (up(b["start"]), up(b["stop"])) and (s["src_start"], s["src_stop"]) == (b["src_start"], b["src_stop"]) == (480, 4320)


def test_bad_formats_raise_before_the_engine_is_called():
    from chatterbox_amd import api
    for cls_name, lang in KINDS:
        eng = _LongEngine()
        m = _tts(getattr(api, cls_name), eng)
        for kw, err, name in ((dict(sample_rate=11025), ValueError, "sample_rate"), (dict(sample_rate=True), TypeError, "sample_rate"), (dict(sample_rate=8000.0), TypeError, "sample_rate"),
                              (dict(encoding="pcm"), ValueError, "encoding"), (dict(encoding=16), TypeError, "encoding")):
            for call in (lambda: m.generate("a.", *lang, **kw), lambda: m.generate_batch(["a.", "b."], *lang, **kw), lambda: m.generate_stream("a.", *lang, **kw),
                         lambda: m.generate_long("a. b.", *lang, **kw)):
                with pytest.raises(err, match=name):
                    call()
        assert eng.calls == []
    vc = api.ChatterboxVC.__new__(api.ChatterboxVC)
    vc.engine, vc.ref_dict, vc.watermarker, vc.analyzer = _FakeSerialEngine(), {}, None, None
    for call in (lambda: vc.generate(s3_tokens=[1, 2], sample_rate=11025), lambda: vc.generate_batch(s3_tokens=[[1, 2]], encoding="pcm"),
                 lambda: vc.generate_stream(s3_tokens=[1, 2], sample_rate=44000)):
        with pytest.raises(ValueError, match="sample_rate|encoding"):
            call()


# ----------------------------------------------------------------------------- streams
class _StreamEngine(_FakeSerialEngine):
    """yields the rounds it was built with, and records the keywords of the call"""

    def __init__(self, rounds):
        super().__init__()
        self.rounds = rounds

    def synthesize_stream(self, text_tokens, t3_conds, gen_ref, **kw):
        self.calls.append(("stream", kw))
        yield from self.rounds


def _rounds(pieces, wrap=lambda w: w):
    return [dict(wavs=[wrap(w)], final=[k == len(pieces) - 1], n_tokens=[0], tokens=[None]) for k, w in enumerate(pieces)]


@pytest.mark.parametrize("cls_name,lang", KINDS)
def test_generate_stream_hands_the_format_to_the_engine_and_passes_its_pieces_on(cls_name, lang):
    from chatterbox_amd import api
    pieces = [torch.arange(5, dtype=torch.int16), torch.zeros(0), torch.arange(3, dtype=torch.int16)]
    eng = _StreamEngine(_rounds(pieces))
    m = _tts(getattr(api, cls_name), eng)
    got = list(m.generate_stream("aaaa.", *lang, sample_rate=16000, encoding="s16"))
    assert eng.calls[0][1]["format"] == FMT and [g.tolist() for g in got] == [[[0, 1, 2, 3, 4]], [[0, 1, 2]]] and all(g.dtype == torch.int16 for g in got)
    eng.calls.clear()
    eng.rounds = _rounds([torch.ones(4), torch.ones(2)])
    got = list(m.generate_stream("aaaa.", *lang))
    assert "format" not in eng.calls[0][1] and [g.shape for g in got] == [(1, 4), (1, 2)] and all(g.dtype == torch.float32 for g in got)


def test_generate_stream_with_a_watermarker_converts_its_pieces_through_one_stream_state(emu):
    """the engine gets no format; every piece is watermarked at 24 kHz and pushed through ONE ops.WaveFormatStream (on the emulator here), so the pieces add up to
    ops.wave_format of the watermarked whole; an empty final round still flushes"""
    from chatterbox_amd import api, ops
    x = torch.from_numpy(C.signal("uniform", 1700, 9))
    for tail in (x[1200:], torch.zeros(0)):
        pieces = [x[:700], torch.zeros(0), x[700:1200], tail]
        eng = _StreamEngine(_rounds(pieces))
        m = _tts(api.ChatterboxTTS, eng)
        log = []
        m.watermarker = _Mark(log)
        fmt = dict(sample_rate=8000, encoding="mulaw")
        got = list(m.generate_stream("aaaa.", **fmt))
        assert "format" not in eng.calls[0][1] and [e[0] for e in log] == ["watermark"] * (3 if tail.numel() else 2)
        whole = ops.wave_format([torch.cat(pieces) * 2.0], fmt)[0]
        assert all(g.dim() == 2 and g.shape[0] == 1 and g.numel() for g in got) and torch.equal(torch.cat(got, 1)[0], whole)


# ----------------------------------------------------------------------------- the engines
def test_vocode_converts_on_the_stream_of_the_waveforms(monkeypatch):
    """ChatterboxEngine.vocode over stand-in stages on the CPU: format=None (or the default format) makes no ops.wave_format call; with a format the cut views go to
    ONE ops.wave_format call; with a join as well the join writes into a zeroed buffer of its capacity and the conversion takes that buffer"""
    from chatterbox_amd import engine, ops, synth
    eng = engine.ChatterboxEngine.__new__(engine.ChatterboxEngine)
    eng.dev, eng.last_timing = CPU, {}
    eng.flow = type("Flow", (), {"precision": 1, "inference": lambda self, tok, lens, ref, **kw: torch.ones(tok.shape[0], 2 * tok.shape[1], 80)})()
    eng.hift = type("Hift", (), {"precision": 1, "inference": staticmethod(lambda mel, lens=None, **kw: (torch.arange(mel.shape[0] * 480 * mel.shape[1], dtype=torch.float32).view(mel.shape[0], -1), None))})()
    calls = []
    monkeypatch.setattr(ops, "wave_format", lambda rows, fmt: calls.append(("format", rows, fmt)) or ["converted"] * len(rows))
    monkeypatch.setattr(ops, "wave_join", lambda rows, **kw: calls.append(("join", rows, kw)) or dict(out=kw.get("out"), rec="rec", n=[r.numel() for r in rows]))
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: None)
    ref = synth.s3gen_ref(n_prompt_tokens=6)
    st = [synth.speech_tokens(n, seed=k) for k, n in enumerate((12, 5, 9))]
    base, _ = eng.vocode(st, ref, drop_last_token=True)
    for fmt in (None, dict(sample_rate=24000), dict(encoding="f32")):
        same, _ = eng.vocode(st, ref, drop_last_token=True, format=fmt)
        assert calls == [] and all(torch.equal(a, b) for a, b in zip(same, base))
    got, mel = eng.vocode(st, ref, drop_last_token=True, format=dict(sample_rate=48000, encoding="s16"))
    assert got == ["converted"] * 3 and len(calls) == 1 and calls[0][2] == dict(sample_rate=48000, encoding="s16")
    assert all(torch.equal(a, b) for a, b in zip(calls[0][1], base)) and len({r.untyped_storage().data_ptr() for r in calls[0][1]}) == 1
    calls.clear()
    piece, _ = eng.vocode(st, ref, drop_last_token=True, join=dict(gaps=[5, 0, 7]), format=dict(sample_rate=8000, encoding="alaw"))
    assert [c[0] for c in calls] == ["join", "format"] and piece["formatted"] == "converted" and piece["format"] == dict(sample_rate=8000, encoding="alaw")
    buf = calls[0][2]["out"]
    assert buf.shape == (sum(w.numel() for w in base) + 12,) and float(buf.abs().max()) == 0.0 and calls[1][1][0] is buf
    for bad, err in ((dict(sample_rate=11025), ValueError), ("s16", TypeError)):
        with pytest.raises(err, match="format"):
            eng.vocode(st, ref, format=bad)
    assert len(calls) == 2


def test_checked_job_validates_the_format():
    from chatterbox_amd import engine
    job = dict(text_tokens=[torch.zeros(3)])
    assert "format" not in engine._checked_job(dict(job, format=None)) and "format" not in engine._checked_job(dict(job, format=dict(sample_rate=24000, encoding="f32")))
    assert engine._checked_job(dict(job, format=dict(sample_rate=8000)))["format"] == dict(sample_rate=8000, encoding="f32")
    with pytest.raises(ValueError, match="format"):
        engine._checked_job(dict(job, format=dict(sample_rate=8000, encoding="opus")))
    with pytest.raises(TypeError, match="format"):
        engine._checked_job(dict(job, format="mulaw"))
