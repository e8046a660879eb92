"""Host tests (no GPU) of long-form streaming with a running loudness: cbx_wave_loudness_push_f32 on the SIMT emulator -- BITWISE against the one-shot meter
after every push (loudness_push_common.run_split; the cases and their reasons there) --, its C ABI and refusals, api.long_stream_plan, and generate_long_stream of
every public class over the recording engines of test_wave_join_host.py (nothing is launched)."""
import ctypes
import inspect
import logging
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

import loudness_common as C  # noqa: E402
import loudness_push_common as P  # noqa: E402
from test_seeded_rng_host import _tts  # noqa: E402  (read-only import)
from test_wave_join_host import CHUNKS, LONG_TEXT, _LongEngine, _LongSerial  # noqa: E402  (read-only import: the engines that know a joined piece)

CPU = torch.device("cpu")
ENTRY = "cbx_wave_loudness_push_f32"


# ----------------------------------------------------------------------------- C ABI
def test_the_entry_is_declared_exported_bound_and_emulated_without_a_version_step():
    from chatterbox_amd import _lib, ops
    import harness
    hdr = open(os.path.join(ROOT, "include", "cbx.h")).read()
    lib = ctypes.CDLL(os.path.join(ROOT, "chatterbox_amd", "libcbx_hip.so"))
    emu = harness.load_emu()
    assert re.search(rf"^int {ENTRY}\(", hdr, re.M) and hasattr(lib, ENTRY) and ENTRY in _lib._SIGS and hasattr(emu, ENTRY)
    assert len(_lib._SIGS[ENTRY][0]) == len(re.search(rf"^int {ENTRY}\((.*?)\);", hdr, re.M | re.S).group(1).split(","))
    assert "#define CBX_ABI_VERSION 16" in hdr and _lib.lib.cbx_abi_version() == 16 and _lib.ABI_VERSION == 16 and emu.cbx_abi_version() == 16, "new functions only: no version step"
    block = hdr[hdr.index(f"/* {ENTRY}:"): hdr.index(f"int {ENTRY}(")]
    assert "tts_turbo.py:223-239" in block and "4 * R * max_r K_r" in block and "bit for bit" in block, "the header states the definition, the reference and the workspace"
    assert callable(ops.wave_loudness_push) and inspect.isclass(ops.WaveLoudnessStream)
    assert inspect.signature(ops.WaveLoudnessStream.__init__).parameters["seg_cap"].default == 4096 and "bit for bit" in ops.WaveLoudnessStream.__doc__


def test_descriptor_errors_return_a_status_and_a_message():
    """the product library on host buffers: every refusal comes before a launch"""
    from chatterbox_amd import _lib, ops
    P.check_push_refusals(_lib.lib, ops, CPU, None, run_good=False)


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
@pytest.mark.parametrize("split", sorted(P.SPLITS_ONE))
def test_one_row_in_pieces_is_the_one_shot_meter_bit_for_bit(emu, split, mis):
    from chatterbox_amd import ops
    P.run_split(ops, [P.short()], [P.SPLITS_ONE[split]], [(-23.0, None, -30.0)[mis % 3]], mis)


@pytest.mark.parametrize("mis", range(4))
def test_three_rows_with_their_own_pieces(emu, mis):
    """different lengths per push, a row that is empty in some pushes, a row that ends early; the target of row 1 is None: gain 1"""
    from chatterbox_amd import ops
    out = P.run_split(ops, [P.long(), P.short(), P.short()], P.SPLITS_THREE, P.TARGETS_THREE, mis)
    assert all(g[1] == 1.0 and st[1, 2] == 1.0 for st, g in out), "a target of None: measure only"
    assert out[-1][1][0] != 1.0 and out[-1][1][2] != 1.0


@pytest.mark.parametrize("mis", range(4))
def test_a_nan_in_the_second_piece_makes_the_peak_nan_and_the_gain_one_from_then_on(emu, mis):
    from chatterbox_amd import ops
    x = P.short()
    x[3000] = np.nan
    out = P.run_split(ops, [x, P.short()], [[2500, 2500, 7000, P.REST]] * 2, [-23.0, -23.0], mis, oracle=False)
    assert not np.isnan(out[0][0][0, 1]) and all(np.isnan(st[0, 1]) and st[0, 2] == 1.0 and g[0] == 1.0 for st, g in out[1:])
    assert not np.isnan(out[-1][0][1]).any() and out[-1][1][1] != 1.0, "the row beside it is measured as ever"


def test_growing_the_record_keeps_the_bits_and_the_entry_refuses_what_would_pass_seg_cap(emu):
    from chatterbox_amd import ops
    a = P.run_split(ops, [P.short()], [P.SPLITS_ONE["ragged"]], [-23.0], 1, seg_cap=2)
    b = P.run_split(ops, [P.short()], [P.SPLITS_ONE["ragged"]], [-23.0], 1)
    assert all(np.array_equal(x[0].view(np.int64), y[0].view(np.int64)) and np.array_equal(x[1].view(np.int32), y[1].view(np.int32)) for x, y in zip(a, b))
    meter = ops.WaveLoudnessStream(1, CPU, seg_cap=3)
    keep = meter.rec.clone()
    with pytest.raises(RuntimeError, match="wave_loudness_push"):
        ops.wave_loudness_push(meter, [torch.from_numpy(C.bursts(4 * P.HOP, 1))], -20.0)
    assert meter.n0 == [0] and meter.cur == 0 and torch.equal(meter.rec, keep), "-22: nothing written, the meter not advanced"
    meter.push([torch.from_numpy(C.bursts(4 * P.HOP, 1))], -20.0)
    assert meter.seg_cap >= 4 and meter.n0 == [4 * P.HOP]
    with pytest.raises(ValueError, match="rows"):
        meter.push([torch.zeros(4), torch.zeros(4)])


def test_the_emulated_entry_refuses_the_same_descriptors_and_runs_the_good_one(emu):
    from chatterbox_amd import ops
    P.check_push_refusals(emu, ops, CPU, None)


# ----------------------------------------------------------------------------- api.long_stream_plan
def _args(**kw):
    from chatterbox_amd import api
    return api._long_args(**dict(dict(max_chars=None, pause=0.15, paragraph_pause=0.4, trim_db=40.0, trim_pad=2, join_fade=240, seed=11, speed=1.25, cjk=False), **kw))


def test_long_stream_plan():
    from chatterbox_amd import api
    chunks = [(f"chunk {k}.", k in (3, 7)) for k in range(12)]
    a = _args()
    for mb in (1, 2, 5, 8, 100):
        assert api.long_stream_plan(chunks, mb, a, None, 2.0) == api.long_plan(chunks, mb, a), "first_batch=None IS long_plan"
    sizes = lambda plan: [len(j["chunks"]) for j in plan]
    assert sizes(api.long_stream_plan(chunks, 8, a, 1, 2.0)) == [1, 2, 4, 5]
    assert sizes(api.long_stream_plan(chunks, 2, a, 1, 2.0)) == [1, 2, 2, 2, 2, 2, 1], "max_batch caps the ramp"
    assert sizes(api.long_stream_plan(chunks, 8, a, 3, 1.0)) == [3, 3, 3, 3] and sizes(api.long_stream_plan(chunks, 8, a, 20, 2.0)) == [8, 4]
    assert sizes(api.long_stream_plan(chunks, 8, a, 1, 1.5)) == [1, 2, 3, 5, 1] and sizes(api.long_stream_plan(chunks, 100, a)) == [1, 2, 4, 5]
    assert sizes(api.long_stream_plan(chunks * 20, 1000, a, 1, 2.0)) == [1, 2, 4, 8, 16, 32, 64, 64, 49], "64 rows: the join's limit"
    whole = api.long_plan(chunks, 12, a)[0]
    for plan in (api.long_stream_plan(chunks, 8, a, 1, 2.0), api.long_stream_plan(chunks, 3, _args(seed=None, speed=1.0), 2, 1.3)):
        seeded = "seeds" in plan[0]
        ref = whole if seeded else api.long_plan(chunks, 12, _args(seed=None, speed=1.0))[0]
        assert [k for j in plan for k in j["chunks"]] == list(range(12)), "text order"
        assert [g for j in plan for g in j["join"]["gaps"]] == ref["join"]["gaps"]
        assert [(j["join"]["first"], j["join"]["last"]) for j in plan] == [(g == 0, g == len(plan) - 1) for g in range(len(plan))]
        assert all({k: v for k, v in j["join"].items() if k not in ("gaps", "first", "last")} == {k: v for k, v in ref["join"].items() if k not in ("gaps", "first", "last")} for j in plan)
        if seeded:
            assert [s for j in plan for s in j["seeds"]] == ref["seeds"] == [api.chunk_seed(11, k) for k in range(12)] and [s for j in plan for s in j["speed"]] == ref["speed"]
        else:
            assert all("seeds" not in j and "speed" not in j for j in plan)
    assert inspect.signature(api.long_plan).parameters.keys() == {"chunks", "max_batch", "a"}, "long_plan keeps its signature"


# ----------------------------------------------------------------------------- generate_long_stream over the recording engines (nothing is launched)
KINDS = [("ChatterboxTTS", ()), ("ChatterboxMultilingualTTS", ("en",)), ("ChatterboxTurboTTS", ())]


def _jobs(calls):
    return [j for kind, kw in calls for j in (kw["jobs"] if kind == "pipelined" else [kw])]


def _same(a, b):
    """two recorded values, tensors compared by value"""
    if torch.is_tensor(a) or torch.is_tensor(b):
        return torch.is_tensor(a) and torch.is_tensor(b) and a.dtype == b.dtype and torch.equal(a, b)
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return type(a) is type(b) and len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return a is b or a == b


class _Counting(_LongEngine):
    """_LongEngine that counts the jobs its throughput schedule has yielded and notes that its generator was closed"""

    def __init__(self):
        super().__init__()
        self.yielded, self.closed = 0, False

    def synthesize_pipelined(self, jobs, **kw):
        try:
            for r in super().synthesize_pipelined(jobs, **kw):
                self.yielded += 1
                yield r
        finally:
            self.closed = True


def _model(cls_name, eng=None):
    from chatterbox_amd import api
    eng = eng or (_LongEngine() if cls_name != "ChatterboxTurboTTS" else _LongSerial())
    m = _tts(getattr(api, cls_name), eng)
    m.max_batch = 2
    return m, eng


@pytest.mark.parametrize("cls_name,lang", KINDS)
def test_first_batch_none_hands_the_engine_the_jobs_of_generate_long_and_the_segments_agree(cls_name, lang):
    m, eng = _model(cls_name)
    kw = dict(max_chars=14, seed=11, speed=1.25, temperature=0.7, top_p=0.9, return_segments=True)
    wav, seg = m.generate_long(LONG_TEXT, *lang, **kw)
    want = list(eng.calls)
    eng.calls.clear()
    got = list(m.generate_long_stream(LONG_TEXT, *lang, **kw, first_batch=None))
    assert _same(eng.calls, want), "exactly generate_long's engine calls"
    assert len(got) == 3 and all(w.dim() == 2 and w.shape[0] == 1 and w.dtype == torch.float32 for w, _ in got)
    assert torch.equal(torch.cat([w for w, _ in got], dim=1), wav) and _same([s for _, ss in got for s in ss], seg)
    assert [[s["text"] for s in ss] for _, ss in got] == [CHUNKS[:2], CHUNKS[2:4], CHUNKS[4:]]
    plain = list(m.generate_long_stream(LONG_TEXT, *lang, max_chars=14, seed=11, first_batch=None))
    assert all(torch.is_tensor(w) for w in plain) and len(plain) == 3, "without return_segments: the waveforms alone"
    eng.calls.clear()
    ramp = list(m.generate_long_stream(LONG_TEXT, *lang, **kw))
    assert [len(j["text_tokens"]) for j in _jobs(eng.calls)] == [1, 2, 2] and _same([s for _, ss in ramp for s in ss], seg), "the ramp moves no sample: the fake pieces do not depend on the batch"
    assert torch.equal(torch.cat([w for w, _ in ramp], dim=1), wav)


@pytest.mark.parametrize("cls_name,lang", KINDS[:2])
def test_the_stream_is_lazy_and_closing_it_closes_the_engines_schedule(cls_name, lang):
    m, eng = _model(cls_name, _Counting())
    it = m.generate_long_stream(LONG_TEXT, *lang, max_chars=14, seed=11)
    assert inspect.isgenerator(it) and eng.calls == [] and eng.yielded == 0, "nothing runs before the first next()"
    first = next(it)
    assert first.shape[0] == 1 and eng.yielded == 1 and len(eng.calls) == 1 and not eng.closed, "one job has left the engine"
    it.close()
    assert eng.yielded == 1 and eng.closed, "close() runs the schedule's finally; no further job"
    with pytest.raises(StopIteration):
        next(it)


def test_the_serial_engine_runs_a_batch_per_piece():
    m, eng = _model("ChatterboxTurboTTS")
    it = m.generate_long_stream(LONG_TEXT, max_chars=14, seed=11)
    next(it)
    assert [k for k, _ in eng.calls] == ["synthesize"]
    next(it)
    assert [k for k, _ in eng.calls] == ["synthesize"] * 2
    it.close()
    assert len(eng.calls) == 2


@pytest.mark.parametrize("cls_name,lang", KINDS)
def test_every_argument_is_validated_at_the_call(cls_name, lang, monkeypatch):
    from chatterbox_amd import api
    m, eng = _model(cls_name)
    touched = []
    monkeypatch.setattr(type(m), "prepare_conditionals", lambda self, *a, **k: touched.append("voice"))
    bad = [(dict(first_batch=0), ValueError, "first_batch"), (dict(first_batch=1.0), TypeError, "first_batch"), (dict(first_batch=True), TypeError, "first_batch"),
           (dict(first_batch="1"), TypeError, "first_batch"), (dict(batch_growth=0.5), ValueError, "batch_growth"), (dict(batch_growth=float("nan")), ValueError, "batch_growth"),
           (dict(batch_growth=float("inf")), ValueError, "batch_growth"), (dict(batch_growth="2"), TypeError, "batch_growth"), (dict(batch_growth=True), TypeError, "batch_growth"),
           (dict(batch_growth=None), TypeError, "batch_growth"),
           (dict(max_chars=0), ValueError, "max_chars"), (dict(pause=-0.1), ValueError, "pause"), (dict(paragraph_pause=None), TypeError, "paragraph_pause"),
           (dict(trim_db=-3), ValueError, "trim_db"), (dict(trim_pad=1.0), TypeError, "trim_pad"), (dict(join_fade=-1), ValueError, "join_fade"), (dict(seed=-1), ValueError, "seed"),
           (dict(speed=0.3), ValueError, "speed"), (dict(temperature="hot"), TypeError, "temperature"), (dict(top_p=float("nan")), ValueError, "top_p"),
           (dict(loudness=-4.0), ValueError, "loudness"), (dict(loudness=[-20.0]), TypeError, "loudness"), (dict(loudness=True), TypeError, "loudness"),
           (dict(sample_rate=12345), ValueError, "sample_rate"), (dict(sample_rate=16000.0), TypeError, "sample_rate"), (dict(encoding="mp3"), ValueError, "encoding")]
    for kw, err, name in bad:
        with pytest.raises(err, match=name):
            m.generate_long_stream(LONG_TEXT, *lang, audio_prompt_path="voice.wav", **kw)
    with pytest.raises(TypeError, match="text"):
        m.generate_long_stream(["a."], *lang, audio_prompt_path="voice.wav")
    if lang:
        with pytest.raises(ValueError, match="language"):
            m.generate_long_stream(LONG_TEXT, "xx", audio_prompt_path="voice.wav")
    assert eng.calls == [] and touched == [], "raised at the call, before the engine or the voice analysis is touched"
    it = m.generate_long_stream(LONG_TEXT, *lang, audio_prompt_path="voice.wav", first_batch=None, batch_growth=1)
    assert touched == ["voice"] and eng.calls == [], "the voice is prepared at the call, the engine waits for next()"
    it.close()
    long_sig, stream_sig = (inspect.signature(getattr(type(m), n)).parameters for n in ("generate_long", "generate_long_stream"))
    assert list(stream_sig)[: len(long_sig)] == list(long_sig) and all(stream_sig[k].default == long_sig[k].default for k in long_sig), "generate_long's arguments, same defaults"
    assert list(stream_sig)[len(long_sig):] == ["first_batch", "batch_growth"] and stream_sig["first_batch"].default == 1 and stream_sig["batch_growth"].default == 2.0
    assert "UNMEASURED" in api.ChatterboxTTS.generate_long_stream.__doc__ and "join_fade=0" in api.ChatterboxTTS.generate_long_stream.__doc__


@pytest.mark.parametrize("cls_name,lang", KINDS)
def test_one_warning_names_the_truncated_chunks_when_the_stream_ends(cls_name, lang, caplog):
    m, eng = _model(cls_name)
    extra = 0 if cls_name == "ChatterboxTurboTTS" else 2
    with caplog.at_level(logging.WARNING, logger="chatterbox_amd.api"):
        it = m.generate_long_stream(LONG_TEXT, *lang, max_chars=14)
        next(it)
        assert not [r for r in caplog.records if "generate_long_stream" in r.getMessage()]
        list(it)
    msgs = [r.getMessage() for r in caplog.records if "generate_long_stream" in r.getMessage()]
    cut = [k for k, c in enumerate(CHUNKS) if (len(c) + extra) % 2 == 0]
    assert len(msgs) == 1 and str(cut) in msgs[0] and "max_chars" in msgs[0]


class _Mark:
    def __init__(self, log):
        self.log = log

    def apply_watermark(self, wav, sample_rate):
        self.log.append(("watermark", wav.copy()))
        return wav * 2.0


@pytest.mark.parametrize("cls_name,lang", KINDS)
def test_a_piece_is_levelled_then_watermarked_then_converted_by_one_meter_and_one_converter(cls_name, lang, monkeypatch):
    from chatterbox_amd import ops
    m, eng = _model(cls_name)
    raw = list(m.generate_long_stream(LONG_TEXT, *lang, max_chars=14, seed=11, first_batch=None))
    eng.calls.clear()
    log = []
    m.watermarker = _Mark(log)

    class Meter:
        def __init__(self, R, device, *a, **k):
            log.append(("meter", R))

        def push(self, rows, target, ceiling=1.0):
            log.append(("loudness", [r.clone() for r in rows], target, ceiling))
            return f"stats{sum(1 for e in log if e[0] == 'loudness')}", "gain"

    class Conv:
        def __init__(self, B, fmt, device):
            log.append(("conv", B, fmt))

        def push(self, rows, final):
            log.append(("format", [r.clone() for r in rows], final))
            return [torch.zeros(2, dtype=torch.int16)]
    monkeypatch.setattr(ops, "WaveLoudnessStream", Meter)
    monkeypatch.setattr(ops, "WaveFormatStream", Conv)
    monkeypatch.setattr(ops, "wave_gain", lambda rows, gain: log.append(("gain", gain)) or rows[0].mul_(0.5))
    out = list(m.generate_long_stream(LONG_TEXT, *lang, max_chars=14, seed=11, first_batch=None, loudness=-19, sample_rate=16000, encoding="s16", return_segments=True))
    assert all("loudness" not in j and "format" not in j for j in _jobs(eng.calls)), "the jobs never carry the target or the format"
    assert [e[0] for e in log] == ["meter", "loudness", "gain", "watermark", "conv", "format"] + ["loudness", "gain", "watermark", "format"] * 2, "ONE meter, ONE converter"
    assert log[0] == ("meter", 1) and log[4] == ("conv", 1, dict(sample_rate=16000, encoding="s16")) and eng.last_loudness == "stats3"
    loud, marks, fmts = ([e for e in log if e[0] == k] for k in ("loudness", "watermark", "format"))
    for k in range(3):
        assert torch.equal(loud[k][1][0], raw[k][0]) and loud[k][2] == [-19.0] and loud[k][3] == 1.0, "the ungained 24 kHz piece enters the meter"
        assert np.array_equal(marks[k][1], raw[k][0].numpy() * 0.5) and torch.equal(fmts[k][1][0], raw[k][0] * 0.5 * 2.0) and fmts[k][2] == [k == 2]
    assert all(w.dtype == torch.int16 and w.shape == (1, 2) for w, _ in out)
    _, seg = m.generate_long(LONG_TEXT, *lang, max_chars=14, seed=11, return_segments=True)
    flat = [s for _, ss in out for s in ss]
    assert [(s["start"], s["stop"]) for s in flat] == [(ops.formatted_len(s["start"], 16000), ops.formatted_len(s["stop"], 16000)) for s in seg]
    assert [(s["src_start"], s["src_stop"]) for s in flat] == [(s["src_start"], s["src_stop"]) for s in seg]


@pytest.mark.parametrize("cls_name,lang", KINDS)
def test_the_default_arguments_touch_neither_meter_nor_converter(cls_name, lang, monkeypatch):
    from chatterbox_amd import ops
    m, eng = _model(cls_name)

    def never(*a, **k):
        raise AssertionError("loudness=None and the default format add no launch, upload or copy")
    for name in ("WaveLoudnessStream", "WaveFormatStream", "wave_gain", "wave_loudness_push", "wave_format", "wave_normalize"):
        monkeypatch.setattr(ops, name, never)
    assert len(list(m.generate_long_stream(LONG_TEXT, *lang, max_chars=14, sample_rate=24000, encoding="f32", loudness=None))) == 3


@pytest.mark.parametrize("cls_name,lang", KINDS)
def test_generate_generate_batch_and_generate_long_are_recorded_as_before(cls_name, lang):
    """the calls the three existing methods hand the engine do not know the new one: the same records before and after a stream ran on the same model"""
    m, eng = _model(cls_name)

    def record():
        eng.calls.clear()
        m.generate("aaaa.", *lang, seed=3)
        m.generate_batch(["x.", "yy.", "zzz."], *lang, seeds=[1, 2, 3])
        m.generate_long(LONG_TEXT, *lang, max_chars=14, seed=11)
        return list(eng.calls)
    before = record()
    list(m.generate_long_stream(LONG_TEXT, *lang, max_chars=14, seed=11))
    it = m.generate_long_stream(LONG_TEXT, *lang, max_chars=14, seed=11)
    next(it), it.close()
    assert _same(record(), before)
    kinds = [k for k, _ in before]
    assert kinds == (["synthesize", "pipelined", "pipelined"] if cls_name != "ChatterboxTurboTTS" else ["synthesize"] * 6)
    long_jobs = _jobs(before)[-3:]
    assert [len(j["text_tokens"]) for j in long_jobs] == [2, 2, 1] and all("join" in j for j in long_jobs)
