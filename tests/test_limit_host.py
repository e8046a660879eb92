"""Host tests (no GPU) of the true-peak limiter: the oracle's own anchors, cbx_wave_limit_f32 on the SIMT emulator against the NumPy oracle of limit_common.py
(tolerances and their reasons there), the C ABI and its refusals, ops.check_true_peak, and the true_peak= keyword of the engines and of every public class over
the recording engines of the existing host tests."""
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

import limit_common as C  # noqa: E402
from test_loudness_host import KINDS, _VCEngine, _jobs, _stand_in_engine  # noqa: E402  (read-only import: the stand-ins of the loudness tests)
from test_seeded_rng_host import _FakeEngine, _FakeSerialEngine, _tts  # noqa: E402  (read-only import: the recording engines)
from test_wave_join_host import LONG_TEXT, _LongEngine, _LongSerial  # noqa: E402  (read-only import: the engines that know a joined piece)

CPU = torch.device("cpu")
ENTRY = "cbx_wave_limit_f32"
CASES = C.cases()


# ----------------------------------------------------------------------------- the definition
def test_the_tables_of_ops_are_the_oracles():
    from chatterbox_amd import ops
    f = ops.true_peak_filter()
    assert (f["U"], f["hl"], f["T"]) == (C.U, C.HL, C.T) == (4, 40, 21) and f["tab"].dtype == np.float32 and f["tab"].shape == (4, 21)
    assert np.abs(f["tab"].astype(np.float64) - C.taps()).max() <= 1e-7, "scipy.signal.firwin's design, restated in NumPy"
    assert ops.true_peak_filter() is f, "built once"
    for H in (1, 3, 120, 480):
        w = ops.limit_window(H)
        assert w.dtype == np.float32 and w.shape == (2 * H + 1,) and np.array_equal(w.astype(np.float64), C.window(H)) and abs(float(w.astype(np.float64).sum()) - 1.0) < 1e-6
    assert ops.limit_window(120) is ops.limit_window() and ops.LIMIT_LOOK == 120
    for bad, err in ((0, ValueError), (481, ValueError), (True, TypeError), (1.5, TypeError)):
        with pytest.raises(err, match="limit_window"):
            ops.limit_window(bad)


def test_the_oracle_reads_the_inter_sample_peak_and_holds_the_ceiling():
    x = C.inter_sample()
    ref = C.oracle(x, C.DB09)
    assert abs(np.abs(x).max() - np.sqrt(0.5)) < 1e-6 and 1.0 <= ref["stats"][0] < 1.02 and ref["stats"][1] < 1.0
    assert C.true_peak(ref["out"]) <= 0.9 * (1 + C.CEIL_PRE) and np.abs(ref["out"]).max() <= 0.9
    assert np.all(1.0 - (1.0 - ref["g"]) <= ref["c"] + 1e-15), "1 - s <= c in exact arithmetic: the min only absorbs rounding"


def test_the_float32_restatement_stays_within_the_measured_figures():
    dg, dout = C.measure()
    print(f"float32 restatement against the fp64 oracle: |dg| {dg:.4g} (REF_G {C.REF_G}), |dout| / max|u| {dout:.4g} (REF_OUT {C.REF_OUT})")
    assert dg <= C.REF_G and dout <= C.REF_OUT and C.TOL_G == 4 * C.REF_G and C.TOL_OUT == 4 * C.REF_OUT


# ----------------------------------------------------------------------------- C ABI
def test_the_entry_is_declared_exported_and_bound():
    from chatterbox_amd import _lib, ops
    import harness
    hdr = open(os.path.join(ROOT, "include", "cbx.h")).read()
    lib = ctypes.CDLL(os.path.join(ROOT, "chatterbox_amd", "libcbx_hip.so"))
    emu = harness.load_emu()
    assert re.search(rf"^int {ENTRY}\(", hdr, re.M) and hasattr(lib, ENTRY) and ENTRY in _lib._SIGS and hasattr(emu, ENTRY)
    assert len(_lib._SIGS[ENTRY][0]) == len(re.search(rf"^int {ENTRY}\((.*?)\);", hdr, re.M | re.S).group(1).split(",")) == 18
    assert "#define CBX_ABI_VERSION 16" in hdr and _lib.lib.cbx_abi_version() == 16 and _lib.ABI_VERSION == 16 and emu.cbx_abi_version() == 16, "new function only: no version step"
    src = open(os.path.join(ROOT, "chatterbox_amd", "csrc", "wave_limit.hip")).read()
    assert "The reference has no" in hdr and "tts.py:272" in hdr and "tts.py:272" in src
    assert "4 * R * ceil(max_r n_r / 1024)" in hdr, "the header states the workspace"
    assert all(callable(getattr(ops, n)) for n in ("true_peak_filter", "limit_window", "check_true_peak", "wave_true_peak", "wave_limit"))


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


def test_the_inter_sample_peak_is_limited(emu):
    from chatterbox_amd import ops
    C.check_inter_sample(ops)


def test_no_gain_vector_is_a_gain_of_ones(emu):
    from chatterbox_amd import ops
    C.check_gain_null(ops)


def test_measure_only_reads_the_same_true_peak_and_writes_nothing(emu):
    from chatterbox_amd import ops
    C.check_measure_only(ops)


def test_a_row_with_a_nan_sample(emu):
    from chatterbox_amd import ops
    C.check_nan_row(ops)


def test_the_result_does_not_depend_on_alignment_or_batch(emu):
    from chatterbox_amd import ops
    C.check_determinism(ops)


def test_a_table_that_is_not_the_products_takes_the_general_tap_loop(emu):
    from chatterbox_amd import ops
    C.check_other_table(emu, ops)


def test_the_emulated_entry_refuses_the_same_descriptors_and_ops_checks_its_arguments(emu):
    from chatterbox_amd import ops
    C.check_refusals(emu, ops, CPU, None)
    out, st = ops.wave_limit([torch.zeros(0), torch.zeros(0)], -1.0)
    assert [o.numel() for o in out] == [0, 0] and st.tolist() == [[0.0, 1.0, 0.0, 0.0]] * 2 and ops.wave_true_peak([torch.zeros(0)]).tolist() == [[0.0, 1.0, 0.0, 0.0]]
    x = torch.from_numpy(C.bursts(1276, 3))
    rows = [x[:600], x[600:]]
    out, st = ops.wave_limit(rows, [-1.0, None])
    assert out[0].untyped_storage().data_ptr() == out[1].untyped_storage().data_ptr() != x.untyped_storage().data_ptr(), "views of ONE new allocation"
    assert out[1].data_ptr() - out[0].data_ptr() == 2400 and torch.equal(out[1], rows[1]), "in the layout of the rows"
    with pytest.raises(ValueError, match="different allocations"):
        ops.wave_limit([torch.zeros(8), torch.zeros(8)], -1.0)
    with pytest.raises(ValueError, match="ceilings"):
        ops.wave_limit(rows, [-1.0])
    with pytest.raises(ValueError, match="limit_window"):
        ops.wave_limit(rows, -1.0, look=500)


# ----------------------------------------------------------------------------- ops.check_true_peak
def test_check_true_peak():
    from chatterbox_amd import ops
    assert ops.check_true_peak(None, 3) is None and ops.check_true_peak([None, None], 2) is None
    assert ops.check_true_peak(-1, 2) == [-1.0, -1.0] and ops.check_true_peak([-1, None, -2.5], 3) == [-1.0, None, -2.5] and ops.check_true_peak((-20, 0), 2) == [-20.0, 0.0]
    for bad, err in ((True, TypeError), ("-1", TypeError), ([-1, "x"], TypeError), ([-1, False], TypeError), ([-1], ValueError), (0.1, ValueError), (-20.1, ValueError),
                     (float("nan"), ValueError), ([-1, float("-inf")], ValueError)):
        with pytest.raises(err, match="true_peak"):
            ops.check_true_peak(bad, 2)
    with pytest.raises(ValueError, match="ceiling"):
        ops.check_true_peak(-30, 1, name="ceiling")


# ----------------------------------------------------------------------------- the public classes over the recording engines (nothing is launched)
@pytest.mark.parametrize("cls_name,lang", KINDS)
def test_the_default_call_passes_no_new_key(cls_name, lang):
    from chatterbox_amd import api
    eng = _FakeEngine() if cls_name != "ChatterboxTurboTTS" else _FakeSerialEngine()
    m = _tts(getattr(api, cls_name), eng)
    m.max_batch = 2
    m.generate("aaaa.", *lang), m.generate("aaaa.", *lang, true_peak=None)
    m.generate_batch(["x.", "yy.", "zzz."], *lang), m.generate_batch(["x.", "yy.", "zzz."], *lang, true_peak=[None, None, None])
    assert all("true_peak" not in j for j in _jobs(eng.calls)) and len(eng.calls) >= 4
    a, b = eng.calls[0][1], eng.calls[1][1]
    assert {k: v for k, v in a.items() if k != "text_tokens"} == {k: v for k, v in b.items() if k != "text_tokens"}, "true_peak=None records exactly the call of today"
    rest = eng.calls[2:]
    strip = lambda calls: [{k: v for k, v in j.items() if k != "text_tokens"} for j in _jobs(calls)]
    assert len(rest) % 2 == 0 and strip(rest[: len(rest) // 2]) == strip(rest[len(rest) // 2:]), "the batch without the keyword and with Nones record the same jobs"


@pytest.mark.parametrize("cls_name,lang", KINDS)
def test_a_ceiling_reaches_the_engine_and_a_list_travels_with_its_requests(cls_name, lang):
    from chatterbox_amd import api
    eng = _FakeEngine() if cls_name != "ChatterboxTurboTTS" else _FakeSerialEngine()
    m = _tts(getattr(api, cls_name), eng)
    m.max_batch = 2
    m.generate("aaaa.", *lang, true_peak=-1, loudness=-16)
    (kind, kw), = eng.calls
    assert kind == "synthesize" and kw["true_peak"] == -1.0 and kw["loudness"] == -16.0
    eng.calls.clear()
    lens = [9, 2, 5, 7, 30]
    peaks = [-1.0, None, -3.0, None, -6.0]
    out = m.generate_batch(["x" * (n - 1) + "." for n in lens], *lang, true_peak=peaks, seeds=[1, 2, 3, 4, 5])
    extra = 0 if cls_name == "ChatterboxTurboTTS" else 2
    of_len = {n + extra: t for n, t in zip(lens, peaks)}
    jobs = _jobs(eng.calls)
    assert [len(j["text_tokens"]) for j in jobs] == [2, 2, 1] and len(out) == 5
    for j in jobs:
        want = [of_len[int(t.numel())] for t in j["text_tokens"]]
        assert j.get("true_peak") == (want if any(v is not None for v in want) else None), "a sub-batch carries the ceilings of ITS requests, in its row order; none: no key"
    eng.calls.clear()
    m.generate_batch(["x.", "yy.", "zzz."], *lang, true_peak=-2)
    assert [j["true_peak"] for j in _jobs(eng.calls)] == [[-2.0] * len(j["text_tokens"]) for j in _jobs(eng.calls)]


class _Mark:
    def __init__(self, log):
        self.log = log

    def apply_watermark(self, wav, sample_rate):
        self.log.append(("watermark", wav.copy()))
        return wav * 2.0


@pytest.mark.parametrize("cls_name,lang", KINDS)
def test_generate_long_limits_the_whole_once_behind_the_loudness_ahead_of_the_watermark_and_the_conversion(cls_name, lang, monkeypatch):
    from chatterbox_amd import api, ops
    eng = _LongEngine() if cls_name != "ChatterboxTurboTTS" else _LongSerial()
    m = _tts(getattr(api, cls_name), eng)
    base = m.generate_long(LONG_TEXT, *lang, max_chars=14, seed=11)
    eng.calls.clear()
    log = []
    m.watermarker = _Mark(log)

    def loudness(rows, target=None, ceiling=1.0, fs=24000):
        log.append(("loudness", [r.clone() for r in rows], target, ceiling))
        return "stats", "gain"

    def limit(rows, ceilings_db, gain=None, look=120, out=None):
        log.append(("limit", [r.clone() for r in rows], ceilings_db, gain))
        return [rows[0] * 0.5], "limit stats"
    monkeypatch.setattr(ops, "wave_loudness", loudness)
    monkeypatch.setattr(ops, "wave_limit", limit)
    monkeypatch.setattr(ops, "wave_normalize", lambda *a, **k: pytest.fail("with a ceiling the gain is the limiter's pre-gain: wave_gain is not launched"))
    monkeypatch.setattr(ops, "wave_format", lambda rows, fmt: log.append(("format", [r.clone() for r in rows], fmt)) or [torch.zeros(2, dtype=torch.int16)])
    wav = m.generate_long(LONG_TEXT, *lang, max_chars=14, seed=11, loudness=-19, true_peak=-1.5, encoding="s16")
    assert all("loudness" not in j and "true_peak" not in j and "format" not in j for j in _jobs(eng.calls)), "the jobs of generate_long never carry the ceiling"
    assert [e[0] for e in log] == ["loudness", "limit", "watermark", "format"]
    assert log[0][2] == [-19.0] and log[0][3] is None, "the full gain: no sample-peak cap where the limiter follows"
    assert log[1][2] == [-1.5] and log[1][3] == "gain" and eng.last_loudness == "stats" and eng.last_limit == "limit stats"
    assert len(log[1][1]) == 1 and torch.equal(log[1][1][0], base[0]), "ONE signal: the assembled waveform"
    assert np.array_equal(log[2][1], base[0].numpy() * 0.5) and torch.equal(log[3][1][0], base[0] * 0.5 * 2.0) and wav.dtype == torch.int16
    log.clear()
    m.watermarker = None
    m.generate_long(LONG_TEXT, *lang, max_chars=14, seed=11, true_peak=-1.5)
    assert [e[0] for e in log] == ["limit"] and log[0][3] is None, "no target: no meter, no gain"


def test_bad_ceilings_raise_before_the_engine_is_called_and_streams_do_not_take_the_keyword():
    from chatterbox_amd import api
    for cls_name, lang in KINDS:
        eng = _LongEngine()
        m = _tts(getattr(api, cls_name), eng)
        for value, err in ((0.5, ValueError), (-21, ValueError), (True, TypeError), ("loud", TypeError), (float("nan"), ValueError)):
            for call in (lambda: m.generate("a.", *lang, true_peak=value), lambda: m.generate_batch(["a.", "b."], *lang, true_peak=value),
                         lambda: m.generate_long("a. b.", *lang, true_peak=value)):
                with pytest.raises(err, match="true_peak"):
                    call()
        for call in (lambda: m.generate("a.", *lang, true_peak=[-1.0]), lambda: m.generate_long("a. b.", *lang, true_peak=[-1.0])):
            with pytest.raises(TypeError, match="true_peak"):
                call()
        with pytest.raises(ValueError, match="true_peak"):
            m.generate_batch(["a.", "b."], *lang, true_peak=[-1.0])
        with pytest.raises(ValueError, match="loudness"):
            m.generate("a.", *lang, loudness=-3, true_peak="x")   # the order of validation: loudness first
        with pytest.raises(TypeError, match="true_peak"):
            m.generate("a.", *lang, true_peak="x", max_pause=-1)  # ... and true_peak ahead of the pauses
        for name in ("generate_stream", "generate_long_stream"):
            with pytest.raises(TypeError, match="true_peak"):
                getattr(m, name)("a.", *lang, true_peak=-1)
        assert "true_peak" not in inspect.signature(m.generate_stream).parameters
        # generate_long_stream's signature is generate_long's plus the ramp (an existing test pins that), so it lists the keyword -- and refuses anything but None
        assert inspect.signature(m.generate_long_stream).parameters["true_peak"].default is None
        with pytest.raises(TypeError, match="does not take true_peak"):
            m.generate_long_stream("a.", *lang, true_peak=-1)
        assert eng.calls == []
        for name in ("generate", "generate_batch", "generate_long"):
            assert inspect.signature(getattr(m, name)).parameters["true_peak"].default is None
    assert "dBTP" in api.ChatterboxTTS.generate.__doc__ and "true_peak" in api.ChatterboxTTS.generate.__doc__
    vc = api.ChatterboxVC.__new__(api.ChatterboxVC)
    vc.engine, vc.ref_dict, vc.watermarker, vc.analyzer = _VCEngine(), {}, None, None
    with pytest.raises(TypeError, match="true_peak"):
        vc.generate_stream(s3_tokens=[1, 2], true_peak=-1)
    with pytest.raises(ValueError, match="true_peak"):
        vc.generate(s3_tokens=[1, 2], true_peak=3)
    assert vc.engine.calls == []
    vc.generate(s3_tokens=[1, 2]), vc.generate(s3_tokens=[1, 2], true_peak=-2), vc.generate_batch(s3_tokens=[[1, 2], [3]], true_peak=[None, -4])
    vc.generate_batch(s3_tokens=[[1, 2], [3]], true_peak=[None, None])
    assert [kw.get("true_peak") for kw in vc.engine.calls] == [None, -2.0, [-4.0, None], None] and "true_peak" not in vc.engine.calls[0] and "true_peak" not in vc.engine.calls[3]


# ----------------------------------------------------------------------------- the engines
def test_vocode_limits_behind_the_loudness_ahead_of_the_format_and_refuses_a_join(monkeypatch):
    from chatterbox_amd import engine, ops, synth
    eng = _stand_in_engine()
    calls = []

    def loudness(rows, target=None, ceiling=1.0, fs=24000):
        calls.append(("loudness", [int(r.numel()) for r in rows], list(target), ceiling))
        return torch.full((len(rows), 4), float(len(calls)), dtype=torch.float64), torch.full((len(rows),), float(len(calls)))

    def limit(rows, ceilings_db, gain=None, look=120, out=None):
        calls.append(("limit", [r.clone() for r in rows], list(ceilings_db), None if gain is None else gain.clone()))
        return [r * 0.5 for r in rows], "limit stats"
    monkeypatch.setattr(ops, "wave_loudness", loudness)
    monkeypatch.setattr(ops, "wave_limit", limit)
    monkeypatch.setattr(ops, "wave_gain", lambda *a, **k: pytest.fail("wave_gain is not launched: the limiter applies the gain"))
    monkeypatch.setattr(ops, "wave_format", lambda rows, fmt: calls.append(("format", [r.clone() for r in rows], fmt)) or ["converted"] * len(rows))
    monkeypatch.setattr(ops, "wave_join", lambda rows, **kw: calls.append(("join", rows, kw)) or dict(out=kw.get("out"), rec="rec", n=[r.numel() for r in rows]))
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: None)
    ref = synth.s3gen_ref(n_prompt_tokens=6)
    st = [synth.speech_tokens(n, seed=k) for k, n in enumerate((12, 5, 9))]
    base, _ = eng.vocode(st, ref, drop_last_token=True)
    for none in (None, [None, None, None]):
        same, _ = eng.vocode(st, ref, drop_last_token=True, true_peak=none)
        assert calls == [] and eng.last_limit is None and all(torch.equal(a, b) for a, b in zip(same, base)), "None is the call without it"
    # a batch that mixes the two kinds: rows 0 (target + ceiling) and 2 (ceiling alone) get the uncapped meter, row 1 (target alone) the sample-peak cap
    got, _ = eng.vocode(st, ref, drop_last_token=True, loudness=[-5, -16, None], true_peak=[-1, None, -3], format=dict(encoding="s16"))
    n = [int(b.numel()) for b in base]
    assert [c[0] for c in calls] == ["loudness", "loudness", "limit", "format"]
    assert calls[0][1:] == ([n[1]], [-16.0], 1.0) and calls[1][1:] == ([n[0], n[2]], [-5.0, None], None)
    assert calls[2][2] == [-1.0, None, -3.0] and calls[2][3].tolist() == [2.0, 1.0, 2.0] and all(torch.equal(a, b) for a, b in zip(calls[2][1], base)), "ALL rows pass the one limiter launch"
    assert eng.last_loudness[:, 0].tolist() == [2.0, 1.0, 2.0] and eng.last_limit == "limit stats"
    assert all(torch.equal(a, b * 0.5) for a, b in zip(calls[3][1], base)) and got == ["converted"] * 3, "the format sees the limited signal"
    calls.clear()
    eng.vocode(st, ref, drop_last_token=True, loudness=[-5, None, None], true_peak=[-1, None, -3])
    assert [c[0] for c in calls] == ["loudness", "limit"] and calls[0][1:] == (n, [-5.0, None, None], None), "no row with a target alone: ONE meter call"
    calls.clear()
    eng.vocode(st, ref, drop_last_token=True, true_peak=-2)
    assert [c[0] for c in calls] == ["limit"] and calls[0][2] == [-2.0] * 3 and calls[0][3] is None, "a ceiling alone: limited, no gain"
    calls.clear()
    with pytest.raises(ValueError, match="true_peak together with join"):
        eng.vocode(st, ref, join=dict(gaps=[5, 0, 7]), true_peak=-1)
    with pytest.raises(ValueError, match="true_peak"):
        eng.vocode(st, ref, true_peak=[-1.0])
    assert calls == []
    eng.vocode(st, ref, join=dict(gaps=[5, 0, 7]), true_peak=None)
    assert [c[0] for c in calls] == ["join"]


def test_synthesize_and_the_jobs_of_the_throughput_schedule_check_the_keyword():
    from chatterbox_amd import engine
    job = dict(text_tokens=[torch.zeros(3), torch.zeros(2)])
    assert "true_peak" not in engine._checked_job(dict(job, true_peak=None)) and "true_peak" not in engine._checked_job(dict(job, true_peak=[None, None]))
    assert engine._checked_job(dict(job, true_peak=-1))["true_peak"] == [-1.0, -1.0] and engine._checked_job(dict(job, true_peak=[None, -9]))["true_peak"] == [None, -9.0]
    with pytest.raises(ValueError, match="true_peak together with join"):
        engine._checked_job(dict(job, true_peak=-1, join=dict(gaps=[0, 0])))
    with pytest.raises(ValueError, match="loudness together with join"):
        engine._checked_job(dict(job, loudness=-20, true_peak=-1, join=dict(gaps=[0, 0])))
    assert "join" in engine._checked_job(dict(job, true_peak=None, join=dict(gaps=[0, 0])))
    with pytest.raises(ValueError, match="true_peak"):
        engine._checked_job(dict(job, true_peak=[-1]))
    d = engine.check_delivery(2, loudness=-16, true_peak=[-1, None], warp=[None, dict(frames=7)])
    assert list(d.kw()) == ["loudness", "true_peak", "warp"] and d.peak == [-1.0, None] and engine.Delivery.OPTIONS[-2:] == ("true_peak", "warp")
    for cls in (engine.ChatterboxEngine, engine.TurboEngine):
        assert inspect.signature(cls.synthesize).parameters["true_peak"].default is None
        eng = cls.__new__(cls)
        eng.dev = CPU
        with pytest.raises(ValueError, match="true_peak together with join"):
            eng.synthesize([torch.zeros(3, dtype=torch.long)], {}, {}, true_peak=-1, join=dict(gaps=[0]))
    assert inspect.signature(engine.S3GenEngine.vocode).parameters["true_peak"].default is None
    for cls in (engine.S3GenEngine, engine.ChatterboxEngine, engine.TurboEngine):
        for name in ("vocode_stream", "synthesize_stream"):
            if hasattr(cls, name):
                assert "true_peak" not in inspect.signature(getattr(cls, name)).parameters, "a running limiter needs a carried look-ahead"
