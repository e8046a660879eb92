"""Host tests (no GPU) of the loudness feature: the sine anchor of ITU-R BS.1770 / EBU Tech 3341 on the oracle and on the kernels, cbx_wave_loudness_f32 /
cbx_wave_gain_f32 on the SIMT emulator against the NumPy / SciPy oracle of loudness_common.py (tolerances and their reasons there), the C ABI and its refusals,
ops.check_loudness, and the loudness= keyword of the engines and of every public class over the recording engines of the existing host tests."""
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

import loudness_common as C  # noqa: E402
from test_seeded_rng_host import _FakeEngine, _FakeSerialEngine, _tts  # noqa: E402  (read-only import: the recording engines)
from test_wave_join_host import LONG_TEXT, _LongEngine, _LongSerial  # noqa: E402  (read-only import: the engines that know a joined piece)

CPU = torch.device("cpu")
ENTRIES = ("cbx_wave_loudness_f32", "cbx_wave_gain_f32")


# ----------------------------------------------------------------------------- the definition
def test_the_coefficients_of_ops_are_the_oracles_and_the_high_pass_has_its_double_pole():
    from chatterbox_amd import ops
    f = ops.loudness_filter(24000)
    (b1, a1), (b2, a2) = C.k_coefficients(24000)
    assert f["hop"] == 2400 and f["coef"].dtype == np.float64 and np.array_equal(f["coef"], np.concatenate([b1, a1[1:], b2, a2[1:]]))
    assert ops.loudness_filter(24000) is f, "built once per rate"
    poles = np.abs(np.roots(a2))
    assert np.allclose(poles, 0.9901, atol=1e-4), poles
    with pytest.raises(ValueError, match="fs"):
        ops.loudness_filter(22055)


def test_the_oracle_reads_the_sine_anchor():
    """997 Hz, full scale, 5 s: -3.01 LKFS (the Recommendation's value) within EBU Tech 3341's 0.1 LU; 20 dB down reads 20 LU less"""
    a, b = C.oracle(C.sine(5 * C.FS)), C.oracle(C.sine(5 * C.FS, amp=0.1))
    print(a, b)
    assert abs(a["L"] + 3.01) <= 0.1 and a["blocks"] == 47 and a["peak"] == 1.0
    assert abs((a["L"] - b["L"]) - 20.0) <= C.TOL_L


def test_the_bursts_put_blocks_on_both_sides_of_both_gates_and_none_near_one():
    for n in (25234, 72007):
        x = C.bursts(n, 10 + n)
        ref = C.oracle(x)
        assert ref["margin"] >= 1.0 and 0 < ref["blocks"] < max(0, n // 2400 - 3), (n, ref)


# ----------------------------------------------------------------------------- C ABI
def test_entry_points_are_declared_exported_and_bound():
    from chatterbox_amd import _lib, ops
    import harness
    hdr = open(os.path.join(ROOT, "include", "cbx.h")).read()
    lib = ctypes.CDLL(os.path.join(ROOT, "chatterbox_amd", "libcbx_hip.so"))
    emu = harness.load_emu()
    for name in ENTRIES:
        assert re.search(rf"^int {name}\(", hdr, re.M) and hasattr(lib, name) and name in _lib._SIGS and hasattr(emu, name)
        assert len(_lib._SIGS[name][0]) == len(re.search(rf"^int {name}\((.*?)\);", hdr, re.M | re.S).group(1).split(","))
    assert "#define CBX_ABI_VERSION 16" in hdr and _lib.lib.cbx_abi_version() == 16 and _lib.ABI_VERSION == 16 and emu.cbx_abi_version() == 16, "new functions only: no version step"
    src = open(os.path.join(ROOT, "chatterbox_amd", "csrc", "wave_loudness.hip")).read()
    assert "tts_turbo.py:223-239" in hdr and "tts_turbo.py:223-239" in src and "DESIGN CHOSEN" in src
    assert "6 * R * ceil(max_r n_r / hop)" in hdr, "the header states the workspace"
    assert all(callable(getattr(ops, n)) for n in ("loudness_filter", "check_loudness", "wave_loudness", "wave_gain", "wave_normalize"))


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


def test_the_kernels_read_the_sine_anchor(emu):
    from chatterbox_amd import ops
    x = C.sine(5 * C.FS)
    st, _ = C.run_case(ops, [x, C.sine(5 * C.FS, amp=0.1)], [None, None], 1)
    assert abs(st[0, 0] + 3.01) <= 0.1 and abs((st[0, 0] - st[1, 0]) - 20.0) <= C.TOL_L and st[0, 3] == 47


@pytest.mark.parametrize("mis", range(4))
def test_one_row_of_every_length_against_the_oracle(emu, mis):
    from chatterbox_amd import ops
    for k, n in enumerate(C.LENGTHS):
        C.run_case(ops, [C.bursts(n, 10 + n)], [C.TARGETS[k % 3]], mis)


@pytest.mark.parametrize("mis", range(4))
@pytest.mark.parametrize("g", range(len(C.GROUPS)))
def test_three_rows_against_the_oracle(emu, g, mis):
    from chatterbox_amd import ops
    C.run_case(ops, [C.bursts(n, 10 + n) for n in C.GROUPS[g]], [C.TARGETS[(g + r) % 3] for r in range(3)], mis)


def test_degenerate_rows_get_gain_one(emu):
    """a silent row, a row shorter than four hops, a row holding a NaN, a row whose target is NaN (None): gain exactly 1, the samples keep their bits"""
    from chatterbox_amd import ops
    bad = C.bursts(12000, 5)
    bad[5000] = np.nan
    sig = [np.zeros(12000, np.float32), C.bursts(9599, 6), bad, C.bursts(12000, 7)]
    st, g = C.run_case(ops, sig, [-20.0, -20.0, -20.0, None], 2)
    assert np.array_equal(g, np.ones(4, np.float32)) and np.array_equal(st[:, 2], np.ones(4))
    assert st[0, 0] == -np.inf and st[0, 1] == 0.0 and st[1, 0] == -np.inf and st[1, 3] == 0 and np.isnan(st[2, 1]) and np.isfinite(st[3, 0])


def test_the_ceiling_limits_the_gain_to_one_over_the_peak(emu):
    from chatterbox_amd import ops
    x = C.bursts(25234, 10 + 25234)
    ref = C.oracle(x, -10.0)
    assert 10.0 ** ((-10.0 - ref["L"]) / 20.0) * ref["peak"] > 1.0, "the case is what it claims: the plain gain would clip"
    st, g = C.run_case(ops, [x, x], [-10.0, -30.0], 3)
    assert g[0] == np.float32(1.0 / ref["peak"]) and st[1, 2] == pytest.approx(10.0 ** ((-30.0 - ref["L"]) / 20.0), rel=1e-9)
    st, g = C.run_case(ops, [x], [-10.0], 0, ceiling=None)
    assert st[0, 2] * ref["peak"] > 1.0, "no ceiling: the plain gain"


def test_wave_normalize_is_the_two_entries_and_the_emulated_entries_refuse_the_same_descriptors(emu):
    from chatterbox_amd import ops
    x = C.bursts(12000, 9)
    buf, rows, _ = C.padded_rows([x, x], 1)
    stats = ops.wave_normalize(rows, [-30.0, None])
    ref = C.oracle(x, -30.0)
    assert np.array_equal(rows[0].numpy(), x * ref["gain32"]) and np.array_equal(rows[1].numpy(), x) and abs(float(stats[0, 0]) - ref["L"]) <= C.TOL_L
    assert abs(C.oracle(rows[0].numpy())["L"] + 30.0) <= 1e-5
    assert ops.wave_normalize([torch.zeros(0), torch.zeros(0)], -20.0).tolist() == [[-np.inf, 0.0, 1.0, 0.0]] * 2
    C.check_refusals(emu, ops, CPU, None)
    with pytest.raises(ValueError, match="different allocations"):
        ops.wave_loudness([torch.zeros(8), torch.zeros(8)])
    with pytest.raises(ValueError, match="targets"):
        ops.wave_loudness(rows, [-20.0])


# ----------------------------------------------------------------------------- ops.check_loudness
def test_check_loudness():
    from chatterbox_amd import ops
    assert ops.check_loudness(None, 3) is None and ops.check_loudness([None, None], 2) is None
    assert ops.check_loudness(-16, 2) == [-16.0, -16.0] and ops.check_loudness([-16, None, -23.5], 3) == [-16.0, None, -23.5] and ops.check_loudness((-50, -5), 2) == [-50.0, -5.0]
    for bad, err in ((True, TypeError), ("-16", TypeError), ([-16, "x"], TypeError), ([-16, False], TypeError), ([-16], ValueError), (-4.9, ValueError), (-50.1, ValueError),
                     (float("nan"), ValueError), ([-16, float("-inf")], ValueError), (0, ValueError)):
        with pytest.raises(err, match="loudness"):
            ops.check_loudness(bad, 2)


# ----------------------------------------------------------------------------- the public classes over the recording engines (nothing is launched)
KINDS = [("ChatterboxTTS", ()), ("ChatterboxMultilingualTTS", ("en",)), ("ChatterboxTurboTTS", ())]


def _jobs(calls):
    return [j for kind, kw in calls for j in (kw["jobs"] if kind == "pipelined" else [kw])]


@pytest.mark.parametrize("cls_name,lang", KINDS)
def test_the_default_call_passes_no_new_key(cls_name, lang):
    from chatterbox_amd import api
    eng = _FakeEngine() if cls_name != "ChatterboxTurboTTS" else _FakeSerialEngine()
    m = _tts(getattr(api, cls_name), eng)
    m.max_batch = 2
    m.generate("aaaa.", *lang), m.generate("aaaa.", *lang, loudness=None)
    m.generate_batch(["x.", "yy.", "zzz."], *lang), m.generate_batch(["x.", "yy.", "zzz."], *lang, loudness=[None, None, None])
    assert all("loudness" not in j for j in _jobs(eng.calls)) and len(eng.calls) >= 4
    a, b = eng.calls[0][1], eng.calls[1][1]
    assert {k: v for k, v in a.items() if k != "text_tokens"} == {k: v for k, v in b.items() if k != "text_tokens"}


@pytest.mark.parametrize("cls_name,lang", KINDS)
def test_a_target_reaches_the_engine_and_a_list_travels_with_its_requests(cls_name, lang):
    from chatterbox_amd import api
    eng = _FakeEngine() if cls_name != "ChatterboxTurboTTS" else _FakeSerialEngine()
    m = _tts(getattr(api, cls_name), eng)
    m.max_batch = 2
    m.generate("aaaa.", *lang, loudness=-20)
    (kind, kw), = eng.calls
    assert kind == "synthesize" and kw["loudness"] == -20.0
    eng.calls.clear()
    lens = [9, 2, 5, 7, 30]
    targets = [-16.0, None, -23.0, None, -30.0]
    out = m.generate_batch(["x" * (n - 1) + "." for n in lens], *lang, loudness=targets, seeds=[1, 2, 3, 4, 5])
    extra = 0 if cls_name == "ChatterboxTurboTTS" else 2
    of_len = {n + extra: t for n, t in zip(lens, targets)}
    jobs = _jobs(eng.calls)
    assert [len(j["text_tokens"]) for j in jobs] == [2, 2, 1] and len(out) == 5
    for j in jobs:
        want = [of_len[int(t.numel())] for t in j["text_tokens"]]
        assert j.get("loudness") == (want if any(v is not None for v in want) else None), "a sub-batch carries the targets of ITS requests, in its row order; none: no key"
    eng.calls.clear()
    m.generate_batch(["x.", "yy.", "zzz."], *lang, loudness=-18)
    assert [j["loudness"] for j in _jobs(eng.calls)] == [[-18.0] * len(j["text_tokens"]) for j in _jobs(eng.calls)]


class _Mark:
    def __init__(self, log):
        self.log = log

    def apply_watermark(self, wav, sample_rate):
        self.log.append(("watermark", wav.copy()))
        return wav * 2.0


@pytest.mark.parametrize("cls_name,lang", KINDS)
def test_generate_long_normalises_the_whole_once_ahead_of_the_watermark_and_the_conversion(cls_name, lang, monkeypatch):
    from chatterbox_amd import api, ops
    eng = _LongEngine() if cls_name != "ChatterboxTurboTTS" else _LongSerial()
    m = _tts(getattr(api, cls_name), eng)
    base = m.generate_long(LONG_TEXT, *lang, max_chars=14, seed=11)
    eng.calls.clear()
    log = []
    m.watermarker = _Mark(log)

    def normalize(rows, target, ceiling=1.0, fs=24000):
        log.append(("loudness", [r.clone() for r in rows], target, ceiling))
        rows[0].mul_(0.5)
        return "stats"
    monkeypatch.setattr(ops, "wave_normalize", normalize)
    monkeypatch.setattr(ops, "wave_format", lambda rows, fmt: log.append(("format", [r.clone() for r in rows], fmt)) or [torch.zeros(2, dtype=torch.int16)])
    wav = m.generate_long(LONG_TEXT, *lang, max_chars=14, seed=11, loudness=-19, encoding="s16")
    assert all("loudness" not in j and "format" not in j for j in _jobs(eng.calls)), "the jobs of generate_long never carry the target"
    assert [e[0] for e in log] == ["loudness", "watermark", "format"] and log[0][2] == [-19.0] and log[0][3] == 1.0 and eng.last_loudness == "stats"
    assert len(log[0][1]) == 1 and torch.equal(log[0][1][0], base[0]), "ONE signal: the assembled waveform"
    assert np.array_equal(log[1][1], base[0].numpy() * 0.5) and torch.equal(log[2][1][0], base[0] * 0.5 * 2.0) and wav.dtype == torch.int16


def test_bad_targets_raise_before_the_engine_is_called_and_streams_do_not_take_the_keyword():
    from chatterbox_amd import api
    for cls_name, lang in KINDS:
        eng = _LongEngine()
        m = _tts(getattr(api, cls_name), eng)
        for value, err in ((-4.0, ValueError), (True, TypeError), ("loud", TypeError), (float("nan"), ValueError)):
            for call in (lambda: m.generate("a.", *lang, loudness=value), lambda: m.generate_batch(["a.", "b."], *lang, loudness=value),
                         lambda: m.generate_long("a. b.", *lang, loudness=value)):
                with pytest.raises(err, match="loudness"):
                    call()
        for call in (lambda: m.generate("a.", *lang, loudness=[-20.0]), lambda: m.generate_long("a. b.", *lang, loudness=[-20.0])):
            with pytest.raises(TypeError, match="loudness"):
                call()
        with pytest.raises(ValueError, match="loudness"):
            m.generate_batch(["a.", "b."], *lang, loudness=[-20.0])
        with pytest.raises(TypeError, match="loudness"):
            m.generate_stream("a.", *lang, loudness=-20)
        assert eng.calls == []
        for name in ("generate", "generate_batch", "generate_long"):
            assert inspect.signature(getattr(m, name)).parameters["loudness"].default is None and "loudness" in getattr(type(m), name).__doc__ or cls_name != "ChatterboxTTS"
    assert "peak of 1.0" in api.ChatterboxTTS.generate.__doc__ and "LUFS" in api.ChatterboxTTS.generate.__doc__
    vc = api.ChatterboxVC.__new__(api.ChatterboxVC)
    vc.engine, vc.ref_dict, vc.watermarker, vc.analyzer = _VCEngine(), {}, None, None
    with pytest.raises(TypeError, match="loudness"):
        vc.generate_stream(s3_tokens=[1, 2], loudness=-20)
    with pytest.raises(ValueError, match="loudness"):
        vc.generate(s3_tokens=[1, 2], loudness=-3)
    assert vc.engine.calls == []
    vc.generate(s3_tokens=[1, 2]), vc.generate(s3_tokens=[1, 2], loudness=-21), vc.generate_batch(s3_tokens=[[1, 2], [3]], loudness=[None, -17])
    vc.generate_batch(s3_tokens=[[1, 2], [3]], loudness=[None, None])
    assert [kw.get("loudness") for kw in vc.engine.calls] == [None, -21.0, [-17.0, None], None] and "loudness" not in vc.engine.calls[0] and "loudness" not in vc.engine.calls[3]


class _VCEngine:
    dev = CPU

    def __init__(self):
        self.calls = []

    def vocode(self, toks, ref, **kw):
        self.calls.append(kw)
        return [torch.zeros(3) for _ in toks], None


# ----------------------------------------------------------------------------- the engines
def _stand_in_engine():
    from chatterbox_amd import engine
    eng = engine.ChatterboxEngine.__new__(engine.ChatterboxEngine)
    eng.dev, eng.last_timing, eng.last_loudness = CPU, {}, None
    eng.flow = type("Flow", (), {"precision": 1, "inference": lambda self, tok, lens, ref, **kw: torch.ones(tok.shape[0], 2 * tok.shape[1], 80)})()
    eng.hift = type("Hift", (), {"precision": 1, "inference": staticmethod(lambda mel, lens=None, **kw: (torch.arange(mel.shape[0] * 480 * mel.shape[1], dtype=torch.float32).view(mel.shape[0], -1), None))})()
    return eng


def test_vocode_normalises_the_cut_rows_ahead_of_the_format_and_refuses_a_join(monkeypatch):
    from chatterbox_amd import ops, synth
    eng = _stand_in_engine()
    calls = []
    monkeypatch.setattr(ops, "wave_normalize", lambda rows, target, ceiling=1.0, fs=24000: calls.append(("loudness", [r.clone() for r in rows], target, ceiling)) or "stats")
    monkeypatch.setattr(ops, "wave_format", lambda rows, fmt: calls.append(("format", rows, fmt)) or ["converted"] * len(rows))
    monkeypatch.setattr(ops, "wave_join", lambda rows, **kw: calls.append(("join", rows, kw)) or dict(out=kw.get("out"), rec="rec", n=[r.numel() for r in rows]))
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: None)
    ref = synth.s3gen_ref(n_prompt_tokens=6)
    st = [synth.speech_tokens(n, seed=k) for k, n in enumerate((12, 5, 9))]
    base, _ = eng.vocode(st, ref, drop_last_token=True)
    for none in (None, [None, None, None]):
        same, _ = eng.vocode(st, ref, drop_last_token=True, loudness=none)
        assert calls == [] and eng.last_loudness is None and all(torch.equal(a, b) for a, b in zip(same, base)), "None is the call without it"
    got, _ = eng.vocode(st, ref, drop_last_token=True, speed=[1.0, 2.0, 1.0], loudness=[-16, None, -23], format=dict(encoding="s16"))
    assert [c[0] for c in calls] == ["loudness", "format"] and calls[0][2] == [-16.0, None, -23.0] and calls[0][3] == 1.0 and eng.last_loudness == "stats"
    assert [r.numel() for r in calls[0][1]] == [base[0].numel(), 480 * ops.scaled_len(base[1].numel() // 480, 2.0), base[2].numel()], "the rows the speed stretch has shaped"
    calls.clear()
    with pytest.raises(ValueError, match="loudness together with join"):
        eng.vocode(st, ref, join=dict(gaps=[5, 0, 7]), loudness=-20)
    with pytest.raises(ValueError, match="loudness"):
        eng.vocode(st, ref, loudness=[-20.0])
    assert calls == []
    piece, _ = eng.vocode(st, ref, join=dict(gaps=[5, 0, 7]), loudness=None)
    assert [c[0] for c in calls] == ["join"]


def test_synthesize_and_the_jobs_of_the_throughput_schedule_check_the_keyword():
    from chatterbox_amd import engine
    job = dict(text_tokens=[torch.zeros(3), torch.zeros(2)])
    assert "loudness" not in engine._checked_job(dict(job, loudness=None)) and "loudness" not in engine._checked_job(dict(job, loudness=[None, None]))
    assert engine._checked_job(dict(job, loudness=-20))["loudness"] == [-20.0, -20.0] and engine._checked_job(dict(job, loudness=[None, -9]))["loudness"] == [None, -9.0]
    with pytest.raises(ValueError, match="loudness together with join"):
        engine._checked_job(dict(job, loudness=-20, join=dict(gaps=[0, 0])))
    assert "join" in engine._checked_job(dict(job, loudness=None, join=dict(gaps=[0, 0])))
    with pytest.raises(ValueError, match="loudness"):
        engine._checked_job(dict(job, loudness=[-20]))
    for cls in (engine.ChatterboxEngine, engine.TurboEngine):
        assert inspect.signature(cls.synthesize).parameters["loudness"].default is None
        eng = cls.__new__(cls)
        eng.dev = CPU
        with pytest.raises(ValueError, match="loudness together with join"):
            eng.synthesize([torch.zeros(3, dtype=torch.long)], {}, {}, loudness=-20, join=dict(gaps=[0]))
    for cls in (engine.S3GenEngine, engine.ChatterboxEngine, engine.TurboEngine):
        for name in ("vocode_stream", "synthesize_stream"):
            if hasattr(cls, name):
                assert "loudness" not in inspect.signature(getattr(cls, name)).parameters, "integrated loudness is not known before the end of a signal"


# ----------------------------------------------------------------------------- the Turbo prompt
def test_norm_loudness_device_goes_through_the_device_meter_and_true_false_stay(monkeypatch, emu):
    from chatterbox_amd import api
    x = C.bursts(25234, 4)
    got = api._norm_loudness_device(x, CPU)
    assert abs(C.oracle(got)["L"] + 27.0) <= 0.01 and got.dtype == np.float32 and not np.shares_memory(got, x)
    loud = (x * np.float32(40.0)).astype(np.float32)
    assert abs(C.oracle(api._norm_loudness_device(loud, CPU, -5.0))["L"] + 5.0) <= 0.01 and np.abs(api._norm_loudness_device(loud, CPU, -5.0)).max() > 1.0, "no ceiling, as the reference applies none"
    seen = []
    monkeypatch.setattr(api, "_norm_loudness_device", lambda w, dev: seen.append("device") or w)
    monkeypatch.setattr(api, "_norm_loudness", lambda w, sr: seen.append("host") or w)

    class _Stop(Exception):
        pass

    def stop(*a, **k):
        raise _Stop
    analyzer = type("A", (), {"tokenizer": type("T", (), {"available": True}), "speaker_encoder": type("S", (), {"available": True}), "ve": object(), "DEC_COND_LEN": 240000, "embed_ref": stop})()
    monkeypatch.setattr("chatterbox_amd.frontend.resample", lambda w, a, b: w)
    for value, want in (("device", ["device"]), (True, ["host"]), (False, [])):
        seen.clear()
        with pytest.raises(_Stop):
            api._prepare_conditionals(analyzer, (x, 24000), 0.0, 375, CPU, norm_loudness=value)
        assert seen == want
    with pytest.raises(ValueError, match="norm_loudness"):
        api._prepare_conditionals(analyzer, (x, 24000), 0.0, 375, CPU, norm_loudness="gpu")
    assert inspect.signature(api.ChatterboxTurboTTS.norm_loudness).parameters.keys() == {"self", "wav", "sr", "target_lufs"}
