"""CPU (-m "not gpu"): pitch control -- cbx_wave_pitch_f32 on the SIMT emulator against the fp64 restatement (wave_pitch_common.py), its C ABI and descriptor
errors, the oracle's own checks (table, sine), ops.check_pitch / check_speed_pitch, and the plumbing of pitch= on the public classes over recording engines
(nothing is launched).  The recording engines are those of test_seeded_rng_host.py / test_wave_join_host.py (read-only imports)."""
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

import wave_pitch_common as P  # noqa: E402
from test_seeded_rng_host import _FakeEngine, _FakeSerialEngine, _tts  # noqa: E402  (read-only import: the recording engines)
from test_wave_join_host import KINDS, LONG_TEXT, _jobs, _LongEngine, _LongSerial  # noqa: E402  (read-only import)

CPU = torch.device("cpu")


# ----------------------------------------------------------------------------- C ABI
def test_entry_point_is_declared_exported_bound_and_documented():
    from chatterbox_amd import _lib, ops
    hdr = open(os.path.join(ROOT, "include", "cbx.h")).read()
    lib = ctypes.CDLL(os.path.join(ROOT, "chatterbox_amd", "libcbx_hip.so"))
    assert re.search(r"^int cbx_wave_pitch_f32\(", hdr, re.M) and hasattr(lib, "cbx_wave_pitch_f32") and "cbx_wave_pitch_f32" in _lib._SIGS
    assert "#define CBX_ABI_VERSION 16" in hdr and _lib.lib.cbx_abi_version() == 16 and _lib.ABI_VERSION == 16, "a new function only: no version step"
    block = hdr[hdr.index("---- pitch control"): hdr.index("int cbx_wave_pitch_f32(")]
    for phrase in ("models/s3gen/s3gen.py:289", "tts.py:272", "vc.py:104", "r = 2^(p / 12)", "s_eff = s / r", "480 scaled_len(K,", "formants move with the pitch",
                   "c = min(1.0, 1.0 / step)", "sinc(t) I0(beta sqrt(1 - (t / Z)^2)) / I0(beta)", "max(0, ceil(x_j - Z / c)) .. min(n - 1, floor(x_j + Z / c))",
                   "u = |x_j - i| * c * L", "k = (long)u, a = (float)(u - k)", "w = fmaf(a, tab[k + 1] - tab[k], tab[k]); acc = fmaf(w, x[i], acc)", "y[j] = (float)c * acc",
                   "floor(2 Z / c) + 2", "returns the input's bits", "Z L + 2 > 4098", "out\n * overlapping wav"):
        assert phrase in block, phrase
    src = open(os.path.join(ROOT, "chatterbox_amd", "csrc", "wave_pitch.hip")).read()
    assert "asm" not in src and "__shared__ float s_tab" in src and "__shared__ float s_x" in src, "plain C++; table and span staged in LDS"
    assert (ops.PITCH_Z, ops.PITCH_L, ops.PITCH_BETA) == (P.Z, P.L, P.BETA) == (16, 256, 9.0) and (ops.PITCH_MIN, ops.PITCH_MAX) == (-12.0, 12.0)
    assert ops.pitch_ratio(12) == 2.0 and ops.pitch_ratio(-12) == 0.5 and ops.pitch_ratio(3.3) == 2.0 ** (3.3 / 12.0) == P.ratio(3.3)


def _host_good(out_fill=7.0):
    """two rows of 960 samples in one host buffer, outputs at 3 and 700 of a prefilled buffer of 1500"""
    wav, out = (ctypes.c_float * 1920)(), (ctypes.c_float * 1500)(*[out_fill] * 1500)
    tab = np.ascontiguousarray(P.table())
    good, keep = P.raw_args(ctypes.addressof(wav), [0, 960], [960, 960], [1.5, 0.75], [600, 600], tab.ctypes.data, ctypes.addressof(out), [3, 700], 1500, None)
    return good, (wav, out, tab, keep)


def test_refused_descriptors_return_a_status_and_write_nothing():
    """on host buffers: a launch of the product library on them would fault, a refusal never gets that far"""
    from chatterbox_amd import _lib
    good, (wav, out, tab, keep) = _host_good()
    held = P.refused(_lib.lib, good)
    assert all(v == 7.0 for v in out), "a refused call writes nothing"
    del held


# ----------------------------------------------------------------------------- the oracle's own checks
def test_interpolated_table_is_within_its_bound_of_the_exact_filter():
    from chatterbox_amd import ops
    f = ops.pitch_filter()
    assert (f["Z"], f["L"], f["beta"]) == (P.Z, P.L, P.BETA) and f["tab"].shape == (4098,)
    err = P.check_table(f["tab"])
    print(f"interpolated table against h: {err:.3e} (bound {np.pi ** 2 / (8 * P.L ** 2) + P.EPS:.3e})")


@pytest.mark.parametrize("p", [-12, -6, -1, 3.3, 6, 12])
def test_restatement_on_the_projects_table_shifts_a_sine_to_f_times_r(p):
    from chatterbox_amd import ops
    print(f"p = {p}: 1 kHz -> {1000 * P.ratio(p):.1f} Hz, SNR {P.check_sine(p, ops.pitch_filter()['tab']):.1f} dB")


def test_restatement_on_the_projects_table_at_step_one_is_the_identity():
    from chatterbox_amd import ops
    x = P.signal("uniform", 777, 3)
    y, S, D = P.restate(x, 1.0, 790, ops.pitch_filter()["tab"])
    assert np.array_equal(y[:777], x.astype(np.float64)) and not y[777:].any() and np.array_equal(S[:777], np.abs(x).astype(np.float64))
    assert P.taps(1.0) == 34 and P.taps(2.0) == 66 and P.taps(0.5) == 34


# ----------------------------------------------------------------------------- the kernel on the SIMT emulator
@pytest.fixture(scope="module")
def emu():
    import build_emu
    if not os.path.exists(build_emu.CLANG):
        pytest.skip("ROCm's clang++ (x86 host compiler of the emulator build) is not installed")
    import harness
    with harness.emulated() as lib:
        yield lib


@pytest.mark.parametrize("p", P.SEMITONES)
@pytest.mark.parametrize("name", ["A", "C"])
def test_wave_pitch_on_the_emulator(emu, name, p):
    from chatterbox_amd import ops
    for aligned in (True, False):
        for tail in ("below", "above"):
            worst = P.check_launch(ops, CPU, name, p, aligned, tail)
            print(f"{name} p = {p} aligned = {aligned} {tail}: worst error / bound = {worst:.3f}")


def test_step_one_returns_the_bits_on_the_emulator(emu):
    from chatterbox_amd import ops
    for name in ("A", "C"):
        for aligned in (True, False):
            P.check_identity(ops, CPU, name, aligned)


def test_nothing_is_written_outside_the_rows_on_the_emulator(emu):
    from chatterbox_amd import ops
    P.check_sentinels(ops, CPU, 3.3)
    P.check_sentinels(ops, CPU, -6)


def test_emulated_entry_refuses_the_same_descriptors_and_runs_the_good_one(emu):
    good, (wav, out, tab, keep) = _host_good()
    rng = np.random.default_rng(4)
    x = rng.uniform(-0.9, 0.9, 1920).astype(np.float32)
    ctypes.memmove(wav, x.ctypes.data, 4 * 1920)
    held = P.refused(emu, good)
    assert all(v == 7.0 for v in out)
    assert emu.cbx_wave_pitch_f32(*good) == 0
    o = np.ctypeslib.as_array(out).copy()
    P.check_bound(o[3:603], x[:960], 1.5, "row 0")
    P.check_bound(o[700:1300], x[960:], 0.75, "row 1")
    assert (o[:3] == 7.0).all() and (o[603:700] == 7.0).all() and (o[1300:] == 7.0).all()
    del held


def test_wrapper_refuses_bad_arguments(emu):
    from chatterbox_amd import ops
    big = torch.zeros(2, 960)
    rows = [big[0], big[1]]
    for steps, lens in (([1.5], [10, 10]), ([1.5, 1.5], [10]), ([1.5, 1.5], [10, -1])):
        with pytest.raises(ValueError, match="wave_pitch"):
            ops.wave_pitch(rows, steps, lens)
    with pytest.raises(RuntimeError, match="wave_pitch"):
        ops.wave_pitch(rows, [1.5, 2.5], [10, 10])
    with pytest.raises(ValueError, match="different allocations"):
        ops.wave_pitch([big[0], torch.zeros(5)], [1.5, 1.5], [10, 10])
    empty = ops.wave_pitch([big[0, :0], big[1, :0]], [1.5, 0.5], [4, 0])
    assert [o.tolist() for o in empty] == [[0.0] * 4, []]


# ----------------------------------------------------------------------------- the checks of the arguments
def test_check_pitch():
    from chatterbox_amd import ops
    assert ops.check_pitch(None, 3) is None and ops.check_pitch(0, 3) is None and ops.check_pitch([None, 0, 0.0], 3) is None
    assert ops.check_pitch(2, 2) == [2.0, 2.0] and ops.check_pitch([None, -3.5, 12], 3) == [0.0, -3.5, 12.0] and ops.check_pitch((-12,), 1) == [-12.0]
    assert ops.check_pitch(ops.check_pitch([1, None], 2), 2) == [1.0, 0.0]
    for bad, err in ((True, TypeError), ("2", TypeError), ([1, "2"], TypeError), ([1, False], TypeError), (dict(p=1), TypeError), (12.01, ValueError), (-13, ValueError),
                     (float("nan"), ValueError), (float("inf"), ValueError), ([1, 2, 3], ValueError), ([1], ValueError), ([1, 99], ValueError)):
        with pytest.raises(err, match="pitch"):
            ops.check_pitch(bad, 2)


def test_check_speed_pitch():
    from chatterbox_amd import ops
    assert ops.check_speed_pitch(None, None, 2) is None and ops.check_speed_pitch(1.5, [0, None], 2) is None
    eff = ops.check_speed_pitch([1.5, None, 0.8], [None, 12, -3], 3)
    assert eff == [1.5, 0.5, 0.8 / 2.0 ** (-3 / 12.0)], "a request without a pitch keeps exactly its speed"
    assert ops.check_speed_pitch(None, -12, 1) == [2.0] and ops.check_speed_pitch(2.0, 12, 1) == [1.0]
    for speed, pitch, B in ((0.9, 12, 1), (1.1, -12, 1), ([1.0, 0.5], [0, 1], 2), (2.0, -0.1, 1), ([None, 1.5], [12, -6], 2)):
        with pytest.raises(ValueError, match=r"speed.*pitch"):
            ops.check_speed_pitch(speed, pitch, B)
    with pytest.raises(ValueError, match="speed"):
        ops.check_speed_pitch(2.5, 1, 1)
    with pytest.raises(ValueError, match="pitch"):
        ops.check_speed_pitch(1.0, 13, 1)


# ----------------------------------------------------------------------------- the public classes over a recording engine (nothing is launched)
LENS = [9, 2, 5, 7, 30]


@pytest.mark.parametrize("cls_name,extra,lang", KINDS)
def test_pitch_reaches_the_engines_and_none_adds_nothing(cls_name, extra, lang):
    from chatterbox_amd import api
    eng = _FakeEngine() if cls_name != "ChatterboxTurboTTS" else _FakeSerialEngine()
    m = _tts(getattr(api, cls_name), eng)
    m.generate("aaaa.", *lang)
    base = eng.calls[-1][1]
    for none in (None, 0, 0.0):
        m.generate("aaaa.", *lang, pitch=none)
        kw = eng.calls[-1][1]
        assert kw.keys() == base.keys() and "pitch" not in base and all(torch.equal(kw[k], base[k]) if torch.is_tensor(base[k]) else True for k in base), "exactly the call of today"
    m.generate("aaaa.", *lang, pitch=-2, speed=1.25)
    assert eng.calls[-1][1]["pitch"] == [-2.0] and eng.calls[-1][1]["speed"] == [1.25] and eng.calls[-1][1].keys() == base.keys() | {"pitch", "speed"}
    # the per-request list travels through the sub-batches with its requests
    eng.calls.clear()
    m.max_batch = 2
    texts = ["x" * (n - 1) + "." for n in LENS]
    pitch = [3, None, 0, -12, 0.5]
    out = m.generate_batch(texts, *lang, pitch=pitch)
    assert [int(w[0, 0]) for w in out] == [n + extra for n in LENS]
    want_of_len = {n + extra: (0.0 if v is None else float(v)) for n, v in zip(LENS, pitch)}
    jobs = _jobs(eng.calls)
    assert [len(j["text_tokens"]) for j in jobs] == [2, 2, 1]
    for j in jobs:
        want = [want_of_len[int(t.numel())] for t in j["text_tokens"]]
        assert (j["pitch"] == want) if any(want) else ("pitch" not in j), (j.get("pitch"), want)
    assert any("pitch" not in j for j in jobs) and any("pitch" in j for j in jobs)
    eng.calls.clear()
    m.generate_batch(texts, *lang, pitch=1.5)
    assert all(j["pitch"] == [1.5] * len(j["text_tokens"]) for j in _jobs(eng.calls))
    eng.calls.clear()
    m.generate_batch(texts, *lang)
    plain = _jobs(eng.calls)
    eng.calls.clear()
    m.generate_batch(texts, *lang, pitch=[None, 0, None, 0.0, None])
    again = _jobs(eng.calls)
    assert [j.keys() for j in again] == [j.keys() for j in plain] and all("pitch" not in j for j in again)


@pytest.mark.parametrize("cls_name,extra,lang", KINDS)
def test_bad_values_raise_at_the_call(cls_name, extra, lang):
    from chatterbox_amd import api
    eng = _LongEngine()
    m = _tts(getattr(api, cls_name), eng)
    texts = ["aaaa.", "bb.", "cccccc."]
    bad = [(dict(pitch=12.5), ValueError, "pitch"), (dict(pitch=-13), ValueError, "pitch"), (dict(pitch="1"), TypeError, "pitch"), (dict(pitch=True), TypeError, "pitch"),
           (dict(pitch=float("nan")), ValueError, "pitch"), (dict(pitch=12, speed=0.9), ValueError, r"speed.*pitch"), (dict(pitch=-6, speed=1.5), ValueError, r"speed.*pitch")]
    for kw, err, name in bad:
        for call in (lambda: m.generate("aaaa.", *lang, **kw), lambda: m.generate_batch(texts, *lang, **kw), lambda: m.generate_long(LONG_TEXT, *lang, **kw),
                     lambda: m.generate_long_stream(LONG_TEXT, *lang, **kw)):
            with pytest.raises(err, match=name):
                call()
    for call in (lambda: m.generate("aaaa.", *lang, pitch=[2]), lambda: m.generate_long(LONG_TEXT, *lang, pitch=[2]), lambda: m.generate_long_stream(LONG_TEXT, *lang, pitch=(2,))):
        with pytest.raises(TypeError, match="pitch"):
            call()
    with pytest.raises(ValueError, match="pitch"):
        m.generate_batch(texts, *lang, pitch=[1, 2])
    with pytest.raises(ValueError, match=r"speed.*pitch"):
        m.generate_batch(texts, *lang, pitch=[0, 12, 0], speed=[1.0, 0.9, 1.0])
    with pytest.raises(TypeError, match="pitch"):
        m.generate_stream("aaaa.", *lang, pitch=2)
    assert eng.calls == []


@pytest.mark.parametrize("cls_name,extra,lang", KINDS)
def test_long_form_jobs_carry_pitch(cls_name, extra, lang):
    from chatterbox_amd import api
    eng = _LongEngine() if cls_name != "ChatterboxTurboTTS" else _LongSerial()
    m = _tts(getattr(api, cls_name), eng)
    m.max_batch = 2
    m.generate_long(LONG_TEXT, *lang, max_chars=14)
    plain = _jobs(eng.calls)
    eng.calls.clear()
    m.generate_long(LONG_TEXT, *lang, max_chars=14, pitch=-3, speed=0.8)
    jobs = _jobs(eng.calls)
    assert [len(j["text_tokens"]) for j in jobs] == [2, 2, 1]
    assert all(j["pitch"] == [-3.0] * len(j["text_tokens"]) and j["speed"] == [0.8] * len(j["text_tokens"]) and "join" in j for j in jobs)
    eng.calls.clear()
    m.generate_long(LONG_TEXT, *lang, max_chars=14, pitch=4)
    assert [j["join"] for j in _jobs(eng.calls)] == [j["join"] for j in plain], "the gaps do not depend on the pitch"
    with_pitch = _jobs(eng.calls)
    eng.calls.clear()
    list(m.generate_long_stream(LONG_TEXT, *lang, max_chars=14, pitch=4, first_batch=None))
    assert [(j["pitch"], j["join"]) for j in _jobs(eng.calls)] == [(j["pitch"], j["join"]) for j in with_pitch], "first_batch=None is generate_long's plan, pitch included"
    eng.calls.clear()
    list(m.generate_long_stream(LONG_TEXT, *lang, max_chars=14, pitch=4))
    assert [j["pitch"] for j in _jobs(eng.calls)] == [[4.0], [4.0, 4.0], [4.0, 4.0]]
    eng.calls.clear()
    m.generate_long(LONG_TEXT, *lang, max_chars=14, pitch=0)
    list(m.generate_long_stream(LONG_TEXT, *lang, max_chars=14, pitch=None))
    assert all("pitch" not in j for j in _jobs(eng.calls)) and [j.keys() for j in _jobs(eng.calls)[: len(plain)]] == [j.keys() for j in plain]


def test_vc_takes_the_argument():
    from chatterbox_amd import api, synth

    class Voc:
        def __init__(self):
            self.calls = []

        def vocode(self, toks, refs, **kw):
            self.calls.append(([int(t.numel()) for t in toks], kw))
            return [torch.full((2,), float(t.numel())) for t in toks], None

    vc = api.ChatterboxVC.__new__(api.ChatterboxVC)
    vc.engine, vc.device, vc.ref_dict, vc.analyzer, vc.watermarker = Voc(), CPU, synth.s3gen_ref(n_prompt_tokens=8), None, None
    vc.MAX_BATCH = 2
    toks = [synth.speech_tokens(n) for n in (30, 10, 20)]
    vc.generate(s3_tokens=toks[0], pitch=-2)
    vc.generate(s3_tokens=toks[0], pitch=None)
    vc.generate(s3_tokens=toks[0], pitch=0)
    assert vc.engine.calls[0][1] == dict(pitch=[-2.0]) and vc.engine.calls[1][1] == {} and vc.engine.calls[2][1] == {}
    vc.engine.calls.clear()
    vc.generate_batch(s3_tokens=toks, pitch=[None, 5, None])
    assert [(l, kw) for l, kw in vc.engine.calls] == [([10, 20], dict(pitch=[5.0, 0.0])), ([30], {})]
    vc.engine.calls.clear()
    for call, err, name in ((lambda: vc.generate(s3_tokens=toks[0], pitch=13), ValueError, "pitch"), (lambda: vc.generate_batch(s3_tokens=toks, pitch=[1, 2]), ValueError, "pitch"),
                            (lambda: vc.generate(s3_tokens=toks[0], pitch=12, speed=0.6), ValueError, r"speed.*pitch"),
                            (lambda: vc.generate_batch(s3_tokens=toks, pitch=-12, speed=[1.0, 1.0, 1.2]), ValueError, r"speed.*pitch"),
                            (lambda: vc.generate_stream(s3_tokens=toks[0], pitch=2), TypeError, "pitch")):
        with pytest.raises(err, match=name):
            call()
    assert vc.engine.calls == []


def test_pipelined_jobs_are_checked_and_a_pitch_of_zero_is_dropped():
    from chatterbox_amd import engine
    tok = [torch.arange(4), torch.arange(6)]
    assert "pitch" not in engine._checked_job(dict(text_tokens=tok, pitch=None)) and "pitch" not in engine._checked_job(dict(text_tokens=tok, pitch=[0, None]))
    assert engine._checked_job(dict(text_tokens=tok, pitch=3, speed=[1.5, None]))["pitch"] == [3.0, 3.0]
    with pytest.raises(ValueError, match=r"speed.*pitch"):
        engine._checked_job(dict(text_tokens=tok, pitch=[0, 12], speed=[1.0, 0.9]))
    with pytest.raises(TypeError, match="pitch"):
        engine._checked_job(dict(text_tokens=tok, pitch="3"))


def test_vocode_transposes_on_the_stream_of_the_waveforms(monkeypatch):
    """ChatterboxEngine.vocode over stand-in stages on the CPU: pitch=None / 0 makes no pitch call and stretches the mel as today; with a pitch ONE mel_time_scale
    call carries speed / r per row (rows without a pitch their plain speed), the pitch call takes the source rows, the ratios and the lengths of the call with
    speed alone, and runs ahead of loudness, pauses and format."""
    from chatterbox_amd import engine, ops, synth
    eng = engine.ChatterboxEngine.__new__(engine.ChatterboxEngine)
    eng.dev, eng.last_timing, eng.last_pauses = CPU, {}, None
    eng.flow = type("Flow", (), {"precision": 1, "inference": lambda self, tok, lens, ref, **kw: torch.ones(tok.shape[0], 2 * tok.shape[1], 80)})()
    eng.hift = type("Hift", (), {"precision": 1, "inference": staticmethod(lambda mel, lens=None, **kw: (torch.arange(mel.shape[0] * 480 * mel.shape[1], dtype=torch.float32).view(mel.shape[0], -1), None))})()
    calls = []

    def stretch(mel, rates, in_lens=None, out=None):
        calls.append(("stretch", list(rates), list(in_lens)))
        O = [ops.scaled_len(m, r) for m, r in zip(in_lens, rates)]
        return torch.ones(mel.shape[0], max(O), 80), torch.tensor(O, dtype=torch.int32)

    def pitch(rows, steps, out_lens):
        calls.append(("pitch", [int(r.numel()) for r in rows], list(steps), list(out_lens)))
        return [torch.zeros(n) for n in out_lens]

    monkeypatch.setattr(ops, "mel_time_scale", stretch)
    monkeypatch.setattr(ops, "wave_pitch", pitch)
    monkeypatch.setattr(ops, "wave_normalize", lambda rows, loud: calls.append(("loud", [int(r.numel()) for r in rows])) or "loudness")
    monkeypatch.setattr(ops, "wave_format", lambda rows, fmt: calls.append(("format", [int(r.numel()) for r in rows])) or [r[: r.numel() // 3] for r in rows])
    monkeypatch.setattr(ops, "wave_join", lambda rows, **kw: calls.append(("join", [int(r.numel()) for r in rows])) or dict(out="out"))
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: None)
    ref = synth.s3gen_ref(n_prompt_tokens=6)
    st = [synth.speech_tokens(n, seed=k) for k, n in enumerate((12, 5, 9))]
    K = [24, 10, 18]
    base, _ = eng.vocode(st, ref)
    for none in (None, 0, [None, 0, 0.0]):
        same, _ = eng.vocode(st, ref, pitch=none)
        assert calls == [] and [w.numel() for w in same] == [w.numel() for w in base] == [480 * k for k in K]
    eng.vocode(st, ref, speed=[1.25, None, 0.8])
    today = list(calls)
    calls.clear()
    eng.vocode(st, ref, speed=[1.25, None, 0.8], pitch=[0, None, 0])
    assert calls == today and [c[0] for c in calls] == ["stretch"], "a pitch of zero is the call with speed alone"
    calls.clear()
    r = [ops.pitch_ratio(p) for p in (3.0, 0.0, -6.0)]
    got, _ = eng.vocode(st, ref, speed=[1.25, None, 0.8], pitch=[3, None, -6], loudness=-23.0, format=dict(sample_rate=8000))
    eff = [1.25 / r[0], 1.0, 0.8 / r[2]]
    n_src = [480 * ops.scaled_len(k, e) for k, e in zip(K, eff)]
    N = [480 * ops.scaled_len(k, s) for k, s in zip(K, (1.25, 1.0, 0.8))]
    assert [c[0] for c in calls] == ["stretch", "pitch", "loud", "format"]
    assert calls[0][1] == eff and calls[0][2] == K and calls[1][1:] == (n_src, r, N) and calls[2][1] == N and calls[3][1] == N
    assert [w.numel() for w in got] == [n // 3 for n in N]
    calls.clear()
    got, _ = eng.vocode(st, ref, pitch=-12, join=dict(gaps=[5, 0, 7]))
    assert [c[0] for c in calls] == ["stretch", "pitch", "join"] and calls[0][1] == [2.0] * 3 and calls[1][2] == [0.5] * 3 and calls[1][3] == calls[2][1] == [480 * k for k in K]
    calls.clear()
    eng.vocode(st, ref, speed=2.0, pitch=12)
    assert [c[0] for c in calls] == ["pitch"] and calls[0][1] == [480 * k for k in K] and calls[0][3] == [480 * (k // 2) for k in K], "s_eff = 1 everywhere: no stretch launch"
    for kw, name in ((dict(pitch=13), "pitch"), (dict(pitch=12, speed=0.9), r"speed.*pitch"), (dict(pitch=[1, 2]), "pitch")):
        with pytest.raises(ValueError, match=name):
            eng.vocode(st, ref, **kw)
