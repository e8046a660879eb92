"""CPU (-m "not gpu"): pause control -- cbx_wave_squeeze_f32 on the SIMT emulator against the NumPy restatement (wave_squeeze_common.py), its C ABI and descriptor
errors, ops.check_pauses, and the plumbing of max_pause= / pause_db= on the public classes over recording engines (nothing is launched).  The recording engines
are those of test_seeded_rng_host.py / test_wave_join_host.py (read-only imports)."""
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

import wave_join_common as W  # noqa: E402
import wave_squeeze_common as S  # noqa: E402
from test_seeded_rng_host import _FakeEngine, _FakeSerialEngine, _tts  # noqa: E402  (read-only import: the recording engines)
from test_wave_join_host import CHUNKS, KINDS, LONG_TEXT, _jobs, _LongEngine, _LongSerial  # noqa: E402  (read-only import)

CPU = torch.device("cpu")


# ----------------------------------------------------------------------------- C ABI
def test_entry_point_is_declared_exported_bound_and_documented():
    from chatterbox_amd import _lib, ops
    hdr = open(os.path.join(ROOT, "include", "cbx.h")).read()
    lib = ctypes.CDLL(os.path.join(ROOT, "chatterbox_amd", "libcbx_hip.so"))
    assert re.search(r"^int cbx_wave_squeeze_f32\(", hdr, re.M) and hasattr(lib, "cbx_wave_squeeze_f32") and "cbx_wave_squeeze_f32" in _lib._SIGS
    assert "#define CBX_ABI_VERSION 16" in hdr and _lib.lib.cbx_abi_version() == 16 and _lib.ABI_VERSION == 16, "a new function only: no version step"
    block = hdr[hdr.index("---- pause control"): hdr.index("int cbx_wave_squeeze_f32(")]
    for phrase in ("m_f <= peak * ratio or m_f == 0", "NaN is NOT", "differs from cbx_wave_edges_f32", "h = K - K / 2, t = K / 2", "[a + h, b - t)", "y[n', n) is written as zeros",
                   "fmaf(ramp[i], x[c1 - F + i] - x[c0 - F + i], x[c0 - F + i])", "map(p) = the number of kept samples in [0, p)", "{n', pauses cut, frames removed, n}",
                   "16 * R * ceil(max_r n_r / 480)", "out overlapping wav", "tts.py:272"):
        assert phrase in block, phrase
    src = open(os.path.join(ROOT, "chatterbox_amd", "csrc", "wave_squeeze.hip")).read()
    assert "cbx_wave_frame_ms(" in src and "wave_frame_ms_kernel" not in src.replace("// ", "") and "wave_block_ms_kernel" not in src and "cbx_wave_block_pass" not in src, \
        "the frame pass is wave_join.hip's instantiation, not one of its own"
    assert "asm" not in src and "__shfl" not in src and "cbx_xor_lane" in src
    assert ops.WAVE_SQUEEZE_TILE == S.TILE and f"WS_TILE = {S.TILE}" in src


def _refusals(lib):
    """Every refused descriptor returns -22 with the entry's name before any launch, and nothing is written (host buffers: a launch of the product library on
    them would fault)."""
    n_buf = 2400
    wav, out, ramp = (ctypes.c_float * n_buf)(), (ctypes.c_float * n_buf)(), (ctypes.c_float * 480)()
    edges, stats, ws = (ctypes.c_int * 4)(5, 6, 7, 8), (ctypes.c_int * 8)(*[9] * 8), (ctypes.c_double * 64)()
    for i in range(n_buf):
        out[i] = 7.0
    off, n, keep = (ctypes.c_long * 2)(0, 1200), (ctypes.c_int * 2)(1200, 1200), (ctypes.c_int * 2)(2, 0)
    neg, noff, k1, kneg = (ctypes.c_int * 2)(1200, -1), (ctypes.c_long * 2)(0, -4), (ctypes.c_int * 2)(2, 1), (ctypes.c_int * 2)(-2, 2)
    a = ctypes.addressof
    need = 16 * 2 * 3
    good = [a(wav), a(off), a(n), a(keep), 2, 1e-4, a(ramp), 240, a(out), n_buf, a(edges), a(stats), a(ws), need, None]
    bad_args = [(0, None), (1, None), (2, None), (3, None), (8, None), (11, None), (12, None), (4, 0), (4, -1), (4, 65), (2, a(neg)), (1, a(noff)), (3, a(k1)), (3, a(kneg)),
                (5, -1.0), (5, float("nan")), (5, float("inf")), (7, -1), (7, 481), (6, None), (8, a(wav)), (8, a(wav) + 4 * 2399), (8, a(wav) - 4 * 2399), (9, 2399), (9, 0),
                (13, need - 1), (13, 0), (12, a(ws) + 4)]
    for i, bad in bad_args:
        args = list(good)
        args[i] = bad
        assert lib.cbx_wave_squeeze_f32(*args) == -22 and b"wave_squeeze" in lib.cbx_last_error(), (i, bad)
    assert all(v == 7.0 for v in out) and list(edges) == [5, 6, 7, 8] and list(stats) == [9] * 8 and not any(ws), "a refused call writes nothing"
    return good, (wav, out, ramp, edges, stats, ws, off, n, keep)


def test_refused_descriptors_return_a_status_and_write_nothing():
    from chatterbox_amd import _lib
    _refusals(_lib.lib)


# ----------------------------------------------------------------------------- the kernels on the SIMT emulator
@pytest.fixture(scope="module")
def emu():
    import build_emu
    if not os.path.exists(build_emu.CLANG):
        pytest.skip("ROCm's clang++ (x86 host compiler of the emulator build) is not installed")
    import harness
    with harness.emulated() as lib:
        yield lib


@pytest.mark.parametrize("name,fade,db", S.CASES, ids=S.CASE_IDS)
def test_wave_squeeze_on_the_emulator(emu, name, fade, db):
    from chatterbox_amd import ops
    S.check_launch(ops, CPU, name, fade, db)


def test_the_cases_are_what_they_claim():
    S.what_the_sets_cover()


def test_exact_fmaf_of_the_restatement():
    """The seam's fmaf rounds once: against exact rational arithmetic on operands chosen to make double rounding likely."""
    from fractions import Fraction
    rng = np.random.RandomState(5)
    a = rng.uniform(0, 1, 4000).astype(np.float32)
    b = (rng.uniform(-1, 1, 4000) * 10.0 ** rng.uniform(-8, 0, 4000)).astype(np.float32)
    c = (rng.uniform(-1, 1, 4000) * 10.0 ** rng.uniform(-8, 0, 4000)).astype(np.float32)
    a[:3], b[:3], c[:3] = [1.0, 0.5, 1.0 + 2.0 ** -23], [1.0 + 2.0 ** -23, 2.0 ** -24, 1.0 + 2.0 ** -23], [2.0 ** -25, 1.0, -1.0]
    got = S.fmaf(a, b, c)

    def rne32(q):  # round an exact rational to float32, ties to even
        if q == 0:
            return np.float32(0.0)
        e = int(np.floor(np.log2(abs(float(q)))))
        while Fraction(2) ** e > abs(q):
            e -= 1
        while Fraction(2) ** (e + 1) <= abs(q):
            e += 1
        ulp = Fraction(2) ** (max(e, -126) - 23)
        k = q / ulp
        lo = k.numerator // k.denominator
        r = k - lo
        k = lo + (1 if r > Fraction(1, 2) or (r == Fraction(1, 2) and lo % 2) else 0)
        return np.float32(float(k * ulp))

    want = np.array([rne32(Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z))) for x, y, z in zip(a, b, c)], dtype=np.float32)
    assert (got.view(np.int32) == want.view(np.int32)).all()
    naive = (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)
    print("double-rounded differs on", int((naive.view(np.int32) != want.view(np.int32)).sum()), "of 4000")


def test_emulated_entry_refuses_the_same_descriptors_and_runs_the_good_one(emu):
    good, keep = _refusals(emu)
    wav, out, ramp, edges, stats, ws = keep[:6]
    assert emu.cbx_wave_squeeze_f32(*good) == 0   # all-zero rows: nothing is removed, the rows are copied, the table is cut into [0, n]
    assert list(stats) == [1200, 0, 0, 1200] * 2 and list(edges) == [5, 6, 7, 8] and not any(out)
    args = list(good)
    args[10] = None                               # no edge table
    assert emu.cbx_wave_squeeze_f32(*args) == 0


def test_two_launches_agree_and_join_composes(emu):
    """ops.wave_join(squeeze=) = edges on the original rows, squeeze (which maps the table), join: against the NumPy composition."""
    from chatterbox_amd import ops
    S.check_composition(ops, CPU, "pauses", 40.0, True, True)
    S.check_composition(ops, CPU, "edges", None, False, True)


def test_check_pauses():
    from chatterbox_amd import ops
    assert ops.check_pauses(None, 3) is None
    assert ops.check_pauses(dict(keep=15), 2) == dict(keep=[15, 15], db=40.0, fade=240)
    assert ops.check_pauses(dict(keep=[2, None], db=3, fade=0), 2) == dict(keep=[2, 0], db=3.0, fade=0)
    assert ops.check_pauses([None, 3000, 0], 3) == dict(keep=[0, 3000, 0], db=40.0, fade=240)
    assert ops.check_pauses([None, 0], 2) is None and ops.check_pauses(dict(keep=0), 2) is None, "no row with a keep: the call without the argument"
    full = ops.check_pauses(dict(keep=[4, 5], db=20.0, fade=480), 2)
    assert ops.check_pauses(full, 2) == full
    for bad, err in ((5, TypeError), ("x", TypeError), (dict(), ValueError), (dict(keep=[2], x=1), ValueError), (dict(keep=[2]), ValueError), (dict(keep=[1, 2]), ValueError),
                     (dict(keep=[-2, 2]), ValueError), (dict(keep=[3001, 2]), ValueError), (dict(keep=[2.0, 2]), TypeError), (dict(keep=[True, 2]), TypeError),
                     (dict(keep="22"), TypeError), (dict(keep=2, db="40"), TypeError), (dict(keep=2, db=-1), ValueError), (dict(keep=2, db=float("nan")), ValueError),
                     (dict(keep=2, fade=481), ValueError), (dict(keep=2, fade=-1), ValueError), (dict(keep=2, fade=1.5), TypeError), ([2, 2, 2], ValueError)):
        with pytest.raises(err, match="pauses"):
            ops.check_pauses(bad, 2)


# ----------------------------------------------------------------------------- the public classes over a recording engine (nothing is launched)
LENS = [9, 2, 5, 7, 30]


def _calls_jobs(calls):
    return [j for kind, kw in calls for j in (kw["jobs"] if kind == "pipelined" else [kw])]


@pytest.mark.parametrize("cls_name,extra,lang", KINDS)
def test_max_pause_reaches_the_engines_and_none_adds_nothing(cls_name, extra, lang):
    from chatterbox_amd import api
    eng = _FakeEngine() if cls_name != "ChatterboxTurboTTS" else _FakeSerialEngine()
    m = _tts(getattr(api, cls_name), eng)
    m.generate("aaaa.", *lang)
    base = eng.calls[-1][1]
    m.generate("aaaa.", *lang, max_pause=None, pause_db=12)
    assert eng.calls[-1][1].keys() == base.keys() and "pauses" not in base, "None adds no keyword to the engine call"
    m.generate("aaaa.", *lang, max_pause=0.3, pause_db=35)
    assert eng.calls[-1][1]["pauses"] == dict(keep=[15], db=35.0, fade=240) and eng.calls[-1][1].keys() == base.keys() | {"pauses"}
    m.generate("aaaa.", *lang, max_pause=0.04)
    assert eng.calls[-1][1]["pauses"] == dict(keep=[2], db=40.0, fade=240)
    # the per-request list travels through the sub-batches with its requests
    eng.calls.clear()
    m.max_batch = 2
    texts = ["x" * (n - 1) + "." for n in LENS]
    mp = [0.1, None, 1.0, None, 60]
    out = m.generate_batch(texts, *lang, max_pause=mp, pause_db=20)
    assert [int(w[0, 0]) for w in out] == [n + extra for n in LENS]
    keep_of_len = {n + extra: (0 if v is None else round(v * 50)) for n, v in zip(LENS, mp)}
    jobs = _calls_jobs(eng.calls)
    assert [len(j["text_tokens"]) for j in jobs] == [2, 2, 1]
    for j in jobs:
        want = [keep_of_len[int(t.numel())] for t in j["text_tokens"]]
        assert (j["pauses"] == dict(keep=want, db=20.0, fade=240)) if any(want) else ("pauses" not in j), (j.get("pauses"), want)
    eng.calls.clear()
    m.generate_batch(texts, *lang, max_pause=0.5)
    assert all(j["pauses"] == dict(keep=[25] * len(j["text_tokens"]), db=40.0, fade=240) for j in _calls_jobs(eng.calls))
    eng.calls.clear()
    m.generate_batch(texts, *lang, max_pause=[None] * 5)
    m.generate_batch(texts, *lang)
    assert all("pauses" not in j for j in _calls_jobs(eng.calls))


@pytest.mark.parametrize("cls_name,extra,lang", KINDS)
def test_bad_values_raise_at_the_call(cls_name, extra, lang):
    from chatterbox_amd import api
    eng = _LongEngine()
    m = _tts(getattr(api, cls_name), eng)
    texts = ["aaaa.", "bb.", "cccccc."]
    bad = [(dict(max_pause=0.03), ValueError, "max_pause"), (dict(max_pause=61), ValueError, "max_pause"), (dict(max_pause="1"), TypeError, "max_pause"),
           (dict(max_pause=True), TypeError, "max_pause"), (dict(max_pause=float("nan")), ValueError, "max_pause"), (dict(max_pause=1, pause_db=-1), ValueError, "pause_db"),
           (dict(pause_db="40"), TypeError, "pause_db"), (dict(pause_db=float("inf")), ValueError, "pause_db"), (dict(pause_db=None), TypeError, "pause_db"),
           (dict(pause_db=[40.0]), TypeError, "pause_db")]
    for kw, err, name in bad:
        for call in (lambda: m.generate("aaaa.", *lang, **kw), lambda: m.generate_batch(texts, *lang, **kw), lambda: m.generate_long(LONG_TEXT, *lang, **kw),
                     lambda: m.generate_long_stream(LONG_TEXT, *lang, **kw)):
            with pytest.raises(err, match=name):
                call()
    for call in (lambda: m.generate("aaaa.", *lang, max_pause=[0.5]), lambda: m.generate_long(LONG_TEXT, *lang, max_pause=[0.5]),
                 lambda: m.generate_long_stream(LONG_TEXT, *lang, max_pause=(0.5,))):
        with pytest.raises(TypeError, match="max_pause"):
            call()
    with pytest.raises(ValueError, match="max_pause"):
        m.generate_batch(texts, *lang, max_pause=[0.5, 0.5])
    with pytest.raises(TypeError, match="max_pause"):
        m.generate_stream("aaaa.", *lang, max_pause=0.5)
    with pytest.raises(TypeError, match="pause_db"):
        m.generate_stream("aaaa.", *lang, pause_db=40)
    assert eng.calls == []


@pytest.mark.parametrize("cls_name,extra,lang", KINDS)
def test_long_form_jobs_carry_pauses(cls_name, extra, lang):
    from chatterbox_amd import api
    eng = _LongEngine() if cls_name != "ChatterboxTurboTTS" else _LongSerial()
    m = _tts(getattr(api, cls_name), eng)
    m.max_batch = 2
    m.generate_long(LONG_TEXT, *lang, max_chars=14, max_pause=0.3, pause_db=30)
    jobs = _jobs(eng.calls)
    assert [len(j["text_tokens"]) for j in jobs] == [2, 2, 1]
    assert all(j["pauses"] == dict(keep=[15] * len(j["text_tokens"]), db=30.0, fade=240) and "join" in j for j in jobs)
    eng.calls.clear()
    list(m.generate_long_stream(LONG_TEXT, *lang, max_chars=14, max_pause=0.3, pause_db=30, first_batch=None))
    assert [(j["pauses"], j["join"]) for j in _jobs(eng.calls)] == [(j["pauses"], j["join"]) for j in jobs], "first_batch=None is generate_long's plan, pauses included"
    eng.calls.clear()
    list(m.generate_long_stream(LONG_TEXT, *lang, max_chars=14, max_pause=0.3))
    assert [j["pauses"]["keep"] for j in _jobs(eng.calls)] == [[15], [15, 15], [15, 15]]
    eng.calls.clear()
    m.generate_long(LONG_TEXT, *lang, max_chars=14)
    list(m.generate_long_stream(LONG_TEXT, *lang, max_chars=14, max_pause=None))
    assert all("pauses" not in j for j in _jobs(eng.calls))


def test_vc_takes_the_arguments():
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
    vc.generate(s3_tokens=toks[0], max_pause=0.2)
    vc.generate(s3_tokens=toks[0], max_pause=None)
    assert vc.engine.calls[0][1] == dict(pauses=dict(keep=[10], db=40.0, fade=240)) and vc.engine.calls[1][1] == {}
    vc.engine.calls.clear()
    vc.generate_batch(s3_tokens=toks, max_pause=[None, 0.5, None], pause_db=10)
    assert [(l, kw) for l, kw in vc.engine.calls] == [([10, 20], dict(pauses=dict(keep=[25, 0], db=10.0, fade=240))), ([30], {})]
    for call, err in ((lambda: vc.generate(s3_tokens=toks[0], max_pause=0.01), ValueError), (lambda: vc.generate_batch(s3_tokens=toks, max_pause=[1, 2]), ValueError),
                      (lambda: vc.generate_stream(s3_tokens=toks[0], max_pause=0.5), TypeError)):
        with pytest.raises(err, match="max_pause"):
            call()


def test_vocode_squeezes_on_the_stream_of_the_waveforms(monkeypatch):
    """ChatterboxEngine.vocode over stand-in stages on the CPU: pauses=None (or no row with a keep) makes no squeeze call and passes no keyword on; with pauses the
    order is loudness, squeeze, format, and a join receives the dict as its squeeze= keyword."""
    from chatterbox_amd import engine, ops, synth
    eng = engine.ChatterboxEngine.__new__(engine.ChatterboxEngine)
    eng.dev, eng.last_timing, eng.last_pauses = CPU, {}, None
    eng.flow = type("Flow", (), {"precision": 1, "inference": lambda self, tok, lens, ref, **kw: torch.ones(tok.shape[0], 2 * tok.shape[1], 80)})()
    eng.hift = type("Hift", (), {"precision": 1, "inference": staticmethod(lambda mel, lens=None, **kw: (torch.arange(mel.shape[0] * 480 * mel.shape[1], dtype=torch.float32).view(mel.shape[0], -1), None))})()
    calls = []
    monkeypatch.setattr(ops, "wave_join", lambda rows, **kw: calls.append(("join", kw)) or dict(pauses="stats", out="out"))
    monkeypatch.setattr(ops, "wave_normalize", lambda rows, loud: calls.append(("loud", loud)) or "loudness")
    monkeypatch.setattr(ops, "wave_format", lambda rows, fmt: calls.append(("format", [int(r.numel()) for r in rows])) or [r[: r.numel() // 3] for r in rows])

    def squeeze(rows, keep, db, fade):
        calls.append(("squeeze", keep, db, fade))
        return dict(rows=[r.clone() for r in rows], stats=torch.tensor([[int(r.numel()) - 480 * k, 1, k, int(r.numel())] for r, k in zip(rows, keep)], dtype=torch.int32), edges=None)

    monkeypatch.setattr(ops, "wave_squeeze", squeeze)
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: None)
    ref = synth.s3gen_ref(n_prompt_tokens=6)
    st = [synth.speech_tokens(n, seed=k) for k, n in enumerate((12, 5, 9))]
    base, _ = eng.vocode(st, ref)
    same, _ = eng.vocode(st, ref, pauses=[None, 0, None])
    assert calls == [] and [w.numel() for w in same] == [w.numel() for w in base] == [960 * 12, 960 * 5, 960 * 9]
    got, _ = eng.vocode(st, ref, pauses=dict(keep=[2, 0, 3], db=30), loudness=-23.0)
    assert [c[0] for c in calls] == ["loud", "squeeze"] and calls[1][1:] == ([2, 0, 3], 30.0, 240)
    assert [w.numel() for w in got] == [960 * 12 - 960, 960 * 5, 960 * 9 - 1440] and eng.last_pauses.tolist()[0] == [960 * 12 - 960, 1, 2, 960 * 12]
    calls.clear()
    got, _ = eng.vocode(st, ref, pauses=[2, 2, 2], format=dict(sample_rate=8000))
    assert [c[0] for c in calls] == ["squeeze", "format"] and calls[1][1] == [960 * 12, 960 * 5, 960 * 9], "the zero-tailed rows are converted"
    assert [w.numel() for w in got] == [(960 * n - 960) // 3 for n in (12, 5, 9)], "and cut to formatted_len(n')"
    calls.clear()
    got, _ = eng.vocode(st, ref, pauses=[2, 2, 2], sync=False)
    assert set(got) == {"rows", "pauses", "format"} and [w.numel() for w in got["rows"]] == [960 * 12, 960 * 5, 960 * 9], "not synchronised: the rows stay n long"
    calls.clear()
    piece, _ = eng.vocode(st, ref, pauses=[2, 0, 2], join=dict(gaps=[5, 0, 7]))
    assert len(calls) == 1 and calls[0][1]["squeeze"] == dict(keep=[2, 0, 2], db=40.0, fade=240) and eng.last_pauses == "stats"
    calls.clear()
    eng.vocode(st, ref, join=dict(gaps=[5, 0, 7]))
    assert "squeeze" not in calls[0][1], "without pauses the join call is exactly the one before"
    with pytest.raises(ValueError, match="pauses"):
        eng.vocode(st, ref, pauses=[1, 2, 2])
