"""CPU (-m "not gpu"): long-form synthesis -- text.split_text, the chunk-seed helper, cbx_wave_edges_f32 / cbx_wave_join_f32 on the SIMT emulator against the NumPy
restatement (wave_join_common.py), their C ABI and descriptor errors, and the plumbing of generate_long on the public classes over a recording engine (nothing is
launched).  The recording engines are those of test_seeded_rng_host.py (read-only import), taught here what a joined piece looks like."""
import ctypes
import logging
import os
import re
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, os.path.join(HERE, "simt")):
    if p not in sys.path:
        sys.path.insert(0, p)

import wave_join_common as W  # noqa: E402
from test_seeded_rng_host import _FakeEngine, _FakeSerialEngine, _tts  # noqa: E402  (read-only import: the recording engines)

CPU = torch.device("cpu")


# ----------------------------------------------------------------------------- split_text
LONG_COMMAS = ", ".join(["a clause of several words"] * 80)          # 2000+ characters, one sentence, commas
LONG_PLAIN = " ".join(["word"] * 400)                                 # 1999 characters, one sentence, no clause mark
TEXTS = [
    "Dr. Smith went to Washington. He met Mr. Jones, e.g. at noon. It cost 3.14 dollars!",
    'She said "Stop!" Then (quietly) "why?" And left...',
    "Version 2.0.1 of e.g.x is out.It is fine. Really?!  Yes.",
    LONG_COMMAS + ".", LONG_PLAIN + ".", "x" * 2000, "alpha - beta - gamma " * 40,
    "你好。我很好！真的吗？是的，今天天气很好、我们去公园吧。" * 12,
    "First paragraph. It has two sentences.\n\nSecond paragraph.\n \n\n  Third one, after blank lines of spaces.\nStill the third.",
    "", "   \n\n \t ", "One",
]


@pytest.mark.parametrize("max_chars", [1, 7, 40, 100, 300])
@pytest.mark.parametrize("text", TEXTS, ids=[f"t{i}" for i in range(len(TEXTS))])
def test_split_text_invariants(text, max_chars):
    from chatterbox_amd.text import split_text
    chunks = split_text(text, max_chars)
    assert chunks == split_text(text, max_chars), "deterministic"
    assert all(isinstance(c, str) and isinstance(p, bool) for c, p in chunks)
    if not text.strip():
        assert chunks == [("", False)], "a blank text is one empty chunk: the normalisers speak their fallback sentence"
        return
    for c, _ in chunks:
        assert c.strip() and c == c.strip() and len(c) <= max_chars, (c, max_chars)
    assert "".join("".join(c for c, _ in chunks).split()) == "".join(text.split()), "the chunks hold the text's non-whitespace characters in order"
    assert not chunks[-1][1], "paragraph_end never marks the final chunk"


def test_split_text_exact_chunks():
    from chatterbox_amd.text import default_max_chars, split_text
    s = lambda t, n: split_text(t, n)
    assert s(TEXTS[0], 300) == [(TEXTS[0], False)]
    assert s(TEXTS[0], 32) == [("Dr. Smith went to Washington.", False), ("He met Mr. Jones, e.g. at noon.", False), ("It cost 3.14 dollars!", False)], "packing keeps Dr. Smith together"
    assert s("Pi is 3.14 and e.g.x is odd. Yes!", 20) == [("Pi is 3.14 and e.g.x", False), ("is odd. Yes!", False)], "3.14 and e.g.x do not end a sentence"
    assert s(TEXTS[1], 16) == [('She said "Stop!"', False), ('Then (quietly)', False), ('"why?"', False), ("And left...", False)], "closing quotes stay with their sentence"
    assert s("你好。我很好！真的吗？是的", 4) == [("你好。", False), ("我很好！", False), ("真的吗？", False), ("是的", False)], "CJK enders need no whitespace behind them"
    assert s(TEXTS[8], 300) == [("First paragraph. It has two sentences.", True), ("Second paragraph.", True), ("Third one, after blank lines of spaces.\nStill the third.", False)]
    assert s("one, two; three: four - five six", 12) == [("one, two;", False), ("three:", False), ("four -", False), ("five six", False)], "the last clause mark inside the limit"
    assert s("some words without marks", 12) == [("some words", False), ("without", False), ("marks", False)], "no clause mark: the last whitespace"
    assert s("abcdefghij", 4) == [("abcd", False), ("efgh", False), ("ij", False)], "text without spaces: a hard cut"
    assert [len(c) for c, _ in s(LONG_COMMAS, 300)] == [296] * 7 + [79] and all(c.endswith(",") for c, _ in s(LONG_COMMAS, 300)[:-1])
    assert all(len(c) == 299 for c, _ in s(LONG_PLAIN, 300)[:-1])
    assert (default_max_chars(False), default_max_chars(True)) == (300, 100) and len(s("x" * 450, None)) == 2 and len(split_text("字" * 450, None, cjk=True)) == 5
    for bad, err in ((0, ValueError), (-3, ValueError), (2.5, TypeError), (True, TypeError), ("9", TypeError)):
        with pytest.raises(err, match="max_chars"):
            split_text("a b", bad)
    with pytest.raises(TypeError, match="text"):
        split_text(None, 10)


# ----------------------------------------------------------------------------- the seed helper
def test_chunk_seed():
    from chatterbox_amd import api
    for seed in (0, 7, 2 ** 63, 2 ** 64 - 1):
        assert api.chunk_seed(seed, 0) == seed
        vals = [api.chunk_seed(seed, k) for k in range(1000)]
        assert all(0 <= v < 2 ** 64 for v in vals) and len(set(vals)) == 1000
    assert api.chunk_seed(1, 1) == 1 + 0x9E3779B97F4A7C15 and api.chunk_seed(2 ** 64 - 1, 1) == 0x9E3779B97F4A7C15 - 1 and api.chunk_seed(5, 2) == (5 + 2 * 0x9E3779B97F4A7C15) % 2 ** 64


# ----------------------------------------------------------------------------- C ABI
def test_entry_points_are_declared_exported_and_bound():
    from chatterbox_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "cbx.h")).read()
    lib = ctypes.CDLL(os.path.join(ROOT, "chatterbox_amd", "libcbx_hip.so"))
    for name in ("cbx_wave_edges_f32", "cbx_wave_join_f32"):
        assert re.search(rf"^int {name}\(", hdr, re.M) and hasattr(lib, name) and name in _lib._SIGS
    assert "#define CBX_ABI_VERSION 16" in hdr and _lib.lib.cbx_abi_version() == 16 and _lib.ABI_VERSION == 16, "new functions only: no version step"
    assert "tts.py:249" in open(os.path.join(ROOT, "chatterbox_amd", "csrc", "wave_join.hip")).read()


def _descriptor_errors(lib):
    """Every refused descriptor returns -22 with the entry's name, before any launch (host buffers: a launch of the product library on them would fault)."""
    wav, out, ramp = (ctypes.c_float * 1920)(), (ctypes.c_float * 4000)(), (ctypes.c_float * 8)()
    rec, ws = (ctypes.c_int * 7)(), (ctypes.c_double * 8)()
    off, n, gaps, neg, noff = (ctypes.c_long * 2)(0, 960), (ctypes.c_int * 2)(960, 960), (ctypes.c_int * 2)(10, 10), (ctypes.c_int * 2)(960, -1), (ctypes.c_long * 2)(0, -4)
    a = ctypes.addressof
    good_e = [a(wav), a(off), a(n), 2, 1e-4, 2, a(rec) + 12, a(ws), 8, None]
    for i, bad in ((0, None), (1, None), (2, None), (6, None), (7, None), (3, 0), (3, -1), (3, 65), (2, a(neg)), (1, a(noff)), (4, -1.0), (4, float("nan")),
                   (4, float("inf")), (5, -1), (8, 3)):
        args = list(good_e)
        args[i] = bad
        assert lib.cbx_wave_edges_f32(*args) == -22 and b"wave_edges" in lib.cbx_last_error(), (i, bad)
    good_j = [a(wav), a(off), a(n), a(gaps), 2, a(rec) + 12, a(ramp), 8, 1, 1, a(out), 4000, a(rec), None]
    for i, bad in ((0, None), (1, None), (2, None), (3, None), (5, None), (10, None), (12, None), (4, 0), (4, 65), (2, a(neg)), (3, a(neg)), (1, a(noff)), (7, -1),
                   (6, None), (11, 1939), (11, 0)):
        args = list(good_j)
        args[i] = bad
        assert lib.cbx_wave_join_f32(*args) == -22 and b"wave_join" in lib.cbx_last_error(), (i, bad)
    return good_e, good_j, rec, out, (wav, ramp, ws, off, n, gaps)   # (the descriptors hold addresses: the buffers must outlive them)


def test_descriptor_errors_return_a_status_and_a_message():
    from chatterbox_amd import _lib
    _descriptor_errors(_lib.lib)


@pytest.mark.parametrize("case", W.ROW_REFUSALS)
@pytest.mark.parametrize("entry", W.ROW_ENTRIES)
def test_every_row_entry_refuses_bad_rows_under_its_own_name(entry, case):
    """the product library on host buffers: the shared row check of wave_common.h carries the name of the entry that called it"""
    from chatterbox_amd import _lib, ops
    W.check_row_refusal(_lib.lib, ops, entry, case)


# ----------------------------------------------------------------------------- the kernels on the SIMT emulator
@pytest.fixture(scope="module")
def emu():
    import build_emu
    if not os.path.exists(build_emu.CLANG):
        pytest.skip("ROCm's clang++ (x86 host compiler of the emulator build) is not installed")
    import harness
    with harness.emulated() as lib:
        yield lib


@pytest.mark.parametrize("name,cfg", W.CASES, ids=W.CASE_IDS)
def test_wave_join_on_the_emulator(emu, name, cfg):
    from chatterbox_amd import ops
    W.check_launch(ops, CPU, name, cfg)


@pytest.mark.parametrize("lengths", W.SEAMS, ids=lambda t: "-".join(map(str, t)))
def test_wave_edges_at_the_block_seams_on_the_emulator(emu, lengths):
    from chatterbox_amd import ops
    W.check_seams(ops, CPU, lengths)


def test_the_cases_the_shapes_are_chosen_for_are_what_they_claim():
    W.what_the_sets_cover()


def test_emulated_entries_refuse_the_same_descriptors_and_run_the_good_one(emu):
    good_e, good_j, rec, out, keep = _descriptor_errors(emu)
    for i in range(4000):
        out[i] = 7.0
    assert emu.cbx_wave_edges_f32(*good_e) == 0      # all-zero rows: nothing is live
    assert list(rec)[3:] == [0, 0, 0, 0]
    args = list(good_j)
    args[11] = 1940                                   # exactly sum n + sum gaps
    assert emu.cbx_wave_join_f32(*args) == 0 and list(rec)[:3] == [0, 0, 0] and all(v == 7.0 for v in out), "empty kept parts: no samples, no gaps"


def test_wrapper_refuses_bad_rows_and_join_dicts(emu):
    from chatterbox_amd import ops
    big = torch.zeros(2, 960)
    with pytest.raises(ValueError, match="different allocations"):
        ops.wave_join([big[0], torch.zeros(960)], [0, 0])
    with pytest.raises(ValueError, match="unit stride"):
        ops.wave_join([big[0, ::2]], [0])
    with pytest.raises(ValueError, match="rows"):
        ops.wave_join([], [])
    with pytest.raises(ValueError, match="gaps"):
        ops.wave_join([big[0], big[1]], [0])
    ok = dict(gaps=[1, 2])
    assert ops.check_join(None, 2) is None
    assert ops.check_join(ok, 2) == dict(gaps=[1, 2], trim_db=None, pad_frames=2, fade=240, first=True, last=True)
    full = dict(gaps=[0, 5], trim_db=40, pad_frames=0, fade=0, first=False, last=True)
    assert ops.check_join(full, 2) == dict(full, trim_db=40.0) and ops.check_join(ops.check_join(full, 2), 2) == ops.check_join(full, 2)
    for bad, err in (([1, 2], TypeError), (dict(), ValueError), (dict(gaps=[1]), ValueError), (dict(gaps=[1, -2]), ValueError), (dict(gaps=[1, 2.0]), TypeError),
                     (dict(gaps=[1, True]), TypeError), (dict(ok, trim_db="40"), TypeError), (dict(ok, trim_db=-1), ValueError), (dict(ok, trim_db=float("nan")), ValueError),
                     (dict(ok, fade=-1), ValueError), (dict(ok, fade=1.5), TypeError), (dict(ok, pad_frames=-1), ValueError), (dict(ok, first=1), TypeError),
                     (dict(ok, last=None), TypeError), (dict(ok, pause=1), ValueError)):
        with pytest.raises(err, match="join"):
            ops.check_join(bad, 2)


# ----------------------------------------------------------------------------- the public classes over a recording engine (nothing is launched)
N_SRC = 4800  # samples the recording engines "synthesise" per chunk; they keep [480, 4320) of each


def _piece(text_tokens, kw):
    """What an engine returns for a job with join=: the layout of the definition over N_SRC-sample rows of which [480, 4320) is kept."""
    j, R = kw["join"], len(text_tokens)
    table = [(480, 4320)] * R
    offs, total = W.layout([N_SRC] * R, table, j["gaps"], j["last"])
    wav = torch.cat([torch.full((total,), 0.0)])
    for r, t in enumerate(text_tokens):
        wav[offs[r]: offs[r] + 3840] = float(t.numel())
    return dict(wav=wav, offsets=offs, total=total, edges=table, n=[N_SRC] * R, truncated=[int(t.numel()) % 2 == 0 for t in text_tokens])


class _LongSerial(_FakeSerialEngine):
    def synthesize(self, text_tokens, t3_conds, gen_ref, **kw):
        if "join" not in kw:
            return super().synthesize(text_tokens, t3_conds, gen_ref, **kw)
        self.calls.append(("synthesize", dict(text_tokens=text_tokens, **kw)))
        return _piece(text_tokens, kw), [torch.full((2,), int(t.numel())) for t in text_tokens]


class _LongEngine(_LongSerial, _FakeEngine):
    def synthesize_pipelined(self, jobs, **kw):
        if not any("join" in j for j in jobs):
            yield from _FakeEngine.synthesize_pipelined(self, jobs, **kw)
            return
        self.calls.append(("pipelined", dict(jobs=jobs, **kw)))
        for job in jobs:
            yield _piece(job["text_tokens"], job), [torch.full((2,), int(t.numel())) for t in job["text_tokens"]], 0.0


LONG_TEXT = "Aaaa bbbb cc. Dd eeee! Ffffff gg hh?\n\nIiii jj. Kk llll mmmm."   # five sentences of 13, 8, 13, 8, 14 characters; two paragraphs
CHUNKS = ["Aaaa bbbb cc.", "Dd eeee!", "Ffffff gg hh?", "Iiii jj.", "Kk llll mmmm."]
KINDS = [("ChatterboxTTS", 2, ()), ("ChatterboxMultilingualTTS", 2, ("en",)), ("ChatterboxTurboTTS", 0, ())]


def _jobs(calls):
    return [j for kind, kw in calls for j in (kw["jobs"] if kind == "pipelined" else [kw])]


@pytest.mark.parametrize("cls_name,extra,lang", KINDS)
@pytest.mark.parametrize("max_batch", [None, 2])
def test_generate_long_plans_its_chunks_gaps_seeds_and_flags(cls_name, extra, lang, max_batch):
    from chatterbox_amd import api
    eng = _LongEngine() if cls_name != "ChatterboxTurboTTS" else _LongSerial()
    m = _tts(getattr(api, cls_name), eng)
    m.max_batch = max_batch
    conds = m.conds
    wav, seg = m.generate_long(LONG_TEXT, *lang, max_chars=14, seed=11, speed=1.25, temperature=0.7, top_p=0.9, return_segments=True)
    assert m.conds is conds
    sizes = [4, 1] if max_batch is None else [2, 2, 1]   # (_FakeT3.MAX_BATCH = 4)
    pipelined = cls_name != "ChatterboxTurboTTS"
    assert [k for k, _ in eng.calls] == (["pipelined"] if pipelined else ["synthesize"] * len(sizes)), "several batches: the throughput schedule where the engine has one"
    jobs = _jobs(eng.calls)
    assert [len(j["text_tokens"]) for j in jobs] == sizes
    assert [int(t.numel()) for j in jobs for t in j["text_tokens"]] == [len(c) + extra for c in CHUNKS], "text order, no length sort"
    gap, para = round(0.15 * 24000 / 1.25), round(0.4 * 24000 / 1.25)
    assert (gap, para) == (2880, 7680)
    assert [g for j in jobs for g in j["join"]["gaps"]] == [gap, gap, para, gap, gap], "the paragraph gap sits behind the paragraph's last chunk; both are divided by speed"
    assert [j["seeds"] for j in jobs] == (lambda s: [s[:4], s[4:]] if max_batch is None else [s[:2], s[2:4], s[4:]])([api.chunk_seed(11, k) for k in range(5)])
    assert jobs[0]["seeds"][0] == 11
    assert [(j["join"]["first"], j["join"]["last"]) for j in jobs] == [(g == 0, g == len(jobs) - 1) for g in range(len(jobs))]
    for j in jobs:
        assert j["speed"] == [1.25] * len(j["text_tokens"]) and j["temperature"] == 0.7 and j["top_p"] == 0.9
        assert (j["join"]["trim_db"], j["join"]["pad_frames"], j["join"]["fade"]) == (40.0, 2, 240)
    # the result: the pieces concatenated, segments in samples of the result
    assert wav.shape == (1, seg[-1]["stop"]) and wav.dtype == torch.float32
    assert [s["text"] for s in seg] == CHUNKS and all((s["src_start"], s["src_stop"]) == (480, 4320) and s["stop"] - s["start"] == 3840 for s in seg)
    assert [b["start"] - a["stop"] for a, b in zip(seg, seg[1:])] == [gap, gap, para, gap]
    for s, c in zip(seg, CHUNKS):
        assert bool((wav[0, s["start"]: s["stop"]] == len(c) + extra).all()) and s["tokens"].tolist() == [len(c) + extra] * 2 and s["truncated"] == ((len(c) + extra) % 2 == 0)
    assert float(wav[0, seg[0]["stop"]: seg[1]["start"]].abs().max()) == 0.0
    assert torch.is_tensor(m.generate_long(LONG_TEXT, *lang, max_chars=14)), "without return_segments: the waveform alone"
    eng.calls.clear()
    m.generate_long("Aaaa bbbb cc. Dd eeee!", *lang, max_chars=14)
    assert [k for k, _ in eng.calls] == ["synthesize"] and len(eng.calls[0][1]["text_tokens"]) == 2, "one batch: the serial schedule"


@pytest.mark.parametrize("cls_name,extra,lang", KINDS)
def test_generate_long_defaults_add_nothing_to_the_jobs(cls_name, extra, lang, caplog):
    """No seed: no seeds key (the call draws as generate_batch does); speed 1.0: no speed key; trim_db=None reaches the join; one warning names the truncated chunks."""
    from chatterbox_amd import api
    eng = _LongEngine()
    m = _tts(getattr(api, cls_name), eng)
    with caplog.at_level(logging.WARNING, logger="chatterbox_amd.api"):
        m.generate_long(LONG_TEXT, *lang, max_chars=14, trim_db=None, trim_pad=0, join_fade=0, pause=0, paragraph_pause=1)
    jobs = _jobs(eng.calls)
    assert all("seeds" not in j and "speed" not in j for j in jobs)
    assert [j["join"] for j in jobs] == [dict(gaps=[0, 0, 24000, 0], trim_db=None, pad_frames=0, fade=0, first=True, last=False),
                                         dict(gaps=[0], trim_db=None, pad_frames=0, fade=0, first=False, last=True)]
    cut = [k for k, c in enumerate(CHUNKS) if (len(c) + extra) % 2 == 0]
    msgs = [r.getMessage() for r in caplog.records if "generate_long" in r.getMessage()]
    assert len(msgs) == 1 and str(cut) in msgs[0] and "max_chars" in msgs[0]
    eng.calls.clear()
    m.generate_long("", *lang)
    (job,) = _jobs(eng.calls)
    assert len(job["text_tokens"]) == 1 and int(job["text_tokens"][0].numel()) == len("You need to add some text for me to talk.") + extra, "the fallback sentence, as generate('') speaks it"
    eng.calls.clear()
    m.generate_long("字" * 250, *lang)
    n_chunks = sum(len(j["text_tokens"]) for j in _jobs(eng.calls))
    assert n_chunks == 1, "300 characters per chunk unless the language is zh / ja / ko"
    if lang:
        eng.calls.clear()
        m.generate_long("字" * 250, "zh")
        assert sum(len(j["text_tokens"]) for j in _jobs(eng.calls)) == 3, "100 characters per chunk for zh / ja / ko"


@pytest.mark.parametrize("cls_name,extra,lang", KINDS)
def test_generate_long_validates_before_the_engine_is_called(cls_name, extra, lang):
    from chatterbox_amd import api
    eng = _LongEngine()
    m = _tts(getattr(api, cls_name), eng)
    bad = [(dict(max_chars=0), ValueError, "max_chars"), (dict(max_chars=2.5), TypeError, "max_chars"), (dict(max_chars=True), TypeError, "max_chars"),
           (dict(pause=-0.1), ValueError, "pause"), (dict(pause="1"), TypeError, "pause"), (dict(pause=float("nan")), ValueError, "pause"),
           (dict(paragraph_pause=float("inf")), ValueError, "paragraph_pause"), (dict(paragraph_pause=None), TypeError, "paragraph_pause"),
           (dict(trim_db=-3), ValueError, "trim_db"), (dict(trim_db="40"), TypeError, "trim_db"), (dict(trim_db=float("nan")), ValueError, "trim_db"),
           (dict(trim_pad=-1), ValueError, "trim_pad"), (dict(trim_pad=1.0), TypeError, "trim_pad"), (dict(join_fade=-1), ValueError, "join_fade"),
           (dict(join_fade=True), TypeError, "join_fade"), (dict(seed=-1), ValueError, "seed"), (dict(seed=2 ** 64), ValueError, "seed"), (dict(seed=1.0), TypeError, "seed"),
           (dict(speed=0.3), ValueError, "speed"), (dict(speed="1"), TypeError, "speed"), (dict(speed=[1.0, 1.0]), ValueError, "speed"),
           (dict(temperature="hot"), TypeError, "temperature"), (dict(top_p=float("nan")), ValueError, "top_p"), (dict(temperature=[0.8]), TypeError, "temperature")]
    for kw, err, name in bad:
        with pytest.raises(err, match=name):
            m.generate_long(LONG_TEXT, *lang, **kw)
            print("did not raise:", kw)
    with pytest.raises(TypeError, match="text"):
        m.generate_long(["a", "b"], *lang)
    if lang:
        with pytest.raises(ValueError, match="language_id"):
            m.generate_long(LONG_TEXT, "xx")
    assert eng.calls == []


@pytest.mark.parametrize("cls_name,extra,lang", KINDS)
def test_generate_and_generate_batch_are_recorded_exactly_as_before(cls_name, extra, lang):
    """The existing entry points know nothing of the feature: no join key reaches the engine, and the calls are those the seeded-RNG tests record."""
    from chatterbox_amd import api
    eng = _LongEngine() if cls_name != "ChatterboxTurboTTS" else _LongSerial()
    m = _tts(getattr(api, cls_name), eng)
    m.generate("aaaa.", *lang, seed=3)
    kind, kw = eng.calls[-1]
    base = dict(max_new_tokens=1000, drop_last_token=bool(lang)) if cls_name != "ChatterboxTurboTTS" else {}
    samp = (dict(temperature=0.8, cfg_weight=0.5, repetition_penalty=1.2, min_p=0.05, top_p=1.0) if cls_name != "ChatterboxTurboTTS"
            else dict(temperature=0.8, top_k=1000, top_p=0.95, repetition_penalty=1.2))
    assert kind == "synthesize" and {k: v for k, v in kw.items() if k != "text_tokens"} == dict(base, **samp, seeds=[3])
    eng.calls.clear()
    texts = ["x" * 8 + ".", "y.", "z" * 4 + "."]
    m.max_batch = 2
    out = m.generate_batch(texts, *lang, seeds=[1, 2, 3])
    assert [int(w[0, 0]) for w in out] == [9 + extra, 2 + extra, 5 + extra]
    jobs = _jobs(eng.calls)
    assert [len(j["text_tokens"]) for j in jobs] == [2, 1] and all("join" not in j for j in jobs) and [j["seeds"] for j in jobs] == [[2, 3], [1]]


def test_vocode_joins_on_the_stream_of_the_waveforms(monkeypatch):
    """ChatterboxEngine.vocode over stand-in stages on the CPU: join=None makes no ops.wave_join call and returns the list of views as ever; with a join dict the
    views (of one padded tensor, in row order, each cut as the call without it cuts them) go to ONE ops.wave_join call with the checked arguments, and its piece
    is what the call returns."""
    from chatterbox_amd import engine, ops, synth
    eng = engine.ChatterboxEngine.__new__(engine.ChatterboxEngine)
    eng.dev, eng.last_timing = CPU, {}
    eng.flow = type("Flow", (), {"precision": 1, "inference": lambda self, tok, lens, ref, **kw: torch.ones(tok.shape[0], 2 * tok.shape[1], 80)})()
    eng.hift = type("Hift", (), {"precision": 1, "inference": staticmethod(lambda mel, lens=None, **kw: (torch.arange(mel.shape[0] * 480 * mel.shape[1], dtype=torch.float32).view(mel.shape[0], -1), None))})()
    calls = []
    monkeypatch.setattr(ops, "wave_join", lambda rows, **kw: calls.append((rows, kw)) or "piece")
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: None)
    ref = synth.s3gen_ref(n_prompt_tokens=6)
    st = [synth.speech_tokens(n, seed=k) for k, n in enumerate((12, 5, 9))]
    base, _ = eng.vocode(st, ref, drop_last_token=True)
    assert calls == [] and [w.numel() for w in base] == [960 * 11, 960 * 4, 960 * 8]
    got, mel = eng.vocode(st, ref, drop_last_token=True, join=dict(gaps=[5, 0, 7], trim_db=40, fade=100, last=False))
    assert got == "piece" and mel.shape == (3, 24, 80) and len(calls) == 1
    rows, kw = calls[0]
    assert kw == dict(gaps=[5, 0, 7], trim_db=40.0, pad_frames=2, fade=100, first=True, last=False)
    assert all(torch.equal(a, b) for a, b in zip(rows, base)) and len({r.untyped_storage().data_ptr() for r in rows}) == 1
    with pytest.raises(ValueError, match="join"):
        eng.vocode(st, ref, join=dict(gaps=[1, 2]))
    assert len(calls) == 1
