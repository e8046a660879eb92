"""Host tests (no GPU) of the dialogue feature: cbx_wave_mix_f32's C ABI and its refusals, every kernel case of wave_mix_common.py on the SIMT emulator (bitwise
against the NumPy oracle there), ops.mix_layout, api.dialogue_plan, and generate_dialogue of the three TTS classes over the recording engines of the existing
host tests, with nothing launched: the device steps of the finish are replaced by recorders (the mixer by the oracle itself)."""
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

import wave_mix_common as C  # noqa: E402
from test_seeded_rng_host import _tts  # noqa: E402  (read-only import: the model over a recording engine)
from test_wave_join_host import KINDS, LONG_TEXT, _jobs, _LongEngine, _LongSerial  # noqa: E402  (read-only import: the engines that know a joined piece)

CPU = torch.device("cpu")
ENTRY = "cbx_wave_mix_f32"
T = 4096
CASES = C.cases(T)


# ----------------------------------------------------------------------------- C ABI
def test_the_entry_is_declared_exported_bound_and_emulated_without_a_version_step():
    from chatterbox_amd import _lib, ops
    import harness
    hdr = open(os.path.join(ROOT, "include", "cbx.h")).read()
    lib = ctypes.CDLL(os.path.join(ROOT, "chatterbox_amd", "libcbx_hip.so"))
    emu = harness.load_emu()
    assert re.search(rf"^int {ENTRY}\(", hdr, re.M) and hasattr(lib, ENTRY) and ENTRY in _lib._SIGS and hasattr(emu, ENTRY)
    assert len(_lib._SIGS[ENTRY][0]) == len(re.search(rf"^int {ENTRY}\((.*?)\);", hdr, re.M | re.S).group(1).split(",")) == 15
    assert "#define CBX_ABI_VERSION 16" in hdr and _lib.lib.cbx_abi_version() == 16 and _lib.ABI_VERSION == 16 and emu.cbx_abi_version() == 16, "new function only: no version step"
    block = hdr[hdr.index("---- dialogue"): hdr.index(f"int {ENTRY}(")]
    assert "ASCENDING r" in block and "order of summation" in block, "the header states the order of summation"
    assert "The\n * reference has no counterpart" in block and all(ref in block for ref in ("tts.py:272", "mtl_tts.py:352", "tts_turbo.py:320"))
    assert "start_r = max(0, front + pending)" in block and "-22 before any launch" in block, "the layout rule and the refusals"
    src = open(os.path.join(ROOT, "chatterbox_amd", "csrc", "wave_mix.hip")).read()
    assert "tts.py:272" in src and f"WM_TILE = {ops.WAVE_MIX_TILE}" in src and ops.WAVE_MIX_TILE == T
    assert callable(ops.mix_layout) and callable(ops.wave_mix)


def test_descriptor_errors_return_a_status_and_a_message():
    """the product library on host buffers: every refusal comes before a launch"""
    from chatterbox_amd import _lib, ops
    C.check_refusals(_lib.lib, ops, CPU, None, run_good=False)


def test_mix_layout():
    from chatterbox_amd import ops
    C.check_mix_layout(ops)


def test_the_oracle_states_the_order_of_summation():
    c = CASES["order"]
    ref = C.oracle(c["rows"], c["starts"], c["flags"], c["out_len"])
    assert C.bits(ref[[500, T - 1]]).tolist() == [0, 0]
    rev = C.oracle(c["rows"][::-1], c["starts"][::-1], c["flags"], c["out_len"])
    assert rev[[500, T - 1]].tolist() == [2.0, 2.0], "descending order gives 2.0: the case separates the orders"


# ----------------------------------------------------------------------------- the kernel on the SIMT emulator
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


@pytest.mark.parametrize("check", ["order", "gap", "gain_null", "split", "nan"])
def test_a_property_of_the_definition(emu, check):
    from chatterbox_amd import ops
    getattr(C, f"check_{check}")(ops, T)


def test_non_negative_gaps_give_the_joins_bits(emu):
    from chatterbox_amd import ops
    C.check_join(ops)


def test_the_emulated_entry_refuses_the_same_descriptors_and_ops_checks_its_arguments(emu):
    from chatterbox_amd import ops
    C.check_refusals(emu, ops, CPU, None)
    x = torch.from_numpy(C.noise(100, 1))
    out = torch.full((120,), 7.0)
    assert ops.wave_mix([x[:0], x[:0]], [0, 120], [3, 3], out) is out and float(out.abs().max()) == 0.0, "empty rows alone: zeros, no launch"
    out.fill_(7.0)
    assert float(ops.wave_mix([x[:0]], [5], [0], out, accumulate=True).min()) == 7.0
    with pytest.raises(ValueError, match="different allocations"):
        ops.wave_mix([torch.zeros(8), torch.zeros(8)], [0, 0], [0, 0], out)
    with pytest.raises(ValueError, match="starts"):
        ops.wave_mix([x[:50], x[50:]], [0], [0, 0], out)
    with pytest.raises(ValueError, match="gain indices"):
        ops.wave_mix([x[:50], x[50:]], [0, 0], [0, 0], out, gain=torch.ones(2), gain_idx=[0])
    with pytest.raises(Exception, match="wave_mix"):
        ops.wave_mix([x[:50], x[50:]], [0, 80], [0, 0], out)   # the second row would end at 130 > 120: the entry's refusal, raised


# ----------------------------------------------------------------------------- api.dialogue_plan
def _a(**over):
    return dict(dict(max_chars=14, pause=0.15, paragraph_pause=0.4, trim_db=40.0, trim_pad=2, join_fade=240, seed=11, speed=None), **over)


def test_dialogue_plan_keeps_script_order_cuts_batches_and_seeds_chunks_over_the_whole_script():
    from chatterbox_amd import api
    from chatterbox_amd.text import split_text
    texts = ["Aaaa bbbb cc. Dd eeee!\n\nFfffff gg hh?", "Iiii jj.", "Kk llll mmmm. Nn oo."]
    turns = [dict(chunks=split_text(t, 14), gap=g, speed=s) for t, g, s in zip(texts, (9.0, -0.2, 0.5), (None, None, 1.25))]
    assert [len(t["chunks"]) for t in turns] == [3, 1, 2]
    plan = api.dialogue_plan(turns, 4, _a())
    assert [r["text"] for r in plan["rows"]] == ["Aaaa bbbb cc.", "Dd eeee!", "Ffffff gg hh?", "Iiii jj.", "Kk llll mmmm.", "Nn oo."], "script order"
    assert [r["turn"] for r in plan["rows"]] == [0, 0, 0, 1, 2, 2]
    # inner chunks: pause / paragraph_pause over the turn's speed; a turn's last chunk: the NEXT turn's gap, not scaled; the first turn's gap is not used
    assert [r["after"] for r in plan["rows"]] == [3600, 9600, -4800, 12000, round(0.15 * 24000 / 1.25), 0]
    assert [j["chunks"] for j in plan["jobs"]] == [[0, 1, 2, 3], [4, 5]], "consecutive batches of at most max_batch, no length sort"
    assert [j["seeds"] for j in plan["jobs"]] == [[api.chunk_seed(11, k) for k in j["chunks"]] for j in plan["jobs"]] and plan["jobs"][0]["seeds"][0] == 11
    assert [j["join"] for j in plan["jobs"]] == [dict(gaps=[0] * n, trim_db=40.0, pad_frames=2, fade=0, first=True, last=True) for n in (4, 2)]
    assert [j["speed"] for j in plan["jobs"]] == [[1.0] * 4, [1.25, 1.25]] and all("pitch" not in j for j in plan["jobs"])
    assert [len(j["chunks"]) for j in api.dialogue_plan(turns, 100, _a())["jobs"]] == [6]
    many = api.dialogue_plan([dict(chunks=[("x.", True)] * 70, gap=0.0)], 100, _a(seed=None, trim_db=None))
    assert [len(j["chunks"]) for j in many["jobs"]] == [64, 6] and all("seeds" not in j and "speed" not in j for j in many["jobs"]), "at most 64 rows: the mixer's limit"
    assert many["jobs"][0]["join"]["trim_db"] is None
    pitched = api.dialogue_plan([dict(chunks=[("x.", True)], gap=0.0, pitch=2.0), dict(chunks=[("y.", True)], gap=0.0)], 1, _a())
    assert [j.get("pitch") for j in pitched["jobs"]] == [[2.0], None]


# ----------------------------------------------------------------------------- generate_dialogue over the recording engines (nothing is launched)
def _voices():
    from chatterbox_amd import api, synth
    return {k: api.Conditionals(api.T3Cond(**synth.t3_cond()), synth.s3gen_ref(n_prompt_tokens=8)) for k in ("a", "b")}


def _model(cls_name, max_batch=2):
    from chatterbox_amd import api
    eng = _LongEngine() if cls_name != "ChatterboxTurboTTS" else _LongSerial()
    m = _tts(getattr(api, cls_name), eng)
    m.max_batch = max_batch
    return m, eng


def _lang_kw(lang):
    return dict(language_id=lang[0]) if lang else {}


class _Mark:
    def __init__(self, log):
        self.log = log

    def apply_watermark(self, wav, sample_rate):
        self.log.append(("watermark", wav.copy()))
        return wav * 2.0


def _record(monkeypatch, log):
    """the device steps of the finish as recorders; the mixer computes the oracle's result"""
    from chatterbox_amd import ops

    def mix(rows, starts, flags, out, gain=None, gain_idx=None, fade=240, accumulate=False):
        log.append(("mix", dict(n=[int(r.numel()) for r in rows], starts=list(starts), flags=list(flags), gain=gain, gain_idx=gain_idx, fade=fade, accumulate=accumulate)))
        res = C.oracle([r.numpy() for r in rows], starts, flags, out.numel(), None if gain is None else gain.tolist(), gain_idx, fade, prev=out.numpy().copy() if accumulate else None)
        return out.copy_(torch.from_numpy(res))

    def loudness(rows, target=None, ceiling=1.0, fs=24000):
        log.append(("loudness", [r.clone() for r in rows], target, ceiling, {r.untyped_storage().data_ptr() for r in rows}))
        return torch.tensor([[-30.0 - r, 0.5, 2.0 + r, 9.0] for r in range(len(rows))], dtype=torch.float64), torch.tensor([2.0 + r for r in range(len(rows))])

    def limit(rows, ceilings_db, gain=None, look=120, out=None):
        log.append(("limit", [r.clone() for r in rows], ceilings_db, gain))
        return [rows[0] * 0.5], "limit stats"
    monkeypatch.setattr(ops, "wave_mix", mix)
    monkeypatch.setattr(ops, "wave_loudness", loudness)
    monkeypatch.setattr(ops, "wave_limit", limit)
    monkeypatch.setattr(ops, "wave_normalize", lambda rows, target, **k: log.append(("normalize", [r.clone() for r in rows], target)) or "normalize stats")
    monkeypatch.setattr(ops, "wave_format", lambda rows, fmt: log.append(("format", [r.clone() for r in rows], fmt)) or [torch.zeros(2, dtype=torch.int16)])


SCRIPT = [("a", "Aaaa bbbb cc. Dd eeee!"), ("b", "Ffffff gg hh?"), dict(voice="a", text="Iiii jj.", gap=-0.2, speed=1.25), (None, "Kk llll mmmm.")]
STARTS = [0, 7440, 18480, 17520, 29520]   # 3840 kept samples per chunk; after = 3600, 7200, -4800, 7200, 0 (ops.mix_layout's walk, by hand)
TOTAL = 33360


@pytest.mark.parametrize("cls_name,extra,lang", KINDS)
def test_the_jobs_carry_per_row_voices_and_the_zero_gap_zero_fade_join_and_the_finish_is_held_back(cls_name, extra, lang, monkeypatch):
    from chatterbox_amd import api
    m, eng = _model(cls_name)
    voices, conds = _voices(), m.conds
    log = []
    _record(monkeypatch, log)
    recorded = []
    run_jobs = m._run_jobs
    monkeypatch.setattr(m, "_run_jobs", lambda jobs, kw: recorded.extend(jobs) or run_jobs(jobs, kw))
    wav, seg = m.generate_dialogue(SCRIPT, voices, **_lang_kw(lang), max_chars=14, seed=11, temperature=0.7, return_segments=True)
    assert m.conds is conds, "self.conds is never written"
    jobs = _jobs(eng.calls)
    assert [len(j["text_tokens"]) for j in jobs] == [2, 2, 1] and [int(t.numel()) for j in jobs for t in j["text_tokens"]] == [13 + extra, 8 + extra, 13 + extra, 8 + extra, 13 + extra]
    assert [j["join"] for j in jobs] == [dict(gaps=[0] * n, trim_db=40.0, pad_frames=2, fade=0, first=True, last=True) for n in (2, 2, 1)]
    assert [j["seeds"] for j in jobs] == (lambda s: [s[:2], s[2:4], s[4:]])([api.chunk_seed(11, k) for k in range(5)])
    assert [j["speed"] for j in jobs] == [[1.0, 1.0], [1.0, 1.25], [1.0]] and all(j["temperature"] == 0.7 for j in jobs)
    assert all(not {"loudness", "true_peak", "format", "pitch", "guard", "words"} & set(j) for j in jobs)
    # the voices of the rows: a a | b a | the model's own
    ex = 0.0 if cls_name == "ChatterboxTurboTTS" else 0.5
    da, db, d0 = (api._t3_dict(c.t3, ex) for c in (voices["a"], voices["b"], conds))
    assert recorded[0]["t3_conds"] is da and recorded[0]["gen_ref"] is voices["a"].gen, "one voice in the batch: the engines' single-voice path"
    assert [d is w for d, w in zip(recorded[1]["t3_conds"], (db, da))] == [True, True] and [g is w for g, w in zip(recorded[1]["gen_ref"], (voices["b"].gen, voices["a"].gen))] == [True, True]
    assert recorded[2]["t3_conds"] is d0 and recorded[2]["gen_ref"] is conds.gen
    assert [e[0] for e in log] == ["mix"] and log[0][1]["accumulate"] is False and log[0][1]["n"] == [3840] * 5, "ONE launch over the rows of all three pieces"
    assert [s for e in log for s in e[1]["starts"]] == STARTS and all(e[1]["gain"] is None and e[1]["gain_idx"] is None and e[1]["fade"] == 240 for e in log)
    assert [f for e in log for f in e[1]["flags"]] == [3] * 5, "480 samples were trimmed at either end of every chunk: every row fades in and out"
    assert wav.shape == (1, TOTAL) and wav.dtype == torch.float32 and m.last_balance is None
    assert [(s["turn"], s["voice"], s["text"]) for s in seg] == [(0, "a", "Aaaa bbbb cc."), (0, "a", "Dd eeee!"), (1, "b", "Ffffff gg hh?"), (2, "a", "Iiii jj."), (3, None, "Kk llll mmmm.")]
    assert [(s["start"], s["stop"], s["src_start"], s["src_stop"]) for s in seg] == [(a, a + 3840, 480, 4320) for a in STARTS]
    assert seg[2]["stop"] - seg[3]["start"] == 4800, "turn 2 comes in 0.2 s before turn 1 has finished"
    assert [s["truncated"] for s in seg] == [(n + extra) % 2 == 0 for n in (13, 8, 13, 8, 13)] and all(set(s) == {"turn", "voice", "text", "start", "stop", "src_start", "src_stop", "truncated"} for s in seg)
    # the overlap is a SUM: the middle of the overlap holds both chunks' values (the engines fill a chunk with its token count)
    assert float(wav[0, 22000]) == 13.0 + extra and float(wav[0, 18000]) == 8.0 + extra and float(wav[0, 20000]) == (13.0 + extra) + (8.0 + extra) and float(wav[0, 7440 - 1]) == 0.0
    assert torch.is_tensor(m.generate_dialogue(SCRIPT, voices, **_lang_kw(lang), max_chars=14)), "without return_segments: the waveform alone"
    assert all("seeds" not in j for j in _jobs(eng.calls)[3:]), "no seed: no seeds key"


@pytest.mark.parametrize("cls_name,extra,lang", KINDS)
def test_the_finish_runs_meter_mix_loudness_limit_watermark_format_in_one_visit(cls_name, extra, lang, monkeypatch):
    m, eng = _model(cls_name)
    voices = _voices()
    log = []
    _record(monkeypatch, log)
    base = m.generate_dialogue(SCRIPT, voices, **_lang_kw(lang), max_chars=14, seed=11, balance=True)
    assert [e[0] for e in log] == ["loudness", "mix"]
    meter = log[0]
    assert meter[2] == [-23.0] * 3 and meter[3] == 1.0, "balance=True: -23 LUFS for every voice, sample peak limited to 1.0"
    assert [int(r.numel()) for r in meter[1]] == [3 * 3840, 3840, 3840], "ONE meter call over the V voices, each voice's rows packed back to back, in order of first appearance"
    assert len(meter[4]) == 1, "views of ONE allocation"
    assert torch.equal(meter[1][0][3840: 2 * 3840], torch.full((3840,), 8.0 + extra)) and torch.equal(meter[1][0][2 * 3840:], torch.full((3840,), 8.0 + extra))
    assert log[1][1]["gain_idx"] == [0, 0, 1, 0, 2] and log[1][1]["gain"].tolist() == [2.0, 3.0, 4.0]
    assert [(b["voice"], b["lufs"], b["gain"], b["blocks"]) for b in m.last_balance] == [("a", -30.0, 2.0, 9), ("b", -31.0, 3.0, 9), (None, -32.0, 4.0, 9)]
    assert float(base[0, 20000]) == 2.0 * (8.0 + extra) + 3.0 * (13.0 + extra), "every voice at its own gain inside the mixer"
    log.clear()
    eng.calls.clear()
    m.watermarker = _Mark(log)
    wav = m.generate_dialogue(SCRIPT, voices, **_lang_kw(lang), max_chars=14, seed=11, balance=-20, loudness=-19, true_peak=-1.5, encoding="s16")
    assert all(not {"loudness", "true_peak", "format"} & set(j) for j in _jobs(eng.calls)), "the jobs of generate_dialogue never carry the finish"
    assert [e[0] for e in log] == ["loudness", "mix", "loudness", "limit", "watermark", "format"]
    assert log[0][2] == [-20.0] * 3 and log[2][2] == [-19.0] and log[2][3] is None, "the mix is ONE signal; the full gain where the limiter follows"
    assert len(log[2][1]) == 1 and torch.equal(log[2][1][0], base[0]) and log[3][2] == [-1.5] and torch.equal(log[3][3], torch.tensor([2.0]))
    assert np.array_equal(log[4][1], base[0].numpy() * 0.5) and torch.equal(log[5][1][0], base[0] * 0.5 * 2.0) and wav.dtype == torch.int16 and wav.shape == (1, 2)
    assert eng.last_limit == "limit stats"
    log.clear()
    m.watermarker = None
    wav, seg = m.generate_dialogue(SCRIPT, voices, **_lang_kw(lang), max_chars=14, loudness=-19, sample_rate=16000, return_segments=True)
    assert [e[0] for e in log] == ["mix", "normalize", "format"] and m.last_balance is None and eng.last_loudness == "normalize stats"
    assert [(s["start"], s["stop"]) for s in seg] == [(-(-a * 2 // 3), -(-(a + 3840) * 2 // 3)) for a in STARTS], "segment ends follow formatted_len"


def test_an_untrimmed_first_start_and_last_end_do_not_fade(monkeypatch):
    """the join's first / last rule: flags 2 .. 3 .. 1"""
    from chatterbox_amd import api
    m, eng = _model("ChatterboxTTS", max_batch=4)
    log = []
    _record(monkeypatch, log)
    synth_ = eng.synthesize

    def untrimmed(text_tokens, t3_conds, gen_ref, **kw):
        piece, st = synth_(text_tokens, t3_conds, gen_ref, **kw)
        n = len(text_tokens)
        return dict(piece, edges=[(0, 4320)] + [(480, 4320)] * (n - 2) + [(480, 4800)], n=[4800] * n, offsets=[0] + [4320 + 3840 * k for k in range(n - 1)],
                    total=2 * 4320 + 3840 * (n - 2), wav=torch.zeros(2 * 4320 + 3840 * (n - 2))), st
    monkeypatch.setattr(eng, "synthesize", untrimmed)
    m.generate_dialogue([(None, "Aaaa bbbb cc. Dd eeee! Ffffff gg hh?")], max_chars=14, join_fade=100)
    (e,) = log
    assert e[1]["flags"] == [2, 3, 1] and e[1]["fade"] == 100 and e[1]["n"] == [4320, 3840, 4320]


def test_a_script_of_more_than_64_chunks_is_mixed_in_launches_of_64(monkeypatch):
    m, eng = _model("ChatterboxTTS", max_batch=4)
    log = []
    _record(monkeypatch, log)
    wav, seg = m.generate_dialogue([(None, "Aa.")] * 70, turn_pause=0.0, return_segments=True)
    assert [(e[1]["accumulate"], len(e[1]["n"])) for e in log] == [(False, 64), (True, 6)] and len(seg) == 70
    assert wav.shape == (1, 70 * 3840) and [s["start"] for s in seg] == [3840 * k for k in range(70)]
    assert float(wav[0, 64 * 3840 + 1000]) == 5.0 and float(wav[0, 1000]) == 5.0


BAD = [
    (dict(turns=("a", "x")), TypeError, "turns"), (dict(turns=[]), ValueError, "turns"), (dict(turns=[("a",)]), TypeError, "turns"),
    (dict(turns=[dict(voice="a", text="x", foo=1)]), TypeError, "turns"), (dict(turns=[dict(voice="a")]), TypeError, "text"), (dict(turns=[("a", 5)]), TypeError, "text"),
    (dict(turns=[("a", "  ")]), ValueError, "empty"), (dict(turns=[("zz", "x")]), ValueError, "voice"), (dict(turns=[([1], "x")]), TypeError, "voice"),
    (dict(turns=[dict(text="x", gap=True)]), TypeError, "gap"), (dict(turns=[dict(text="x", gap=61)]), ValueError, "gap"),
    (dict(turns=[dict(text="x", gap=float("nan"))]), ValueError, "gap"), (dict(turns=[dict(text="x", speed=3)]), ValueError, "speed"),
    (dict(turns=[dict(text="x", speed="1")]), TypeError, "speed"), (dict(turns=[dict(text="x", speed=[1.0])]), TypeError, "speed"),
    (dict(turns=[dict(text="x", pitch=13)]), ValueError, "pitch"), (dict(turns=[dict(text="x", pitch=True)]), TypeError, "pitch"),
    (dict(turns=[dict(text="x", speed=0.5, pitch=12)]), ValueError, "pitch"), (dict(turns=[dict(text="x", exaggeration="x")]), TypeError, "exaggeration"),
    (dict(turns=[dict(text="x", exaggeration=float("inf"))]), ValueError, "exaggeration"), (dict(voices=[1]), TypeError, "voices"),
    (dict(turn_pause=True), TypeError, "turn_pause"), (dict(turn_pause=-61), ValueError, "turn_pause"), (dict(balance="loud"), TypeError, "balance"),
    (dict(balance=-3), ValueError, "balance"), (dict(balance=[-23]), TypeError, "balance"), (dict(loudness=-3), ValueError, "loudness"),
    (dict(true_peak=1), ValueError, "true_peak"), (dict(sample_rate=12345), ValueError, "sample_rate"), (dict(seed=-1), ValueError, "seed"),
    (dict(seed=1.5), TypeError, "seed"), (dict(max_chars=0), ValueError, "max_chars"), (dict(join_fade=-1), ValueError, "join_fade"),
    (dict(pause=-1), ValueError, "pause"), (dict(temperature="x"), TypeError, "temperature"),
    (dict(word_times=True), TypeError, "word_times"), (dict(max_pause=1.0), TypeError, "max_pause"), (dict(duration=3.0), TypeError, "duration"),
    (dict(timing=[0.0]), TypeError, "timing"), (dict(speed=1.25), TypeError, "speed"), (dict(audio_prompt_path="x.wav"), TypeError, "audio_prompt_path"),
]


@pytest.mark.parametrize("cls_name,extra,lang", KINDS)
def test_bad_arguments_raise_at_the_call_before_the_engine_is_touched(cls_name, extra, lang, monkeypatch):
    from chatterbox_amd import api
    m, eng = _model(cls_name)
    voices = _voices()
    monkeypatch.setattr(m, "_analyse", lambda *a, **k: pytest.fail("the voice analysis is not touched"))
    for over, err, match in BAD:
        kw = dict(dict(turns=[("a", "Aaaa.")], voices=dict(voices, c="prompt.wav")), **_lang_kw(lang), **over)
        with pytest.raises(err, match=match):
            m.generate_dialogue(kw.pop("turns"), kw.pop("voices"), **kw)
    many = {k: voices["a"] for k in range(65)}
    with pytest.raises(ValueError, match="balance"):
        m.generate_dialogue([(k, "x.") for k in range(65)], many, **_lang_kw(lang), balance=True)
    if cls_name == "ChatterboxTurboTTS":
        with pytest.raises(TypeError, match="guard"):
            m.generate_dialogue([("a", "x.")], voices, guard=True)
    else:
        with pytest.raises(ValueError, match="guard"):
            m.generate_dialogue([("a", "x.")], voices, **_lang_kw(lang), guard="x")
    if lang:
        with pytest.raises(ValueError, match="language_id"):
            m.generate_dialogue([dict(voice="a", text="x.", language_id="xx")], voices, language_id="en")
        with pytest.raises(ValueError, match="language_id"):
            m.generate_dialogue([("a", "x.")], voices, language_id="xx")
        with pytest.raises(TypeError, match="language_id"):
            m.generate_dialogue([dict(voice="a", text="x.", language_id=5)], voices, language_id="en")
    else:
        with pytest.raises(TypeError):
            m.generate_dialogue([dict(voice="a", text="x.", language_id="en")], voices)
    m.conds = None
    with pytest.raises(AssertionError, match="prepare_conditionals"):
        m.generate_dialogue([(None, "x.")], voices, **_lang_kw(lang))
    assert eng.calls == []
    sig = inspect.signature(m.generate_dialogue).parameters
    assert sig["turn_pause"].default == api.DIALOGUE_TURN_PAUSE == 0.3 and api.DIALOGUE_BALANCE == -23.0 and sig["voices"].default is None
    assert all(sig[k].kind is inspect.Parameter.KEYWORD_ONLY for k in sig if k not in ("turns", "voices"))
    assert "UNMEASURED" in api.ChatterboxTTS.generate_dialogue.__doc__ and not hasattr(api.ChatterboxVC, "generate_dialogue")


@pytest.mark.parametrize("cls_name,extra,lang", KINDS)
def test_prompts_in_voices_are_analysed_once_per_call_and_a_guard_travels_with_every_job(cls_name, extra, lang, monkeypatch):
    m, eng = _model(cls_name)
    voices = _voices()
    log, seen = [], []
    _record(monkeypatch, log)
    monkeypatch.setattr(m, "_analyse", lambda wav, ex, **kw: seen.append((wav, ex, kw)) or voices["b"])
    script = [("p", "Aaaa."), ("q", "Bbbb."), ("p", "Cccc."), ("a", "Dddd.")]
    m.generate_dialogue(script, dict(voices, p="one.wav", q="one.wav"), **_lang_kw(lang))
    assert [s[0] for s in seen] == ["one.wav"], "equal prompts are analysed once per call"
    if cls_name != "ChatterboxTurboTTS":
        eng.calls.clear()
        eng.last_guard = ["r0", "r1"]
        monkeypatch.setattr(m, "_take_guard", lambda reports, who: log.append(("guard", list(reports), who)))
        _, seg = m.generate_dialogue(script, dict(voices, p=voices["a"], q=voices["b"]), **_lang_kw(lang), guard=True, return_segments=True)
        assert all(isinstance(j["guard"], dict) for j in _jobs(eng.calls)) and [s["guard"] for s in seg] == ["r0", "r1", "r0", "r1"]
        assert [e for e in log if e[0] == "guard"] == [("guard", ["r0", "r1", "r0", "r1"], "generate_dialogue")]


def _norm(obj):
    if torch.is_tensor(obj):
        return ("T", obj.tolist())
    if isinstance(obj, dict):
        return {k: _norm(v) for k, v in obj.items()}
    if isinstance(obj, (list, tuple)):
        return [_norm(v) for v in obj]
    return obj


@pytest.mark.parametrize("cls_name,extra,lang", KINDS)
def test_the_existing_methods_record_the_same_engine_calls_before_and_after_a_dialogue(cls_name, extra, lang, monkeypatch, caplog):
    m, eng = _model(cls_name)
    _record(monkeypatch, [])

    def existing():
        eng.calls.clear()
        m.generate("aaaa.", *lang, seed=3)
        m.generate_batch(["x.", "yy.", "zzz."], *lang, seeds=[1, 2, 3])
        m.generate_long(LONG_TEXT, *lang, max_chars=14, seed=11)
        return _norm(eng.calls)
    with caplog.at_level(logging.ERROR):
        before, conds = existing(), m.conds
        m.generate_dialogue(SCRIPT, _voices(), **_lang_kw(lang), max_chars=14, seed=5, balance=True)
        assert existing() == before and m.conds is conds
