"""CPU (-m "not gpu"): word timestamps -- both kernels on the SIMT emulator against the NumPy restatements (word_times_common.py), their C ABI and refused
descriptors, text.word_groups, the frame -> sample mapping, and the plumbing of word_times= on the public classes over recording engines (nothing is launched).
The recording engines build on those of test_seeded_rng_host.py (a read-only import)."""
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

import word_times_common as W  # noqa: E402
from test_seeded_rng_host import _FakeEngine, _FakeSerialEngine, _tts  # noqa: E402  (read-only import: the recording engines)

CPU = torch.device("cpu")


@pytest.fixture(scope="module")
def emu():
    import build_emu
    if not os.path.exists(build_emu.CLANG):
        pytest.skip("ROCm's clang++ (x86 host compiler of the emulator build) is not installed")
    import harness
    with harness.emulated() as lib:
        yield lib


def _cols(rows):
    return [[r[i] for r in rows] for i in range(4)]


# ----------------------------------------------------------------------------- the kernels on the emulator
@pytest.mark.parametrize("case", range(len(W.MASS_CASES)), ids=[c[0].split(":")[0] for c in W.MASS_CASES])
def test_text_mass_on_the_emulator(emu, case):
    from chatterbox_amd import ops
    name, H, heads, rows = W.MASS_CASES[case]
    q, k = W.mass_inputs(H, rows, 100 + case)
    ref = W.mass_ref(q, k, heads, *_cols(rows), 0.125, 0.5)
    mass = W.run_mass(ops, CPU, q, k, heads, rows, weight=0.5)
    print(f"{name}: worst err / (1 + |ref|) = {W.check_mass(mass, ref, rows):.3g}")
    assert torch.equal(mass, W.run_mass(ops, CPU, q, k, heads, rows, weight=0.5, poison=True)), "NaN keys nobody sees changed the result"


def test_text_mass_accumulates_and_takes_wide_scores_on_the_emulator(emu):
    from chatterbox_amd import ops
    rows = [(5, 9, 2, 6), (6, 70, 3, 66)]
    q, k = W.mass_inputs(3, rows, 6)
    acc = W.run_mass(ops, CPU, q, k, [2], rows, weight=0.5)
    acc = W.run_mass(ops, CPU, q, k, [0, 2], rows, weight=0.5, accumulate=True, mass=acc)
    ref = [a + b for a, b in zip(W.mass_ref(q, k, [2], *_cols(rows), 0.125, 0.5), W.mass_ref(q, k, [0, 2], *_cols(rows), 0.125, 0.5))]
    W.check_mass(acc, ref, rows)
    q, k = W.mass_inputs(2, rows, 8, spread=27.0)  # scores of about +-80
    W.check_mass(W.run_mass(ops, CPU, q, k, [1, 0], rows), W.mass_ref(q, k, [1, 0], *_cols(rows), 0.125, 1.0), rows)


@pytest.mark.parametrize("kind", ["random", "halves"])
def test_align_path_on_the_emulator(emu, kind):
    from chatterbox_amd import ops
    scores = [W.path_scores(n, m, 40 + i, kind) for i, (n, m) in enumerate(W.PATH_SHAPES)]
    for s in scores:
        W.check_path(*W.run_path(ops, CPU, [s]), [s])
    W.check_path(*W.run_path(ops, CPU, scores), scores)
    d = W.path_scores(70, 9, 0, "diagonal")
    spans, frame_tok = W.run_path(ops, CPU, [d])
    W.check_path(spans, frame_tok, [d])
    assert np.array_equal(frame_tok[0, :70], W.diagonal_tok(70, 9))


def test_the_restated_path_has_the_properties_the_header_states():
    for kind in ("random", "halves"):
        for i, (n, m) in enumerate(W.PATH_SHAPES):
            sp, ft = W.path_ref(W.path_scores(n, m, i, kind), n, m)
            assert ft[0] == 0 and set(np.diff(ft).tolist()) <= {0, 1}
            assert n < m or (ft[-1] == m - 1 and (sp[:, 1] > sp[:, 0]).all())
            assert n >= m or (sp[ft[-1] + 1:] == n).all()
    assert W.path_ref(np.zeros((3, 2), np.float32), 3, 2)[1].tolist() == [0, 1, 1], "a tie stays, -inf does not"


# ----------------------------------------------------------------------------- C ABI
def test_entry_points_are_declared_exported_bound_and_documented():
    from chatterbox_amd import _lib, ops
    hdr = open(os.path.join(ROOT, "include", "cbx.h")).read()
    lib = ctypes.CDLL(os.path.join(ROOT, "chatterbox_amd", "libcbx_hip.so"))
    for e in ("cbx_attn_text_mass_f32", "cbx_align_path_f32"):
        assert re.search(rf"^int {e}\(", hdr, re.M) and hasattr(lib, e) and e in _lib._SIGS, e
    assert "#define CBX_ABI_VERSION 16" in hdr and _lib.lib.cbx_abi_version() == 16 and _lib.ABI_VERSION == 16, "new functions only: no version step"
    block = hdr[hdr.index("---- word timestamps"): hdr.index("int cbx_align_path_f32(")]
    for phrase in ("over ALL visible keys j <= ctx0 + i", "t0 + t_len <= ctx0 + 1", "in list order", "a repeated head counts twice", "ctx0 + q_len <= 4608", "t_len <= 1024",
                   "-22 before any launch, nothing written", "D[0][0] = score[0][0]; D[0][t > 0] = -inf", "a tie stays", "the lowest t <= n - 1 with the largest D[n-1][t]",
                   "(n, n) for t > e", "ws_cap >= 8 * nz * max_z n[z] * ceil(max_z m[z] / 64)", "no log is taken"):
        assert phrase in block, phrase
    src = open(os.path.join(ROOT, "chatterbox_amd", "csrc", "attn_align.hip")).read()
    assert "asm" not in src and "atomic" not in src.replace("no atomics", ""), "plain C++, no atomics"
    assert callable(ops.attn_text_mass) and callable(ops.align_path)


def test_refused_descriptors_return_a_status_and_write_nothing():
    """on host buffers: a launch of the product library on them would fault, a refusal never gets that far"""
    from chatterbox_amd import _lib
    lib = _lib.lib
    q, k, mass = (ctypes.c_float * 512)(), (ctypes.c_float * 1536)(), (ctypes.c_float * 32)(*[7.0] * 32)

    def mass_call(heads=(0,), n_sel=1, q_len=(2,), ctx0=(8,), t0=(1,), t_len=(8,), nz=1, m_si=8, q_null=False):
        a = [W.c_ints(list(v)) for v in (heads, q_len, ctx0, t0, t_len)]
        return lib.cbx_attn_text_mass_f32(None if q_null else ctypes.addressof(q), ctypes.addressof(k), ctypes.addressof(mass), a[0], n_sel, 2, None, a[1], a[2], a[3], a[4],
                                          nz, 512, 128, 1536, 128, 64, 32, m_si, 0.125, 1.0, 0, None)
    for bad in (dict(q_null=True), dict(heads=(2,)), dict(heads=(-1,)), dict(n_sel=0), dict(n_sel=17), dict(nz=0), dict(nz=65), dict(q_len=(-1,)), dict(ctx0=(4607,)),
                dict(t_len=(1025,)), dict(t0=(2,)), dict(t0=(-1,)), dict(m_si=7)):
        assert mass_call(**bad) == -22 and b"attn_text_mass" in lib.cbx_last_error(), bad
    assert all(v == 7.0 for v in mass), "a refused call writes nothing"

    score, spans, ft, ws = (ctypes.c_float * 96)(), (ctypes.c_int * 32)(*[-7] * 32), (ctypes.c_int * 12)(*[-7] * 12), (ctypes.c_longlong * 64)()

    def path_call(n=(6, 3), m=(8, 2), nz=2, s_si=8, sp_sb=16, ft_sb=6, ws_cap=512, ws_off=0, ws_null=False):
        return lib.cbx_align_path_f32(ctypes.addressof(score), 48, s_si, W.c_ints(list(n)), W.c_ints(list(m)), nz, ctypes.addressof(spans), sp_sb, ctypes.addressof(ft), ft_sb,
                                      None if ws_null else ctypes.addressof(ws) + ws_off, ws_cap, None)
    for bad in (dict(ws_null=True), dict(nz=0), dict(nz=65), dict(n=(0, 3)), dict(n=(4097, 3)), dict(m=(0, 2)), dict(m=(1025, 2)), dict(s_si=7), dict(sp_sb=15),
                dict(ft_sb=5), dict(ws_cap=95), dict(ws_off=4)):
        assert path_call(**bad) == -22 and b"align_path" in lib.cbx_last_error(), bad
    assert all(v == -7 for v in spans) and all(v == -7 for v in ft), "a refused call writes nothing"


# ----------------------------------------------------------------------------- words
def test_word_groups():
    from chatterbox_amd.text import word_groups as g
    S = "[SPACE]"
    assert g(["[START]", "he", "llo", S, "wor", "ld", ".", "[STOP]"]) == [(1, 3), (4, 7)], "SOT / EOT and spaces belong to no word; punctuation joins the word before"
    assert g([S, S, "a", S]) == [(2, 3)], "leading and trailing spaces"
    assert g(["a", S, S, "b"]) == [(0, 1), (3, 4)], "double spaces"
    assert g(["he", "llo", S, ",", S, "x", "!", "?"]) == [(0, 4), (5, 8)], "punctuation behind a space still joins the word before it"
    assert g(["a", "b", "c"]) == [(0, 3)], "no spaces at all: one word"
    assert g([",", "a"]) == [(0, 2)] and g(["[en]", ".", S]) == [(1, 2)], "punctuation with no word before it starts one"
    assert g([]) == [] and g([S, "[START]", ""]) == []
    assert g(["a", "_", "b"], space="_") == [(0, 1), (2, 3)]


def test_frames_count_valid_tokens_and_map_to_samples():
    from chatterbox_amd import engine as E, ops
    t = torch.tensor([5, 9000, 7, 6561, 8, 6562, 3])
    assert E.valid_frame_counts(torch.tensor([5, 7, 8, 6562])) == [0, 1, 2, 3, 3]
    # an id outside the codebook in the middle shifts what follows; a sampled start token drops everything up to it, the end token everything from it
    assert E.valid_frame_counts(torch.tensor([5, 9000, 7, 8])) == [0, 1, 1, 2, 3]
    assert E.valid_frame_counts(t) == [0, 0, 0, 0, 0, 1, 1, 1] and int(E.drop_invalid_tokens(t).numel()) == 1
    for toks in (t, torch.tensor([1, 2, 3]), torch.tensor([6562]), torch.tensor([7000, 1])):
        assert E.valid_frame_counts(toks)[-1] == int(E.drop_invalid_tokens(toks).numel())
    assert [E.frame_sample(f) for f in (0, 1, 7)] == [0, 960, 6720]
    for s in (0.5, 0.8, 1.25, 2.0):
        for f in (0, 1, 2, 9, 40):
            j = E.frame_sample(f, speed=s) // 480
            assert E.frame_sample(f, speed=s) == 480 * j and E.stretch_position(j, s) >= 2 * f and (j == 0 or E.stretch_position(j - 1, s) < 2 * f), (s, f)
        assert E.frame_sample(40, speed=s) <= 480 * ops.scaled_len(80, s) + 480
    r = ops.pitch_ratio(3.0)
    assert E.frame_sample(10, speed=1.0, pitch=3.0) == int(480 * E._first_frame_at(20.0, 1.0 / r) / r + 0.5), "under a pitch: the stretch at speed / r, read back at step r"
    assert abs(E.frame_sample(10, speed=1.0, pitch=3.0) - 9600) <= 480, "a pitch keeps the length"


# ----------------------------------------------------------------------------- plumbing over recording engines
class _WordsEngine(_FakeEngine):
    """records like _FakeEngine; a call with words= returns synthesize's 3-tuple: every text token owns 2 frames, the waveform has 960 * 2 * tokens samples"""
    def synthesize(self, text_tokens, t3_conds, gen_ref, **kw):
        self.calls.append(("synthesize", dict(text_tokens=text_tokens, **kw)))
        sp = kw.get("speed")
        wavs = [torch.zeros(1920 * t.numel() if kw.get("words") else 3) for t in text_tokens]
        if kw.get("words") is None:
            return wavs, None
        al = [dict(frames=[(2 * i, 2 * i + 2) for i in range(t.numel())], n_frames=2 * t.numel(), speed=None if sp is None else sp[b], pitch=None)
              for b, t in enumerate(text_tokens)]
        return wavs, None, al


class _Pieces:
    SPACE = "_"

    def text_to_tokens(self, text, language_id=None):
        return torch.tensor([ord(c) for c in text], dtype=torch.int32).unsqueeze(0)

    def pieces(self, ids):
        return ["[START]" if i == 255 else "[STOP]" if i == 0 else "_" if chr(i) == " " else chr(i) for i in ids]


def _model(cls_name="ChatterboxTTS", engine=None):
    from chatterbox_amd import api
    m = _tts(getattr(api, cls_name), engine or _WordsEngine())
    m.tokenizer = _Pieces()
    return m


def test_word_times_false_records_the_calls_of_the_parent():
    from chatterbox_amd import api
    for cls_name in ("ChatterboxTTS", "ChatterboxMultilingualTTS"):
        lang = ("en",) if cls_name == "ChatterboxMultilingualTTS" else ()
        a, b = _model(cls_name), _model(cls_name)
        ra = a.generate("Hi there.", *lang, seed=3)
        rb = b.generate("Hi there.", *lang, seed=3, word_times=False)
        assert torch.is_tensor(ra) and torch.is_tensor(rb) and torch.equal(ra, rb)
        a.generate_batch(["Hi there.", "Yes."], *(["en"] if lang else []), seeds=[1, 2])
        b.generate_batch(["Hi there.", "Yes."], *(["en"] if lang else []), seeds=[1, 2], word_times=False)
        assert len(a.engine.calls) == len(b.engine.calls) == 2
        for (ka, kwa), (kb, kwb) in zip(a.engine.calls, b.engine.calls):
            assert ka == kb and sorted(kwa) == sorted(kwb) and "words" not in kwb and str(kwa) == str(kwb)


def test_generate_returns_words_in_samples_of_the_result():
    m = _model()
    wav, words = m.generate("Hi yo, a.", seed=3, word_times=True)
    kind, kw = m.engine.calls[-1]
    assert kind == "synthesize" and kw["words"] == dict(heads=None)
    assert [w["text"] for w in words] == ["Hi", "yo,", "a."]
    # tokens: [START] H i _ y o , _ a . [STOP]; a token owns 2 frames of 960 samples; a word ends where the next begins, the last where its frames end
    assert [w["tokens"] for w in words] == [(1, 3), (4, 7), (8, 10)] and [w["frames"] for w in words] == [(2, 6), (8, 14), (16, 20)]
    assert [(w["start"], w["stop"]) for w in words] == [(1920, 7680), (7680, 15360), (15360, 19200)] and words[-1]["stop"] <= wav.shape[-1]
    wav, toks = m.generate("Hi yo.", seed=3, word_times="tokens")
    assert len(toks) == 8 and toks[0]["text"] == "[START]" and toks[0]["start"] == 0 and toks[-1]["stop"] == wav.shape[-1] == 8 * 1920
    assert all(a["stop"] == b["start"] for a, b in zip(toks, toks[1:]))
    m.align_heads = ((0, 1),)
    m.generate("Hi.", word_times=True)
    assert m.engine.calls[-1][1]["words"] == dict(heads=((0, 1),))


def test_speed_and_sample_rate_map_the_boundaries():
    from chatterbox_amd import engine as E, ops
    m = _model()
    wav, words = m.generate("Hi yo.", seed=3, speed=1.25, word_times=True)
    assert [(w["start"], w["stop"]) for w in words] == [(E.frame_sample(2, 1.25), E.frame_sample(8, 1.25)), (E.frame_sample(8, 1.25), E.frame_sample(14, 1.25))]
    m.watermarker = type("Wm", (), {"apply_watermark": staticmethod(lambda x, sample_rate: x)})()  # the engine then returns 24 kHz and _finish converts: no device
    m._to_format = lambda wav, fmt: wav[: ops.formatted_len(wav.numel(), fmt["sample_rate"])]
    wav, words = m.generate("Hi yo.", seed=3, sample_rate=16000, word_times=True)
    assert wav.shape[-1] == ops.formatted_len(8 * 1920, 16000)
    assert [(w["start"], w["stop"]) for w in words] == [(ops.formatted_len(1920, 16000), ops.formatted_len(7680, 16000)), (ops.formatted_len(7680, 16000), ops.formatted_len(13440, 16000))]


def test_batch_words_run_the_serial_schedule_and_follow_their_requests():
    m = _model()
    m.max_batch = 2
    texts = ["Hi yo.", "A.", "Hi yo, a."]
    out = m.generate_batch(texts, seeds=[1, 2, 3], word_times=True)
    assert [k for k, _ in m.engine.calls] == ["synthesize", "synthesize"], "two sub-batches, one after the other: no pipelined call"
    assert all(kw["words"] == dict(heads=None) for _, kw in m.engine.calls)
    assert [[w["text"] for w in words] for _, words in out] == [["Hi", "yo."], ["A."], ["Hi", "yo,", "a."]]
    assert all(torch.is_tensor(w) and words[-1]["stop"] <= w.shape[-1] for w, words in out)
    plain = _model()
    plain.max_batch = 2
    plain.generate_batch(texts, seeds=[1, 2, 3])
    assert [k for k, _ in plain.engine.calls] == ["pipelined"]


def test_what_is_refused():
    from chatterbox_amd import api, engine as E
    m = _model()
    for call in (lambda: m.generate("Hi.", max_pause=0.3, word_times=True), lambda: m.generate_batch(["Hi."], max_pause=[0.3], word_times="tokens"),
                 lambda: m.generate_long("Hi.", return_segments=True, max_pause=0.3, word_times=True)):
        with pytest.raises(ValueError, match="max_pause.*word_times"):
            call()
    with pytest.raises(ValueError, match="return_segments"):
        m.generate_long("Hi.", word_times=True)
    with pytest.raises(ValueError, match="word_times"):
        m.generate("Hi.", word_times="syllables")
    assert m.engine.calls == [], "everything is refused before the engine is called"
    bare = _tts(api.ChatterboxTTS, _WordsEngine())  # test_seeded_rng_host's tokenizer: no pieces
    with pytest.raises(ValueError, match="pieces"):
        bare.generate("Hi.", word_times="words")
    wav, toks = bare.generate("Hi.", word_times="tokens")
    assert len(toks) == 5 and toks[1]["text"] == "0", '"tokens" needs no pieces: the ids'
    job = dict(text_tokens=[torch.zeros(3, dtype=torch.long)], t3_conds=None, gen_ref=None)
    with pytest.raises(ValueError, match="synthesize"):
        E._checked_job(dict(job, words=dict(heads=None)))
    assert "words" not in E._checked_job(dict(job, words=None))
    with pytest.raises(ValueError):
        E.check_words(dict(head=1))
    import inspect
    for cls_name, method in (("ChatterboxTTS", "generate_stream"), ("ChatterboxMultilingualTTS", "generate_stream"), ("ChatterboxTurboTTS", "generate"),
                             ("ChatterboxTurboTTS", "generate_batch"), ("ChatterboxTurboTTS", "generate_long"), ("ChatterboxVC", "generate")):
        assert "word_times" not in inspect.signature(getattr(getattr(api, cls_name), method)).parameters, (cls_name, method)
    # generate_long_stream's signature is generate_long's plus the ramp (test_loudness_push_host.py holds it to that), so the name is listed -- and refused
    for cls_name, lang in (("ChatterboxTTS", ()), ("ChatterboxMultilingualTTS", ("en",))):
        s = _model(cls_name)
        for value in (True, "words", "tokens"):
            with pytest.raises(TypeError, match="does not take word_times"):
                s.generate_long_stream("Hi.", *lang, word_times=value)
        assert s.engine.calls == []


def test_align_heads_are_checked_against_the_model():
    from chatterbox_amd.t3 import T3Engine
    eng = T3Engine.__new__(T3Engine)
    eng.L = 2
    assert T3Engine.ALIGN_HEADS == ((9, 2), (12, 15), (13, 11))
    with pytest.raises(ValueError, match="layer 9"):
        eng.check_align_heads(None)
    with pytest.raises(ValueError, match="head 16"):
        eng.check_align_heads(((1, 16),))
    with pytest.raises(ValueError):
        eng.check_align_heads(())
    assert eng.check_align_heads([(0, 3), [1, 15]]) == ((0, 3), (1, 15))
    eng.L = 30
    assert eng.check_align_heads() == T3Engine.ALIGN_HEADS
