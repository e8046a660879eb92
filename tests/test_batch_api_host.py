"""CPU (-m "not gpu"): generate_batch on the public classes -- argument broadcasting and validation before any launch, execution order and sub-batch
boundaries -- the C ABI of the two kernels behind it (cbx_prefill_embed, cbx_kv_prefix_paste_f32), and those kernels plus the mixed-voice prefix cache of
the GPT-2 engine on the SIMT emulator (tests/simt), bit for bit against the per-utterance host loop they replace."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, os.path.join(HERE, "simt")):
    if p not in sys.path:
        sys.path.insert(0, p)

CPU = torch.device("cpu")


# ----------------------------------------------------------------------------- per-utterance sampling parameters
def test_sampler_rows_scalars_give_the_old_buffer_and_sequences_their_own_rows():
    from chatterbox_amd.t3 import per_utterance, sampler_rows
    cols = (("cfg_weight", 0.5), ("temperature", 0.8), ("min_p", 0.05), ("top_p", 1.0), ("repetition_penalty", 1.2), ("top_k", 0.0), ("ban_token", -1.0),
            ("ban_from", 0.0))
    old = torch.tensor([0.5, 0.8, 0.05, 1.0, 1.2, 0.0, -1.0, 0.0]).repeat(3, 1)  # what generate() wrote before per-utterance parameters
    assert torch.equal(sampler_rows(3, cols), old)
    mixed = sampler_rows(3, (("cfg_weight", [0.5, 0.0, 0.3]),) + cols[1:3] + (("top_p", torch.tensor([1.0, 0.9, 0.8])),) + cols[4:])
    assert mixed[:, 0].tolist() == pytest.approx([0.5, 0.0, 0.3]) and mixed[:, 3].tolist() == pytest.approx([1.0, 0.9, 0.8]) and torch.equal(mixed[:, 1], old[:, 1])
    assert per_utterance(0.7, 2, "t") == [0.7, 0.7] and per_utterance((1, 2), 2, "t") == [1.0, 2.0]
    for bad in ([0.8, 0.9], (0.8,) * 4, torch.ones(2)):
        with pytest.raises(ValueError, match="temperature"):
            per_utterance(bad, 3, "temperature")


def test_batch_plan_sorts_by_length_and_cuts_at_max_batch():
    from chatterbox_amd.api import batch_plan
    assert batch_plan([5], 4) == [[0]]
    assert batch_plan([5, 3, 9, 3], 4) == [[1, 3, 0, 2]]                      # B = MAX_BATCH: one sub-batch, stable for equal lengths
    assert batch_plan([5, 3, 9, 3, 1], 4) == [[4, 1, 3, 0], [2]]              # B = MAX_BATCH + 1: the longest text runs alone
    plan = batch_plan([7, 1, 64, 2, 2, 30, 8, 9, 3], 4)
    assert sorted(i for sub in plan for i in sub) == list(range(9)) and [len(s) for s in plan] == [4, 4, 1]


# ----------------------------------------------------------------------------- the public classes over a recording engine (nothing is launched)
class _FakeT3:
    MAX_BATCH = 4


class _FakeSerialEngine:
    """Records the calls generate_batch makes; every 'waveform' is its request's text length, so the caller's order can be checked.  Like TurboEngine it has no
    throughput schedule."""
    dev = CPU

    def __init__(self):
        self.t3, self.calls = _FakeT3(), []

    def synthesize(self, text_tokens, t3_conds, gen_ref, **kw):
        self.calls.append(("synthesize", dict(text_tokens=text_tokens, t3_conds=t3_conds, gen_ref=gen_ref, **kw)))
        return [torch.full((3,), float(t.numel())) for t in text_tokens], None


class _FakeEngine(_FakeSerialEngine):
    def synthesize_pipelined(self, jobs, **kw):
        self.calls.append(("pipelined", dict(jobs=jobs, **kw)))
        for job in jobs:
            yield [torch.full((3,), float(t.numel())) for t in job["text_tokens"]], None, 0.0


class _Tok:
    def text_to_tokens(self, text, language_id=None):
        return torch.arange(len(text), dtype=torch.int32).unsqueeze(0)


def _tts(cls, engine=None, conds="default"):
    from chatterbox_amd import api, synth
    m = cls.__new__(cls)
    m.engine, m.tokenizer, m.device, m.analyzer, m.watermarker = engine or _FakeEngine(), _Tok(), CPU, None, None
    m.conds = api.Conditionals(api.T3Cond(**synth.t3_cond()), synth.s3gen_ref(n_prompt_tokens=8)) if conds == "default" else conds
    return m


def test_generate_batch_validates_every_argument_before_anything_runs():
    from chatterbox_amd import api
    m = _tts(api.ChatterboxMultilingualTTS)
    texts = ["aaaa", "bb", "cccccc"]
    for kw in (dict(temperature=[0.8, 0.9]), dict(top_p=[1.0] * 4), dict(cfg_weight=(0.5,)), dict(exaggeration=[0.5, 0.5]), dict(min_p=[0.0] * 2),
               dict(repetition_penalty=[1.2] * 5), dict(conds=[m.conds, m.conds]), dict(audio_prompt_paths=["a.wav"] * 2)):
        with pytest.raises(ValueError):
            m.generate_batch(texts, "en", **kw)
    with pytest.raises(ValueError, match="language_ids"):
        m.generate_batch(texts, ["en", "fr"])
    with pytest.raises(ValueError, match="'xx'.*request 1"):
        m.generate_batch(texts, ["en", "xx", "fr"])
    with pytest.raises(AssertionError, match="prepare_conditionals"):
        _tts(api.ChatterboxTTS, conds=None).generate_batch(texts)
    with pytest.raises(AssertionError, match="prepare_conditionals"):
        _tts(api.ChatterboxTTS).generate_batch(texts, conds=[m.conds, None, m.conds])
    # what counts as ONE entry is decided per argument, by type: a bare number, tensor or pair is not a language id / voice / path
    for kw, lang in ((dict(conds=m.conds.t3), "en"), (dict(audio_prompt_paths=3), "en"), ({}, 7)):
        with pytest.raises(TypeError):
            m.generate_batch(texts, lang, **kw)
    assert api._per_request("a.wav", 2, "p", api._PATH) == ["a.wav"] * 2 and api._per_request(None, 2, "p", api._PATH) == [None, None]
    pair = (torch.zeros(8), 16000)   # a (waveform, sample_rate) pair is an entry: as the whole argument it reads as a list of 2 entries
    assert api._per_request([pair, "b.wav"], 2, "p", api._PATH) == [pair, "b.wav"] and api._per_request(pair, 2, "p", api._PATH) == list(pair)
    with pytest.raises(ValueError):
        api._per_request(pair, 3, "p", api._PATH)
    assert m.engine.calls == []


def test_generate_batch_restores_the_callers_order_and_cuts_sub_batches():
    from chatterbox_amd import api, synth
    m = _tts(api.ChatterboxTTS)
    own = m.conds
    other = api.Conditionals(api.T3Cond(**synth.t3_cond(seed=5)), synth.s3gen_ref(seed=6, n_prompt_tokens=8))

    def run(lens, **kw):
        m.engine.calls.clear()
        out = m.generate_batch(["x" * (n - 1) + "." for n in lens], **kw)   # (ends in punctuation: punc_norm_en adds nothing)
        assert [tuple(w.shape) for w in out] == [(1, 3)] * len(lens) and all(w.dtype == torch.float32 for w in out)
        assert [int(w[0, 0]) for w in out] == [n + 2 for n in lens], "waveforms come back in the caller's order (text + SOT + EOT tokens)"
        return m.engine.calls

    calls = run([9])                                     # B = 1
    assert [c[0] for c in calls] == ["synthesize"] and calls[0][1]["temperature"] == [0.8] and isinstance(calls[0][1]["t3_conds"], dict)
    calls = run([9, 2, 5, 7], temperature=[0.1, 0.2, 0.3, 0.4], conds=[own, other, own, other])   # B = MAX_BATCH: one serial sub-batch, sorted by length
    kw = calls[0][1]
    assert [c[0] for c in calls] == ["synthesize"] and [int(t.numel()) for t in kw["text_tokens"]] == [4, 7, 9, 11]
    assert kw["temperature"] == [0.2, 0.3, 0.4, 0.1] and kw["cfg_weight"] == [0.5] * 4 and kw["max_new_tokens"] == 1000 and kw["drop_last_token"] is False
    assert [c is kw["t3_conds"][0] for c in kw["t3_conds"]] == [True, False, True, False], "per-request voices follow their requests (other, own, other, own)"
    assert kw["gen_ref"][0] is other.gen and kw["gen_ref"][1] is own.gen and "uniforms" not in kw
    calls = run([9, 2, 5, 7, 30], top_p=[1.0, 0.9, 0.8, 0.7, 0.6])   # B = MAX_BATCH + 1: two sub-batches through the throughput schedule
    assert [c[0] for c in calls] == ["pipelined"] and [len(j["text_tokens"]) for j in calls[0][1]["jobs"]] == [4, 1]
    assert calls[0][1]["jobs"][1]["top_p"] == [0.6] and calls[0][1]["jobs"][0]["top_p"] == [0.9, 0.8, 0.7, 1.0]
    assert m.conds is own, "generate_batch never overwrites self.conds"
    # the same voice at the same exaggeration is the same dict of the same tensors from call to call (the engine's prefix cache matches by identity)
    d1 = run([3, 4], exaggeration=[0.5, 0.9])[0][1]["t3_conds"]
    d2 = run([3, 4], exaggeration=[0.5, 0.9])[0][1]["t3_conds"]
    assert d1[0] is d2[0] and d1[1] is d2[1] and d1[0] is not d1[1] and float(d1[1]["emotion_adv"]) == pytest.approx(0.9)
    assert d1[0]["speaker_emb"] is own.t3.speaker_emb and d1[1]["speaker_emb"] is own.t3.speaker_emb
    # a generator draws the sampling uniforms of every sub-batch up front, in execution order: two calls with the same seed are identical
    u = [run([3, 4, 5, 6, 7], generator=torch.Generator().manual_seed(7))[0][1]["jobs"] for _ in range(2)]
    assert all(torch.equal(a["uniforms"], b["uniforms"]) for a, b in zip(*u)) and u[0][0]["uniforms"].shape == (4, 1000)


def test_turbo_and_vc_generate_batch_validate_and_order():
    from chatterbox_amd import api, synth

    class Enc:
        def __call__(self, text, **kw):
            return type("E", (), {"input_ids": torch.arange(len(text)).unsqueeze(0)})()

    eng = _FakeSerialEngine()
    m = _tts(api.ChatterboxTurboTTS, eng)
    m.tokenizer, m.model_label = Enc(), "Turbo"
    with pytest.raises(ValueError, match="top_k"):
        m.generate_batch(["aa", "b"], top_k=[10, 20, 30])
    assert eng.calls == []
    eng.t3.MAX_BATCH = 2
    out = m.generate_batch(["aaa.", ".", "c."], top_k=[10, 20, 30])   # (end in punctuation: punc_norm_turbo adds nothing)
    assert [int(w[0, 0]) for w in out] == [4, 1, 2] and [c[0] for c in eng.calls] == ["synthesize", "synthesize"]
    assert eng.calls[0][1]["top_k"] == [20.0, 30.0] and eng.calls[1][1]["top_k"] == [10.0] and eng.calls[0][1]["max_gen_len"] == 1000

    class Voc:
        calls = []

        def vocode(self, toks, refs):
            self.calls.append((toks, refs))
            return [torch.full((2,), float(t.numel())) for t in toks], None

    vc = api.ChatterboxVC.__new__(api.ChatterboxVC)
    vc.engine, vc.device, vc.ref_dict, vc.analyzer, vc.watermarker = Voc(), CPU, None, None, None
    toks = [synth.speech_tokens(n) for n in (30, 10, 20)]
    with pytest.raises(AssertionError, match="prepare_conditionals"):
        vc.generate_batch(s3_tokens=toks)
    refs = [synth.s3gen_ref(seed=s, n_prompt_tokens=8) for s in (1, 2, 3)]
    with pytest.raises(ValueError, match="ref_dicts"):
        vc.generate_batch(s3_tokens=toks, ref_dicts=refs[:2])
    assert Voc.calls == []
    vc.MAX_BATCH = 2
    out = vc.generate_batch(s3_tokens=toks, ref_dicts=refs)
    assert [int(w[0, 0]) for w in out] == [30, 10, 20] and [len(c[0]) for c in Voc.calls] == [2, 1]
    assert Voc.calls[0][1][0] is refs[1] and Voc.calls[0][1][1] is refs[2] and Voc.calls[1][1] is refs[0]


# ----------------------------------------------------------------------------- C ABI
def test_new_entry_points_are_declared_exported_and_bound():
    import ctypes
    import re
    from chatterbox_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "cbx.h")).read()
    lib = ctypes.CDLL(os.path.join(ROOT, "chatterbox_amd", "libcbx_hip.so"))
    for name in ("cbx_prefill_embed", "cbx_kv_prefix_paste_f32"):
        assert re.search(rf"^int {name}\(", hdr, re.M) and hasattr(lib, name) and name in _lib._SIGS
    assert _lib.lib.cbx_abi_version() == 16, "new functions and a new struct only: no version step"
    d = _lib.PrefillEmbed()
    assert _lib.lib.cbx_prefill_embed(None, None) == -22 and _lib.lib.cbx_prefill_embed(ctypes.byref(d), None) == -22
    assert _lib.lib.cbx_kv_prefix_paste_f32(None, 1, None, None, 1, 1, 1, 1, 0, 0, 0, None) == -22


def test_prefill_embed_ctypes_struct_matches_the_c_header(tmp_path):
    """cbx_prefill_embed_t: the size and every field offset of the ctypes mirror equal what gcc gives include/cbx.h."""
    import ctypes
    import shutil
    import subprocess
    from chatterbox_amd import _lib
    if shutil.which("gcc") is None:
        pytest.skip("no C compiler")
    cname, cls = "cbx_prefill_embed_t", _lib.PrefillEmbed
    lines = [f'printf("{cname} %zu\\n", sizeof({cname}));'] + [f'printf("{cname}.{f} %zu\\n", offsetof({cname}, {f}));' for f, _ in cls._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "cbx.h"\nint main(void) {\n' + "\n".join(lines) + "\nreturn 0; }\n")
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "layout")])
    got = dict(l.split() for l in subprocess.check_output([str(tmp_path / "layout")], text=True).splitlines())
    assert int(got[cname]) == ctypes.sizeof(cls)
    for f, _ in cls._fields_:
        assert int(got[f"{cname}.{f}"]) == getattr(cls, f).offset, f


# ----------------------------------------------------------------------------- the kernels on the SIMT emulator
@pytest.fixture(scope="module")
def emu():
    import build_emu
    if not os.path.exists(build_emu.CLANG):
        pytest.skip("ROCm's clang++ (x86 host compiler of the emulator build) is not installed")
    import harness
    with harness.emulated() as lib:
        yield lib


@pytest.mark.parametrize("cached", [False, True], ids=["with_conditioning", "behind_cached_prefix"])
@pytest.mark.parametrize("llama", [True, False], ids=["llama_layout", "gpt2_layout"])
def test_ragged_prefill_assembly_on_the_emulator(emu, llama, cached):
    """Lengths {1, 7, 64} mixed in one batch: cbx_prefill_embed == the per-utterance host loop == the NumPy restatement, bit for bit; pos / crow / last too."""
    import batch_api_common as c
    from chatterbox_amd import ops
    tb = c.tables(CPU, D=64)
    tt = c.texts([7, 64, 1])
    n_prompt = [33, 33, 33] if (llama or cached) else [20, 33, 5]   # GPT-2 layout without a cache: voices whose prompts differ in length
    P = [34] * 3 if llama else [1 + n for n in n_prompt]
    g = torch.Generator().manual_seed(11)
    ce = [torch.randn(p, 64, generator=g) for p in P]
    P0 = P[0] if cached else 0
    want = c.host_loop_llama(ops, tb, tt, ce, P0) if llama else c.host_loop_gpt2(ops, tb, tt, ce, n_prompt, P0)
    got = c.call_kernel(ops, tb, tt, None if cached else ce, P, P0, llama)
    for w, g_, what in zip(want, got, ("x", "positions", "cache_rows", "last")):
        assert w.shape == g_.shape and w.dtype == g_.dtype and torch.equal(w, g_), what
    assert torch.equal(got[0], torch.from_numpy(c.numpy_layout(tb, tt, None if cached else ce, P, P0, llama)))


def test_prefix_paste_by_voice_index_on_the_emulator(emu):
    import batch_api_common as c
    from chatterbox_amd import ops
    g = torch.Generator().manual_seed(5)
    L, R, H, ctx, P = 2, 5, 3, 40, 19   # P * 16 float4 not a multiple of the 256-thread pass
    for voice_of in ([0] * 4, [1, 0, 0, 1], [0, 1, 2, 3]):
        prefixes = [(torch.randn(L, H, P, 64, generator=g), torch.randn(L, H, P, 64, generator=g)) for _ in range(max(voice_of) + 1)]
        base = torch.randn(2, L, R, H, ctx, 64, generator=g)
        want, got = base.clone(), base.clone()
        c.paste_by_copy(want[0], want[1], prefixes, voice_of)
        ops.kv_prefix_paste(prefixes, voice_of, got[0], got[1])
        assert torch.equal(want, got), voice_of   # row 4 and positions >= P untouched
    with pytest.raises(AssertionError):
        ops.kv_prefix_paste(prefixes, [0, 4], got[0], got[1])


def _turbo(share):
    from chatterbox_amd import synth
    from chatterbox_amd.t3_turbo import T3TurboEngine
    # (512 wide, not 256: LayerNorm has a form of its own for C == 256 and >= 64 rows, so a 256-wide toy model rounds a 39-row prefix-only prefill unlike the
    # full prefill; the real backbones are 768 / 1024 wide)
    eng = T3TurboEngine(synth.t3_turbo_state_dict(1, 512, 0), CPU)
    eng.share_prefix = share
    return eng


def test_turbo_mixed_voice_prefix_cache_equals_the_full_prefill_on_the_emulator(emu):
    """T3TurboEngine.generate on a batch of three voices: first call (all miss: one prefix-only prefill, then text only), second call (all hit), a call with one new
    voice and per-utterance sampling parameters -- prefill logits, tokens and KV cache equal an engine that never shares (the full prefill)."""
    from chatterbox_amd import synth
    voices = [synth.t3_cond(seed=s, prompt_len=12) for s in (2, 3, 4, 5)]
    a, b = _turbo(True), _turbo(False)
    tt = [synth.turbo_text_tokens(n, seed=i + 1) for i, n in enumerate((7, 1, 12, 5))]
    u = synth.rand((4, 5), seed=3)
    for pick, n_cached in (((0, 1, 2, 0), 3), ((0, 1, 2, 0), 3), ((1, 3, 3, 2), 4)):
        res = []
        for eng in (a, b):
            toks, logits = eng.generate([voices[i] for i in pick], tt, max_gen_len=4, uniforms=u, ban_eos=True, debug_logits=True, temperature=[0.8, 0.7, 1.0, 0.9],
                                        top_p=[0.95, 1.0, 0.9, 0.8], top_k=[1000, 50, 1000, 10])
            st = next(iter(eng._state.values()))
            res.append(([t.tolist() for t in toks], logits.clone(), st["kc"].clone(), st["vc"].clone(), st["samp_dev"].clone()))
        assert res[0][0] == res[1][0]
        for x, y, what in zip(res[0][1:], res[1][1:], ("logits of every step", "k cache", "v cache", "sampling rows")):
            assert torch.equal(x, y), what
        assert len(a._prefix_cache) == n_cached and not b._prefix_cache
        assert res[0][4][:, 5].tolist() == [1000.0, 50.0, 1000.0, 10.0] and res[0][4][:, 1].tolist() == pytest.approx([0.8, 0.7, 1.0, 0.9])
