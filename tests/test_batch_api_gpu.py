"""GPU (-m gpu): the batched public API (generate_batch on the four classes) and what the engines gained for it -- the voice-prefix cache for a batch that mixes
voices, per-utterance sampling parameters -- on synthetic weights (no checkpoints).  The kernel-level tests of the two new launches are in
test_turbo_stream_batch_kernels_gpu.py."""
import collections
import math
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

from test_baseline_shapes_gpu import SAMP, TOL_MEL, TOL_WAV_E2E_8S, _need, _window_rmse  # noqa: E402  (read-only import: the stated tolerances)

pytestmark = pytest.mark.gpu


def _first_diff(a, b):
    d = (a != b).nonzero()
    return f"{len(d)} elements differ, first at {d[0].tolist() if len(d) else None}"


# ----------------------------------------------------------------------------- the voice-prefix cache for a batch that mixes voices
def test_t3_mixed_voice_prefix_cache_equals_the_full_prefill(dev, layers=2, steps=6):
    """Three voices in one batch: prefill logits, tokens and KV cache of an engine that shares prefixes -- first call (all miss: one prefix-only prefill of the three
    voices, then text only), second call (all hit), a call where one voice is new -- are torch.equal to an engine that never shares (the full prefill)."""
    from chatterbox_amd import synth
    from chatterbox_amd.t3 import T3Engine
    sd = synth.t3_state_dict(layers, 0)
    voices = [synth.t3_cond(seed=s) for s in (2, 3, 4, 5)]
    a, b = T3Engine(sd, dev), T3Engine(sd, dev)
    b.share_prefix = False
    lens = (12, 20, 7, 31)
    tt = [synth.text_tokens(n, seed=i + 1) for i, n in enumerate(lens)]
    u = synth.rand((len(lens), steps), seed=3)
    for pick, n_cached in (((0, 1, 2, 0), 3), ((0, 1, 2, 0), 3), ((1, 3, 3, 2), 4)):
        res = []
        for eng in (a, b):
            toks, logits = eng.generate([voices[i] for i in pick], tt, max_new_tokens=steps, uniforms=u, ban_eos=True, return_prefill_logits=True, **SAMP)
            st = next(iter(eng._state.values()))
            S = 34 + max(lens) + 2
            res.append(([t.tolist() for t in toks], logits.cpu(), st["kc"][:, :, :, :S].cpu().clone(), st["vc"][:, :, :, :S].cpu().clone()))
        assert res[0][0] == res[1][0], f"tokens, voices {pick}"
        for x, y, what in zip(res[0][1:], res[1][1:], ("prefill logits", "k cache", "v cache")):
            assert torch.equal(x, y), f"shared prefixes vs the full prefill: {what}, voices {pick}: {_first_diff(x, y)}"
        assert len(a._prefix_cache) == n_cached and not b._prefix_cache


@pytest.mark.parametrize("nano", [False, True], ids=["turbo_1024", "nano_768"])
def test_turbo_mixed_voice_prefix_cache_equals_the_full_prefill(dev, nano, steps=5):
    """The same claim for the GPT-2 backbones (376-position prefixes): logits of every step (the first = the prefill's), tokens and KV cache."""
    from chatterbox_amd import synth
    from chatterbox_amd.t3_turbo import T3TurboEngine
    sd = synth.t3_turbo_state_dict(2, 768 if nano else 1024, 0)
    voices = [synth.t3_cond(seed=s, prompt_len=375) for s in (2, 3, 4, 5)]
    a, b = T3TurboEngine(sd, dev), T3TurboEngine(sd, dev)
    b.share_prefix = False
    tt = [synth.turbo_text_tokens(n, seed=i + 1) for i, n in enumerate((7, 1, 64, 20))]
    u = synth.rand((4, steps + 1), seed=3)
    for pick, n_cached in (((0, 1, 2, 0), 3), ((0, 1, 2, 0), 3), ((1, 3, 3, 2), 4)):
        res = []
        for eng in (a, b):
            toks, logits = eng.generate([voices[i] for i in pick], tt, max_gen_len=steps, uniforms=u, ban_eos=True, debug_logits=True)
            st = next(iter(eng._state.values()))
            res.append(([t.tolist() for t in toks], logits.cpu(), st["kc"].cpu().clone(), st["vc"].cpu().clone()))
        assert res[0][0] == res[1][0], f"tokens, voices {pick}"
        for x, y, what in zip(res[0][1:], res[1][1:], ("logits of every step", "k cache", "v cache")):
            assert torch.equal(x, y), f"shared prefixes vs the full prefill: {what}, voices {pick}: {_first_diff(x, y)}"
        assert len(a._prefix_cache) == n_cached and not b._prefix_cache


# ----------------------------------------------------------------------------- per-utterance sampling parameters
def test_t3_per_utterance_sampling_params_in_one_batch(dev):
    """The two settings of test_t3_sampling_params_live_in_device_memory as ONE batch -- row 0 on s1, row 1 on s2: each row gets exactly the tokens of a fresh engine
    run with that row's setting for the whole batch, and the decode graph is not re-captured."""
    from chatterbox_amd import synth
    from chatterbox_amd.t3 import T3Engine
    sd = synth.t3_state_dict(2, 0)
    tt = [synth.text_tokens(12, seed=1), synth.text_tokens(20, seed=2)]
    u = synth.rand((2, 24), seed=3)
    kw = dict(max_new_tokens=24, uniforms=u, ban_eos=True)
    s1 = dict(temperature=0.8, cfg_weight=0.5, repetition_penalty=1.2, min_p=0.05, top_p=1.0)
    s2 = dict(temperature=1.3, cfg_weight=0.2, repetition_penalty=1.0, min_p=0.0, top_p=0.9)
    a = T3Engine(sd, dev)
    captured = lambda: (lambda st: st["cloop"] if a.c_loop else st["graph"])(next(iter(a._state.values())))
    a.generate(synth.t3_cond(), tt, **kw, **s1)
    g1 = captured()
    mixed = a.generate(synth.t3_cond(), tt, **kw, **{k: [s1[k], s2[k]] for k in s1})
    assert captured() is g1 and g1 is not None, "the decode graph must not be re-captured"
    b = T3Engine(sd, dev)
    f1, f2 = b.generate(synth.t3_cond(), tt, **kw, **s1), b.generate(synth.t3_cond(), tt, **kw, **s2)
    assert mixed[0].tolist() == f1[0].tolist() and mixed[1].tolist() == f2[1].tolist()
    assert f1[1].tolist() != f2[1].tolist(), "the two settings must differ on row 1 for the test to mean anything"
    with pytest.raises(ValueError, match="temperature"):
        a.generate(synth.t3_cond(), tt, **kw, temperature=[0.8, 0.9, 1.0])


# ----------------------------------------------------------------------------- generate_batch == the single requests
class _Tok:
    """Stand-in tokenizer of the synthetic models: ids from the characters (the API's text normalisation runs in front of it)."""

    def __init__(self, vocab):
        self.vocab = vocab

    def _ids(self, text):
        return torch.tensor([(7 * ord(ch) + 3 * i) % (self.vocab - 300) + 260 for i, ch in enumerate(text)], dtype=torch.int32)

    def text_to_tokens(self, text, language_id=None):
        return self._ids(("" if language_id is None else f"[{language_id}]") + text).unsqueeze(0)

    def __call__(self, text, **kw):
        return type("Enc", (), {"input_ids": self._ids(text).long().unsqueeze(0)})()


TEXTS = ["Hello there.", "A considerably longer request, so that the batch is ragged and padded.", "Hi.", "Numbers one two three four.", "The fifth and last one!"]
N_TOK = 24


class _Inject:
    """Engine-level injection (as test_baseline_shapes_gpu.py injects `uniforms`, `z`, `phase`, `noise`): every request owns its sampling draws and its flow /
    vocoder noise, keyed by its text ids, whatever batch, row or sub-batch it runs in.  Also bounds the sampled tokens (synthetic weights rarely sample EOS)."""

    def __init__(self, engine, budget_key, n_draws):
        self.eng, self.key, self.n_draws = engine, budget_key, n_draws
        self.order, self.tokens = collections.deque(), {}
        self.t3_generate, self.vocode = engine.t3.generate, engine.vocode
        engine.t3.generate, engine.vocode = self.gen, self.voc

    @staticmethod
    def seed_of(ids):
        return int(sum((i + 1) * int(v) for i, v in enumerate(ids.tolist())) % 100003)

    def gen(self, conds, text_tokens, **kw):
        from chatterbox_amd import synth
        seeds = [self.seed_of(t) for t in text_tokens]
        kw[self.key] = N_TOK
        kw["uniforms"] = torch.stack([synth.rand((self.n_draws,), seed=s) for s in seeds])
        kw["ban_eos"] = True
        self.order.append(seeds)
        return self.t3_generate(conds, text_tokens, **kw)

    def voc(self, speech_tokens, gen_ref, **kw):
        from chatterbox_amd import synth
        seeds = self.order.popleft()
        refs = gen_ref if isinstance(gen_ref, (list, tuple)) else [gen_ref] * len(speech_tokens)
        P, Nmax = int(refs[0]["prompt_token"].numel()), max(int(t.numel()) for t in speech_tokens)
        dev = self.eng.dev
        kw["z"] = torch.stack([synth.randn((2 * (P + N_TOK + 8), 80), seed=s + 1) for s in seeds])[:, : 2 * (P + Nmax)].to(dev)
        ph = torch.stack([(synth.rand((9, 1), seed=s + 2) * 2 - 1) * math.pi for s in seeds])
        ph[:, 0] = 0
        kw["phase"] = ph
        kw["noise"] = torch.stack([synth.randn((9, 960 * (N_TOK + 8)), seed=s + 3) for s in seeds])[:, :, : 960 * Nmax].to(dev)
        for s, t in zip(seeds, speech_tokens):
            self.tokens.setdefault(s, []).append(t.tolist())
        return self.vocode(speech_tokens, gen_ref, **kw)


def _rmse(a, b):
    assert a.shape == b.shape, (a.shape, b.shape)
    return float((a.double() - b.double()).pow(2).mean().sqrt())


def _check_batch_equals_singles(model, inj, batch_call, single_call, n=5):
    batch = batch_call()
    assert len(batch) == n and all(w.dim() == 2 and w.shape[0] == 1 and w.dtype == torch.float32 and w.device.type == "cpu" for w in batch)
    tok_batch = {s: v[-1] for s, v in inj.tokens.items()}
    assert len(tok_batch) == n
    for k in range(n):
        inj.tokens.clear()
        single = single_call(k)
        (seed, toks), = inj.tokens.items()
        assert toks[-1] == tok_batch[seed], f"request {k}: speech tokens in the batch differ from the single run"
        err = _rmse(batch[k], single)
        print(f"request {k}: {batch[k].shape[1]} samples, waveform RMSE batch vs single {err:.3e} (tolerance {TOL_WAV_E2E_8S:.1e})")
        assert err <= TOL_WAV_E2E_8S, f"request {k}: waveform RMSE {err:.3e}"


def _two_voices(api, synth, turbo=False):
    mk = lambda s: api.Conditionals(api.T3Cond(**(dict(synth.t3_cond(seed=s, prompt_len=375), emotion_adv=None) if turbo else synth.t3_cond(seed=s))),
                                    synth.s3gen_ref(seed=s))
    return mk(11), mk(12)


PER = dict(temperature=[0.8, 1.1, 0.7, 0.9, 1.0], top_p=[1.0, 0.9, 0.95, 0.8, 1.0])


@pytest.mark.parametrize("cls_name", ["ChatterboxTTS", "ChatterboxMultilingualTTS"])
@pytest.mark.parametrize("max_batch", [None, 2], ids=["one_batch_serial", "sub_batches_pipelined"])
def test_generate_batch_equals_single_generates(dev, cls_name, max_batch):
    """B = 5 ragged requests, two voices, per-utterance temperature / top_p / cfg_weight through generate_batch -- as one device batch (synthesize) and as three
    sub-batches (synthesize_pipelined) -- against five generate() calls fed the same draws: identical speech tokens, waveforms within TOL_WAV_E2E_8S."""
    from chatterbox_amd import api, synth
    cls = getattr(api, cls_name)
    m = cls.from_synthetic(dev, t3_layers=2)
    m.tokenizer, m.max_batch = _Tok(cls._TEXT_VOCAB), max_batch
    inj = _Inject(m.engine, "max_new_tokens", 1000)
    va, vb = _two_voices(api, synth)
    conds = [va, vb, va, va, vb]
    cfg = [0.5, 0.3, 0.0, 0.5, 0.7]
    lang = dict(language_ids=["en", "fr", "de", "en", "es"]) if cls_name == "ChatterboxMultilingualTTS" else {}
    own = m.conds

    def single(k):
        m.conds = conds[k]
        kw = dict(language_id=lang["language_ids"][k]) if lang else {}
        return m.generate(TEXTS[k], temperature=PER["temperature"][k], top_p=PER["top_p"][k], cfg_weight=cfg[k], **kw)

    _check_batch_equals_singles(m, inj, lambda: m.generate_batch(TEXTS, conds=conds, cfg_weight=cfg, **PER, **lang), single)
    m.conds = own
    m.generate_batch(TEXTS[:2], conds=conds[:2], **({"language_ids": "en"} if lang else {}))
    assert m.conds is own, "generate_batch never overwrites self.conds"


def test_turbo_generate_batch_equals_single_generates(dev):
    from chatterbox_amd import api, synth
    m = api.ChatterboxTurboTTS.from_synthetic(dev, t3_layers=2)
    m.tokenizer = _Tok(50000)
    inj = _Inject(m.engine, "max_gen_len", 1001)
    va, vb = _two_voices(api, synth, turbo=True)
    conds = [va, vb, va, va, vb]
    top_k = [1000, 50, 1000, 20, 400]

    def single(k):
        m.conds = conds[k]
        return m.generate(TEXTS[k], temperature=PER["temperature"][k], top_p=PER["top_p"][k], top_k=top_k[k])

    _check_batch_equals_singles(m, inj, lambda: m.generate_batch(TEXTS, conds=conds, top_k=top_k, **PER), single)


def test_vc_generate_batch_equals_single_generates(dev):
    """Five conversions of ragged length onto two target voices in one call (two sub-batches of MAX_BATCH = 3) against five generate() calls with the same noise."""
    from chatterbox_amd import api, synth
    m = api.ChatterboxVC.from_synthetic(dev)
    m.MAX_BATCH = 3
    toks = [synth.speech_tokens(n, seed=k) for k, n in enumerate((40, 25, 60, 33, 47))]
    refs = [synth.s3gen_ref(seed=11), synth.s3gen_ref(seed=12)]
    ref_of = [refs[0], refs[1], refs[0], refs[0], refs[1]]
    vocode = m.engine.vocode

    def voc(speech_tokens, gen_ref, **kw):
        seeds = [_Inject.seed_of(t) for t in speech_tokens]
        rl = gen_ref if isinstance(gen_ref, (list, tuple)) else [gen_ref] * len(speech_tokens)
        P, Nmax = int(rl[0]["prompt_token"].numel()), max(int(t.numel()) for t in speech_tokens)
        kw["z"] = torch.stack([synth.randn((2 * (P + 64), 80), seed=s + 1) for s in seeds])[:, : 2 * (P + Nmax)].to(dev)
        ph = torch.stack([(synth.rand((9, 1), seed=s + 2) * 2 - 1) * math.pi for s in seeds])
        ph[:, 0] = 0
        kw["phase"], kw["noise"] = ph, torch.stack([synth.randn((9, 960 * 64), seed=s + 3) for s in seeds])[:, :, : 960 * Nmax].to(dev)
        return vocode(speech_tokens, gen_ref, **kw)

    m.engine.vocode = voc
    batch = m.generate_batch(s3_tokens=toks, ref_dicts=ref_of)
    assert len(batch) == 5
    for k in range(5):
        m.ref_dict = ref_of[k]
        single = m.generate(s3_tokens=toks[k])
        err = _rmse(batch[k], single)
        print(f"conversion {k}: {batch[k].shape[1]} samples, waveform RMSE batch vs single {err:.3e} (tolerance {TOL_WAV_E2E_8S:.1e})")
        assert batch[k].shape == (1, 960 * toks[k].numel()) and err <= TOL_WAV_E2E_8S


# ----------------------------------------------------------------------------- against the reference, through the per-utterance plumbing
def test_e2e_b8_vs_reference_through_per_utterance_arguments(dev):
    """test_e2e_synthesize_b8_250_tokens_vs_reference with LISTS where it passes scalars / one dict: eight equal entries per sampling parameter, a list of eight
    cond dicts over the same tensors and a list of eight S3Gen references (golden draws injected).  Same three bounds: the reference's tokens, the waveform
    windows within TOL_WAV_E2E_8S, and the CFM mel of utterance 0 inside the ragged batch (a second vocode on those tokens, list of references) within TOL_MEL[16]."""
    from chatterbox_amd import synth
    from chatterbox_amd.engine import ChatterboxEngine, drop_invalid_tokens
    e, t3g = _need("e2e_b8"), _need("t3_l30_b8")
    B, steps, P = int(t3g["B"]), int(t3g["steps"]), int(e["P"])
    eng = ChatterboxEngine(synth.t3_state_dict(30, 0), synth.s3gen_state_dict(0), dev, n_t3_layers=30)
    texts = [synth.text_tokens(int(t3g["n_text"]), seed=1 + b) for b in range(B)]
    u = torch.from_numpy(t3g["uniforms"]).to(dev)
    ns = [int(drop_invalid_tokens(torch.from_numpy(t3g["tokens"][b]).long()).numel()) for b in range(B)]
    N0, Nmax = int(e["N"]), max(ns)
    T0, Tmax = 2 * (P + N0), 2 * (P + Nmax)
    z = synth.randn((B, Tmax, 80), seed=77)
    z[0, :T0] = synth.randn((1, 80, T0), seed=105)[0].t()
    phase = (synth.rand((B, 9, 1), seed=78) * 2 - 1) * math.pi
    phase[0] = (synth.rand((1, 9, 1), seed=106) * 2 - 1)[0] * math.pi
    phase[:, 0] = 0
    noise = synth.randn((B, 9, 960 * Nmax), seed=79)
    noise[0, :, : 960 * N0] = synth.randn((1, 9, 960 * N0), seed=106)[0]
    cond, ref = synth.t3_cond(), synth.s3gen_ref(n_prompt_tokens=P)
    wavs, st = eng.synthesize(texts, [dict(cond) for _ in range(B)], [ref] * B, max_new_tokens=steps, uniforms=u, z=z.to(dev), phase=phase, noise=noise,
                              drop_last_token=False, **{k: [v] * B for k, v in SAMP.items()})
    assert [int(t.numel()) for t in st] == ns
    for b in range(B):
        assert st[b].tolist() == drop_invalid_tokens(torch.from_numpy(t3g["tokens"][b]).long()).tolist(), f"utterance {b}: speech tokens differ from the reference's"
    assert torch.equal(st[0].cpu(), torch.from_numpy(e["tokens"]).long())
    w0 = wavs[0].float().cpu()
    assert w0.numel() == 960 * N0
    rmse = _window_rmse(w0, dict(win_start=e["win_start"], wav_win=e["wav_win"][None]), 0)
    print(f"end-to-end waveform RMSE {rmse:.3e} (tolerance {TOL_WAV_E2E_8S:.1e})")
    assert rmse <= TOL_WAV_E2E_8S, f"end-to-end waveform RMSE {rmse:.3e} (signal rms {float(e['wav_rms']):.3e})"
    assert eng.flow.precision == 16 and eng.flow.use_planes
    _, mel = eng.vocode(st, [ref] * B, z=z.to(dev), phase=phase, noise=noise)
    err = (mel[0, : 2 * N0].float().cpu() - torch.from_numpy(e["mel"]).t()).abs()
    print(f"mel of utterance 0: L1 {err.mean():.3e} max {err.max():.3e} (tolerance {TOL_MEL[16][0]:.0e} / {TOL_MEL[16][1]:.0e})")
    assert err.mean() <= TOL_MEL[16][0] and err.max() <= TOL_MEL[16][1], f"mel L1 {err.mean():.3e} max {err.max():.3e}"


# ----------------------------------------------------------------------------- generator=
def _short(m, key="max_new_tokens"):
    """Bound the sampled tokens of a synthetic model (it rarely samples EOS); nothing is injected: every draw comes from the generator / the global RNG."""
    gen = m.engine.t3.generate
    m.engine.t3.generate = lambda conds, tt, **kw: gen(conds, tt, **{**kw, key: N_TOK, "ban_eos": True})


@pytest.mark.parametrize("max_batch", [None, 2], ids=["one_batch_serial", "sub_batches_pipelined"])
def test_generate_batch_is_repeatable_with_a_generator(dev, max_batch):
    """Two calls with equally seeded device generators return equal waveforms -- sampling draws, flow noise, vocoder phase and noise all come from the generator, on
    the serial schedule and on the throughput schedule (T3 enqueued by a second host thread) --, another seed gives other audio, and the global RNG is not consumed."""
    from chatterbox_amd import api, synth
    m = api.ChatterboxTTS.from_synthetic(dev, t3_layers=2)
    m.tokenizer, m.max_batch = _Tok(m._TEXT_VOCAB), max_batch
    _short(m)
    va, vb = _two_voices(api, synth)
    conds = [va, vb, va, va, vb]
    g = lambda seed: torch.Generator(device=dev).manual_seed(seed)
    torch.manual_seed(123)
    state = torch.cuda.get_rng_state(dev)
    a = m.generate_batch(TEXTS, conds=conds, generator=g(7), **PER)
    b = m.generate_batch(TEXTS, conds=conds, generator=g(7), **PER)
    c = m.generate_batch(TEXTS, conds=conds, generator=g(8), **PER)
    assert torch.equal(torch.cuda.get_rng_state(dev), state), "a call with a generator leaves the global RNG alone"
    for k in range(5):
        assert a[k].shape == b[k].shape and torch.equal(a[k], b[k]), f"request {k}: same seed, other audio"
    assert any(x.shape != y.shape or not torch.equal(x, y) for x, y in zip(a, c)), "another seed must give other audio"


def test_generate_batch_without_a_generator_draws_from_the_global_rng_as_synthesize_does(dev):
    """generator=None: the call consumes the global RNG exactly as the engine always did -- under the same global seed generate_batch returns what
    engine.synthesize returns for the same batch (uniforms, z, phase, noise drawn in the same order from the same stream of numbers)."""
    from chatterbox_amd import api, synth
    m = api.ChatterboxTTS.from_synthetic(dev, t3_layers=2)
    m.tokenizer = _Tok(m._TEXT_VOCAB)
    _short(m)
    texts = ["Same length one.", "Same length two."]   # equal token counts: the length sort keeps the caller's order
    torch.manual_seed(99)
    got = m.generate_batch(texts, **{k: v[:2] for k, v in PER.items()})
    from chatterbox_amd.text import punc_norm_en
    tts = [torch.cat([torch.tensor([255]), m.tokenizer.text_to_tokens(punc_norm_en(t)).view(-1).long(), torch.tensor([0])]) for t in texts]
    torch.manual_seed(99)
    wavs, _ = m.engine.synthesize(tts, m.conds.t3.as_dict(), m.conds.gen, max_new_tokens=1000, drop_last_token=False, cfg_weight=0.5, repetition_penalty=1.2,
                                  min_p=0.05, **{k: v[:2] for k, v in PER.items()})
    for k in range(2):
        assert torch.equal(got[k][0], wavs[k].float().cpu()), f"request {k}"
    torch.manual_seed(100)
    other = m.generate_batch(texts, **{k: v[:2] for k, v in PER.items()})
    assert not all(x.shape == y.shape and torch.equal(x, y) for x, y in zip(got, other)), "another global seed must give other audio"
