"""GPU (-m gpu): word_times= through T3Engine.align, the engine and the public API on the synthetic 2-layer models of test_loudness_api_gpu.py (token budget 20,
EOS banned), with explicit align_heads on layers 0 and 1 and a stand-in tokenizer that has pieces().

The pass against an independent forward: last_alignment["mass"] against the fp64 restatement of the conditional row over the WHOLE sequence [34 conditioning | text
| BOS BOS | speech] -- weights from the synthetic state dict, K / V recomputed at every position, nothing read from the cache (word_times_common.llama_layers64,
pinned against oracle.ref_torch.llama_forward below) -- within |err| <= 2e-5 (1 + |ref|), the tolerance of the kernel tests: ahead of the attention the only
error is that of the prefill's fp32 GEMMs.  The test prints the worst figure.
The path: the device spans are the NumPy recurrence run on the device mass, bit for bit.
The kernel-level tests are in test_turbo_stream_word_times_kernels_gpu.py."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import word_times_common as W  # noqa: E402
from test_loudness_api_gpu import N_TOK, _model  # noqa: E402  (read-only import: the synthetic models of that module, token budget 20, EOS banned)
from test_seeded_api_gpu import SEEDS, TEXTS, _Tok  # noqa: E402  (read-only import: the stand-in tokenizer, the requests)

pytestmark = pytest.mark.gpu

HEADS = ((0, 3), (1, 5), (1, 9))


class _PiecesTok(_Tok):
    """_Tok that remembers the characters its ids came from: pieces() of the engine's tokens [SOT | ids | EOT]"""
    SPACE = "[SPACE]"

    def __init__(self, vocab):
        super().__init__(vocab)
        self.seen = {}

    def _ids(self, text):
        ids = super()._ids(text)
        self.seen[tuple(ids.tolist())] = [self.SPACE if c == " " else c for c in text]
        return ids

    def pieces(self, ids):
        return ["[START]"] + self.seen[tuple(ids[1:-1])] + ["[STOP]"]


@pytest.fixture()
def tts(dev):
    m, _ = _model(dev, "ChatterboxTTS")
    saved = m.tokenizer, m.align_heads
    m.tokenizer, m.align_heads = _PiecesTok(type(m)._TEXT_VOCAB), HEADS
    yield m
    m.tokenizer, m.align_heads = saved


def _sd64():
    from chatterbox_amd import api, synth
    return {k: v.double() for k, v in synth.t3_state_dict(2, 0, text_vocab=api.ChatterboxTTS._TEXT_VOCAB).items()}


def _layers64(sd, n):
    g = lambda i, name: sd[f"tfmr.layers.{i}.{name}.weight"].numpy()
    return [dict(ln1=g(i, "input_layernorm"), ln2=g(i, "post_attention_layernorm"), wq=g(i, "self_attn.q_proj"), wk=g(i, "self_attn.k_proj"), wv=g(i, "self_attn.v_proj"),
                 wo=g(i, "self_attn.o_proj"), wg=g(i, "mlp.gate_proj"), wu=g(i, "mlp.up_proj"), wd=g(i, "mlp.down_proj")) for i in range(n)]


def test_the_restated_layers_are_the_oracles():
    """word_times_common.llama_layers64 against oracle.ref_torch.llama_forward on fp64 weights and inputs, same cos / sin tables: equal to fp64 rounding once the
    restatement takes the mean square of its RMSNorms in fp32 as the oracle does (rms_norm: x.float()); with its own fp64 norm, the form the engine is compared
    with, the two agree to that fp32 step's rounding (no GPU involved)"""
    from oracle import ref_torch
    sd = _sd64()
    x = torch.randn(1, 23, 1024, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    want, _ = ref_torch.llama_forward(sd, x, 2)
    cos, sin = ref_torch.rope_cos_sin(torch.arange(23), ref_torch.llama3_inv_freq(64))
    errs = []
    for oracle_norm in (True, False):
        h, qk = W.llama_layers64(x[0].numpy(), _layers64(sd, 2), cos.double().numpy(), sin.double().numpy(), 16, oracle_norm=oracle_norm)
        got = ref_torch.rms_norm(torch.from_numpy(h), sd["tfmr.norm.weight"]).numpy()
        errs.append(float(np.abs(got - want[0].numpy()).max() / np.abs(want[0].numpy()).max()))
    print(f"restated layers against the oracle: max relative error {errs[0]:.3g} (the oracle's fp32 mean square), {errs[1]:.3g} (fp64 throughout)")
    assert errs[0] <= 1e-12 and errs[1] <= 1e-6 and len(qk) == 2 and qk[0][0].shape == (23, 16, 64)


def _restated_mass(m, tokens, toks, heads):
    """the fp64 text mass of ONE request from an independent forward over the whole sequence of its conditional row"""
    t3 = m.engine.t3
    sd = _sd64()
    n, tl = int(toks.numel()), int(tokens.numel())
    emb = lambda k: sd[k].numpy()
    cond = t3.cond_embeds(m.conds.t3.as_dict()).double().cpu().numpy()  # (34, D): the conditioning positions are the request's input
    text = emb("text_emb.weight")[tokens.numpy()] + emb("text_pos_emb.emb.weight")[:tl]
    bos = (emb("speech_emb.weight")[6561] + emb("speech_pos_emb.emb.weight")[0])[None].repeat(2, 0)
    speech = emb("speech_emb.weight")[toks[: n - 1].numpy()] + emb("speech_pos_emb.emb.weight")[1:n]
    x = np.concatenate([cond, text, bos, speech])
    S = x.shape[0]
    assert S == 34 + tl + 2 + n - 1
    _, qk = W.llama_layers64(x, _layers64(sd, 2), t3.cos[:S].double().cpu().numpy(), t3.sin[:S].double().cpu().numpy(), 16, upto=max(l for l, _ in heads) + 1)
    ref = np.zeros((n, tl))
    for l, h in heads:
        q, k = qk[l]
        ref += W.mass_ref(q[None, 34 + tl + 1:], k[None], [h], [n], [34 + tl + 1], [34], [tl], 0.125, 1.0 / len(heads))[0]
    return ref


def test_the_pass_is_the_independent_forward_and_the_path_is_the_recurrence(dev, tts):
    """Measured on one MI355X: worst err / (1 + |ref|) = 1.23e-7 over the three requests, against the bound 2e-5 of the kernel tests -- no wider constant was
    needed, so the flash_attn prefill path was not measured for one."""
    from chatterbox_amd import engine as E
    m = tts
    reqs = [m._engine_tokens(m._text_ids(t)) for t in (TEXTS[0], TEXTS[3], TEXTS[2])]
    with torch.cuda.device(dev):
        wavs, st, al = m.engine.synthesize(reqs, m.conds.t3.as_dict(), m.conds.gen, seeds=[11, 12, 13], words=dict(heads=HEADS), drop_last_token=False)
        la = m.engine.t3.last_alignment
        mass, spans, frame_tok = la["mass"].cpu().numpy(), la["spans"].cpu().numpy(), la["frame_tok"].cpu().numpy()
        assert la["n"] == [N_TOK] * 3 and la["m"] == [int(t.numel()) for t in reqs]
        worst = 0.0
        for b in (0, 1, 2):
            n, tl = la["n"][b], la["m"][b]
            ref = _restated_mass(m, reqs[b], la["tokens"][b], HEADS)
            assert np.isfinite(mass[b, :n, :tl]).all()
            worst = max(worst, float((np.abs(mass[b, :n, :tl] - ref) / (1.0 + np.abs(ref))).max()))
            sp, ft = W.path_ref(mass[b], n, tl)
            assert np.array_equal(spans[b, :tl], sp) and np.array_equal(frame_tok[b, :n], ft), "the device path is the recurrence on the device mass, bit for bit"
            c = E.valid_frame_counts(la["tokens"][b])
            assert al[b]["frames"] == [(c[f0], c[f1]) for f0, f1 in sp.tolist()] and al[b]["n_frames"] == c[-1] == int(st[b].numel()), "frames count the valid tokens"
            assert 0.0 < mass[b, :n, :tl].sum(1).min() and mass[b, :n, :tl].sum(1).max() <= 1.0 + 1e-5, "a frame's text mass is a share of its attention"
    print(f"alignment pass against the independent fp64 forward: worst err / (1 + |ref|) = {worst:.3g} (bound {W.MASS_TOL})")
    assert worst <= W.MASS_TOL, worst


def _check_words(words, n):
    assert words and all(set(w) == {"text", "start", "stop", "tokens", "frames"} for w in words)
    assert all(0 <= w["start"] <= w["stop"] <= n for w in words) and all(a["stop"] == b["start"] for a, b in zip(words, words[1:]))


def test_words_cover_the_waveform_and_a_batch_gives_each_request_its_own(dev, tts):
    m = tts
    texts, seeds = [TEXTS[0], TEXTS[3], TEXTS[2]], [SEEDS[0], SEEDS[3], SEEDS[2]]
    plain = m.generate(texts[0], seed=seeds[0])
    off = m.generate(texts[0], seed=seeds[0], word_times=False)
    assert torch.is_tensor(off) and torch.equal(plain, off), "word_times=False: a tensor, bitwise the call without the argument"
    alone = [m.generate(t, seed=s, word_times=True) for t, s in zip(texts, seeds)]
    assert torch.equal(alone[0][0], plain), "the pass changes nothing the vocoder reads"
    for (wav, words), t in zip(alone, texts):
        _check_words(words, wav.shape[-1])
        assert [w["text"] for w in words] == t.split(), "the words are the text's"
    batch = m.generate_batch(texts, seeds=seeds, word_times=True)
    for (wav, words), (wav1, words1) in zip(batch, alone):
        _check_words(words, wav.shape[-1])
        assert wav.shape == wav1.shape
        assert [(w["tokens"], w["frames"], w["start"], w["stop"]) for w in words] == [(w["tokens"], w["frames"], w["start"], w["stop"]) for w in words1], \
            "a request's frames do not depend on the batch around it"
    toks = m.generate(texts[2], seed=seeds[2], word_times="tokens")[1]
    assert len(toks) == len(texts[2]) + 2 and toks[0]["text"] == "[START]" and [t["tokens"] for t in toks] == [(i, i + 1) for i in range(len(toks))]


def test_speed_and_sample_rate_map_the_boundaries(dev, tts):
    from chatterbox_amd import engine as E, ops
    m = tts
    wav1, base = m.generate(TEXTS[3], seed=SEEDS[3], word_times=True)
    wav, words = m.generate(TEXTS[3], seed=SEEDS[3], speed=1.25, sample_rate=16000, word_times=True)
    n24 = 480 * ops.scaled_len(wav1.shape[-1] // 480, 1.25)
    assert wav.shape[-1] == ops.formatted_len(n24, 16000)
    _check_words(words, wav.shape[-1])
    assert [w["frames"] for w in words] == [w["frames"] for w in base], "T3 and its tokens do not depend on speed or the format"
    at = lambda f: min(wav.shape[-1], ops.formatted_len(E.frame_sample(f, 1.25), 16000))
    assert [w["start"] for w in words] == [at(w["frames"][0]) for w in words] and words[-1]["stop"] == at(words[-1]["frames"][1])


def test_generate_long_puts_every_word_inside_its_segment(dev, tts):
    m = tts
    text = "Hello there. Numbers one two three four. Hi."
    wav, segs = m.generate_long(text, max_chars=30, seed=5, return_segments=True, word_times=True)
    assert len(segs) >= 2
    for seg in segs:
        _check_words(seg["words"], wav.shape[-1])
        assert all(seg["start"] <= w["start"] and w["stop"] <= seg["stop"] for w in seg["words"]), "every word lies inside its segment"
        assert [w["text"] for w in seg["words"]] == seg["text"].split()
    plain, plain_segs = m.generate_long(text, max_chars=30, seed=5, return_segments=True)
    assert torch.equal(plain, wav) and all("words" not in s for s in plain_segs)
    with pytest.raises(ValueError, match="return_segments"):
        m.generate_long(text, word_times=True)


def test_what_does_not_take_the_argument(dev, tts):
    turbo, _ = _model(dev, "ChatterboxTurboTTS")
    with pytest.raises(TypeError, match="word_times"):
        turbo.generate(TEXTS[2], word_times=True)
    for call in (lambda: tts.generate_stream(TEXTS[2], word_times=True), lambda: tts.generate_long_stream(TEXTS[2], word_times=True)):
        with pytest.raises(TypeError, match="word_times"):
            call()
    with pytest.raises(ValueError, match="max_pause.*word_times"):
        tts.generate(TEXTS[2], max_pause=0.2, word_times=True)
    with pytest.raises(ValueError, match="layer 9"):
        tts.engine.synthesize([tts._engine_tokens(tts._text_ids(TEXTS[2]))], tts.conds.t3.as_dict(), tts.conds.gen, words=dict(heads=None))
    jobs = [dict(text_tokens=[tts._engine_tokens(tts._text_ids(TEXTS[2]))], t3_conds=tts.conds.t3.as_dict(), gen_ref=tts.conds.gen, words=dict(heads=HEADS))]
    with pytest.raises(ValueError, match="synthesize"):
        next(iter(tts.engine.synthesize_pipelined(jobs)))
