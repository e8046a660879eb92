"""Chunked ("streaming") synthesis of the GPT-2 backbones (-m gpu): TurboEngine.synthesize_stream, the chunked T3TurboEngine decode (generate(async_mode=True) /
advance / peek on the library's token loop cbx_gpt2_loop_*) and the public generate_stream of the three TTS classes.  The schedule's oracle is the one of
tests/test_stream_gpu.py, restated here for Turbo on the CPU oracle's meanflow stage functions (O.flow_inference(meanflow=True, hold_back=...),
O.hift_inference(cache_source=...)) with the final round's three S3GEN_SIL tokens; the bounds are that file's bounds for the same schedule."""
import ctypes
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
TURBO = dict(temperature=0.8, top_k=1000, top_p=0.95, repetition_penalty=1.2)
SIL, EOS = 4299, 6562


def _oracle_stream(O, s3_sd, tokens, ref, z, phase, noise, first, chunk, lookahead, fade, n_steps=2):
    """The schedule of TurboEngine.synthesize_stream for ONE utterance whose `tokens` (valid ids, in order) are all sampled before the last round: round
    r vocodes its first n_r ids, the final round those + three S3GEN_SIL tokens with every token kept."""
    N, P = tokens.numel(), ref["prompt_token"].shape[1]
    pieces, emitted, tail, cache, n = [], 0, None, None, min(N, first + lookahead)
    ramp = torch.linspace(0.0, 1.0, fade + 2)[1:-1]
    sil = torch.full((3,), SIL, dtype=torch.long)
    while True:
        final = n >= N
        hold = 0 if final else 2 * lookahead
        toks = torch.cat([tokens[:n], sil]) if final else tokens[:n]
        m = toks.numel()
        mel = O.flow_inference(s3_sd, toks[None], torch.tensor([m]), ref, z[:, :, : 2 * (P + m)], n_steps, meanflow=True, hold_back=torch.tensor([hold]))
        frames = 2 * m - hold
        wav, src = O.hift_inference(s3_sd, mel[:, :, :frames], phase, noise[:, :, : 480 * frames], cache_source=cache)
        wav = O.trim_fade(wav)[0]
        cache = src[:, :, : 480 * frames]
        avail = min(480 * frames, m * 960) if final else 480 * frames
        end = avail if final else max(emitted, avail - fade)
        new = wav[emitted:end].clone()
        if tail is not None and new.numel():
            k = min(tail.numel(), new.numel())
            new[:k] = tail[:k] * (1 - ramp[:k]) + new[:k] * ramp[:k]
        tail = None if final else wav[end: min(avail, end + fade)].clone()
        emitted = end
        pieces.append(new)
        if final:
            return pieces
        n = min(N, n + max(1, int(round(chunk))))


def _setup(dev, B, nano, n_tok, P=8, eos_bias=None):
    """2-layer Turbo (D = 1024) or Nano (D = 768) T3, S3Gen with n_mid=2, n_enc=1, n_up_enc=1; B utterances of one voice; n_tok = max_gen_len + 1 tokens;
    injected uniforms / z / phase / noise sized for n_tok + 3 tokens."""
    from chatterbox_amd import synth
    from chatterbox_amd.engine import TurboEngine
    t3_sd = synth.t3_turbo_state_dict(2, 768 if nano else 1024, 0)
    if eos_bias is not None:
        t3_sd["speech_head.bias"][EOS] = eos_bias
    s3_sd = synth.s3gen_state_dict(0, meanflow=True, n_mid=2, n_enc=1, n_up_enc=1)
    eng = TurboEngine(t3_sd, s3_sd, dev, n_t3_layers=2)
    texts = [synth.turbo_text_tokens(n, seed=s) for n, s in ((10, 1), (17, 2), (5, 3))[:B]]
    cond, ref = synth.t3_cond(prompt_len=24), synth.s3gen_ref(n_prompt_tokens=P)
    M = n_tok + 3
    z = synth.randn((B, 80, 2 * (P + M)), seed=5)
    phase = (synth.rand((B, 9, 1), seed=6) * 2 - 1) * math.pi
    phase[:, 0] = 0
    noise = synth.randn((B, 9, 960 * M), seed=6)
    kw = dict(max_gen_len=n_tok - 1, uniforms=synth.rand((B, n_tok), seed=3), z=z.transpose(1, 2).contiguous(), phase=phase, noise=noise, **TURBO)
    return eng, t3_sd, s3_sd, texts, cond, ref, z, phase, noise, kw


@pytest.mark.parametrize("nano", [False, True], ids=["turbo", "nano"])
@pytest.mark.parametrize("B", [1, 3], ids=["B1_row_path", "B3_packed_path"])
@pytest.mark.parametrize("overlap", [True, False], ids=["overlapped", "serial"])
def test_turbo_stream_matches_oracle_schedule(dev, nano, B, overlap):
    """Streamed == oracle-streamed (RMSE <= 2e-3), per-round piece lengths == the oracle's, total length == synthesize()'s, tokens == the one-shot run's,
    seams no rougher than twice the one-shot waveform's largest step (+ 1e-3).  Measured on the MI355X (profiles/turbo_stream_tests.log): RMSE 4.8e-5 ..
    1.35e-4 over the 16 utterance cases, identical for overlap on and off; the streamed waveform's largest step at most 1.08x the one-shot one's."""
    from oracle import ref_torch as O
    n_tok, P, first, chunk, look, fade = 20, 8, 6, 7, 3, 240
    eng, _, s3_sd, texts, cond, ref, z, phase, noise, kw = _setup(dev, B, nano, n_tok, P)
    rounds = list(eng.synthesize_stream(texts, cond, ref, first_chunk=first, chunk=chunk, lookahead=look, fade=fade, overlap=overlap, ban_eos=True,
                                        ban_from=6561, **kw))
    assert len(rounds) == 3 and rounds[0]["n_tokens"] == [9] * B and rounds[-1]["final"] == [True] * B  # 9 -> 16 -> 20 tokens (+ 3 silence)
    full, toks = eng.synthesize(texts, cond, ref, ban_eos=True, ban_from=6561, **kw)
    for b in range(B):
        assert rounds[-1]["tokens"][b].tolist() == toks[b].tolist(), f"utt {b}: streamed tokens differ from the one-shot run"
        streamed = torch.cat([r["wavs"][b] for r in rounds])
        pieces = _oracle_stream(O, s3_sd, toks[b][:-3], ref, z[b:b + 1], phase[b:b + 1], noise[b:b + 1], first, chunk, look, fade)
        rmse = (streamed - torch.cat(pieces)).pow(2).mean().sqrt().item() if streamed.numel() == sum(p.numel() for p in pieces) else float("nan")
        jump = (streamed[1:] - streamed[:-1]).abs().max().item()
        step = (full[b].cpu()[1:] - full[b].cpu()[:-1]).abs().max().item()
        print(f"[turbo-stream] nano={nano} B={B} overlap={overlap} utt={b}: pieces {[r['wavs'][b].numel() for r in rounds]} oracle {[p.numel() for p in pieces]} "
              f"total {streamed.numel()} one-shot {full[b].numel()} RMSE {rmse:.3e} max seam step {jump:.3e} one-shot max step {step:.3e}")
        assert [p.numel() for p in pieces] == [r["wavs"][b].numel() for r in rounds]
        assert streamed.numel() == (n_tok + 3) * 960 == full[b].numel()
        assert rmse <= 2e-3, f"utt {b}: streamed vs oracle-streamed RMSE {rmse:.3e}"
        assert jump <= 2.0 * step + 1e-3


def test_turbo_stream_last_round_is_the_full_synthesis(dev):
    """Beyond the vocoder's receptive field (8000 samples) past the cache seam the last round reproduces synthesize() to 1e-5."""
    n_tok, P = 30, 8
    eng, _, s3_sd, texts, cond, ref, z, phase, noise, kw = _setup(dev, 1, False, n_tok, P)
    rounds = list(eng.synthesize_stream(texts, cond, ref, first_chunk=6, chunk=40, lookahead=3, fade=240, ban_eos=True, ban_from=6561, **kw))
    assert len(rounds) == 2
    full, _ = eng.synthesize(texts, cond, ref, ban_eos=True, ban_from=6561, **kw)
    streamed = torch.cat([r["wavs"][0] for r in rounds])
    cache_end = 480 * (2 * 9 - 6)
    a, c = streamed[cache_end + 8000:], full[0].cpu()[cache_end + 8000:]
    err = (a - c).abs().max().item()
    print(f"[turbo-stream] last round vs synthesize(): {a.numel()} samples compared, max |diff| {err:.3e}")
    assert a.numel() > 10000 and err <= 1e-5


def test_turbo_stream_ends_on_the_round_that_sampled_eos(dev):
    """EOS inside the stream: with the EOS bias of the speech head raised (chosen on the one-shot path so that EOS falls in round >= 1, well before
    max_gen_len) the stream ends on that round with final=True, its tokens are the one-shot tokens and its length the one-shot length."""
    from chatterbox_amd import synth
    from chatterbox_amd.t3_turbo import T3TurboEngine
    n_tok, P, first, chunk, look = 41, 8, 6, 7, 3   # rounds after 9, 16, 23, 30, 37, 41 sampled tokens
    cond, text, u = synth.t3_cond(prompt_len=24), synth.turbo_text_tokens(10, seed=1), synth.rand((1, n_tok), seed=3)
    chosen = None
    for bias in (2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0, 9.0, 10.0, 12.0, 14.0):
        sd = synth.t3_turbo_state_dict(2, 1024, 0)
        sd["speech_head.bias"][EOS] = bias
        t3 = T3TurboEngine(sd, dev)
        t3.generate(cond, [text], max_gen_len=n_tok - 1, uniforms=u, **TURBO)
        n_gen = int(next(iter(t3._state.values()))["n_generated"][0])
        done = bool(next(iter(t3._state.values()))["done"][0])
        if done and first + look < n_gen <= 30:
            chosen = (bias, n_gen)
            break
    print(f"[turbo-stream] EOS bias {chosen}")
    assert chosen is not None, "no EOS bias puts the EOS into rounds 1 .. 3"
    eng, _, _, texts, cond, ref, z, phase, noise, kw = _setup(dev, 1, False, n_tok, P, eos_bias=chosen[0])
    rounds = list(eng.synthesize_stream(texts, cond, ref, first_chunk=first, chunk=chunk, lookahead=look, fade=240, **kw))
    toks = eng.t3.generate(cond, texts, max_gen_len=n_tok - 1, uniforms=kw["uniforms"], **TURBO)
    m = int((toks[0] < 6561).sum()) + 3
    one = dict(kw, z=kw["z"][:, : 2 * (P + m)].contiguous(), noise=kw["noise"][:, :, : 960 * m].contiguous())
    full, st = eng.synthesize(texts, cond, ref, **one)
    schedule = [9, 16, 23, 30, 37, 41]
    want_rounds = next(r for r, n_r in enumerate(schedule) if n_r >= chosen[1]) + 1
    print(f"[turbo-stream] EOS after {chosen[1]} tokens: {len(rounds)} rounds (want {want_rounds}), length {sum(r['wavs'][0].numel() for r in rounds)} "
          f"vs one-shot {full[0].numel()}")
    assert len(rounds) == want_rounds >= 2 and rounds[-1]["final"] == [True] and not any(r["final"][0] for r in rounds[:-1])
    assert rounds[-1]["tokens"][0].tolist() == st[0].tolist()
    assert sum(r["wavs"][0].numel() for r in rounds) == full[0].numel()


def _snapshot(st):
    snap = {k: v.clone() for k, v in st.items() if torch.is_tensor(v)}
    snap.update({("dws", k): v.clone() for k, v in st["dws"].items()})
    return snap


def _restore(st, snap):
    for k, v in snap.items():
        (st["dws"][k[1]] if isinstance(k, tuple) else st[k]).copy_(v)


@pytest.mark.parametrize("B", [1, 3], ids=["B1_row_path", "B3_packed_path"])
@torch.inference_mode()
def test_gpt2_token_loop_in_c_equals_the_python_replay_loop(dev, B):
    """cbx_gpt2_loop_run of n steps == n replays of the torch-captured Python step from the same state (out_tokens, n_generated, logits bit for bit);
    poll_every > 0 stops at the first poll once every row is done and *steps_run reports the steps enqueued; chunked generate == one-shot generate."""
    from chatterbox_amd import synth
    from chatterbox_amd._lib import check, lib
    from chatterbox_amd.t3_turbo import T3TurboEngine
    n = 24
    eng = T3TurboEngine(synth.t3_turbo_state_dict(2, 1024, 0), dev)
    texts = [synth.turbo_text_tokens(k, seed=s) for k, s in ((10, 1), (17, 2), (5, 3))[:B]]
    cond, u = synth.t3_cond(prompt_len=24), synth.rand((B, n + 1), seed=3)
    h = eng.generate(cond, texts, max_gen_len=n, uniforms=u, ban_eos=True, async_mode=True, run_steps=1, **TURBO)
    st = h["st"]
    torch.cuda.synchronize()
    snap = _snapshot(st)
    eng._capture(st)
    for _ in range(n):
        st["graph"].replay()
    want = {k: st[k].clone() for k in ("out_tokens", "n_generated", "logits", "kc", "vc")}
    _restore(st, snap)
    assert eng._run_c_loop(st, n, 0) == n
    for k, v in want.items():
        assert torch.equal(v, st[k]), f"cbx_gpt2_loop_run differs from the Python replay loop in {k}"
    _restore(st, snap)
    st["done"].fill_(1)
    ran = ctypes.c_int(-1)
    check(lib.cbx_gpt2_loop_run(eng._c_loop(st), 12, 4, torch.cuda.current_stream().cuda_stream, ctypes.byref(ran)), "cbx_gpt2_loop_run")
    assert ran.value == 4, ran.value
    st["done"].zero_()
    check(lib.cbx_gpt2_loop_run(eng._c_loop(st), 12, 4, torch.cuda.current_stream().cuda_stream, ctypes.byref(ran)), "cbx_gpt2_loop_run")
    assert ran.value == 12, ran.value
    # chunked decoding through the C loop == the one-shot Python replay loop
    one = eng.generate(cond, texts, max_gen_len=n, uniforms=u, ban_eos=True, **TURBO)
    h = eng.generate(cond, texts, max_gen_len=n, uniforms=u, ban_eos=True, async_mode=True, run_steps=5, **TURBO)
    while eng.advance(h, 7):
        pass
    assert [t.tolist() for t in eng.collect(h)] == [t.tolist() for t in one]


class _Watermarker:
    def __init__(self):
        self.calls = 0

    def apply_watermark(self, wav, sample_rate):
        self.calls += 1
        return wav


class _TokLlama:
    def __init__(self, toks):
        self.toks = toks

    def text_to_tokens(self, text, language_id=None):
        return self.toks


class _TokTurbo:
    def __init__(self, toks):
        self.toks = toks

    def __call__(self, text, **kw):
        return type("Enc", (), {"input_ids": self.toks[None]})()


@pytest.mark.parametrize("cls_name", ["ChatterboxTurboTTS", "ChatterboxTTS", "ChatterboxMultilingualTTS"])
def test_generate_stream_public_api(dev, cls_name):
    """generate_stream of each TTS class == the engine's synthesize_stream on the same text tokens (same seed), pieces (1, n) float32 CPU tensors, the
    watermarker applied once per piece."""
    from chatterbox_amd import api, synth
    cls = getattr(api, cls_name)
    turbo = cls_name == "ChatterboxTurboTTS"
    m = cls.from_synthetic(dev, t3_layers=2)
    if turbo:
        tt = synth.turbo_text_tokens(12)
        m.tokenizer = _TokTurbo(tt)
    else:
        tt = synth.text_tokens(12, vocab=cls._TEXT_VOCAB)[1:-1]  # ids inside the class's text embedding (704 rows for ChatterboxTTS)
        m.tokenizer = _TokLlama(tt)
    wm = _Watermarker()
    m.watermarker = wm
    kw = dict(first_chunk=10, chunk=60, chunk_growth=2.0)
    torch.manual_seed(7)
    if cls_name == "ChatterboxMultilingualTTS":
        pieces = list(m.generate_stream("hello", "en", **kw))
    else:
        pieces = list(m.generate_stream("hello", **kw))
    torch.manual_seed(7)
    if turbo:
        rounds = m.engine.synthesize_stream([tt], m.conds.t3.as_dict(), m.conds.gen, temperature=0.8, top_k=1000, top_p=0.95, repetition_penalty=1.2, **kw)
    else:
        tt2 = torch.cat([torch.tensor([255]), tt.long(), torch.tensor([0])])
        rounds = m.engine.synthesize_stream([tt2], m.conds.t3.as_dict(), m.conds.gen, max_new_tokens=1000, drop_last_token=cls_name != "ChatterboxTTS",
                                            temperature=0.8, cfg_weight=0.5, repetition_penalty=1.2, min_p=0.05, top_p=1.0, **kw)
    want = [r["wavs"][0] for r in rounds if r["wavs"][0].numel()]
    print(f"[turbo-stream] {cls_name}.generate_stream: {len(pieces)} pieces of {[p.shape[1] for p in pieces]} samples")
    assert len(pieces) == len(want) >= 1 and wm.calls == len(pieces)
    for p, w in zip(pieces, want):
        assert p.dim() == 2 and p.shape[0] == 1 and p.dtype == torch.float32 and p.device.type == "cpu"
        assert torch.equal(p[0], w)
