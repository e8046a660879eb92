"""GPU (-m gpu): per-request seeds through the engines and the public API on synthetic 2-layer models -- the seeded draws are exactly what cbx_rng_fill_f32
gives for the request's key, a request's result does not depend on the batch around it (identical speech tokens, waveform within TOL_WAV_E2E_8S: the standard
of the batch-vs-single tests; the kernels pick forms by row count, so not bit equality), seeded calls repeat and leave torch's RNG alone, and a seeded windowed
stream fills its noise round by round with the values of the full fill.  The kernel-level tests are in test_turbo_stream_seeded_rng_kernels_gpu.py."""
import math
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import seeded_rng_common as R  # noqa: E402
from test_baseline_shapes_gpu import SAMP, TOL_WAV_E2E_8S  # noqa: E402  (read-only import: the stated tolerance)

pytestmark = pytest.mark.gpu


# ----------------------------------------------------------------------------- draws filled in the test, from the keys (stream ids and layouts restated here)
def _uniforms(dev, seeds, n):
    from chatterbox_amd import ops
    return ops.rng_fill(torch.empty(len(seeds), n, device=dev), R.key_tensor([(s, 0, 0) for s in seeds], dev))


def _z(dev, seeds, frames):
    from chatterbox_amd import ops
    z = torch.empty(len(seeds), frames * 80, device=dev)   # one row per request, column = frame * 80 + channel
    return ops.rng_fill(z, R.key_tensor([(s, 0, 1) for s in seeds], dev), normal=True).view(len(seeds), frames, 80)


def _phase(dev, seeds):
    from chatterbox_amd import ops
    u = ops.rng_fill(torch.empty(len(seeds), 9, device=dev), R.key_tensor([(s, 0, 2) for s in seeds], dev))
    ph = (u * 2 - 1) * math.pi
    ph[:, 0] = 0
    return ph


def _noise(dev, seeds, n):
    from chatterbox_amd import ops
    x = torch.empty(len(seeds) * 9, n, device=dev)          # substream = harmonic, column = absolute sample
    return ops.rng_fill(x, R.key_tensor([(s, h, 3) for s in seeds for h in range(9)], dev), normal=True).view(len(seeds), 9, n)


# ----------------------------------------------------------------------------- the seeded draws are what the kernel says
def test_t3_seeds_equal_injected_uniforms_of_the_same_keys(dev, steps=8):
    from chatterbox_amd import synth
    from chatterbox_amd.t3 import T3Engine
    eng = T3Engine(synth.t3_state_dict(2, 0), dev)
    tt = [synth.text_tokens(n, seed=i + 1) for i, n in enumerate((12, 20, 7))]
    seeds = [5, 2 ** 63 + 7, 12345]
    kw = dict(max_new_tokens=steps, ban_eos=True, **SAMP)
    torch.manual_seed(1)
    state = torch.cuda.get_rng_state(dev)
    a = eng.generate(synth.t3_cond(), tt, seeds=seeds, **kw)
    assert torch.equal(torch.cuda.get_rng_state(dev), state), "a seeded call consumes no torch RNG"
    b = eng.generate(synth.t3_cond(), tt, uniforms=_uniforms(dev, seeds, steps), **kw)
    assert [t.tolist() for t in a] == [t.tolist() for t in b] and all(t.numel() == steps for t in a)
    c = eng.generate(synth.t3_cond(), tt, seeds=[5, 2 ** 63 + 7, 12346], **kw)
    assert [t.tolist() for t in c[:2]] == [t.tolist() for t in a[:2]] and c[2].tolist() != a[2].tolist()
    inj = eng.generate(synth.t3_cond(), tt, seeds=[1, 2, 3], uniforms=_uniforms(dev, seeds, steps), **kw)   # injected uniforms win over the seeds
    assert [t.tolist() for t in inj] == [t.tolist() for t in a]
    with pytest.raises(ValueError, match="generator"):
        eng.generate(synth.t3_cond(), tt, seeds=seeds, generator=torch.Generator(device=dev), **kw)
    with pytest.raises(ValueError, match="seeds"):
        eng.generate(synth.t3_cond(), tt, seeds=seeds[:2], **kw)


@pytest.mark.parametrize("B", [1, 3], ids=["row_path_b1", "b3"])
def test_turbo_t3_seeds_equal_injected_uniforms_of_the_same_keys(dev, B, steps=7):
    from chatterbox_amd import synth
    from chatterbox_amd.t3_turbo import T3TurboEngine
    eng = T3TurboEngine(synth.t3_turbo_state_dict(2, 768, 0), dev)
    tt = [synth.turbo_text_tokens(n, seed=i + 1) for i, n in enumerate((7, 20, 1)[:B])]
    seeds = [2 ** 64 - 1, 0, 77][:B]
    cond = synth.t3_cond(prompt_len=375)
    a = eng.generate(cond, tt, max_gen_len=steps, ban_eos=True, seeds=seeds)
    b = eng.generate(cond, tt, max_gen_len=steps, ban_eos=True, uniforms=_uniforms(dev, seeds, steps + 1))
    assert [t.tolist() for t in a] == [t.tolist() for t in b] and all(t.numel() == steps + 1 for t in a)
    with pytest.raises(ValueError, match="generator"):
        eng.generate(cond, tt, max_gen_len=steps, seeds=seeds, generator=torch.Generator(device=dev))


def test_vocode_seeds_equal_injected_noise_of_the_same_keys(dev):
    """Ragged batch of three: vocode(seeds=) is torch.equal to vocode(z=, phase=, noise=) filled from the same keys (z over the padded frames, noise over the
    padded samples: row b reads its own columns), and consumes no torch RNG; an injected tensor wins over the seed."""
    from chatterbox_amd import synth
    from chatterbox_amd.engine import ChatterboxEngine
    P = 6
    eng = ChatterboxEngine(synth.t3_state_dict(2, 0), synth.s3gen_state_dict(0, n_mid=1, n_enc=1, n_up_enc=1), dev, n_t3_layers=2)
    ref = synth.s3gen_ref(n_prompt_tokens=P)
    st = [synth.speech_tokens(n, seed=k) for k, n in enumerate((9, 5, 12))]
    seeds, Nmax = [11, 2 ** 40, 13], 12
    torch.manual_seed(3)
    state = torch.cuda.get_rng_state(dev)
    a, mel_a = eng.vocode(st, ref, seeds=seeds, n_cfm_timesteps=2)
    assert torch.equal(torch.cuda.get_rng_state(dev), state), "a seeded call consumes no torch RNG"
    z, ph, nz = _z(dev, seeds, 2 * (P + Nmax)), _phase(dev, seeds), _noise(dev, seeds, 960 * Nmax)
    b, mel_b = eng.vocode(st, ref, z=z, phase=ph, noise=nz, n_cfm_timesteps=2)
    assert torch.equal(mel_a, mel_b)
    for k in range(3):
        assert a[k].shape == (960 * st[k].numel(),) and torch.equal(a[k], b[k]), f"utterance {k}"
    c, _ = eng.vocode(st, ref, seeds=[1, 2, 3], z=z, phase=ph, noise=nz, n_cfm_timesteps=2)   # every injected tensor wins
    assert all(torch.equal(x, y) for x, y in zip(a, c))
    d, _ = eng.vocode(st, ref, seeds=[11, 2 ** 40, 14], n_cfm_timesteps=2)
    assert not torch.equal(d[2], a[2]), "another seed must give that utterance other audio"
    with pytest.raises(ValueError, match="generator"):
        eng.vocode(st, ref, seeds=seeds, generator=torch.Generator(device=dev))


# ----------------------------------------------------------------------------- a request's result does not depend on the batch around it
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
SEEDS = [1001, 2 ** 64 - 1, 0, 2 ** 32 + 5, 424242]
N_TOK = 8
PER = dict(temperature=[0.8, 1.1, 0.7, 0.9, 1.0], top_p=[1.0, 0.9, 0.95, 0.8, 1.0])


def _bound_and_record(engine, key):
    """Bound the sampled tokens (synthetic weights rarely sample EOS: `key` = N_TOK and ban_eos) and record the speech tokens every seeded request is vocoded from:
    {seed: [token lists, in call order]}.  Nothing is injected."""
    rec = {}
    if engine.t3 is not None:
        gen = engine.t3.generate
        engine.t3.generate = lambda conds, tt, **kw: gen(conds, tt, **{**kw, key: N_TOK, "ban_eos": True})
    voc = engine.vocode

    def vocode(speech_tokens, gen_ref, **kw):
        for s, t in zip(kw.get("seeds") or [], speech_tokens):
            rec.setdefault(s, []).append(t.tolist())
        return voc(speech_tokens, gen_ref, **kw)

    engine.vocode = vocode
    return rec


def _rmse(a, b):
    assert a.shape == b.shape, (a.shape, b.shape)
    return float((a.double() - b.double()).pow(2).mean().sqrt())


def _two_voices(api, synth, turbo=False):
    mk = lambda s: api.Conditionals(api.T3Cond(**(dict(synth.t3_cond(seed=s, prompt_len=375), emotion_adv=None) if turbo else synth.t3_cond(seed=s))),
                                    synth.s3gen_ref(seed=s))
    return mk(11), mk(12)


def _check_compositions(rec, batch_call, single_call, set_max_batch, n=5):
    """The singles once; then the batch as one device batch and as sub-batches of two, and with requests and seeds both reversed: per request the speech tokens
    of the single call, and its waveform within TOL_WAV_E2E_8S."""
    singles, tok_single = [], {}
    for k in range(n):
        rec.clear()
        singles.append(single_call(k))
        (seed, toks), = rec.items()
        assert seed == SEEDS[k]
        tok_single[seed] = toks[-1]
    for max_batch in (None, 2):
        set_max_batch(max_batch)
        for order in (list(range(n)), list(range(n))[::-1]):
            rec.clear()
            batch = batch_call(order)
            assert len(batch) == n and all(w.dim() == 2 and w.shape[0] == 1 and w.dtype == torch.float32 and w.device.type == "cpu" for w in batch)
            assert {s: v[-1] for s, v in rec.items()} == tok_single, f"max_batch={max_batch}, order {order}: speech tokens differ from the single runs"
            for pos, k in enumerate(order):
                err = _rmse(batch[pos], singles[k])
                print(f"max_batch={max_batch} order {order} request {k}: {batch[pos].shape[1]} samples, waveform RMSE batch vs single {err:.3e} (tolerance {TOL_WAV_E2E_8S:.1e})")
                assert err <= TOL_WAV_E2E_8S, f"request {k}: waveform RMSE {err:.3e}"


@pytest.mark.parametrize("cls_name", ["ChatterboxTTS", "ChatterboxMultilingualTTS"])
def test_seeded_generate_batch_equals_seeded_single_generates(dev, cls_name):
    from chatterbox_amd import api, synth
    cls = getattr(api, cls_name)
    m = cls.from_synthetic(dev, t3_layers=2)
    m.tokenizer = _Tok(cls._TEXT_VOCAB)
    rec = _bound_and_record(m.engine, "max_new_tokens")
    va, vb = _two_voices(api, synth)
    conds = [va, vb, va, va, vb]
    langs = ["en", "fr", "de", "en", "es"] if cls_name == "ChatterboxMultilingualTTS" else None

    def single(k):
        m.conds = conds[k]
        return m.generate(TEXTS[k], *([langs[k]] if langs else []), temperature=PER["temperature"][k], top_p=PER["top_p"][k], seed=SEEDS[k])

    def batch(order):
        pick = lambda v: [v[k] for k in order]
        return m.generate_batch(pick(TEXTS), *([pick(langs)] if langs else []), conds=pick(conds), seeds=pick(SEEDS), **{k: pick(v) for k, v in PER.items()})

    _check_compositions(rec, batch, single, lambda mb: setattr(m, "max_batch", mb))


def test_seeded_turbo_generate_batch_equals_seeded_single_generates(dev):
    from chatterbox_amd import api, synth
    m = api.ChatterboxTurboTTS.from_synthetic(dev, t3_layers=2)
    m.tokenizer = _Tok(50000)
    rec = _bound_and_record(m.engine, "max_gen_len")
    va, vb = _two_voices(api, synth, turbo=True)
    conds = [va, vb, va, va, vb]

    def single(k):
        m.conds = conds[k]
        return m.generate(TEXTS[k], temperature=PER["temperature"][k], top_p=PER["top_p"][k], seed=SEEDS[k])

    def batch(order):
        pick = lambda v: [v[k] for k in order]
        return m.generate_batch(pick(TEXTS), conds=pick(conds), seeds=pick(SEEDS), **{k: pick(v) for k, v in PER.items()})

    _check_compositions(rec, batch, single, lambda mb: setattr(m, "max_batch", mb))


def test_seeded_vc_generate_batch_equals_seeded_single_generates(dev):
    from chatterbox_amd import api, synth
    m = api.ChatterboxVC.from_synthetic(dev)
    rec = _bound_and_record(m.engine, None)
    toks = [synth.speech_tokens(n, seed=k) for k, n in enumerate((20, 12, 30, 16, 23))]
    refs = [synth.s3gen_ref(seed=11), synth.s3gen_ref(seed=12)]
    ref_of = [refs[0], refs[1], refs[0], refs[0], refs[1]]

    def single(k):
        m.ref_dict = ref_of[k]
        w = m.generate(s3_tokens=toks[k], seed=SEEDS[k])
        assert w.shape == (1, 960 * toks[k].numel())
        return w

    def batch(order):
        pick = lambda v: [v[k] for k in order]
        return m.generate_batch(s3_tokens=pick(toks), ref_dicts=pick(ref_of), seeds=pick(SEEDS))

    _check_compositions(rec, batch, single, lambda mb: setattr(m, "MAX_BATCH", mb or 8))


# ----------------------------------------------------------------------------- repeatability and isolation
def test_seeded_calls_repeat_leave_torch_rng_alone_and_isolate_requests(dev):
    from chatterbox_amd import api, synth
    m = api.ChatterboxTTS.from_synthetic(dev, t3_layers=2)
    m.tokenizer = _Tok(m._TEXT_VOCAB)
    rec = _bound_and_record(m.engine, "max_new_tokens")
    va, vb = _two_voices(api, synth)
    conds = [va, vb, va, va, vb]
    torch.manual_seed(123)
    state = torch.cuda.get_rng_state(dev)
    a = m.generate_batch(TEXTS, conds=conds, seeds=SEEDS, **PER)
    tok_a = {s: v[-1] for s, v in rec.items()}
    b = m.generate_batch(TEXTS, conds=conds, seeds=SEEDS, **PER)
    s1 = m.generate(TEXTS[0], seed=SEEDS[0])
    s2 = m.generate(TEXTS[0], seed=SEEDS[0])
    pieces = list(m.generate_stream(TEXTS[0], seed=SEEDS[0], first_chunk=4, chunk=4, overlap=False))
    assert torch.equal(torch.cuda.get_rng_state(dev), state), "seeded calls consume no torch RNG"
    for k in range(5):
        assert a[k].shape == b[k].shape and torch.equal(a[k], b[k]), f"request {k}: same seed, other audio"
    assert torch.equal(s1, s2) and sum(p.shape[1] for p in pieces) > 0
    rec.clear()
    other = list(SEEDS)
    other[2] += 1
    c = m.generate_batch(TEXTS, conds=conds, seeds=other, **PER)
    tok_c = {s: v[-1] for s, v in rec.items()}
    assert c[2].shape != a[2].shape or not torch.equal(c[2], a[2]), "another seed must give that request other audio"
    for k in (0, 1, 3, 4):
        assert tok_c[SEEDS[k]] == tok_a[SEEDS[k]], f"request {k}: its tokens must not depend on another request's seed"
    with pytest.raises(ValueError, match="generator"):
        m.generate_batch(TEXTS, conds=conds, seeds=SEEDS, generator=torch.Generator(device=dev))


# ----------------------------------------------------------------------------- streaming
@pytest.mark.parametrize("turbo", [False, True], ids=["llama", "turbo"])
@pytest.mark.parametrize("windowed", [True, False], ids=["window_9", "window_none"])
def test_seeded_stream_equals_the_stream_with_full_fills_injected(dev, turbo, windowed, monkeypatch):
    """synthesize_stream(seeds=, window=W) against the same call with z, phase and noise injected as full-budget fills from the same keys: every piece torch.equal.
    W = 9 tokens is the smallest check_stream_window accepts at fade = 480; 36 tokens in chunks of 6 make the window start at tokens 0, 0, 2, 8, 14, 20
    (stream_window_schedule) when no sampled id is dropped.  The seeded windowed run never fills a budget-sized tensor: every fill is exactly what its round reads."""
    from chatterbox_amd import ops, synth
    from chatterbox_amd.engine import ChatterboxEngine, TurboEngine, check_stream_window, stream_window_schedule
    W = 9 if windowed else None
    if windowed:
        check_stream_window(W, 480)
        with pytest.raises(ValueError):
            check_stream_window(W - 1, 480)
        assert any(a > 0 for a, _ in stream_window_schedule(36, first_chunk=6, chunk=6, lookahead=3, window=W, fade=480))
    P, B, seeds = 10, 2, [31337, 2 ** 50 + 3]
    ref = synth.s3gen_ref(n_prompt_tokens=P)
    s3 = synth.s3gen_state_dict(0, n_mid=1, n_enc=1, n_up_enc=1, **({"meanflow": True} if turbo else {}))
    if turbo:
        eng = TurboEngine(synth.t3_turbo_state_dict(2, 768, 0), s3, dev, n_t3_layers=2)
        tt, cond = [synth.turbo_text_tokens(n, seed=i + 1) for i, n in enumerate((7, 12))], synth.t3_cond(prompt_len=375)
        kw, budget = dict(max_gen_len=35), 36 + 3   # T3 samples max_gen_len + 1 tokens; the final round appends 3 silence tokens
    else:
        eng = ChatterboxEngine(synth.t3_state_dict(2, 0), s3, dev, n_t3_layers=2)
        tt, cond = [synth.text_tokens(n, seed=i + 1) for i, n in enumerate((12, 20))], synth.t3_cond()
        kw, budget = dict(max_new_tokens=36, n_cfm_timesteps=2), 36
    kw.update(first_chunk=6, chunk=6, lookahead=3, fade=480, window=W, ban_eos=True, overlap=False)
    fills = []
    real_fill = ops.rng_fill

    def spy(out, keys, n=None, col0=0, normal=False):
        fills.append((out.shape[0], out.shape[1] if n is None else n, col0, normal))
        return real_fill(out, keys, n=n, col0=col0, normal=normal)

    monkeypatch.setattr(ops, "rng_fill", spy)
    torch.manual_seed(9)
    state = torch.cuda.get_rng_state(dev)
    got = list(eng.synthesize_stream(tt, cond, ref, seeds=seeds, **kw))
    assert torch.equal(torch.cuda.get_rng_state(dev), state), "a seeded stream consumes no torch RNG"
    seeded_fills = list(fills)
    monkeypatch.setattr(ops, "rng_fill", real_fill)
    z, ph, nz = _z(dev, seeds, 2 * (P + budget)), _phase(dev, seeds), _noise(dev, seeds, 960 * budget)
    want = list(eng.synthesize_stream(tt, cond, ref, seeds=seeds, z=z, phase=ph, noise=nz, **kw))
    assert len(got) == len(want) >= 5
    for r, (g, w) in enumerate(zip(got, want)):
        assert g["final"] == w["final"] and g["n_tokens"] == w["n_tokens"]
        for b in range(B):
            assert torch.equal(g["tokens"][b], w["tokens"][b]) and g["wavs"][b].shape == w["wavs"][b].shape and torch.equal(g["wavs"][b], w["wavs"][b]), f"round {r}, utterance {b}"
    normal_fills = {(rows, n, col0) for rows, n, col0, normal in seeded_fills if normal}
    if windowed:
        # What a round READS, restated from what the stream yielded: the window starts at token a = max(0, E // 960 - W), E = the fewest samples handed out so
        # far to an open utterance, and spans Nk = max_b(n_b - a) tokens, n_b = the valid tokens of utterance b in that round.  (Nk is not bounded by
        # W + chunk + lookahead + 1 here: ids >= 6561 are dropped per utterance, so the rows are ragged and the origin follows the shortest.)  The round fills
        # exactly z frames [0, 2P) + [2 (P + a), 2 (P + a + Nk)) and noise samples [960 a, 960 (a + Nk)) -- nothing else, and never the budget.
        expect, emitted, closed = set(), [0] * B, [False] * B
        for g in got:
            live = [emitted[b] for b in range(B) if not closed[b]]
            a = max(0, min(live) // 960 - W)
            Nk = max(n - a for n in g["n_tokens"])
            assert any(2 * (n - a) - (0 if f else 2 * 3) > 0 for n, f in zip(g["n_tokens"], g["final"])), "every round of this stream has frames to vocode"
            expect |= {(B, 80 * 2 * (P + Nk), 0)} if a == 0 else {(B, 80 * 2 * P, 0), (B, 80 * 2 * Nk, 80 * 2 * (P + a))}
            expect.add((9 * B, 960 * Nk, 960 * a))
            emitted = [e + int(w.numel()) for e, w in zip(emitted, g["wavs"])]
            closed = list(g["final"])
        assert normal_fills == expect, "a seeded windowed round fills what it reads, at its own columns"
        assert max(n for rows, n, _ in normal_fills if rows == 9 * B) < 960 * budget and max(n for rows, n, _ in normal_fills if rows == B) < 80 * 2 * (P + budget), \
            "a seeded windowed stream never fills a budget-sized tensor"
        assert any(col0 > 0 for rows, _, col0 in normal_fills if rows == 9 * B), "the window moved: later rounds fill from their own first sample"
    else:
        assert normal_fills == {(B, 80 * 2 * (P + budget), 0), (9 * B, 960 * budget, 0)}, "window=None: the defaults are filled once at today's sizes"
