"""GPU (-m gpu): guard= through T3Engine.generate, the engine and the public API on a synthetic 2-layer model (from_synthetic), B = 1, 3 and 9, 24 steps, explicit heads
on layers 0 and 1.  B = 9 is 18 rows: the step of more than 16 rows (T3Engine._forward_decode, plain q/k/v rows) with its own hook, where B <= 8 takes the
packed 5-launch layer (_forward_decode_v2, q as split-K parts); the requests have different text lengths, so every row decodes at its own position.

With every rule off the hooks only read: the tokens are the unguarded call's bit for bit, eagerly and under the captured graph.  The mass history against the
independent fp64 forward test_word_times_api_gpu.py uses for the alignment pass (K / V recomputed at every position, nothing read from the cache), within
MASS_TOL = 2e-5 (1 + |ref|); the test prints the worst figure.  Trace, state and reasons are the NumPy state machine replayed over the device's own history and
tokens, exactly.  A rule that fires stops ONE row of three and leaves the others' tokens untouched.  The public generate returns shorter audio and says why.
The kernel-level tests are in test_turbo_stream_guard_kernels_gpu.py."""
import os
import sys
import warnings

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import guard_common as G  # noqa: E402
from test_seeded_api_gpu import SEEDS, TEXTS, _Tok  # noqa: E402  (read-only import: the stand-in tokenizer, the requests)
from test_word_times_api_gpu import _restated_mass  # noqa: E402  (read-only import: the independent fp64 forward of one request)

pytestmark = pytest.mark.gpu

HEADS = ((0, 3), (1, 5), (1, 9))
N_TOK = 24
SAMP = dict(temperature=0.8, cfg_weight=0.5, repetition_penalty=1.2, min_p=0.05, top_p=1.0)
INF = float("inf")
_MODEL = {}


def _model(dev):
    """One synthetic ChatterboxTTS for the module: token budget N_TOK, EOS NOT banned (the guard must be able to force it)"""
    if "m" not in _MODEL:
        from chatterbox_amd import api
        m = api.ChatterboxTTS.from_synthetic(dev, t3_layers=2)
        m.tokenizer, m.watermarker, m.align_heads = _Tok(api.ChatterboxTTS._TEXT_VOCAB), None, HEADS
        syn, pip = m.engine.synthesize, m.engine.synthesize_pipelined
        m.engine.synthesize = lambda *a, **kw: syn(*a, **{**kw, "max_new_tokens": N_TOK})
        m.engine.synthesize_pipelined = lambda jobs, **kw: pip(jobs, **{**kw, "max_new_tokens": N_TOK})
        _MODEL["m"] = m
    return _MODEL["m"]


def _requests(m, B):
    texts = (TEXTS[0], TEXTS[3], TEXTS[4], TEXTS[1], TEXTS[2], TEXTS[3] + " Five.", "Hello.", TEXTS[0] + " And more.", TEXTS[4])
    return [m._engine_tokens(m._text_ids(t)) for t in texts[:B]]


def _uniforms(B):
    return torch.rand(B, N_TOK, generator=torch.Generator().manual_seed(7 + B))


@pytest.mark.parametrize("B", [1, 3, 9])
def test_with_every_rule_off_the_tokens_are_the_unguarded_ones_and_the_history_is_the_independent_forward(dev, B):
    """Measured on one MI355X: worst err / (1 + |ref|) = 9.67e-8 (B = 1), 8.90e-8 (B = 3) and 1.24e-7 (B = 9, the step of more than 16 rows) against the bound 2e-5 -- the decode path needed no wider
    constant than the alignment pass."""
    m = _model(dev)
    t3, reqs, u, conds = m.engine.t3, _requests(m, B), _uniforms(B), m.conds.t3.as_dict()
    off = dict(G.OFF, heads=HEADS)
    with torch.cuda.device(dev):
        plain = t3.generate(conds, reqs, max_new_tokens=N_TOK, uniforms=u, **SAMP)
        eager = t3.generate(conds, reqs, max_new_tokens=N_TOK, uniforms=u, use_graph=False, guard=off, **SAMP)
        st = next(s for k, s in t3._state.items() if k[0] == B and k[3] == 0)
        assert (t3.decode_mode == "v2" and st["rows"] <= 16) == (B <= 8), "B = 9 runs the hook of the step for more than 16 rows"
        graph = t3.generate(conds, reqs, max_new_tokens=N_TOK, uniforms=u, guard=off, **SAMP)
        d, rep = t3.last_guard_device, t3.last_guard
        mass, trace, state, sums = (d[k].cpu().numpy() for k in ("mass", "trace", "state", "sums"))
        for a, b, c in zip(plain, eager, graph):
            assert torch.equal(a, b) and torch.equal(a, c), "the hooks only read: same tokens eagerly and under the captured graph"
        worst = 0.0
        thr = G.thr_row(**G.OFF)
        for b in range(B):
            n, tl = int(graph[b].numel()), int(reqs[b].numel())
            ref = _restated_mass(m, reqs[b], graph[b], HEADS)
            got = mass[b, 1:n, :tl].astype(np.float64)
            assert np.isfinite(got).all() and 0.0 < got.sum(1).min() and got.sum(1).max() <= 1.0 + 1e-5
            worst = max(worst, float((np.abs(got - ref[1:n]) / (1.0 + np.abs(ref[1:n]))).max()))
            tr, s, f = G.replay(mass[b], graph[b].tolist(), tl, thr, N_TOK)
            assert trace[b].tolist() == tr and state[b].tolist() == s.tolist() and np.array_equal(sums[b], f), "the device followed the state machine on its own history"
            assert rep[b]["reason"] == ("eos" if int(graph[b][-1]) == G.EOS else "length") and rep[b]["tokens"] == n and rep[b]["position"] == int(s[0])
    print(f"guard mass history against the independent fp64 forward, B = {B}: worst err / (1 + |ref|) = {worst:.3g} (bound {G.MASS_TOL})")
    assert worst <= G.MASS_TOL, worst


def test_the_default_rules_follow_the_state_machine_and_hold_eos(dev):
    m = _model(dev)
    t3, reqs, u, conds = m.engine.t3, _requests(m, 3), _uniforms(3), m.conds.t3.as_dict()
    guard = dict(heads=HEADS, tail=0.4, repeat=0.3, token_run=2)   # thresholds low enough to matter within 24 steps of a random-init model
    with torch.cuda.device(dev):
        toks = t3.generate(conds, reqs, max_new_tokens=N_TOK, uniforms=u, guard=guard, **SAMP)
        h = t3.generate(conds, reqs, max_new_tokens=N_TOK, uniforms=u, guard=guard, async_mode=True, **SAMP)
        again = t3.collect(h)
        d, rep = t3.last_guard_device, t3.last_guard
        mass, trace, state = (d[k].cpu().numpy() for k in ("mass", "trace", "state"))
    assert all(torch.equal(a, b) for a, b in zip(toks, again)), "async_mode + collect gives the one-shot call's tokens"
    thr = G.thr_row(**{k: v for k, v in guard.items() if k != "heads"})
    for b in range(3):
        tl, tk = int(reqs[b].numel()), toks[b].tolist()
        tr, s, _ = G.replay(mass[b], tk, tl, thr, N_TOK)
        assert trace[b].tolist() == tr and state[b].tolist() == s.tolist()
        held = [i for i in range(1, len(tk)) if tr[i] >> 17 & 1]
        assert all(tk[i] != G.EOS for i in held), "EOS is not sampled at a step that ran under the ban"
        fired = int(s[3])
        assert rep[b]["reason"] == (("eos", "tail", "repeat", "run")[fired] if fired or tk[-1] == G.EOS else "length")
        if fired:
            assert tk[-1] == G.EOS and len(tk) == int(s[4]) + 1
    print("reports:", rep)
    with pytest.raises(ValueError, match="advance"):
        t3.advance(h, 1)


def test_a_rule_that_fires_stops_one_row_of_three(dev):
    """end_tokens = 3, tail = 0 on a text of 3 tokens: complete at once, so `tail` holds at step 1 for that row alone"""
    m = _model(dev)
    t3, conds, u = m.engine.t3, m.conds.t3.as_dict(), _uniforms(3)
    long = _requests(m, 3)
    reqs = [long[1], torch.tensor([255, 300, 0], dtype=long[0].dtype), long[2]]
    guard = dict(heads=HEADS, end_tokens=3, tail=0.0, repeat=INF, token_run=0, hold_eos=False, ahead=0, back=0)   # (ahead = back = 0: the long rows never complete)
    with torch.cuda.device(dev):
        plain = t3.generate(conds, reqs, max_new_tokens=N_TOK, uniforms=u, **SAMP)
        toks = t3.generate(conds, reqs, max_new_tokens=N_TOK, uniforms=u, guard=guard, **SAMP)
        rep = t3.last_guard
    assert toks[1].tolist() == [int(plain[1][0]), G.EOS] and rep[1]["reason"] == "tail" and rep[1]["fired_at"] == 1 and rep[1]["tokens"] == 2
    assert torch.equal(toks[0], plain[0]) and torch.equal(toks[2], plain[2]), "the other rows' tokens are bit for bit their unguarded ones"
    assert rep[0]["fired_at"] is None and rep[2]["fired_at"] is None


def test_guarded_and_unguarded_requests_alternate_on_one_state(dev):
    m = _model(dev)
    t3, reqs, u, conds = m.engine.t3, _requests(m, 3), _uniforms(3), m.conds.t3.as_dict()
    guard = dict(heads=HEADS, tail=0.4, repeat=0.3, token_run=2)
    other = dict(guard, heads=((1, 2),))
    with torch.cuda.device(dev):
        p0 = t3.generate(conds, reqs, max_new_tokens=N_TOK, uniforms=u, **SAMP)
        g0 = t3.generate(conds, reqs, max_new_tokens=N_TOK, uniforms=u, guard=guard, **SAMP)
        r0 = t3.last_guard
        p1 = t3.generate(conds, reqs, max_new_tokens=N_TOK, uniforms=u, **SAMP)
        o0 = t3.generate(conds, reqs, max_new_tokens=N_TOK, uniforms=u, guard=other, **SAMP)
        g1 = t3.generate(conds, reqs, max_new_tokens=N_TOK, uniforms=u, guard=guard, **SAMP)
        st = next(s for k, s in t3._state.items() if k[0] == 3 and k[3] == 0)
        assert all(torch.equal(a, b) for a, b in zip(p0, p1)) and all(torch.equal(a, b) for a, b in zip(g0, g1)) and t3.last_guard == r0
        assert len(o0) == 3 and set(st["guard_graphs"]) == {HEADS, ((1, 2),)}, "one captured graph per set of heads, each replayed by its own requests"
        assert st["graph"] is None and "cloop" in st, "the unguarded requests stayed on the library's token loop"


def test_the_public_calls_report_and_a_fired_request_is_shorter(dev):
    m = _model(dev)
    fire = dict(end_tokens=3, tail=0.0, repeat=INF, token_run=0, hold_eos=False)   # `tail` holds as soon as the position reaches the last 3 text tokens
    with torch.cuda.device(dev):
        plain = m.generate(TEXTS[2], seed=SEEDS[2])
        assert torch.equal(plain, m.generate(TEXTS[2], seed=SEEDS[2], guard=None)) and m.last_guard is None
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            cut = m.generate(TEXTS[2], seed=SEEDS[2], guard=fire)
        r = m.last_guard[0]
        print("generate:", r)
        assert r["reason"] == "tail" and r["tokens"] == r["fired_at"] + 1 < N_TOK and cut.shape[-1] < plain.shape[-1], "shorter audio, and last_guard says why"
        assert len(w) == 1 and "'tail'" in str(w[0].message)
        texts = [TEXTS[3], TEXTS[2], TEXTS[0], TEXTS[4]]
        m.max_batch = 2
        try:
            with warnings.catch_warnings(record=True):
                warnings.simplefilter("always")
                out = m.generate_batch(texts, seeds=[SEEDS[3], SEEDS[2], SEEDS[0], SEEDS[4]], guard=fire)   # two sub-batches: both slots of the throughput schedule
                reps = m.last_guard
                alone = []
                for t, s in zip(texts, (SEEDS[3], SEEDS[2], SEEDS[0], SEEDS[4])):
                    m.generate(t, seed=s, guard=fire)
                    alone.append(m.last_guard[0])
        finally:
            m.max_batch = None
        assert [r["text_tokens"] for r in reps] == [int(m._engine_tokens(m._text_ids(t)).numel()) for t in texts], "the reports come back in the caller's order"
        assert [r["text_tokens"] for r in alone] == [r["text_tokens"] for r in reps] and len(out) == 4
        wav, segs = m.generate_long("Hello there. Numbers one two three four. Hi.", max_chars=30, seed=5, return_segments=True, guard=dict(G.OFF))
        assert len(segs) >= 2 and [s["guard"] for s in segs] == m.last_guard and all(s["guard"]["reason"] in ("eos", "length") for s in segs)
        plain_long = m.generate_long("Hello there. Numbers one two three four. Hi.", max_chars=30, seed=5)
        assert torch.equal(wav, plain_long), "with every rule off the long form is the unguarded one"
    with pytest.raises(TypeError, match="guard"):
        m.generate_stream(TEXTS[2], guard=True)
    with pytest.raises(ValueError, match="layer 9"):
        m.generate(TEXTS[2], guard=dict(heads=None))
