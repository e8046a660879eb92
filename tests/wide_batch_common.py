"""Bodies of tests/test_wide_batch_decode_gpu.py (they take `dev` first; tests/test_simt_kernels.py runs the small ones on the emulator with a CPU device).

Both T3 engines pick their token step by the row count.  T3TurboEngine (one row per utterance): the few-row kernels up to 2 rows, the packed 5-launch layer up
to 16, the 7-launch form (_forward_decode: add_rmsnorm in its LayerNorm form, packed-weight GEMVs on a row-major x with bias / gelu / split-K) from 17 to
MAX_BATCH = 64, sub-batches beyond.  T3Engine (rows = 2 B): the packed layer up to 16 rows, the 9-launch form above, sub-batches beyond MAX_BATCH = 32.  The bodies
here put every one of these regimes, at both of its ends and at every 16-row tile boundary of the decode GEMV, against the CPU oracle (oracle/ref_torch.py), and
the launches only the wide forms issue against fp64 torch.

Requests are a function of the utterance index b alone (text, voice, row b of one table of uniforms), so an utterance's oracle run and its batch-1 run are
computed once and shared by every batch size that holds it.  Nothing here changes a cached result.
"""
import math

import torch
import torch.nn.functional as F

SENT = -12345.0
LOGIT_TOL = 1e-3   # raw logits against the oracle (the bound of tests/test_models_gpu.py)
TURBO = dict(temperature=0.8, top_k=1000, top_p=0.95, repetition_penalty=1.2)                     # the samplers of tests/test_models_gpu.py
SAMP = dict(temperature=0.8, cfg_weight=0.5, repetition_penalty=1.2, min_p=0.05, top_p=1.0)

TURBO_ROWS = (2, 3, 16, 17, 32, 33, 48, 49, 64)   # each path of T3TurboEngine._forward at both ends + every row-tile boundary of the 7-launch form
LLAMA_B = (9, 17, 24, 25)                          # 18, 34, 48, 50 rows: first above the seam, three tiles, three tiles full, four tiles
# utterances compared with the oracle: their conditional row b or unconditional row B + b sits on a 16-row tile edge (or is the batch's last row)
LLAMA_ORACLE_UTTS = {9: (0, 6, 7),      # rows 0 / 9, 6 / 15, 7 / 16
                     17: (0, 15, 16),   # rows 0 / 17, 15 / 32, 16 / 33
                     24: (8, 15, 23),   # rows 8 / 32, 15 / 39, 23 / 47
                     25: (16, 23, 24)}  # rows 16 / 41, 23 / 48, 24 / 49
GEMV_M = (17, 32, 33, 48, 49, 64)
# (N, K, ksplit, waves): a ragged last column tile everywhere; K blocks per wave 1, 3 (a partly filled last batch at depth 2), 6, 1, 1, 1
GEMV_SHAPES = ((40, 256, 1, 8), (40, 768, 1, 8), (40, 768, 1, 4), (24, 1024, 8, 4), (40, 512, 2, 8), (33, 256, 2, 4))
ADD_NORM_CASES = tuple((rows, ks) for rows in (17, 64) for ks in (2, 8))

_CACHE = {}


def _r(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


def _close(got, ref, tol, what):
    """|got - ref| <= tol * (1 + |ref|) elementwise against an fp64 reference (the rule of tests/test_ops_gpu.py); prints and returns the worst error."""
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    assert torch.isfinite(got).all(), f"{what}: non-finite output"
    err = (got - ref).abs()
    bad = err > tol * (1.0 + ref.abs())
    print(f"{what}: max err {float(err.max()):.3e} (tol {tol:.1e} * (1 + |ref|))")
    assert not bad.any(), f"{what}: max err {err.max():.3e} (ref max {ref.abs().max():.3e}), {int(bad.sum())} / {bad.numel()} over tol {tol}"
    return float(err.max())


class _Window:
    """A (.., rows, cols) tensor inside a buffer full of SENT with one sentinel row above, two below, 4 sentinel columns to the left and 4 .. 7 to the right
    (the leading dimension stays a multiple of 4, and differs from the width): `v` is the strided view handed to the kernel."""

    def __init__(self, t, dev):
        *lead, rows, cols = t.shape
        ld = (cols + 3) // 4 * 4 + 8
        buf = torch.full((*lead, rows + 3, ld), SENT)
        buf[..., 1:1 + rows, 4:4 + cols] = t
        self.buf, self.rows, self.cols = buf.to(dev), rows, cols
        self.v = self.buf[..., 1:1 + rows, 4:4 + cols]
        assert self.v.stride(-2) == ld and ld % 4 == 0 and ld != cols

    def guards_intact(self, what):
        b = self.buf.cpu().clone()
        b[..., 1:1 + self.rows, 4:4 + self.cols] = SENT
        assert bool((b == SENT).all()), f"{what}: {int((b != SENT).sum())} guard elements written"


def _empty(shape, dev):
    return _Window(torch.full(shape, SENT), dev)


# ---------------------------------------------------------------------------------------------------------------- section 3: the launches only the wide forms issue
def check_gemv_wide_rows_packed_weight(dev, M, N, K, ks, nw):
    """cbx_gemv_f32 with w_packed = 1, a row-major strided x, a bias and M > 16 -- what the 7-launch form issues -- against fp64 F.linear.  ks = 1: bias, and
    bias + gelu_new; ks > 1: every partial slice against its own fp64 partial sum (the bias belongs to slice 0 alone) and their sum.  x and out are windows of
    sentinel-filled buffers (ld != width): every guard row and column comes back untouched.  GEMV_PRE_EPI gives the same bits."""
    from chatterbox_amd import ops
    x, w, b = _r((M, K), 1), _r((N, K), 2, 1 / math.sqrt(K)), _r((N,), 3)
    xw, wp, bd = _Window(x, dev), ops.pack_gemv_weight(w.to(dev)), b.to(dev)
    x64, w64, b64 = x.double(), w.double(), b.double()
    tol = 3e-5 * max(1.0, math.sqrt(K / 256))
    what = f"gemv M {M} N {N} K {K} ks {ks} nw {nw}"
    if ks == 1:
        for act, fn, name in ((ops.NONE, lambda t: t, "bias"), (ops.GELU_TANH, lambda t: F.gelu(t, approximate="tanh"), "bias + gelu_new")):
            out, pre = _empty((M, N), dev), _empty((M, N), dev)
            ops.gemv(xw.v, wp, out.v, N=N, bias=bd, nw=nw, act=act, w_packed=True)
            _close(out.v, fn(F.linear(x64, w64, b64)), tol, f"{what}, {name}")
            out.guards_intact(f"{what}, {name}")
            ops.gemv(xw.v, wp, pre.v, N=N, bias=bd, nw=nw, act=act, w_packed=True, flags=ops.gemv_flags(pre_epi=1))
            assert torch.equal(pre.buf, out.buf), f"{what}, {name}: the epilogue-prefetch form differs from the plain one"
    else:
        out, pre = _empty((ks, M, N), dev), _empty((ks, M, N), dev)
        ops.gemv(xw.v, wp, out.v, N=N, bias=bd, ksplit=ks, nw=nw, w_packed=True)
        kd = K // ks
        for j in range(ks):  # slice j contracts k in [j K / ks, (j + 1) K / ks)
            ref = F.linear(x64[:, j * kd:(j + 1) * kd], w64[:, j * kd:(j + 1) * kd], b64 if j == 0 else None)
            _close(out.v[j], ref, 3e-5 * max(1.0, math.sqrt(kd / 256)), f"{what}, slice {j}")
        _close(out.v.sum(0), F.linear(x64, w64, b64), tol, f"{what}, sum of the slices")
        out.guards_intact(what)
        ops.gemv(xw.v, wp, pre.v, N=N, bias=bd, ksplit=ks, nw=nw, w_packed=True, flags=ops.gemv_flags(pre_epi=1))
        assert torch.equal(pre.buf, out.buf), f"{what}: the epilogue-prefetch form differs from the plain one"
    xw.guards_intact(f"{what}: x")


def check_add_norm_layernorm_wide(dev, rows, ks, C=256):
    """ops.add_rmsnorm(..., bias=, rms=False) above 16 rows: x += sum_k part[k]; h = LayerNorm(x) w + b against fp64, at the 2e-5 of
    tests/test_frontend_ops_gpu.py::test_add_norm_layernorm_form (which stops at 16 rows).  x, part and h are windows of sentinel-filled buffers."""
    from chatterbox_amd import ops
    x, part = _r((rows, C), 1, 2.0) + 0.5, _r((ks, rows, C), 2)
    w, b = 1 + 0.1 * _r((C,), 3), 0.1 * _r((C,), 4)
    xw, pw, h = _Window(x, dev), _Window(part, dev), _empty((rows, C), dev)
    ops.add_rmsnorm(xw.v, pw.v, w.to(dev), h.v, 1e-5, bias=b.to(dev), rms=False)
    s = x.double() + part.double().sum(0)
    what = f"add_norm rows {rows} C {C} ks {ks}"
    _close(xw.v, s, 2e-5, f"{what}: residual stream")
    _close(h.v, F.layer_norm(s, (C,), w.double(), b.double(), 1e-5), 2e-5, f"{what}: layernorm")
    for win, name in ((xw, "x"), (pw, "part"), (h, "h")):
        win.guards_intact(f"{what}: {name}")


# ---------------------------------------------------------------------------------------------------------------- section 1: T3TurboEngine
def _turbo_sd(L, d):
    from chatterbox_amd import synth
    key = ("turbo_sd", L, d)
    if key not in _CACHE:
        _CACHE[key] = synth.t3_turbo_state_dict(L, d, 0)
    return _CACHE[key]


def _engine(kind, dev, *shape):
    """One engine per model for the module on the GPU; a CPU device (the emulated library of one pytest module) gets a fresh one."""
    def make():
        if kind == "turbo":
            from chatterbox_amd.t3_turbo import T3TurboEngine
            return T3TurboEngine(_turbo_sd(*shape), dev)
        from chatterbox_amd.t3 import T3Engine
        return T3Engine(_llama_sd(*shape), dev)
    if dev.type != "cuda":
        return make()
    key = (kind, str(dev), *shape)
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _voices(prompt_len):
    from chatterbox_amd import synth
    key = ("voices", prompt_len)
    if key not in _CACHE:  # three voices: the SAME dict serves every utterance of a voice (the engines tell voices apart by identity)
        _CACHE[key] = [synth.t3_cond(seed=2 + v, **({} if prompt_len is None else dict(prompt_len=prompt_len))) for v in range(3)]
    return _CACHE[key]


def turbo_requests(B, n_draws=6):
    """(conds, texts, uniforms (B, n_draws)) of utterances 0 .. B - 1: voice 2 + b % 3 with 24 prompt tokens, 5 + 3 b % 11 text tokens (5 .. 15), seed 1 + b."""
    from chatterbox_amd import synth
    v = _voices(24)
    return [v[b % 3] for b in range(B)], [synth.turbo_text_tokens(5 + (3 * b) % 11, seed=1 + b) for b in range(B)], synth.rand((B, n_draws), seed=11)


def _turbo_oracle(L, d, cond, text, steps, u, b):
    key = ("turbo_oracle", L, d, b, steps, tuple(u.tolist()))
    if key not in _CACHE:
        from oracle import ref_torch as O
        _CACHE[key] = O.t3_inference_turbo(_turbo_sd(L, d), L, d // 64, cond, text, steps, u, ban_eos=True, return_logits=True, **TURBO)
    return _CACHE[key]


def _counted(eng, names):
    """Count the calls of the engine's step forms (instance attributes over the methods; _forward looks them up on the instance)."""
    calls = {n: 0 for n in names}
    for n in names:
        def wrap(st, _n=n, _f=getattr(type(eng), n)):
            calls[_n] += 1
            return _f(eng, st)
        setattr(eng, n, wrap)
    return calls


def _uncounted(eng, names):
    for n in names:
        eng.__dict__.pop(n, None)


_TURBO_FORMS = ("_forward_decode_row", "_forward_decode_v2", "_forward_decode")


def _turbo_form(B):
    return _TURBO_FORMS[0] if B <= 2 else _TURBO_FORMS[1] if B <= 16 else _TURBO_FORMS[2]


def check_turbo_engine_vs_oracle(dev, B, L=1, d=256, steps=5, extra_last_slot_step=False):
    """T3TurboEngine.generate of B utterances (three voices, texts of 5 .. 15 tokens) against oracle runs of every utterance: sampled tokens equal, the raw logits
    of every step within LOGIT_TOL, eagerly (debug_logits) -- and the oracle's tokens again from the captured graph on the GPU.  Which step form ran is asserted.
    extra_last_slot_step: see check_turbo_last_cache_slot.  Returns (worst prefill error, worst decode error)."""
    eng = _engine("turbo", dev, L, d)
    conds, texts, u = turbo_requests(B, steps + 1 + int(extra_last_slot_step))
    want = _turbo_form(B)
    calls = _counted(eng, _TURBO_FORMS)
    try:
        toks, logits = eng.generate(conds, texts, max_gen_len=steps, uniforms=u[:, :steps + 1], ban_eos=True, debug_logits=True, **TURBO)
        st = next(iter(eng._state.values()))
        assert st["B"] == B and eng._row(st) == (B <= 2) and eng._use_c_step(st) == (B <= 16), "the state's own account of its path"
        assert calls == {n: (steps if n == want else 0) for n in _TURBO_FORMS}, f"B = {B} decodes on {want}: {calls}"
        assert logits.shape[:2] == (steps + 1, B)
        logits = logits.cpu()
        worst, bad = [0.0, 0.0], []
        n_or = steps + int(extra_last_slot_step)
        refs = [_turbo_oracle(L, d, conds[b], texts[b], n_or, u[b, :n_or + 1], b) for b in range(B)]
        for b, (rt, rl) in enumerate(refs):
            err = (logits[:, b].double() - rl[:steps + 1].double()).abs().amax(1)
            worst = [max(worst[0], float(err[0])), max(worst[1], float(err[1:].max()))]
            if toks[b].tolist() != rt[:steps + 1].tolist():
                bad.append((b, toks[b].tolist(), rt[:steps + 1].tolist(), [f"{e:.2e}" for e in err.tolist()]))
        msg = f"B = {B} (L {L}, d {d}, {want}): worst |logit - oracle| prefill {worst[0]:.3e}, decode {worst[1]:.3e} (bound {LOGIT_TOL})"
        print(msg)
        assert not bad, f"{msg}; {len(bad)} utterances sample other tokens; (utterance, tokens, oracle tokens, per-step logit error) of the first: {bad[:3]}"
        assert max(worst) <= LOGIT_TOL, msg
        if extra_last_slot_step:
            _turbo_step_into_the_last_slot(eng, st, refs, steps)
        if dev.type == "cuda":  # the product path: the step captured by torch and replayed
            for n in calls:
                calls[n] = 0
            toks_g = eng.generate(conds, texts, max_gen_len=steps, uniforms=u[:, :steps + 1], ban_eos=True, use_graph=True, **TURBO)
            assert [n for n in _TURBO_FORMS if calls[n]] in ([want], []), f"B = {B}: the captured step is {want}: {calls}"   # ([]: the state kept its graph)
            st = next(iter(eng._state.values()))
            assert st["graph"] is not None and ("cstep" not in st or B <= 16)
            for b, (rt, _) in enumerate(refs):
                assert toks_g[b].tolist() == rt[:steps + 1].tolist(), f"graph replay, B = {B}, utterance {b}: {toks_g[b].tolist()} vs oracle {rt.tolist()}"
    finally:
        _uncounted(eng, _TURBO_FORMS)
    return worst


def _turbo_step_into_the_last_slot(eng, st, refs, steps):
    """After a request whose longest utterance ends at S + n_samples = max_ctx, the sampler has left every row ready for one more token step; generate() itself
    never issues it (its last sampled token is not fed back), so the highest position its steps append is max_ctx - 2.  That one further forward -- the longest
    utterance appends at position max_ctx - 1 and attends over all max_ctx slots -- is issued here and compared with step `steps + 1` of an oracle run one token
    longer on the same draws (its first steps + 1 tokens are the request's)."""
    pos = st["positions"].cpu()
    assert int(pos.max()) == st["max_ctx"] - 1 and int(st["ctx_lens"].max()) == st["max_ctx"], (pos.tolist(), st["max_ctx"])
    eng._forward(st)
    got = st["logits"].cpu().double()
    err = max(float((got[b] - rl[steps + 1].double()).abs().max()) for b, (_, rl) in enumerate(refs))
    print(f"the step that appends at position max_ctx - 1 = {st['max_ctx'] - 1}: worst |logit - oracle| {err:.3e} (bound {LOGIT_TOL})")
    assert err <= LOGIT_TOL, f"the step into the last cache slot: worst |logit - oracle| {err:.3e}"


def check_turbo_last_cache_slot(dev):
    """B = 17, max_gen_len = 22, longest text 15 tokens: S + n_samples = 41 + 23 = 64 = max_ctx, the tightest request this cache size serves."""
    conds, texts, _ = turbo_requests(17, 1)
    assert max(int(t.numel()) for t in texts) == 15 and 1 + 24 + 15 + 1 + 22 + 1 == 64
    return check_turbo_engine_vs_oracle(dev, 17, steps=22, extra_last_slot_step=True)


def check_turbo_chunked_decoding(dev, B=17, L=1, d=256, steps=5):
    """generate(async_mode=True, run_steps=1) + advance in chunks of 2 (above 16 rows: the step captured by torch on first use) + collect == the one-shot call."""
    eng = _engine("turbo", dev, L, d)
    conds, texts, u = turbo_requests(B, steps + 1)
    kw = dict(max_gen_len=steps, uniforms=u, ban_eos=True, **TURBO)
    one_shot = eng.generate(conds, texts, **kw)
    h = eng.generate(conds, texts, async_mode=True, run_steps=1, **kw)
    assert h["next_i"] == 1 and not eng._c_loop_serves(h["st"]), "more than 16 rows are not served by the library's token loop"
    ran = []
    while h["next_i"] < h["max_new_tokens"]:
        ran.append(eng.advance(h, 2))
    assert ran == [2, 2, 1] and eng.advance(h, 2) == 0, ran
    if dev.type == "cuda":
        assert h["st"]["graph"] is not None and "cloop" not in h["st"], "advance() replays the torch-captured step"
    got = eng.collect(h)
    assert [t.tolist() for t in got] == [t.tolist() for t in one_shot]
    for b in (0, 16):
        rt, _ = _turbo_oracle(L, d, conds[b], texts[b], steps, u[b], b)
        assert got[b].tolist() == rt.tolist(), f"utterance {b}"


def check_turbo_sub_batches(dev, B=65, L=1, d=256, steps=5):
    """B = MAX_BATCH + 1: 65 results in order; utterances 0, 63 and 64 are the oracle's; the whole result is generate on [0:64] followed by [64:65]."""
    eng = _engine("turbo", dev, L, d)
    assert eng.MAX_BATCH == B - 1
    conds, texts, u = turbo_requests(B, steps + 1)
    kw = dict(max_gen_len=steps, ban_eos=True, **TURBO)
    sizes = []
    orig = type(eng)._get_state
    eng._get_state = lambda Bn, *a: (sizes.append(Bn), orig(eng, Bn, *a))[1]
    try:
        out = eng.generate(conds, texts, uniforms=u, **kw)
    finally:
        del eng._get_state
    assert sizes == [64, 1] and len(out) == B
    parts = eng.generate(conds[:64], texts[:64], uniforms=u[:64], **kw) + eng.generate(conds[64:], texts[64:], uniforms=u[64:], **kw)
    assert [t.tolist() for t in out] == [t.tolist() for t in parts]
    for b in (0, 63, 64):
        rt, _ = _turbo_oracle(L, d, conds[b], texts[b], steps, u[b], b)
        assert out[b].tolist() == rt.tolist(), f"utterance {b}: {out[b].tolist()} vs oracle {rt.tolist()}"


# ---------------------------------------------------------------------------------------------------------------- section 2: T3Engine above 16 rows
LLAMA_L, LLAMA_STEPS, LLAMA_MAX_B = 2, 6, 33


def _llama_sd(L):
    from chatterbox_amd import synth
    key = ("llama_sd", L)
    if key not in _CACHE:
        _CACHE[key] = synth.t3_state_dict(L, 0)
    return _CACHE[key]


def llama_requests(B):
    """(conds, texts, uniforms (B, 6)) of utterances 0 .. B - 1: voice 2 + b % 3, 5 + 3 b % 11 text tokens between SOT and EOT, seed 1 + b; row b of ONE table of
    draws, so utterance b is the same request in every batch."""
    from chatterbox_amd import synth
    assert B <= LLAMA_MAX_B
    v = _voices(None)
    return ([v[b % 3] for b in range(B)], [synth.text_tokens(5 + (3 * b) % 11, seed=1 + b) for b in range(B)],
            synth.rand((LLAMA_MAX_B, LLAMA_STEPS), seed=11)[:B].clone())


def _llama_oracle(b):
    key = ("llama_oracle", b)
    if key not in _CACHE:
        from oracle import ref_torch as O
        conds, texts, u = llama_requests(b + 1)
        _CACHE[key] = O.t3_inference(_llama_sd(LLAMA_L), LLAMA_L, conds[b], torch.stack([texts[b], texts[b]]), LLAMA_STEPS, u[b], ban_eos=True,
                                     return_logits=True, **SAMP)
    return _CACHE[key]


def _llama_alone(eng, b):
    """Utterance b as a batch of one (2 rows: the packed layer through the C step and the library's token loop)."""
    key = ("llama_alone", str(eng.dev), b)
    if key not in _CACHE:
        conds, texts, u = llama_requests(b + 1)
        _CACHE[key] = eng.generate(conds[b], [texts[b]], max_new_tokens=LLAMA_STEPS, uniforms=u[b:b + 1], ban_eos=True, **SAMP)[0].tolist()
    return _CACHE[key]


_LLAMA_FORMS = ("_forward_decode_v2", "_forward_decode")


def check_llama_engine_above_16_rows(dev, B):
    """T3Engine.generate of B utterances (2 B > 16 rows: the 9-launch step, no C step): three utterances on tile edges against the oracle -- tokens, and the raw
    logits of rows b and B + b at every step within LOGIT_TOL (the tokens being the oracle's, every step saw the oracle's inputs) -- and every other utterance
    against its own batch-1 run, token for token (rows never interact; the two forms sum in different orders, so tokens are compared, not logits).  The captured
    graph gives the eager run's tokens.  Returns (worst prefill error, worst decode error)."""
    eng = _engine("llama", dev, LLAMA_L)
    conds, texts, u = llama_requests(B)
    kw = dict(max_new_tokens=LLAMA_STEPS, uniforms=u, ban_eos=True, **SAMP)
    calls = _counted(eng, _LLAMA_FORMS)
    try:
        toks, logits = eng.generate(conds, texts, debug_logits=True, **kw)
        st = next(s for k, s in eng._state.items() if k[0] == B)
        assert st["rows"] == 2 * B > 16 and not eng._use_c_step(st) and "cstep" not in st and "cloop" not in st
        assert calls == dict(_forward_decode_v2=0, _forward_decode=LLAMA_STEPS - 1), calls
        if dev.type == "cuda":
            toks_g = eng.generate(conds, texts, **kw)
            assert [t.tolist() for t in toks_g] == [t.tolist() for t in toks], "the captured 9-launch step gives the eager tokens"
            assert st["graph"] is not None and "cstep" not in st and calls["_forward_decode_v2"] == 0
    finally:
        _uncounted(eng, _LLAMA_FORMS)
    logits = logits.cpu()
    assert logits.shape[:2] == (LLAMA_STEPS, 2 * B)
    worst = [0.0, 0.0]
    for b in LLAMA_ORACLE_UTTS[B]:
        rt, rl = _llama_oracle(b)
        err = (torch.stack([logits[:, b], logits[:, B + b]], 1).double() - rl.double()).abs().amax((1, 2))
        worst = [max(worst[0], float(err[0])), max(worst[1], float(err[1:].max()))]
        assert toks[b].tolist() == rt.tolist(), f"B = {B}, utterance {b}: {toks[b].tolist()} vs oracle {rt.tolist()} (per-step logit error {err.tolist()})"
    msg = f"T3Engine B = {B} ({2 * B} rows): worst |logit - oracle| prefill {worst[0]:.3e}, decode {worst[1]:.3e} (bound {LOGIT_TOL})"
    print(msg)
    assert max(worst) <= LOGIT_TOL, msg
    for b in range(B):
        if b not in LLAMA_ORACLE_UTTS[B]:
            assert toks[b].tolist() == _llama_alone(eng, b), f"B = {B}, utterance {b} differs from its batch-1 run"
    return worst


def check_llama_sub_batches(dev, B=33):
    """B = MAX_BATCH + 1: results in order; utterance 32 (alone in the second sub-batch) equals its batch-1 run, utterances 0 and 31 equal the oracle; every
    other one equals its batch-1 run as well."""
    eng = _engine("llama", dev, LLAMA_L)
    assert eng.MAX_BATCH == B - 1
    conds, texts, u = llama_requests(B)
    sizes = []
    orig = type(eng)._get_state
    eng._get_state = lambda Bn, *a: (sizes.append(Bn), orig(eng, Bn, *a))[1]
    try:
        out = eng.generate(conds, texts, max_new_tokens=LLAMA_STEPS, uniforms=u, ban_eos=True, **SAMP)
    finally:
        del eng._get_state
    assert sizes == [32, 1] and len(out) == B
    for b in (0, 31):
        rt, _ = _llama_oracle(b)
        assert out[b].tolist() == rt.tolist(), f"utterance {b}: {out[b].tolist()} vs oracle {rt.tolist()}"
    for b in range(1, B):
        if b != 31:
            assert out[b].tolist() == _llama_alone(eng, b), f"utterance {b} differs from its batch-1 run"
