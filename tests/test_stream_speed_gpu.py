"""`speed=` on the streaming entry points, on the MI355X (-m gpu): synthesize_stream(speed=) of both engines, ChatterboxEngine.vocode_stream(speed=) and
ChatterboxVC.generate_stream(speed=).  The round shape, N and the engines are those of test_stream_window_gpu.py (read-only import).
  A  speed=1.0 and speed=None are the stream without the argument, piece for piece and bit for bit, with and without a window;
  B  at s in {0.5, 0.8, 1.25, 2.0} an utterance's pieces add up to exactly the length vocode(speed=s) / synthesize(speed=s) returns, both window forms, ragged rows;
  C  the last round of a window=None stream vocodes the very stretched mel the one-shot call vocodes (a spy on hift.inference; torch.equal);
  D  a windowed stream at s = 0.8 and s = 1.25 == the rate-aware restatement on the CPU oracle (stream_speed_common.oracle_window_stream), under the conditions of
     test_stream_window_gpu._against_oracle: piece lengths equal, waveform RMSE <= 2e-3 (the project's bound for chunked synthesis), seams no
     rougher than twice the one-shot waveform's largest step + 1e-3;
  E  exactly one cbx_mel_time_scale_win_f32 launch per round at a rate and none without; no flow call sees more than W + chunk + lookahead + 1 tokens;
  F  ChatterboxVC.generate_stream(speed=1.25, window=20) on 130 tokens;
  G  with seed= and speed= every round of a windowed stream draws the source noise of ITS stretched samples: the columns [480 j0, ...) of one ops.seeded_noise fill
     from column 0, which is what the one-shot request at that seed and speed reads.
The kernel-level tests are in test_turbo_stream_speed_window_kernels_gpu.py; the host arithmetic is tested in test_stream_speed_host.py."""
import math
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import mel_speed_common as S  # noqa: E402
import stream_speed_common as C  # noqa: E402
import test_stream_window_gpu as WG  # noqa: E402  (read-only import: _llama / _turbo, SHAPE, N, _against_oracle)

pytestmark = pytest.mark.gpu
SHAPE, N, SIL = WG.SHAPE, WG.N, WG.SIL
W = 12                                   # the smallest legal window at s = 1.25 and fade 240 (engine.check_stream_window); legal at 0.8 too
WIN = {0.5: 12, 0.8: 12, 1.25: 12, 2.0: 19}
# rounds of 6, 10, 14, 18, 22, 26 tokens; at window 12 and BOTH rates of check D the window starts at token 0, 0, 0, 0, 4, 8: it slides in the last two rounds
ORIGINS = [0, 0, 0, 0, 4, 8]
_CACHE = {}


def _engine(dev, backbone):
    if backbone not in _CACHE:
        _CACHE[backbone] = (WG._llama if backbone == "llama" else WG._turbo)(dev)
    return _CACHE[backbone]


def _at(kw, B, n_tok, s, seed=6):
    """the keyword set with a source noise of the STRETCHED length, 480 * out_len(2 n_tok, s)"""
    from chatterbox_amd import synth
    return dict(kw, noise=synth.randn((B, 9, 480 * S.out_len(2 * n_tok, s)), seed=seed))


def _vc_setup(dev):
    if "vc" not in _CACHE:
        from chatterbox_amd import synth
        from chatterbox_amd.api import ChatterboxVC
        s3_sd = synth.s3gen_state_dict(0, n_mid=2, n_enc=1, n_up_enc=1)
        eng = ChatterboxVC._engine(s3_sd, dev)
        P, lens = 8, [N, 19]
        ref = synth.s3gen_ref(n_prompt_tokens=P)
        toks = [synth.speech_tokens(n, seed=3 + b) for b, n in enumerate(lens)]
        z = synth.randn((2, 80, 2 * (P + N)), seed=5)
        phase = (synth.rand((2, 9, 1), seed=6) * 2 - 1) * math.pi
        phase[:, 0] = 0
        kw = dict(z=z.transpose(1, 2).contiguous(), phase=phase, noise=synth.randn((2, 9, 960 * N), seed=6), n_cfm_timesteps=3)
        _CACHE["vc"] = (eng, s3_sd, toks, lens, ref, z, phase, kw)
    return _CACHE["vc"]


def _same_stream(tag, got, want):
    assert len(got) == len(want), tag
    for r, (a, b) in enumerate(zip(want, got)):
        assert a["final"] == b["final"] and a["n_tokens"] == b["n_tokens"], (tag, r)
        for x, y in zip(a["wavs"], b["wavs"]):
            assert x.shape == y.shape and torch.equal(x, y), f"{tag} round {r}: max |diff| {(x - y).abs().max().item():.3e}"


class _LibSpy:
    """every call into the library goes through ops.lib: the names, in order"""
    def __init__(self, real):
        self.real, self.calls = real, []

    def __getattr__(self, name):
        self.calls.append(name)
        return getattr(self.real, name)


# ----------------------------------------------------------------------------------------------------------------- A
@pytest.mark.parametrize("window", [None, 9], ids=["no_window", "window_9"])
@pytest.mark.parametrize("backbone", ["llama", "gpt2"])
def test_speed_one_and_none_are_the_stream_without_the_argument(dev, backbone, window, monkeypatch):
    """A for synthesize_stream: the same pieces and (serial form: one host thread) the same library calls in the same order; the same pieces overlapped."""
    from chatterbox_amd import ops
    eng, _, texts, cond, ref, _, _, _, kw = _engine(dev, backbone)
    spy = _LibSpy(ops.lib)
    monkeypatch.setattr(ops, "lib", spy)
    list(eng.synthesize_stream(texts, cond, ref, overlap=False, window=window, **SHAPE, **kw))   # (whatever a first run of this engine sets up is set up now)
    spy.calls.clear()
    base = list(eng.synthesize_stream(texts, cond, ref, overlap=False, window=window, **SHAPE, **kw))
    base_calls = list(spy.calls)
    assert len(base) == 6 and "cbx_mel_time_scale_win_f32" not in base_calls
    for speed in (1.0, None):
        spy.calls.clear()
        _same_stream(f"{backbone} window={window} speed={speed!r}", list(eng.synthesize_stream(texts, cond, ref, overlap=False, window=window, speed=speed, **SHAPE, **kw)), base)
        assert spy.calls == base_calls, "speed=1.0 / None: launch for launch the stream without it"
    _same_stream(f"{backbone} window={window} overlapped", list(eng.synthesize_stream(texts, cond, ref, window=window, speed=1.0, **SHAPE, **kw)),
                 list(eng.synthesize_stream(texts, cond, ref, window=window, **SHAPE, **kw)))


@pytest.mark.parametrize("window", [None, 9], ids=["no_window", "window_9"])
def test_vocode_stream_speed_one_and_none_are_the_stream_without_the_argument(dev, window):
    eng, _, toks, _, ref, _, _, kw = _vc_setup(dev)
    base = list(eng.vocode_stream(toks, ref, window=window, **SHAPE, **kw))
    for speed in (1.0, None, 1):
        _same_stream(f"vocode_stream window={window} speed={speed!r}", list(eng.vocode_stream(toks, ref, window=window, speed=speed, **SHAPE, **kw)), base)


# ----------------------------------------------------------------------------------------------------------------- B, C
def _spy_hift(eng, seen):
    hift = eng.hift.inference
    eng.hift.inference = lambda mel, *a, **k: (seen.append((mel, k.get("lens"), k.get("noise"))), hift(mel, *a, **k))[1]
    return hift


@pytest.mark.parametrize("s", [0.5, 0.8, 1.25, 2.0])
def test_pieces_add_up_to_the_one_shot_length_and_the_last_round_vocodes_its_mel(dev, s):
    """B + C for vocode_stream over ragged rows (26 and 19 tokens) and for the Llama synthesize_stream (the last token dropped)."""
    from chatterbox_amd import engine as E
    eng, _, toks, lens, ref, _, _, kw = _vc_setup(dev)
    kw = _at(kw, 2, N, s)
    trips, seen = E.RANGE_TRIPS, []
    hift = _spy_hift(eng, seen)
    try:
        full, _ = eng.vocode(toks, ref, speed=s, **kw)
        one_shot_mel = seen[-1][0]
        assert [w.numel() for w in full] == [480 * S.out_len(2 * n, s) for n in lens]
        for window in (None, WIN[s]):
            seen.clear()
            rounds = list(eng.vocode_stream(toks, ref, window=window, speed=s, **SHAPE, **kw))
            got = [sum(r["wavs"][b].numel() for r in rounds) for b in range(2)]
            print(f"[stream-speed] vocode_stream s={s} window={window}: pieces {[[r['wavs'][b].numel() for r in rounds] for b in range(2)]}")
            assert got == [w.numel() for w in full], f"s={s} window={window}: {got} samples streamed, {[w.numel() for w in full]} in one shot"
            assert rounds[-1]["final"] == [True, True] and all(torch.isfinite(w).all() for r in rounds for w in r["wavs"])
            if window is None and E.RANGE_TRIPS == trips:
                assert len(seen) == len(rounds) and seen[-1][0].shape == one_shot_mel.shape and torch.equal(seen[-1][0], one_shot_mel), "C: the last round's vocoder input"
    finally:
        eng.hift.inference = hift
    eng, _, texts, cond, ref, _, _, _, kw = _engine(dev, "llama")
    kw = _at(kw, 2, N, s)
    seen = []
    hift = _spy_hift(eng, seen)
    try:
        full, _ = eng.synthesize(texts, cond, ref, drop_last_token=True, speed=s, **kw)
        one_shot_mel = seen[-1][0]
        assert [w.numel() for w in full] == [480 * S.out_len(2 * (N - 1), s)] * 2
        for window in (None, WIN[s]):
            seen.clear()
            rounds = list(eng.synthesize_stream(texts, cond, ref, window=window, speed=s, overlap=window is None, **SHAPE, **kw))
            got = [sum(r["wavs"][b].numel() for r in rounds) for b in range(2)]
            assert got == [w.numel() for w in full], f"llama s={s} window={window}: {got} samples streamed, {[w.numel() for w in full]} in one shot"
            if window is None and E.RANGE_TRIPS == trips:
                assert torch.equal(seen[-1][0], one_shot_mel), "C: the last round's vocoder input"
    finally:
        eng.hift.inference = hift


# ----------------------------------------------------------------------------------------------------------------- D
def test_the_shape_of_check_d_slides_its_window_at_both_rates():
    """Host arithmetic: the schedule check D relies on, literally (and the restated rules give the same origins)."""
    from chatterbox_amd.engine import stream_speed_schedule
    for s, j0s in ((0.8, [0, 0, 0, 0, 11, 21]), (1.25, [0, 0, 0, 0, 7, 13])):
        for drop in (False, True):
            sch = stream_speed_schedule(N, s, window=W, drop_last_token=drop, **SHAPE)
            assert [a for a, _, _, _ in sch] == ORIGINS and [n for _, n, _, _ in sch] == [6, 10, 14, 18, 22, 26] and [j for _, _, j, _ in sch] == j0s
            assert [C.window_origin(e, W, s) for _, _, _, e in sch[:-1]] == ORIGINS[1:] and [C.origin_frame(2 * a, s) for a in ORIGINS] == j0s


@pytest.mark.parametrize("s", [0.8, 1.25])
@pytest.mark.parametrize("backbone", ["llama", "gpt2"])
def test_windowed_stream_at_a_rate_matches_the_oracle_schedule(dev, backbone, s):
    """D for synthesize_stream: six rounds, the window slides in the last two (a = 4, 8).  Measured on the MI355X: RMSE 5.1e-5 .. 1.7e-4 over the eight utterance
    cases (bound 2e-3), the largest seam step at most 1.73x the one-shot waveform's (bound 2x + 1e-3)."""
    from oracle import ref_torch as O
    llama = backbone == "llama"
    eng, s3_sd, texts, cond, ref, z, phase, _, kw = _engine(dev, backbone)
    n_tok = N if llama else N + 3
    kw = _at(kw, 2, n_tok, s)
    rounds = list(eng.synthesize_stream(texts, cond, ref, window=W, speed=s, **SHAPE, **kw))
    assert len(rounds) == 6 and rounds[-1]["final"] == [True, True] and not any(any(r["final"]) for r in rounds[:-1])
    full, toks = eng.synthesize(texts, cond, ref, speed=s, **({"drop_last_token": True} if llama else {}), **kw)
    for b in range(2):
        assert rounds[-1]["tokens"][b].tolist() == toks[b].tolist()
        sampled = toks[b] if llama else toks[b][:-3]
        assert sampled.numel() == N
        want = C.oracle_window_stream(O, s3_sd, sampled, ref, z[b:b + 1], phase[b:b + 1], kw["noise"][b:b + 1], window=W, n_steps=3 if llama else 2, rate=s,
                                      meanflow=not llama, sil=None if llama else torch.full((3,), SIL, dtype=torch.long), drop_last=llama,
                                      **{("first" if k == "first_chunk" else k): v for k, v in SHAPE.items()})
        WG._against_oracle(f"{backbone} s={s} utt {b}", [r["wavs"][b] for r in rounds], full[b].cpu(), want)


def test_windowed_vocode_stream_at_a_rate_matches_the_oracle_schedule_for_ragged_lengths(dev):
    """D for vocode_stream at s = 0.8: 26 and 19 tokens; the short utterance is final one round before the long one and only rides along in the last."""
    from oracle import ref_torch as O
    s = 0.8
    eng, s3_sd, toks, lens, ref, z, phase, kw = _vc_setup(dev)
    kw = _at(kw, 2, N, s)
    rounds = list(eng.vocode_stream(toks, ref, window=W, speed=s, **SHAPE, **kw))
    assert [r["final"] for r in rounds] == [[False, False]] * 4 + [[False, True], [True, True]] and rounds[-1]["n_tokens"] == lens
    full, _ = eng.vocode(toks, ref, speed=s, **kw)
    for b, n in enumerate(lens):
        want = C.oracle_window_stream(O, s3_sd, toks[b], ref, z[b:b + 1], phase[b:b + 1], kw["noise"][b:b + 1], window=W, n_steps=3, rate=s, drop_last=False,
                                      **{("first" if k == "first_chunk" else k): v for k, v in SHAPE.items()})
        assert full[b].numel() == 480 * S.out_len(2 * n, s)
        WG._against_oracle(f"vocode_stream s={s} utt {b}", [r["wavs"][b] for r in rounds], full[b].cpu(), want)


# ----------------------------------------------------------------------------------------------------------------- E
@pytest.mark.parametrize("s", [0.8, 1.25])
def test_one_window_launch_per_round_and_a_bounded_number_of_tokens(dev, s, monkeypatch):
    from chatterbox_amd import engine as E, ops
    eng, _, texts, cond, ref, _, _, _, kw = _engine(dev, "llama")
    trips, flows, flow = E.RANGE_TRIPS, [], eng.flow.inference
    eng.flow.inference = lambda tok, *a, **k: (flows.append(int(tok.shape[1])), flow(tok, *a, **k))[1]
    spy = _LibSpy(ops.lib)
    monkeypatch.setattr(ops, "lib", spy)
    try:
        for window in (W, None):
            flows.clear()
            spy.calls.clear()
            rounds = list(eng.synthesize_stream(texts, cond, ref, window=window, speed=s, overlap=False, **SHAPE, **_at(kw, 2, N, s)))
            assert E.RANGE_TRIPS == trips, "a round was repeated at bf16x6: the counts below assume one pass per round"
            assert len(rounds) == 6 and spy.calls.count("cbx_mel_time_scale_win_f32") == 6 and "cbx_mel_time_scale_f32" not in spy.calls
            print(f"[stream-speed] s={s} window={window}: tokens per round {flows}")
            if window is not None:
                assert flows == [n - a for a, n in zip(ORIGINS, (6, 10, 14, 18, 22, 26))] and max(flows) <= W + SHAPE["chunk"] + SHAPE["lookahead"] + 1
        spy.calls.clear()
        list(eng.synthesize_stream(texts, cond, ref, window=W, overlap=False, **SHAPE, **kw))
        assert "cbx_mel_time_scale_win_f32" not in spy.calls and "cbx_mel_time_scale_f32" not in spy.calls
    finally:
        eng.flow.inference = flow


# ----------------------------------------------------------------------------------------------------------------- F
def test_vc_generate_stream_at_a_rate(dev):
    from chatterbox_amd import synth
    from chatterbox_amd.api import ChatterboxVC
    from chatterbox_amd.engine import stream_speed_schedule
    vc = ChatterboxVC.from_synthetic(dev, tokenizer_layers=1)
    vc.watermarker = None
    ref, src = vc.ref_dict, synth.speech_tokens(130, seed=2)
    torch.manual_seed(3)
    whole = vc.generate(s3_tokens=src, speed=1.25)
    assert whole.shape == (1, 480 * S.out_len(260, 1.25))
    flows, flow = [], vc.engine.flow.inference
    vc.engine.flow.inference = lambda tok, *a, **k: (flows.append(int(tok.shape[1])), flow(tok, *a, **k))[1]
    torch.manual_seed(3)
    gen = vc.generate_stream(s3_tokens=src, first_chunk=10, chunk=25, window=20, speed=1.25)
    assert flows == [], "nothing is synthesised before the first next()"
    first = next(gen)
    assert set(flows) == {13}, "the first piece arrives after one round of first_chunk + lookahead tokens"
    pieces = [first] + list(gen)
    sched = stream_speed_schedule(130, 1.25, first_chunk=10, chunk=25, window=20)
    print(f"[stream-speed] VC.generate_stream(speed=1.25): pieces {[p.shape[1] for p in pieces]}, tokens per round {flows}")
    assert all(p.dim() == 2 and p.shape[0] == 1 and p.dtype == torch.float32 and p.device.type == "cpu" and torch.isfinite(p).all() for p in pieces)
    assert [p.shape[1] for p in pieces] == [e1 - e0 for (_, _, _, e0), (_, _, _, e1) in zip([(0, 0, 0, 0)] + sched, sched)]
    assert sum(p.shape[1] for p in pieces) == whole.shape[1] and len(pieces) == len(sched)
    assert sorted(set(flows)) == sorted({n - a for a, n, _, _ in sched}) and max(flows) <= 20 + 25 + 3 + 1 and max(flows) < 130
    assert vc.ref_dict is ref and float(torch.cat(pieces, 1).abs().max()) <= 0.99


# ----------------------------------------------------------------------------------------------------------------- G
def test_seeded_stream_at_a_rate_draws_the_noise_of_its_stretched_samples(dev):
    from chatterbox_amd import ops
    from chatterbox_amd.engine import stream_speed_schedule
    s, seeds = 1.25, [11, 2 ** 40]
    eng, _, toks, lens, ref, _, _, kw = _vc_setup(dev)
    seen = []
    hift = _spy_hift(eng, seen)
    try:
        rounds = list(eng.vocode_stream(toks, ref, window=W, speed=s, seeds=seeds, n_cfm_timesteps=3, **SHAPE))
    finally:
        eng.hift.inference = hift
    sch = stream_speed_schedule(N, s, window=W, **SHAPE)
    whole = ops.seeded_noise(seeds, 480 * S.out_len(2 * N, s), dev)
    assert len(seen) == len(rounds) == len(sch) and [j0 for _, _, j0, _ in sch][-2:] == [7, 13]
    for r, ((mel, lens_r, noise), (_, _, j0, _)) in enumerate(zip(seen, sch)):
        n = 480 * mel.shape[1]
        assert noise.shape == (2, 9, n) and torch.equal(noise, whole[:, :, 480 * j0: 480 * j0 + n]), f"round {r}: the noise of stretched samples [{480 * j0}, {480 * j0 + n})"
    assert sum(r["wavs"][0].numel() for r in rounds) == 480 * S.out_len(2 * N, s)
