"""Bounded-cost ("windowed") streaming on the MI355X (-m gpu): synthesize_stream(window=) of both engines, ChatterboxEngine.vocode_stream and
ChatterboxVC.generate_stream.
  A  a window wider than the utterance adds no arithmetic: every yielded sample is the window=None stream's, bit for bit;
  B  a stream whose window slides == the same schedule restated on the CPU oracle (stream_window_common.oracle_window_stream: O.flow_inference on the
     window, O.source_module with the carry as a phase, O.hift_decode), within the project's bound for chunked synthesis (waveform RMSE <= 2e-3, DESIGN.md
     section 1), piece for piece, and its seams are no rougher than twice the one-shot waveform's largest step (+ 1e-3);
  C  the cost of a round is bounded: no flow / vocoder call of a windowed stream sees more than W + chunk + lookahead + 1 tokens, and once the window slides
     every round sees the same number;
  D  ChatterboxVC.generate_stream: pieces of the length generate returns, the first after one round, one watermarker call per piece, ref_dict untouched."""
import math
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

pytestmark = pytest.mark.gpu
SIL = 4299
# first_chunk 5 + lookahead 1, chunks of 4, fade 240 -> the smallest legal window, 9 tokens: 26 tokens run in rounds of 6, 10, 14, 18, 22, 26 tokens whose
# windows start at token 0, 0, 0, 3, 7, 11
SHAPE = dict(first_chunk=5, chunk=4, lookahead=1, fade=240)
W, N = 9, 26


def _llama(dev):
    import test_stream_gpu as S
    eng, s3_sd, texts, cond, ref, z, phase, noise, kw = S._setup(dev, N, 8)
    return eng, s3_sd, texts, cond, ref, z, phase, noise, kw


def _turbo(dev, B=2):
    import test_turbo_stream_gpu as S
    eng, _, s3_sd, texts, cond, ref, z, phase, noise, kw = S._setup(dev, B, False, N, 8)
    return eng, s3_sd, texts, cond, ref, z, phase, noise, dict(kw, ban_eos=True, ban_from=6561)


@pytest.mark.parametrize("overlap", [False, True], ids=["serial", "overlapped"])
@pytest.mark.parametrize("backbone", ["llama", "gpt2"])
def test_a_window_wider_than_the_utterance_is_the_stream_without_a_window(dev, backbone, overlap):
    """A: every a_r = 0 -- the windowed path (carry = the scan's own zero start, emission through cbx_stream_emit_f32) yields the bits of window=None."""
    eng, _, texts, cond, ref, _, _, _, kw = (_llama if backbone == "llama" else _turbo)(dev)
    none = list(eng.synthesize_stream(texts, cond, ref, overlap=overlap, **SHAPE, **kw))
    wide = list(eng.synthesize_stream(texts, cond, ref, overlap=overlap, window=10 ** 6, **SHAPE, **kw))
    assert len(none) == len(wide) == 6
    for r, (a, b) in enumerate(zip(none, wide)):
        assert a["final"] == b["final"] and a["n_tokens"] == b["n_tokens"]
        for x, y in zip(a["wavs"], b["wavs"]):
            assert x.shape == y.shape and x.numel() > 0 and torch.equal(x, y), f"round {r}: max |diff| {(x - y).abs().max().item():.3e}"


def _against_oracle(tag, pieces_of, one_shot, oracle_pieces):
    streamed, want = torch.cat(pieces_of), torch.cat(oracle_pieces)
    lens_ok = [p.numel() for p in pieces_of[: len(oracle_pieces)]] == [p.numel() for p in oracle_pieces] and all(p.numel() == 0 for p in pieces_of[len(oracle_pieces):])
    rmse = (streamed - want).pow(2).mean().sqrt().item() if streamed.numel() == want.numel() else float("nan")
    jump = (streamed[1:] - streamed[:-1]).abs().max().item()
    step = (one_shot[1:] - one_shot[:-1]).abs().max().item()
    print(f"[stream-window] {tag}: pieces {[p.numel() for p in pieces_of]} oracle {[p.numel() for p in oracle_pieces]} total {streamed.numel()} one-shot {one_shot.numel()} "
          f"RMSE {rmse:.3e} max step {jump:.3e} one-shot max step {step:.3e}")
    assert lens_ok, f"{tag}: piece lengths differ from the oracle's"
    assert streamed.numel() == one_shot.numel(), f"{tag}: {streamed.numel()} samples streamed, {one_shot.numel()} in one shot"
    assert rmse <= 2e-3, f"{tag}: windowed stream vs the oracle's restatement, RMSE {rmse:.3e}"
    assert jump <= 2.0 * step + 1e-3, f"{tag}: a seam steps by {jump:.3e}, the one-shot waveform by at most {step:.3e}"


@pytest.mark.parametrize("backbone", ["llama", "gpt2"])
def test_windowed_stream_matches_the_oracle_schedule(dev, backbone):
    """B for synthesize_stream: six rounds, the window slides in the last three (a = 3, 7, 11)."""
    import stream_window_common as c
    from chatterbox_amd.engine import stream_window_schedule
    from oracle import ref_torch as O
    llama = backbone == "llama"
    eng, s3_sd, texts, cond, ref, z, phase, noise, kw = (_llama if llama else _turbo)(dev)
    sched = stream_window_schedule(N, window=W, **SHAPE)
    assert [a for a, _ in sched] == [0, 0, 0, 3, 7, 11]
    rounds = list(eng.synthesize_stream(texts, cond, ref, window=W, **SHAPE, **kw))
    assert len(rounds) == 6 and rounds[-1]["final"] == [True, True] and not any(any(r["final"]) for r in rounds[:-1])
    full, toks = eng.synthesize(texts, cond, ref, **({"drop_last_token": True} if llama else {}), **kw)
    for b in range(2):
        assert rounds[-1]["tokens"][b].tolist() == toks[b].tolist()
        sampled = toks[b] if llama else toks[b][:-3]
        assert sampled.numel() == N
        want = c.oracle_window_stream(O, s3_sd, sampled, ref, z[b:b + 1], phase[b:b + 1], noise[b:b + 1], window=W, n_steps=3 if llama else 2, meanflow=not llama,
                                      sil=None if llama else torch.full((3,), SIL, dtype=torch.long), drop_last=llama,
                                      **{("first" if k == "first_chunk" else k): v for k, v in SHAPE.items()})
        _against_oracle(f"{backbone} utt {b}", [r["wavs"][b] for r in rounds], full[b].cpu(), want)


def test_windowed_vocode_stream_matches_the_oracle_schedule_for_ragged_lengths(dev):
    """B for vocode_stream on the T3-less engine ChatterboxVC builds: 26 and 19 tokens; the short utterance is final in round 4 (window at token 7), the long
    one goes on alone."""
    import stream_window_common as c
    from chatterbox_amd import synth
    from chatterbox_amd.api import ChatterboxVC
    from oracle import ref_torch as O
    s3_sd = synth.s3gen_state_dict(0, n_mid=2, n_enc=1, n_up_enc=1)
    eng = ChatterboxVC._engine(s3_sd, dev)
    assert eng.t3 is None
    P, lens = 8, [N, 19]
    ref = synth.s3gen_ref(n_prompt_tokens=P)
    toks = [synth.speech_tokens(n, seed=3 + b) for b, n in enumerate(lens)]
    z = synth.randn((2, 80, 2 * (P + N)), seed=5)
    phase = (synth.rand((2, 9, 1), seed=6) * 2 - 1) * math.pi
    phase[:, 0] = 0
    noise = synth.randn((2, 9, 960 * N), seed=6)
    kw = dict(z=z.transpose(1, 2).contiguous(), phase=phase, noise=noise, n_cfm_timesteps=3)
    rounds = list(eng.vocode_stream(toks, ref, window=W, **SHAPE, **kw))
    assert [r["final"] for r in rounds] == [[False, False]] * 4 + [[False, True], [True, True]] and rounds[-1]["n_tokens"] == lens
    full, _ = eng.vocode(toks, ref, **kw)
    for b, n in enumerate(lens):
        want = c.oracle_window_stream(O, s3_sd, toks[b], ref, z[b:b + 1], phase[b:b + 1], noise[b:b + 1], window=W, n_steps=3, drop_last=False,
                                      **{("first" if k == "first_chunk" else k): v for k, v in SHAPE.items()})
        assert full[b].numel() == 960 * n
        _against_oracle(f"vocode_stream utt {b}", [r["wavs"][b] for r in rounds], full[b].cpu(), want)


def test_a_windowed_round_sees_a_bounded_number_of_tokens(dev):
    """C: spies on flow.inference and hift.inference of a windowed and of a window=None stream (constant chunks)."""
    from chatterbox_amd import engine as E
    eng, _, texts, cond, ref, _, _, _, kw = _llama(dev)
    trips = E.RANGE_TRIPS
    seen = {"flow": [], "hift": []}
    flow, hift = eng.flow.inference, eng.hift.inference
    eng.flow.inference = lambda tok, *a, **k: (seen["flow"].append(int(tok.shape[1])), flow(tok, *a, **k))[1]
    eng.hift.inference = lambda mel, *a, **k: (seen["hift"].append(int(mel.shape[1])), hift(mel, *a, **k))[1]
    rounds = list(eng.synthesize_stream(texts, cond, ref, window=W, overlap=False, **SHAPE, **kw))
    bound = W + SHAPE["chunk"] + SHAPE["lookahead"] + 1
    print(f"[stream-window] tokens per round, window={W}: {seen['flow']} (bound {bound})")
    assert len(rounds) == 6 and max(seen["flow"]) <= bound and seen["hift"] == [2 * n for n in seen["flow"]]
    assert E.RANGE_TRIPS == trips, "a round was repeated at bf16x6: the call counts below assume one pass per round"
    assert seen["flow"] == [6, 10, 14, 15, 15, 15] and len(set(seen["flow"][3:])) == 1
    seen["flow"].clear()
    seen["hift"].clear()
    list(eng.synthesize_stream(texts, cond, ref, overlap=False, **SHAPE, **kw))
    assert seen["flow"] == [6, 10, 14, 18, 22, 26], "without a window a round re-runs every token so far"


class _Watermarker:
    def __init__(self):
        self.calls = 0

    def apply_watermark(self, wav, sample_rate):
        self.calls += 1
        return wav


@pytest.mark.parametrize("source", ["s3_tokens", "waveform"])
def test_vc_generate_stream(dev, source):
    """D: from_synthetic model; 130 source tokens resp. a 3 s waveform (75 tokens) through the S3 tokenizer, window 20 / chunks of 25 so that the window slides."""
    from chatterbox_amd import synth
    from chatterbox_amd.api import ChatterboxVC
    vc = ChatterboxVC.from_synthetic(dev, tokenizer_layers=1)
    ref = vc.ref_dict
    src = dict(s3_tokens=synth.speech_tokens(130, seed=2)) if source == "s3_tokens" else dict(audio=(synth.prompt_wav(3.0, 16000, seed=3).numpy(), 16000))
    n_tok = 130 if source == "s3_tokens" else 75
    vc.watermarker = None
    torch.manual_seed(3)
    whole = vc.generate(**src)
    assert whole.shape == (1, 960 * n_tok)
    wm = vc.watermarker = _Watermarker()
    flows, flow = [], vc.engine.flow.inference
    vc.engine.flow.inference = lambda tok, *a, **k: (flows.append(int(tok.shape[1])), flow(tok, *a, **k))[1]
    torch.manual_seed(3)
    gen = vc.generate_stream(first_chunk=10, chunk=25, window=20, **src)
    assert flows == [], "nothing is synthesised before the first next()"
    first = next(gen)
    assert set(flows) == {13}, "the first piece arrives after one round of first_chunk + lookahead tokens"
    pieces = [first] + list(gen)
    from chatterbox_amd.engine import stream_window_schedule
    sched = stream_window_schedule(n_tok, first_chunk=10, chunk=25, window=20)
    print(f"[stream-window] VC.generate_stream({source}): pieces {[p.shape[1] for p in pieces]}, tokens per round {flows}")
    assert all(p.dim() == 2 and p.shape[0] == 1 and p.dtype == torch.float32 and p.device.type == "cpu" and torch.isfinite(p).all() for p in pieces)
    assert first.shape[1] == 960 * 10 - 480 and sum(p.shape[1] for p in pieces) == whole.shape[1]
    assert wm.calls == len(pieces) == len(sched) and sorted(set(flows)) == sorted({n - a for a, n in sched}) and max(flows) <= 20 + 25 + 3 + 1 and max(flows) < n_tok
    assert vc.ref_dict is ref
    assert float(torch.cat(pieces, 1).abs().max()) <= 0.99
