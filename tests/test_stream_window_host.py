"""CPU (-m "not gpu"): bounded-cost ("windowed") streaming -- the round schedule as host arithmetic (engine.stream_window_schedule), the validation of
`window` and of ChatterboxVC.generate_stream before anything is launched, the two kernels behind it on the SIMT emulator (tests/simt) bit for bit against the
full-length source resp. the torch expression they replace, and the engine's round function with the CPU oracle's stages in place of the device engines
against the same schedule restated in tests/stream_window_common.py."""
import math
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
SCHEDULES = [dict(n_tokens=250, first_chunk=25, chunk=50, lookahead=3, chunk_growth=1.0, fade=480), dict(n_tokens=1000, first_chunk=25, chunk=50, lookahead=3, chunk_growth=1.0, fade=480),
             dict(n_tokens=1500, first_chunk=25, chunk=50, lookahead=3, chunk_growth=1.0, fade=480), dict(n_tokens=97, first_chunk=6, chunk=7, lookahead=3, chunk_growth=1.0, fade=240),
             dict(n_tokens=400, first_chunk=10, chunk=20, lookahead=2, chunk_growth=1.3, fade=960), dict(n_tokens=60, first_chunk=5, chunk=3, lookahead=0, chunk_growth=1.0, fade=0),
             dict(n_tokens=9, first_chunk=25, chunk=50, lookahead=3, chunk_growth=1.0, fade=480)]


def _emitted_before_each_round(sched, n_tokens, lookahead, fade):
    """E_r of an utterance that does not end early, and the total, by the engine's emission rule (all but `fade` samples of what a round could vocode)."""
    E, e = [], 0
    for _, n in sched:
        E.append(e)
        final = n >= n_tokens
        avail = 480 * (2 * n - (0 if final else 2 * lookahead))
        e = avail if final else max(e, avail - fade)
    return E, e


@pytest.mark.parametrize("kw", SCHEDULES, ids=lambda k: f"N{k['n_tokens']}_c{k['chunk']}_g{k['chunk_growth']}_f{k['fade']}")
def test_window_none_is_the_token_schedule_with_every_window_at_zero(kw):
    from chatterbox_amd.engine import stream_token_schedule, stream_window_schedule
    sk = {k: v for k, v in kw.items() if k != "fade"}
    assert stream_window_schedule(window=None, **kw) == [(0, n) for n in stream_token_schedule(**sk)]
    assert stream_window_schedule(**kw) == stream_window_schedule(window=None, **kw)


@pytest.mark.parametrize("window", [None, "min", 20, 200, 100000])
@pytest.mark.parametrize("kw", SCHEDULES, ids=lambda k: f"N{k['n_tokens']}_c{k['chunk']}_g{k['chunk_growth']}_f{k['fade']}")
def test_window_schedule_properties(kw, window):
    """n_r is the unchanged token schedule; a_r never moves left; a round's window reaches at least 8000 + fade samples left of the first sample it has not
    emitted yet (the vocoder's receptive field and the cross-fade); a round is at most W + chunk_r + lookahead + 1 tokens long; the emitted ranges tile
    [0, total) exactly once."""
    from chatterbox_amd.engine import stream_token_schedule, stream_window_schedule
    fade, look, N = kw["fade"], kw["lookahead"], kw["n_tokens"]
    need = -(-(8000 + fade) // 960)
    W = need if window == "min" else window
    if W is not None and W < need:
        pytest.skip(f"window {W} is below this fade's minimum {need}")
    sched = stream_window_schedule(window=W, **kw)
    totals = stream_token_schedule(**{k: v for k, v in kw.items() if k != "fade"})
    assert [n for _, n in sched] == totals and sched[0][0] == 0 and sched[-1][1] == N
    E, total = _emitted_before_each_round(sched, N, look, fade)
    assert total == 960 * N, "the last round hands out the rest"
    c = float(kw["chunk"])
    for r, (a, n) in enumerate(sched):
        assert r == 0 or a >= sched[r - 1][0], "a_r is non-decreasing"
        assert 0 <= a < n
        if W is None:
            assert a == 0
            continue
        assert 960 * a <= max(0, E[r] - fade - 8000), f"round {r}: the window starts right of E_r - fade - 8000"
        assert a == max(0, E[r] // 960 - W)
        if r > 0:
            assert n - a <= W + (n - sched[r - 1][1]) + look + 1, f"round {r} is {n - a} tokens long"
            assert n - sched[r - 1][1] <= max(1, int(round(c)))
            c *= kw["chunk_growth"]
    # tiling: round r emits [E_r, E_{r+1}); consecutive by construction, so exactly once iff monotone from 0 to the total
    ends = E[1:] + [total]
    assert E[0] == 0 and all(e1 >= e0 for e0, e1 in zip(E, ends)) and ends[-1] == total
    if W is not None and kw["chunk_growth"] == 1.0 and len(sched) > 4:
        slid = [n - a for a, n in sched[:-1] if a > 0]
        assert len(set(slid)) <= 1, f"once the window slides every round but the last has one length: {slid}"


def test_window_schedule_bounds_the_work_of_long_utterances():
    """Without a window 250 tokens cost 890 token-rounds and 1000 tokens 11 060 (eleven times the one-shot synthesis; the last round alone is one); with
    window=200 no round exceeds 254 tokens."""
    from chatterbox_amd.engine import stream_window_schedule
    work = lambda N, W: [n - a for a, n in stream_window_schedule(N, window=W)]
    assert sum(work(250, None)) == 28 + 78 + 128 + 178 + 228 + 250 == 890
    assert sum(work(1000, None)) == 20 * 28 + 50 * 190 + 1000 == 11060 and max(work(1000, None)) == 1000
    assert max(work(1000, 200)) <= 254 and max(work(1500, 200)) <= 254
    assert sum(work(1500, 200)) < 0.35 * sum(work(1500, None))


@pytest.mark.parametrize("bad", [0, 5, 8, -1, 9.0, "200", True])
def test_a_window_below_the_receptive_field_is_refused(bad):
    from chatterbox_amd.engine import check_stream_window, stream_window_schedule
    assert check_stream_window(None, 480) is None and check_stream_window(9, 480) == 9 and check_stream_window(9, 0) == 9
    with pytest.raises(ValueError, match="window"):
        check_stream_window(bad, 480)
    with pytest.raises(ValueError, match="window"):
        stream_window_schedule(100, window=bad)
    with pytest.raises(ValueError, match="window"):
        check_stream_window(9, 960)   # (8000 + 960) / 960 -> 10 tokens


# ----------------------------------------------------------------------------- the public classes over recording engines (nothing is launched)
class _RecordingEngine:
    dev = CPU

    def __init__(self):
        self.calls = []

    def synthesize_stream(self, *a, **kw):
        self.calls.append(("synthesize_stream", kw))
        yield dict(wavs=[torch.ones(5)], final=[True], n_tokens=[1], tokens=[torch.zeros(1)])

    def vocode_stream(self, toks, ref, **kw):
        self.calls.append(("vocode_stream", dict(toks=toks, ref=ref, **kw)))
        yield dict(wavs=[torch.zeros(0)], final=[False], n_tokens=[1], tokens=toks)
        yield dict(wavs=[torch.ones(7)], final=[False], n_tokens=[1], tokens=toks)
        yield dict(wavs=[torch.ones(3)], final=[True], n_tokens=[1], tokens=toks)


class _Tok:
    def text_to_tokens(self, text, language_id=None):
        return torch.arange(len(text), dtype=torch.int32).unsqueeze(0)

    def __call__(self, text, **kw):
        return type("Enc", (), {"input_ids": torch.arange(len(text))[None]})()


@pytest.mark.parametrize("cls_name", ["ChatterboxTTS", "ChatterboxMultilingualTTS", "ChatterboxTurboTTS"])
def test_tts_generate_stream_checks_window_when_called_and_passes_it_through(cls_name):
    from chatterbox_amd import api, synth
    cls = getattr(api, cls_name)
    m = cls.__new__(cls)
    m.engine, m.tokenizer, m.device, m.analyzer, m.watermarker, m.model_label = _RecordingEngine(), _Tok(), CPU, None, None, "Turbo"
    m.conds = api.Conditionals(api.T3Cond(**synth.t3_cond()), synth.s3gen_ref(n_prompt_tokens=8))
    args = ("hello.", "en") if cls_name == "ChatterboxMultilingualTTS" else ("hello.",)
    for bad in (3, 9.5, "wide"):
        with pytest.raises(ValueError, match="window"):
            m.generate_stream(*args, window=bad)     # raised by the CALL, not by the first next()
    with pytest.raises(ValueError, match="window"):
        m.generate_stream(*args, window=9, fade=960)
    assert m.engine.calls == []
    assert [tuple(p.shape) for p in m.generate_stream(*args, window=12)] == [(1, 5)]
    assert m.engine.calls[-1][1]["window"] == 12
    list(m.generate_stream(*args))
    assert m.engine.calls[-1][1]["window"] is None, "the default keeps today's schedule"


def _vc(ref="default"):
    from chatterbox_amd import api, synth
    m = api.ChatterboxVC.__new__(api.ChatterboxVC)
    m.engine, m.device, m.analyzer, m.watermarker = _RecordingEngine(), CPU, None, None
    m.s3gen = m.engine
    m.ref_dict = synth.s3gen_ref(n_prompt_tokens=8) if ref == "default" else ref
    return m


def test_vc_generate_stream_validates_before_anything_runs():
    m = _vc()
    toks = torch.arange(40)
    for kw in (dict(window=3), dict(window=9, fade=960), dict(window=12.0), dict(first_chunk=0), dict(chunk=0), dict(chunk=2.5), dict(lookahead=-1), dict(fade=-1),
               dict(chunk_growth=0.5), dict(fade=True)):
        with pytest.raises(ValueError, match=next(iter(kw))):
            m.generate_stream(s3_tokens=toks, **kw)
    with pytest.raises(ValueError, match="audio or s3_tokens"):
        m.generate_stream()
    with pytest.raises(ValueError, match="no S3 tokens"):
        m.generate_stream(s3_tokens=torch.zeros(0, dtype=torch.long))
    with pytest.raises(AssertionError, match="target_voice_path"):
        _vc(ref=None).generate_stream(s3_tokens=toks)
    with pytest.raises(RuntimeError, match="tokenizer"):
        m.generate_stream(audio=(torch.zeros(16000).numpy(), 16000))     # a waveform needs the S3 tokenizer: this model has no analyzer
    assert m.engine.calls == []


def test_vc_generate_stream_yields_finished_pieces_and_keeps_the_voice():
    """Defaults window=200, chunk=50 (the 250-token round); pieces are (1, n) float32 on the host, empty rounds are not yielded, the watermarker sees each
    piece once, self.ref_dict is the caller's object before and after, and the stream keeps the voice it was called with."""
    m = _vc()
    ref = m.ref_dict

    class WM:
        calls = 0

        def apply_watermark(self, wav, sample_rate):
            WM.calls += 1
            assert sample_rate == 24000
            return wav
    m.watermarker = WM()
    gen = m.generate_stream(s3_tokens=[3, 4, 5, 6])
    assert m.engine.calls == [], "nothing runs before the first next()"
    m.ref_dict = None   # (a later change of the model's voice does not reach into the running stream)
    pieces = list(gen)
    m.ref_dict = ref
    name, kw = m.engine.calls[0]
    assert name == "vocode_stream" and kw["ref"] is ref and [t.tolist() for t in kw["toks"]] == [[3, 4, 5, 6]] and kw["toks"][0].dtype == torch.long
    assert {k: kw[k] for k in ("first_chunk", "chunk", "chunk_growth", "lookahead", "fade", "window")} == dict(first_chunk=25, chunk=50, chunk_growth=1.0,
                                                                                                              lookahead=3, fade=480, window=200)
    assert [tuple(p.shape) for p in pieces] == [(1, 7), (1, 3)] and all(p.dtype == torch.float32 and p.device.type == "cpu" for p in pieces)
    assert WM.calls == 2
    list(m.generate_stream(s3_tokens=[1, 2], window=None))
    assert m.engine.calls[-1][1]["window"] is None


# ----------------------------------------------------------------------------- the kernels on the SIMT emulator
@pytest.fixture(scope="module")
def emu():
    import build_emu
    if not os.path.exists(build_emu.CLANG):
        pytest.skip("ROCm's clang++ (x86 host compiler of the emulator build) is not installed")
    import harness
    with harness.emulated() as lib:
        yield lib


def test_source_with_phase_carry_equals_the_full_length_source_on_the_emulator(emu):
    import stream_window_common as c
    from chatterbox_amd import ops
    c.check_source_carry(ops, CPU)


@pytest.mark.parametrize("name", ["first_round_no_tails", "steady_window", "short_tails_finals_closed", "no_fade"])
def test_stream_emit_equals_the_torch_expression_on_the_emulator(emu, name):
    import stream_window_common as c
    from chatterbox_amd import ops
    faded = c.check_stream_emit(ops, CPU, name)
    assert (faded > 0) == (name in ("steady_window", "short_tails_finals_closed"))


def test_stream_emit_refuses_bad_arguments(emu):
    from chatterbox_amd import ops
    wav, meta = torch.zeros(1, 960), torch.zeros(4, 1, dtype=torch.int32)
    t, t2 = torch.zeros(1, 4), torch.zeros(1, 4)
    args = lambda **k: dict(dict(w=wav.data_ptr(), ld=960, o=0, m=meta.data_ptr(), ti=t.data_ptr(), to=t2.data_ptr(), fade=4), **k)

    def call(w, ld, o, m, ti, to, fade, keep=[]):
        out, ramp = torch.zeros(1, 8), torch.zeros(4)
        keep.append((out, ramp))
        return emu.cbx_stream_emit_f32(w, ld, o, m, m + 4, m + 8, ti, m + 12, ramp.data_ptr(), fade, out.data_ptr(), 8, to, 1, None)
    assert call(**args()) == 0
    assert call(**args(w=None)) != 0 and call(**args(o=-1)) != 0 and call(**args(ld=0)) != 0
    assert call(**args(to=t.data_ptr())) != 0 and b"distinct" in emu.cbx_last_error()   # tail_in == tail_out would race
    assert call(**args(ti=None)) != 0


def test_hift_f0_source_carry_c_entry_point_on_the_emulator(emu):
    """cbx_hift_f0_source_carry against HiFTEngine.f0_predict + source(cum_in=), bit for bit, ragged batch of 2 x 4 mel frames."""
    import test_turbo_stream_window_kernels_gpu as K
    K.test_f0_source_with_carry_through_the_c_entry_point_equals_the_python_sequence(CPU, B=2, T=4)


# ----------------------------------------------------------------------------- the engine's round function over the oracle's stages
class _OracleFlow:
    """FlowEngine.inference's contract (channel-last mel, hold_back; a row of a ragged batch gets the values of its batch-1 run) on O.flow_inference, row by row
    (the oracle's own batched run is not padding-invariant); records the tokens each call was given."""
    precision = 1

    def __init__(self, O, sd, meanflow=False):
        self.O, self.sd, self.meanflow, self.seen = O, sd, meanflow, []

    def co_resident(self, on):
        pass

    def inference(self, tokens, token_lens, ref, z=None, n_steps=10, hold_back=None, generator=None):
        self.seen.append(tuple(tokens.shape))
        B, N = tokens.shape
        P = ref["prompt_token"].shape[1]
        mel = torch.zeros(B, 2 * N, 80)
        for b in range(B):
            n = int(token_lens[b])
            m = self.O.flow_inference(self.sd, tokens[b:b + 1, :n], torch.tensor([n]), ref, z[b:b + 1, : 2 * (P + n)].transpose(1, 2), n_steps, meanflow=self.meanflow,
                                      hold_back=torch.tensor([int(hold_back[b])]))
            mel[b, : 2 * n] = m[0].t()
        return mel


class _OracleHift:
    """HiFTEngine.inference's contract (lens, fade, cache_source, cum_in, .frame_cum) on the oracle's f0_predict / source_module / hift_decode, row by row."""
    precision = 1

    def __init__(self, O, sd):
        self.O, self.sd, self.frame_cum, self.seen = O, sd, None, []

    def inference(self, mel, phase=None, noise=None, lens=None, fade=True, cache_source=None, generator=None, cum_in=None):
        O, (B, T, _) = self.O, mel.shape
        self.seen.append((T, None if cum_in is None else cum_in.clone(), fade))
        wav, src, cum = torch.zeros(B, 480 * T), torch.zeros(B, 480 * T), torch.zeros(B, 9, T, dtype=torch.float64)
        mult = torch.arange(1, 10, dtype=torch.float32)[None, :, None]
        for b in range(B):
            n = int(lens[b])
            m = mel[b:b + 1, :n].transpose(1, 2)
            f0 = O.f0_predict(self.sd, m)
            carry = torch.zeros(1, 9, dtype=torch.float64) if cum_in is None else cum_in[b:b + 1]
            ph = phase[b].view(1, 9, 1).double() + 2 * math.pi * (carry - carry.floor())[:, :, None]
            s = O.source_module(self.sd, f0, ph.float(), noise[b:b + 1, :, : 480 * n])
            if cache_source is not None and cache_source.shape[1]:
                k = min(cache_source.shape[1], 480 * n)
                s = s.clone()
                s[0, 0, :k] = cache_source[b, :k]
            w = O.hift_decode(self.sd, m, s)
            wav[b, : 480 * n] = (O.trim_fade(w) if fade else w)[0]
            src[b, : 480 * n] = s[0, 0]
            inc = 480.0 * ((f0[:, None, :] * mult) / 24000.0).double()
            cum[b, :, :n] = (carry[:, :, None] + torch.cumsum(inc, 2) - inc)[0]
            cum[b, :, n:] = cum[b, :, n - 1: n] + inc[0, :, -1:]
        self.frame_cum = cum
        return wav, src


def _oracle_engine(meanflow=False):
    from chatterbox_amd import synth
    from chatterbox_amd.engine import ChatterboxEngine
    from oracle import ref_torch as O
    sd = synth.s3gen_state_dict(0, meanflow=meanflow, n_mid=1, n_enc=1, n_up_enc=1)
    eng = ChatterboxEngine.__new__(ChatterboxEngine)
    eng.dev, eng.t3, eng.flow, eng.hift, eng.last_timing = CPU, None, _OracleFlow(O, sd, meanflow), _OracleHift(O, sd), {}
    return eng, O, sd


def test_vocode_stream_rounds_equal_the_restated_windowed_schedule(emu):
    """ChatterboxEngine.vocode_stream(window=9) with the oracle's stages in place of the device engines (the emission is the emulated cbx_stream_emit_f32) ==
    stream_window_common.oracle_window_stream, sample for sample, for a ragged pair; the window slides in two rounds at least, every round obeys the token
    bound, the carry handed to the vocoder is the previous round's scan at the frame the window starts, and trim_fade is applied while a == 0 only."""
    import stream_window_common as c
    from chatterbox_amd import synth
    from chatterbox_amd.engine import stream_window_schedule
    eng, O, sd = _oracle_engine()
    P, first, chunk, look, fade, W, n_steps = 4, 5, 4, 1, 240, 9, 2
    lens = [26, 19]
    ref = synth.s3gen_ref(n_prompt_tokens=P)
    toks = [synth.speech_tokens(n, seed=3 + b) for b, n in enumerate(lens)]
    z = synth.randn((2, 80, 2 * (P + max(lens))), seed=5)
    phase = (synth.rand((2, 9, 1), seed=6) * 2 - 1) * math.pi
    phase[:, 0] = 0
    noise = synth.randn((2, 9, 960 * max(lens)), seed=6)
    kw = dict(first_chunk=first, chunk=chunk, lookahead=look, fade=fade, n_cfm_timesteps=n_steps, z=z.transpose(1, 2).contiguous(), phase=phase, noise=noise,
              drop_last_token=False)
    rounds = list(eng.vocode_stream(toks, ref, window=W, **kw))
    sched = stream_window_schedule(max(lens), first, chunk, look, 1.0, W, fade)
    assert len(rounds) == len(sched) and sum(a > 0 for a, _ in sched) >= 2
    assert [s[1] for s in eng.flow.seen] == [n - a for a, n in sched], "a round's flow sees tokens [a_r, n_r)"
    assert max(s[1] for s in eng.flow.seen) <= W + chunk + look + 1
    assert [s[2] for s in eng.hift.seen] == [a == 0 for a, _ in sched], "trim_fade belongs to sample 0"
    assert eng.hift.seen[0][1] is None and all(s[1] is not None for s in eng.hift.seen[1:])
    assert [r["final"] for r in rounds][-1] == [True, True] and rounds[-1]["n_tokens"] == lens
    for b, n in enumerate(lens):
        got = [r["wavs"][b] for r in rounds]
        want = c.oracle_window_stream(O, sd, toks[b], ref, z[b:b + 1], phase[b:b + 1], noise[b:b + 1], first, chunk, look, fade, W, n_steps, drop_last=False)
        assert [g.numel() for g in got[: len(want)]] == [w.numel() for w in want] and all(g.numel() == 0 for g in got[len(want):])
        assert sum(g.numel() for g in got) == 960 * n
        err = (torch.cat(got) - torch.cat(want)).abs().max().item()
        assert err <= 1e-6, f"utterance {b}: max |diff| {err:.3e}"
    # window wider than the utterance == the schedule without a window, bit for bit (equal lengths: no row finishes before the other)
    eng2, _, _ = _oracle_engine()
    same = [toks[0], synth.speech_tokens(lens[0], seed=9)]
    wide = list(eng2.vocode_stream(same, ref, window=10000, **kw))
    eng3, _, _ = _oracle_engine()
    none = list(eng3.vocode_stream(same, ref, window=None, **kw))
    assert len(wide) == len(none)
    for rw, rn in zip(wide, none):
        assert all(torch.equal(x, y) for x, y in zip(rw["wavs"], rn["wavs"])) and rw["final"] == rn["final"]
