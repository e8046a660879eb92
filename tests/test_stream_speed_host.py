"""CPU (-m "not gpu"): `speed=` on the streaming entry points -- the host arithmetic of a stream at a speaking rate (engine.stream_speed_schedule and the functions
under it) against its restatement in stream_speed_common.py, engine.check_stream_window with a rate, cbx_mel_time_scale_win_f32 on the SIMT emulator (the checks
the MI355X runs in test_turbo_stream_speed_window_kernels_gpu.py), its C ABI, and the plumbing of generate_stream(speed=) over recording engines (nothing is
launched).  The recording engines are those of test_seeded_rng_host.py (read-only import)."""
import ctypes
import itertools
import math
import os
import re
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, os.path.join(HERE, "simt")):
    if p not in sys.path:
        sys.path.insert(0, p)

import mel_speed_common as S  # noqa: E402
import stream_speed_common as C  # noqa: E402
from test_seeded_rng_host import _FakeSerialEngine, _tts  # noqa: E402  (read-only import: the recording engine)

CPU = torch.device("cpu")
RATES = (0.5, 0.6, 2 / 3, 0.8, 0.9, 1.0, 1.1, 1.25, 4 / 3, 1.5, 5 / 3, 1.9, 2.0)
SHAPES = ((5, 4, 1, 240), (25, 50, 3, 480), (10, 25, 3, 480), (5, 4, 0, 0), (3, 7, 2, 100), (4, 1, 0, 480))  # first_chunk, chunk, lookahead, fade


def _min_window(E, fade, s):
    w = 1
    while True:
        try:
            return E.check_stream_window(w, fade, E.check_stream_speed(s))
        except ValueError:
            w += 1


# ----------------------------------------------------------------------------- the host functions against their restatement
def test_host_rules_equal_their_restatement():
    from chatterbox_amd import engine as E
    for s in RATES:
        for M in list(range(0, 70)) + [499, 500, 4001]:
            assert E.stream_ready_frames(M, s) == C.ready_frames(M, s), (M, s)
        for a in (0, 1, 2, 3, 7, 20, 333):
            j0 = E.stream_origin_frame(a, s)
            assert j0 == C.origin_frame(2 * a, s) and (a > 0 or j0 == 0)
            if a:
                i0, _, _ = C.abs_taps(j0 - 1, 2, s)
                assert C.position(j0, s) >= 2 * a + 0.25 > C.position(j0 - 1, s) and i0[1] >= 2 * a
        for E_ in (0, 479, 480, 5520, 15120, 99999, 10 ** 6):
            for W in (9, 20, 200):
                assert E.stream_window_origin(E_, W, s) == C.window_origin(E_, W, s)
    for E_ in range(0, 40000, 37):   # at s = 1 the origin is today's E // 960 - W
        assert E.stream_window_origin(E_, 9, 1.0) == max(0, E_ // 960 - 9)
    assert E.stream_round_frames(61, 1.25, True) == S.out_len(61, 1.25) and E.stream_round_frames(61, 1.25, False) == C.ready_frames(61, 1.25)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda v: "fc%d_c%d_la%d_f%d" % v)
def test_speed_schedule_over_the_grid(shape):
    """n_tokens x rate x window for one round shape: at s = 1 the schedule is stream_window_schedule's; a_r and j0_r never move left; a round is at most
    W + chunk + lookahead + 1 tokens; whenever a > 0 the window holds the vocoder's receptive field + fade in front of the first sample not emitted,
    480 (je - j0) >= 8000 + fade; the pieces add up to 480 * out_len(2 keep, s); and no frame a non-final round vocodes has a tap at or beyond the M_abs unscaled
    frames it holds, nor left of 2a (the restated taps)."""
    from chatterbox_amd import engine as E
    fc, ch, L, fade = shape
    for n, s, drop in itertools.product((1, 7, 26, 60, 131) + ((400,) if ch >= 25 else ()), RATES, (False, True)):   # (400 tokens in chunks of 50 / 25: a long stream)
        for W in (None, _min_window(E, fade, s), _min_window(E, fade, s) + 3, 200):
            sch = E.stream_speed_schedule(n, s, fc, ch, L, 1.0, W, fade, drop)
            tag = (n, s, W, drop)
            if s == 1.0:
                assert [(a, nr) for a, nr, _, _ in sch] == E.stream_window_schedule(n, fc, ch, L, 1.0, W, fade) and all(j0 == 2 * a for a, _, j0, _ in sch), tag
            assert [nr for _, nr, _, _ in sch] == E.stream_token_schedule(n, fc, ch, L, 1.0)
            prev_e, prev_a, prev_j = 0, 0, 0
            for r, (a, nr, j0, em) in enumerate(sch):
                final = r == len(sch) - 1
                assert a >= prev_a and j0 >= prev_j and (final or em >= prev_e), tag
                assert (W is None and a == 0) or nr - a <= W + ch + L + 1, f"{tag}: round {r} synthesises {nr - a} tokens"
                if a > 0:
                    assert 480 * (prev_e // 480 - j0) >= 8000 + fade, f"{tag}: round {r}, {480 * (prev_e // 480 - j0)} samples of context"
                if s != 1.0 and em > prev_e:
                    M_abs = 2 * nr - (0 if final else 2 * L)
                    R = em // 480 if final else (em + fade) // 480   # frames the round vocoded (a non-final round emits all but `fade` samples of them)
                    assert final or R == C.ready_frames(M_abs, s), tag
                    i0, i1, _ = C.abs_taps(j0, R - j0, s)
                    assert R > j0 and i0.min() >= 2 * a, f"{tag}: round {r} needs a tap left of its window"
                    assert final or i1.max() <= M_abs - 1, f"{tag}: round {r} vocodes a frame whose right tap does not exist yet"
                prev_e, prev_a, prev_j = em, a, j0
            keep = max(1, n - 1) if drop else n
            assert sch[-1][3] == 480 * S.out_len(2 * keep, s), tag


def test_check_stream_window_with_a_rate():
    from chatterbox_amd import engine as E
    for fade in (0, 240, 480):
        base = -(-(8000 + fade) // 960)
        assert E.check_stream_window(base, fade) == base and E.check_stream_window(None, fade, 1.25) is None
        with pytest.raises(ValueError, match="window"):
            E.check_stream_window(base - 1, fade)
        for s in RATES:
            rate = E.check_stream_speed(s)
            assert (rate is None) == (s == 1.0)
            need = _min_window(E, fade, s)
            F = -(-(8000 + fade) // 480)
            assert need >= base and (s == 1.0 or need == max(base, -int(-(F * s + max(0.0, s - 1.0) + 0.5) // 2))), (fade, s, need)
            assert need <= math.ceil((8000 + fade) * max(1.0, s) / 960) + 1, "no more than the rule of thumb: ceil((8000 + fade) max(1, s) / 960) + 1"
            for w in (need - 1, 0, -3, True, 9.0, "9"):
                with pytest.raises(ValueError, match="window"):
                    E.check_stream_window(w, fade, rate)
    assert E.check_stream_window(12, 240, 1.25) == 12 and E.check_stream_window(19, 480, 2.0) == 19 and E.check_stream_window(9, 480, 0.5) == 9
    with pytest.raises(ValueError, match="speed=1.25"):
        E.check_stream_window(11, 240, 1.25)


def test_check_stream_speed():
    from chatterbox_amd import engine as E
    assert E.check_stream_speed(None) is None and E.check_stream_speed(1.0) is None and E.check_stream_speed(1) is None
    assert E.check_stream_speed(1.25) == 1.25 and E.check_stream_speed(2) == 2.0 and isinstance(E.check_stream_speed(2), float)
    for bad, err in ((True, TypeError), ("1", TypeError), ([1.25], TypeError), ((0.8,), TypeError), (float("nan"), ValueError), (0.49, ValueError), (2.01, ValueError)):
        with pytest.raises(err, match="speed"):
            E.check_stream_speed(bad)


# ----------------------------------------------------------------------------- C ABI
def test_window_entry_point_is_declared_exported_and_bound():
    from chatterbox_amd import _lib, ops
    hdr = open(os.path.join(ROOT, "include", "cbx.h")).read()
    lib = ctypes.CDLL(os.path.join(ROOT, "chatterbox_amd", "libcbx_hip.so"))
    assert re.search(r"^int cbx_mel_time_scale_win_f32\(", hdr, re.M) and hasattr(lib, "cbx_mel_time_scale_win_f32") and "cbx_mel_time_scale_win_f32" in _lib._SIGS
    assert "#define CBX_ABI_VERSION 16" in hdr and _lib.lib.cbx_abi_version() == 16 and _lib.ABI_VERSION == 16, "a new function only: no version step"
    src = open(os.path.join(ROOT, "chatterbox_amd", "csrc", "mel_speed.hip")).read()
    assert "s3gen.py:289" in src and 'extern "C" int cbx_mel_time_scale_win_f32(' in src and callable(ops.mel_time_scale_window)
    assert len(re.findall(r"\(double\)j \+ 0\.5\) \* s - 0\.5", src)) == 1, "one position expression, shared by both kernels"


def test_descriptor_errors_return_a_status_and_a_message():
    from chatterbox_amd import _lib
    C.descriptor_errors(_lib.lib)


# ----------------------------------------------------------------------------- the kernel on the SIMT emulator
@pytest.fixture(scope="module")
def emu():
    import build_emu
    if not os.path.exists(build_emu.CLANG):
        pytest.skip("ROCm's clang++ (x86 host compiler of the emulator build) is not installed")
    import harness
    with harness.emulated() as lib:
        yield lib


@pytest.mark.parametrize("strided", [False, True], ids=["contiguous_float4", "row_stride_83_scalar"])
@pytest.mark.parametrize("i_org", [0, 6, 7, 40])
@pytest.mark.parametrize("rate", [0.5, 0.9, 1.0, 1.25, 2.0])
def test_window_launch_on_the_emulator(emu, rate, i_org, strided):
    from chatterbox_amd import ops
    C.check_window_launch(ops, CPU, rate, i_org, strided)


@pytest.mark.parametrize("rate", [0.5, 0.9, 1.0, 1.25, 2.0])
def test_far_window_on_the_emulator(emu, rate):
    from chatterbox_amd import ops
    C.check_far_window(ops, CPU, rate)


def test_emulated_entry_refuses_the_same_descriptors_and_clamps_what_the_host_passes(emu):
    """Memory safety does not rest on the host's choice of j0 / i_org / lens: taps left of the window and beyond in_lens are clamped into it, out_lens beyond T_out
    is cut (the buffers are exactly as large as the descriptor says; a sentinel row behind the output must survive)."""
    C.descriptor_errors(emu)
    mel = S.log_mel((1, 8, 80), seed=5)
    buf = torch.full((2, 4, 80), 777.0)
    lens = torch.tensor([8, 6], dtype=torch.int32)   # out_lens 6 > T_out 4
    for j0, i_org in ((0, 50), (10 ** 6, 0), (3, 3)):   # every tap left of the window; every tap right of it; an ordinary one
        assert emu.cbx_mel_time_scale_win_f32(mel.data_ptr(), 640, 80, 8, lens.data_ptr(), 1.25, j0, i_org, buf.data_ptr(), 320, 80, 4, lens.data_ptr() + 4, 1, 80, None) == 0
        assert torch.isfinite(buf).all() and bool((buf[1] == 777.0).all()), "out_lens > T_out must not overrun the output"
        if i_org == 50:
            assert torch.equal(buf[0], mel[0, :1].expand(4, 80))
        if j0 == 10 ** 6:
            assert torch.equal(buf[0], mel[0, 7:8].expand(4, 80))


def test_wrapper_refuses_bad_arguments_before_the_call(emu):
    from chatterbox_amd import ops
    mel = S.log_mel((2, 8, 80), seed=1)
    for kw in (dict(in_lens=[8], out_lens=[4, 4]), dict(in_lens=[8, 9], out_lens=[4, 4]), dict(in_lens=[8, 8], out_lens=[4, -1]), dict(in_lens=[8, 8], out_lens=[4, 4], rate=2.5),
               dict(in_lens=[8, 8], out_lens=[4, 4], j0=-1), dict(in_lens=[8, 8], out_lens=[4, 4], i_org=-2), dict(in_lens=[8, 8], out_lens=[4, 5], out=torch.zeros(2, 4, 80))):
        args = dict(dict(rate=1.25, j0=0, i_org=0, out=None), **kw)
        with pytest.raises(ValueError, match="mel_time_scale_window"):
            ops.mel_time_scale_window(mel, args["rate"], args["j0"], args["i_org"], args["in_lens"], args["out_lens"], out=args["out"])


# ----------------------------------------------------------------------------- generate_stream(speed=) over recording engines (nothing is launched)
class _StreamEngine(_FakeSerialEngine):
    def synthesize_stream(self, text_tokens, t3_conds, gen_ref, **kw):
        self.calls.append(("synthesize_stream", kw))
        yield dict(wavs=[torch.zeros(5)])


BAD = ((True, TypeError), ("1", TypeError), ([1.25], TypeError), (float("nan"), ValueError), (0.49, ValueError), (2.01, ValueError))


@pytest.mark.parametrize("cls_name", ["ChatterboxTTS", "ChatterboxMultilingualTTS", "ChatterboxTurboTTS"])
def test_tts_generate_stream_passes_speed_and_validates_it_when_called(cls_name):
    import inspect
    from chatterbox_amd import api
    eng = _StreamEngine()
    m = _tts(getattr(api, cls_name), eng)
    lang = ("en",) if cls_name == "ChatterboxMultilingualTTS" else ()
    assert list(inspect.signature(m.generate_stream).parameters)[-1] == "speed" and inspect.signature(m.generate_stream).parameters["speed"].default == 1.0
    for v, err in BAD:
        with pytest.raises(err, match="speed"):
            m.generate_stream("aaaa.", *lang, speed=v)     # raised by the CALL: no next()
    with pytest.raises(ValueError, match="window"):
        m.generate_stream("aaaa.", *lang, speed=2.0, window=18)   # legal without a rate, too short at 2.0
    assert eng.calls == []
    pieces = list(m.generate_stream("aaaa.", *lang, speed=1.25, window=20, seed=3))
    assert len(pieces) == 1 and eng.calls[-1][1]["speed"] == 1.25 and eng.calls[-1][1]["window"] == 20 and eng.calls[-1][1]["seeds"] == [3]
    for same in (1.0, None, 1):
        list(m.generate_stream("aaaa.", *lang, speed=same))
        assert "speed" not in eng.calls[-1][1], "at speed 1.0 / None the engine call is exactly the one without the argument"
    list(m.generate_stream("aaaa.", *lang))
    assert eng.calls[-1][1] == eng.calls[-2][1]


def test_vc_generate_stream_passes_speed_and_validates_it_when_called():
    import inspect
    from chatterbox_amd import api, synth

    class Voc:
        def __init__(self):
            self.calls = []

        def vocode_stream(self, toks, ref, **kw):
            self.calls.append(kw)
            yield dict(wavs=[torch.zeros(5)])

    vc = api.ChatterboxVC.__new__(api.ChatterboxVC)
    vc.engine, vc.device, vc.ref_dict, vc.analyzer, vc.watermarker = Voc(), CPU, synth.s3gen_ref(n_prompt_tokens=8), None, None
    toks = synth.speech_tokens(30)
    assert list(inspect.signature(vc.generate_stream).parameters)[-1] == "speed"
    for v, err in BAD:
        with pytest.raises(err, match="speed"):
            vc.generate_stream(s3_tokens=toks, speed=v)
    with pytest.raises(ValueError, match="window"):
        vc.generate_stream(s3_tokens=toks, speed=2.0, window=18)
    assert vc.engine.calls == []
    list(vc.generate_stream(s3_tokens=toks, speed=1.25, window=20, first_chunk=10, chunk=25))
    assert vc.engine.calls[-1]["speed"] == 1.25 and vc.engine.calls[-1]["window"] == 20
    for same in (1.0, None):
        list(vc.generate_stream(s3_tokens=toks, speed=same))
        assert "speed" not in vc.engine.calls[-1]
    list(vc.generate_stream(s3_tokens=toks))
    assert vc.engine.calls[-1] == vc.engine.calls[-2]


def test_engine_stream_entry_points_take_speed():
    import inspect
    from chatterbox_amd import engine as E
    for fn in (E.ChatterboxEngine.synthesize_stream, E.ChatterboxEngine.vocode_stream, E.TurboEngine.synthesize_stream, E.TurboEngine.vocode_stream, E._synthesize_stream,
               E._stream_rounds):
        assert inspect.signature(fn).parameters["speed"].default is None, fn


# ----------------------------------------------------------------------------- the engine's rounds at a rate, on the CPU oracle's stages
@pytest.mark.parametrize("s", [0.8, 1.25])
def test_vocode_stream_rounds_at_a_rate_equal_the_restated_schedule(emu, s):
    """ChatterboxEngine.vocode_stream(window=12, speed=s) with the oracle's stages in place of the device engines (test_stream_window_host._oracle_engine, read-only
    import; the stretch is the emulated cbx_mel_time_scale_win_f32, the emission the emulated cbx_stream_emit_f32) == stream_speed_common.oracle_window_stream for
    a ragged pair: the same piece lengths, adding up to 480 * out_len(2 n, s); the flow sees tokens [a_r, n_r) of the host schedule, the vocoder frames
    [j0_r, R_r) of it, trim_fade while j0 == 0 only.  The two differ in the stretch alone (fp32 blend against the fp64 restatement: 4 * 2^-24 * |mel| per mel value),
    so the waveforms are held to the project's bound for chunked synthesis, RMSE <= 2e-3; the measured difference is printed."""
    from chatterbox_amd import synth
    from chatterbox_amd.engine import stream_speed_schedule
    from test_stream_window_host import _oracle_engine
    eng, O, sd = _oracle_engine()
    P, first, chunk, look, fade, W, n_steps = 4, 5, 4, 1, 240, 12, 2
    lens = [26, 19]
    ref = synth.s3gen_ref(n_prompt_tokens=P)
    toks = [synth.speech_tokens(n, seed=3 + b) for b, n in enumerate(lens)]
    z = synth.randn((2, 80, 2 * (P + max(lens))), seed=5)
    phase = (synth.rand((2, 9, 1), seed=6) * 2 - 1) * math.pi
    phase[:, 0] = 0
    noise = synth.randn((2, 9, 480 * S.out_len(2 * max(lens), s)), seed=6)
    kw = dict(first_chunk=first, chunk=chunk, lookahead=look, fade=fade, n_cfm_timesteps=n_steps, z=z.transpose(1, 2).contiguous(), phase=phase, noise=noise,
              drop_last_token=False)
    rounds = list(eng.vocode_stream(toks, ref, window=W, speed=s, **kw))
    sched = stream_speed_schedule(max(lens), s, first, chunk, look, 1.0, W, fade)
    assert len(rounds) == len(sched) and [a for a, _, _, _ in sched] == [0, 0, 0, 0, 4, 8]
    assert [t[1] for t in eng.flow.seen] == [n - a for a, n, _, _ in sched], "a round's flow sees tokens [a_r, n_r)"
    assert max(t[1] for t in eng.flow.seen) <= W + chunk + look + 1
    assert [t[2] for t in eng.hift.seen] == [j0 == 0 for _, _, j0, _ in sched], "trim_fade belongs to sample 0"
    assert [t[0] for t in eng.hift.seen[:-1]] == [(e + fade) // 480 - j0 for _, _, j0, e in sched[:-1]], "a non-final round vocodes stretched frames [j0, R)"
    assert rounds[-1]["final"] == [True, True] and rounds[-1]["n_tokens"] == lens
    for b, n in enumerate(lens):
        got = [r["wavs"][b] for r in rounds]
        want = C.oracle_window_stream(O, sd, toks[b], ref, z[b:b + 1], phase[b:b + 1], noise[b:b + 1], first, chunk, look, fade, W, n_steps, s, drop_last=False)
        assert [g.numel() for g in got[: len(want)]] == [w.numel() for w in want] and all(g.numel() == 0 for g in got[len(want):])
        assert sum(g.numel() for g in got) == 480 * S.out_len(2 * n, s)
        diff = torch.cat(got) - torch.cat(want)
        print(f"s={s} utterance {b}: RMSE {diff.pow(2).mean().sqrt().item():.3e} max |diff| {diff.abs().max().item():.3e}")
        assert diff.pow(2).mean().sqrt().item() <= 2e-3
    # without a window every round stretches the whole mel so far: the same total, and the last round vocodes all out_len(2 n, s) frames
    eng2, _, _ = _oracle_engine()
    none = list(eng2.vocode_stream(toks, ref, window=None, speed=s, **kw))
    assert [sum(r["wavs"][b].numel() for r in none) for b in range(2)] == [480 * S.out_len(2 * n, s) for n in lens]
    assert eng2.hift.seen[-1][0] == S.out_len(2 * max(lens), s) and all(t[2] for t in eng2.hift.seen)
