"""CPU (-m "not gpu"): speed control -- cbx_mel_time_scale_f32 on the SIMT emulator against the NumPy fp64 restatement of its definition, its C ABI and
descriptor errors, the host helpers (ops.scaled_len, ops.check_speed) and the plumbing of `speed=` on the public classes over a recording engine (nothing is
launched).  The recording engines are those of test_seeded_rng_host.py (read-only import)."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, os.path.join(HERE, "simt")):
    if p not in sys.path:
        sys.path.insert(0, p)

import mel_speed_common as S  # noqa: E402
from test_seeded_rng_host import LENS, _FakeEngine, _FakeSerialEngine, _sub_batches, _tts  # noqa: E402  (read-only import: the recording engines)

CPU = torch.device("cpu")


# ----------------------------------------------------------------------------- host helpers
def test_scaled_len_is_floor_with_a_minimum_of_one():
    from chatterbox_amd import ops
    assert [ops.scaled_len(n, 1.25) for n in (0, 1, 2, 5, 10, 499)] == [1, 1, 1, 4, 8, 399]
    assert [ops.scaled_len(n, 0.8) for n in (0, 1, 4, 499)] == [1, 1, 5, 623]
    assert ops.scaled_len(7, 0.9) == 7 and ops.scaled_len(61, 2.0) == 30 and ops.scaled_len(61, 0.5) == 122 and ops.scaled_len(1, 2.0) == 1
    for n in (0, 1, 7, 61, 500, 4000):
        for s in (0.5, 0.75, 0.9, 1.0, 1.1, 1.25, 1.5, 2.0):
            assert ops.scaled_len(n, s) == S.out_len(n, s) and isinstance(ops.scaled_len(n, s), int)


def test_check_speed():
    from chatterbox_amd import ops
    assert ops.check_speed(None, 3) is None and ops.check_speed(1.0, 3) is None and ops.check_speed(1, 2) is None and ops.check_speed([1.0, None], 2) is None
    assert ops.check_speed(1.25, 2) == [1.25, 1.25] and ops.check_speed([0.5, None, 2], 3) == [0.5, 1.0, 2.0] and ops.check_speed((0.8,), 1) == [0.8]
    assert all(isinstance(v, float) for v in ops.check_speed([1, 2], 2))
    for bad, err in ((True, TypeError), ("1", TypeError), ([1.0, "1"], TypeError), ([1.0, False], TypeError), (torch.tensor([1.0, 1.2]), TypeError),
                     (float("nan"), ValueError), (float("inf"), ValueError), (0.49, ValueError), (2.01, ValueError), ([1.0, 0.49], ValueError), (-1.0, ValueError),
                     ([1.0], ValueError), ([1.0, 1.0, 1.0], ValueError)):
        with pytest.raises(err, match="speed"):
            ops.check_speed(bad, 2)
    with pytest.raises(ValueError, match="rate"):
        ops.check_speed(3.0, 1, "rate")


# ----------------------------------------------------------------------------- C ABI
def test_mel_time_scale_entry_point_is_declared_exported_and_bound():
    from chatterbox_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "cbx.h")).read()
    lib = ctypes.CDLL(os.path.join(ROOT, "chatterbox_amd", "libcbx_hip.so"))
    assert re.search(r"^int cbx_mel_time_scale_f32\(", hdr, re.M) and hasattr(lib, "cbx_mel_time_scale_f32") and "cbx_mel_time_scale_f32" in _lib._SIGS
    assert "#define CBX_ABI_VERSION 16" in hdr and _lib.lib.cbx_abi_version() == 16, "a new function only: no version step"
    assert "s3gen.py:289" in open(os.path.join(ROOT, "chatterbox_amd", "csrc", "mel_speed.hip")).read()


def _descriptor_errors(lib):
    """Every refused descriptor returns nonzero with a message, before any launch (host buffers: a launch of the product library on them would fault)."""
    f = lib.cbx_mel_time_scale_f32   # (bound by _lib._SIGS on both handles)
    buf, rate, lens = (ctypes.c_float * 64)(), (ctypes.c_double * 1)(1.25), (ctypes.c_int * 2)(4, 3)
    a = ctypes.addressof
    good = [a(buf), 32, 8, 4, a(lens), a(rate), a(buf) + 128, 32, 8, 4, a(lens) + 4, 1, 8, None]
    for i, bad in ((0, None), (5, None), (6, None), (10, None), (12, 0), (12, -3), (1, 7), (2, 7), (7, 7), (8, 7)):
        args = list(good)
        args[i] = bad
        assert f(*args) == -22 and b"mel_time_scale" in lib.cbx_last_error(), (i, bad)
    args = list(good)
    args[11] = 0   # B = 0: nothing to do, no launch
    assert f(*args) == 0
    args = list(good)
    args[9] = 0    # T_out = 0
    assert f(*args) == 0


def test_descriptor_errors_return_a_status_and_a_message():
    from chatterbox_amd import _lib
    _descriptor_errors(_lib.lib)


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
@pytest.mark.parametrize("rates", [(0.5, 0.9), (2.0, 1.25), (1.1, 0.75)])
def test_mel_time_scale_on_the_emulator(emu, rates, strided):
    """B = 2, lens (1, 7) inside T_in = 8: both forms of the kernel against the fp64 restatement; NaN beyond in_lens and in the pad columns of the strided run."""
    from chatterbox_amd import ops
    S.check_launch(ops, CPU, (1, 7), rates, 8, strided)


def test_emulated_entry_refuses_the_same_descriptors_and_clamps_out_lens(emu):
    _descriptor_errors(emu)
    mel = S.log_mel((1, 8, 80), seed=5)
    buf = torch.full((2, 4, 80), 777.0)
    rate, lens = torch.tensor([1.25], dtype=torch.float64), torch.tensor([8, 6], dtype=torch.int32)   # out_lens 6 > T_out 4
    assert emu.cbx_mel_time_scale_f32(mel.data_ptr(), 640, 80, 8, lens.data_ptr(), rate.data_ptr(), buf.data_ptr(), 320, 80, 4, lens.data_ptr() + 4, 1, 80, None) == 0
    assert np.abs(buf[0].double().numpy() - S.reference(mel[0].numpy(), 8, 1.25)[:4]).max() <= 4 * S.U * float(mel.abs().max())
    assert bool((buf[1] == 777.0).all()), "out_lens > T_out must not overrun the output"
    out, ol = ops_mel(mel, [1.0], None)            # in_lens NULL: every row has T_in frames; rate 1.0 is the identity map (x = j, lambda = 0)
    assert ol.tolist() == [8] and torch.equal(out, mel)


def ops_mel(mel, rates, in_lens):
    from chatterbox_amd import ops
    return ops.mel_time_scale(mel, rates, in_lens=in_lens)


def test_wrapper_refuses_bad_shapes_before_the_call(emu):
    from chatterbox_amd import ops
    mel = S.log_mel((2, 8, 80), seed=1)
    with pytest.raises(ValueError):
        ops.mel_time_scale(mel, [1.25], in_lens=[8, 8])
    with pytest.raises(ValueError):
        ops.mel_time_scale(mel, [1.25, 1.25], in_lens=[8, 9])
    with pytest.raises(ValueError):
        ops.mel_time_scale(mel, [0.5, 1.25], in_lens=[8, 8], out=torch.zeros(2, 15, 80))


# ----------------------------------------------------------------------------- the public classes over a recording engine (nothing is launched)
SPEEDS = [1.25, 0.8, None, 2.0, 0.5]


@pytest.mark.parametrize("cls_name,extra", [("ChatterboxTTS", 2), ("ChatterboxMultilingualTTS", 2), ("ChatterboxTurboTTS", 0)])
@pytest.mark.parametrize("max_batch", [None, 2])
def test_speeds_follow_their_requests_through_the_batch_plan(cls_name, extra, max_batch):
    from chatterbox_amd import api
    eng = _FakeEngine() if cls_name != "ChatterboxTurboTTS" else _FakeSerialEngine()
    m = _tts(getattr(api, cls_name), eng)
    m.max_batch = max_batch
    texts = ["x" * (n - 1) + "." for n in LENS]
    args = (texts, "en") if cls_name == "ChatterboxMultilingualTTS" else (texts,)
    out = m.generate_batch(*args, speed=SPEEDS, seeds=list(range(5)))
    assert [int(w[0, 0]) for w in out] == [n + extra for n in LENS], "waveforms come back in the caller's order"
    jobs = [j for kind, kw in eng.calls for j in (kw["jobs"] if kind == "pipelined" else [kw])]
    assert [len(j["text_tokens"]) for j in jobs] == ([4, 1] if max_batch is None else [2, 2, 1])
    speed_of_len = {n + extra: (1.0 if s is None else s) for n, s in zip(LENS, SPEEDS)}
    seed_of_len = {n + extra: k for k, n in enumerate(LENS)}
    for j in jobs:
        lens = [int(t.numel()) for t in j["text_tokens"]]
        assert j["speed"] == [speed_of_len[n] for n in lens] and j["seeds"] == [seed_of_len[n] for n in lens], "a sub-batch carries the speeds of ITS requests, in its row order"
    eng.calls.clear()
    m.generate_batch(*args, speed=1.25)   # a number: the same speed for every request
    assert all(j["speed"] == [1.25] * len(j["text_tokens"]) for kind, kw in eng.calls for j in (kw["jobs"] if kind == "pipelined" else [kw]))
    for same in (1.0, None, [1.0, None, 1, 1.0, 1.0]):
        eng.calls.clear()
        m.generate_batch(*args, speed=same)   # nothing scaled: the jobs are exactly those of a call without the argument
        assert all("speed" not in j for kind, kw in eng.calls for j in (kw["jobs"] if kind == "pipelined" else [kw])) and _sub_batches(eng.calls)


@pytest.mark.parametrize("cls_name", ["ChatterboxTTS", "ChatterboxMultilingualTTS", "ChatterboxTurboTTS"])
def test_speed_arguments_are_validated_before_the_engine_is_called(cls_name):
    from chatterbox_amd import api
    eng = _FakeEngine()
    m = _tts(getattr(api, cls_name), eng)
    texts = ["aaaa.", "bb.", "cccccc."]
    lang = ("en",) if cls_name == "ChatterboxMultilingualTTS" else ()
    bad = ((True, TypeError), ("1", TypeError), (float("nan"), ValueError), (0.49, ValueError), (2.01, ValueError))
    for v, err in bad + (([1.0, 1.2], ValueError), ([1.0, 1.2, 0.9, 1.0], ValueError), ([1.0, "1", 1.0], TypeError)):
        with pytest.raises(err, match="speed"):
            m.generate_batch(texts, *lang, speed=v)
    for v, err in bad:
        with pytest.raises(err, match="speed"):
            m.generate("aaaa.", *lang, speed=v)
    assert eng.calls == []
    m.generate("aaaa.", *lang, speed=1.25, seed=3)
    assert eng.calls[-1][0] == "synthesize" and eng.calls[-1][1]["speed"] == [1.25] and eng.calls[-1][1]["seeds"] == [3]
    m.generate("aaaa.", *lang)
    assert "speed" not in eng.calls[-1][1], "at speed 1.0 the engine call is exactly the one without the argument"


def test_vc_speeds_follow_their_requests_and_are_validated():
    from chatterbox_amd import api, synth

    class Voc:
        def __init__(self):
            self.calls = []

        def vocode(self, toks, refs, **kw):
            self.calls.append(([int(t.numel()) for t in toks], kw))
            return [torch.full((2,), float(t.numel())) for t in toks], None

    vc = api.ChatterboxVC.__new__(api.ChatterboxVC)
    vc.engine, vc.device, vc.ref_dict, vc.analyzer, vc.watermarker = Voc(), CPU, synth.s3gen_ref(n_prompt_tokens=8), None, None
    vc.MAX_BATCH = 2
    toks = [synth.speech_tokens(n) for n in (30, 10, 20)]
    for v, err in (([1.0, 1.2], ValueError), (2.5, ValueError), ([1.0, 1.0, "1"], TypeError), (True, TypeError)):
        with pytest.raises(err, match="speed"):
            vc.generate_batch(s3_tokens=toks, speed=v)
    with pytest.raises(ValueError, match="speed"):
        vc.generate(s3_tokens=toks[0], speed=0.25)
    assert vc.engine.calls == []
    out = vc.generate_batch(s3_tokens=toks, speed=[0.8, 1.25, None])
    assert [int(w[0, 0]) for w in out] == [30, 10, 20]
    assert [(l, kw.get("speed")) for l, kw in vc.engine.calls] == [([10, 20], [1.25, 1.0]), ([30], [0.8])]
    vc.engine.calls.clear()
    vc.generate(s3_tokens=toks[1], speed=1.5)
    vc.generate(s3_tokens=toks[1])
    vc.generate(s3_tokens=toks[1], speed=1.0)
    assert vc.engine.calls[0][1] == dict(speed=[1.5]) and vc.engine.calls[1][1] == {} and vc.engine.calls[2][1] == {}


def test_vocode_trim_rule_on_a_recording_engine(monkeypatch):
    """ChatterboxEngine.vocode over stand-in stages on the CPU: the flow's mel is stretched by ONE ops.mel_time_scale call over M_b = 2 n_b - short_b frames, the
    vocoder gets the stretched mel with lens = O_b, the returned mel is the unscaled one, and row b's waveform is max(1, floor(K_b / s_b)) * 480 samples where the
    call without speed returns K_b * 480 -- also with the last token dropped.  speed=None and 1.0 make no such call."""
    from chatterbox_amd import engine, ops, synth
    eng = engine.ChatterboxEngine.__new__(engine.ChatterboxEngine)
    eng.dev, eng.last_timing, seen = CPU, {}, {}
    eng.flow = type("Flow", (), {"precision": 1, "inference": lambda self, tok, lens, ref, **kw: torch.ones(tok.shape[0], 2 * tok.shape[1], 80)})()

    def hift_inference(mel, lens=None, **kw):
        seen.update(mel=mel, lens=lens)
        return torch.zeros(mel.shape[0], 480 * mel.shape[1]), None
    eng.hift = type("Hift", (), {"precision": 1, "inference": staticmethod(hift_inference)})()
    calls = []

    def fake_scale(mel, rates, in_lens=None, out=None):
        calls.append((tuple(mel.shape), list(rates), list(in_lens)))
        O = [ops.scaled_len(m, r) for m, r in zip(in_lens, rates)]
        return torch.zeros(mel.shape[0], max(O), 80), torch.tensor(O, dtype=torch.int32)
    monkeypatch.setattr(ops, "mel_time_scale", fake_scale)
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: None)
    ref = synth.s3gen_ref(n_prompt_tokens=6)
    st = [synth.speech_tokens(n, seed=k) for k, n in enumerate((12, 5, 9))]
    for drop in (False, True):
        base, mel0 = eng.vocode(st, ref, drop_last_token=drop)
        assert calls == [] and seen["mel"] is mel0
        same, _ = eng.vocode(st, ref, drop_last_token=drop, speed=[1.0, None, 1])
        assert calls == [] and [w.numel() for w in same] == [w.numel() for w in base]
        K = [w.numel() // 480 for w in base]
        assert K == ([22, 8, 16] if drop else [24, 10, 18])
        speeds = [0.8, 1.25, 2.0]
        wavs, mel = eng.vocode(st, ref, drop_last_token=drop, speed=speeds)
        assert calls == [((3, 24, 80), speeds, [24, 10, 18])] and mel.shape == (3, 24, 80)
        assert seen["mel"].shape == (3, 30, 80) and seen["lens"].tolist() == [30, 8, 9]
        assert [w.numel() for w in wavs] == [480 * max(1, int(k / s)) for k, s in zip(K, speeds)]
        calls.clear()
