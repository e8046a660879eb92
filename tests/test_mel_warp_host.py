"""CPU (-m "not gpu"): timing control -- cbx_mel_time_warp_f32 on the SIMT emulator against the NumPy fp64 restatement of its definition (mel_warp_common.py) and,
for one-segment tables, against ops.mel_time_scale bit for bit; its C ABI and descriptor errors; the host arithmetic of the plan (ops.warp_plan / warp_place,
check_duration / check_timing, every refused combination); the plumbing of `duration=` / `timing=` on the public classes over recording engines (nothing is
launched); ChatterboxEngine.vocode(warp=) over stand-in stages.  The recording engines are those of test_seeded_rng_host.py and test_word_times_host.py (read-only
imports)."""
import ctypes
import itertools
import math
import os
import re
import sys
import warnings

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, os.path.join(HERE, "simt")):
    if p not in sys.path:
        sys.path.insert(0, p)

import mel_speed_common as S  # noqa: E402
import mel_warp_common as W  # noqa: E402
from test_seeded_rng_host import LENS, _FakeEngine, _FakeSerialEngine, _sub_batches, _tts  # noqa: E402  (read-only import: the recording engines)
from test_word_times_host import _model, _WordsEngine  # noqa: E402  (read-only import: the engine that returns an alignment, the tokenizer with pieces)

CPU = torch.device("cpu")
RATES = (0.5, 0.75, 0.9, 1.1, 1.25, 1.5, 2.0)
IN_LENS, T_IN = (1, 7, 8), 8
FORMS = pytest.mark.parametrize("strided", [False, True], ids=["contiguous_float4", "row_stride_83_scalar"])


# ----------------------------------------------------------------------------- host arithmetic: the plan
def test_warp_plan_unclamped_and_its_inverse():
    from chatterbox_amd import ops
    p = ops.warp_plan(40, [(10, 15), (20, 22), (30, 40)], end=50)
    assert p["table"] == [(0, 0.0, 10 / 15), (15, 10.0, 10 / 7), (22, 20.0, 10 / 18), (40, 30.0, 1.0)]
    assert p["frames"] == 50 and p["achieved"] == [15, 22, 40] and p["clamped"] == [] and p["dropped"] == []
    assert (p["table"], p["frames"], p["achieved"], p["clamped"]) == W.plan(40, [(10, 15), (20, 22), (30, 40)], end=50), "the restatement agrees"
    for (x, _), o in zip([(10, 15), (20, 22), (30, 40)], p["achieved"]):
        assert ops.warp_place(p["table"], x) == o == W.place(p["table"], x), "at an anchor the inverse map is exactly o_k"
    assert ops.warp_place(p["table"], 0) == 0 and abs(ops.warp_place(p["table"], 40) - 50) < 1e-9 and abs(ops.warp_place(p["table"], 5) - 7.5) < 1e-12
    for (o0, a0, s0), (o1, a1, _) in zip(p["table"], p["table"][1:]):
        assert abs(a0 + (o1 - o0) * s0 - a1) < 1e-9, "seg_a is continuous"
    assert all(0.5 <= s <= 2.0 for _, _, s in p["table"])
    # end not given: the tail at rate 1
    q = ops.warp_plan(40, [(10, 15)])
    assert q["table"] == [(0, 0.0, 10 / 15), (15, 10.0, 1.0)] and q["frames"] == 45 and q["clamped"] == []
    # no anchors: a duration
    assert ops.warp_plan(20, [], end=25) == dict(table=[(0, 0.0, 0.8)], frames=25, achieved=[], clamped=[], dropped=[])
    assert ops.warp_plan(20, []) == dict(table=[(0, 0.0, 1.0)], frames=20, achieved=[], clamped=[], dropped=[])


def test_warp_plan_clamps_both_ways_and_later_anchors_still_aim_at_their_targets():
    from chatterbox_amd import ops
    p = ops.warp_plan(40, [(10, 30), (20, 31), (30, 41)], end=51)   # 10 frames into 30: held at rate 0.5 (20 frames); then 10 into 11: fine again
    assert p["achieved"] == [20, 31, 41] and p["clamped"] == [0] and p["frames"] == 51
    assert [s for _, _, s in p["table"]] == [0.5, 10 / 11, 1.0, 1.0]
    p = ops.warp_plan(40, [(10, 2), (20, 12)], end=13)              # 10 frames into 2: held at rate 2.0 (5); 10 into 7; the tail 20 into 1: held at 2.0 (10)
    assert p["achieved"] == [5, 12] and p["clamped"] == [0, "end"] and p["frames"] == 22 and [s for _, _, s in p["table"]] == [2.0, 10 / 7, 2.0]
    p = ops.warp_plan(9, [(3, 0)])                                  # a target behind the plan: the minimum, ceil(3 / 2) = 2 frames
    assert p["achieved"] == [2] and p["clamped"] == [0] and p["table"][0] == (0, 0.0, 1.5)
    assert ops.warp_plan(20, [], end=5)["frames"] == 10 and ops.warp_plan(20, [], end=5)["clamped"] == ["end"]
    assert ops.warp_plan(20, [], end=100)["frames"] == 40 and ops.warp_plan(21, [], end=5)["frames"] == 11, "ceil(K / 2)"
    for K, anchors, end in ((40, [(10, 30), (20, 31), (30, 41)], 51), (40, [(10, 2), (20, 12)], 13), (9, [(3, 0)], None)):
        q = ops.warp_plan(K, anchors, end=end)
        assert (q["table"], q["frames"], q["achieved"], [k for k in q["clamped"] if k != "end"]) == W.plan(K, anchors, end=end)


def test_warp_plan_drops_anchors_without_input_in_front_of_them():
    from chatterbox_amd import ops
    p = ops.warp_plan(20, [(0, 5), (4, 6), (4, 9), (10, 12)])
    assert p["dropped"] == [0, 2] and p["achieved"] == [0, 6, 6, 12] and p["clamped"] == [0, 2], "x = 0 and a repeated x cannot be moved: reported as not honoured"
    assert p["table"] == [(0, 0.0, 4 / 6), (6, 4.0, 1.0), (12, 10.0, 1.0)] and p["frames"] == 22
    assert ops.warp_plan(20, [(0, 0), (4, 4), (4, 4)])["clamped"] == [], "a dropped anchor whose target is where its frame already is counts as met"
    p = ops.warp_plan(20, [(20, 30)], end=35)   # an anchor at the end closes the plan: `end` has nothing left to stretch
    assert p["frames"] == 30 and p["clamped"] == ["end"] and len(p["table"]) == 1
    # K = 1
    assert ops.warp_plan(1, []) == dict(table=[(0, 0.0, 1.0)], frames=1, achieved=[], clamped=[], dropped=[])
    assert ops.warp_plan(1, [], end=2)["table"] == [(0, 0.0, 0.5)] and ops.warp_plan(1, [], end=3)["frames"] == 2 and ops.warp_plan(1, [], end=1)["clamped"] == []
    assert ops.warp_plan(1, [(1, 2)])["frames"] == 2 and ops.warp_plan(1, [(0, 2)])["dropped"] == [0]
    for bad in ((0, []), (5, [(6, 1)]), (5, [(3, 1), (2, 2)]), (5, [(-1, 0)])):
        with pytest.raises(ValueError, match="warp_plan"):
            ops.warp_plan(*bad)


def test_targets_on_a_uniform_stretch_never_clamp_exhaustively():
    """Integer anchors x_k with targets floor(c x_k + 0.5) and end = floor(c K + 0.5) never clamp for c in {1.0, 1.25, 1.5}: consecutive targets differ by 1 or 2
    when L = 1 and by at most c L + 1 <= 2 L when L >= 2 (and by at least c L - 1 >= L / 2).  Every anchor SET over K <= 12 is enumerated, and every set of at
    most 3 anchors over K <= 40 (a segment only sees its two ends: pairs of consecutive anchors are what matters, and every pair over K <= 40 occurs).  The
    precondition of the unclamped GPU test of timing=."""
    from chatterbox_amd import ops
    r = lambda v: int(math.floor(v + 0.5))
    n = 0
    for c in (1.0, 1.25, 1.5):
        for K in range(1, 41):
            sets = itertools.chain.from_iterable(itertools.combinations(range(1, K), m) for m in (range(K) if K <= 12 else range(4)))
            for xs in sets:
                p = ops.warp_plan(K, [(x, r(c * x)) for x in xs], end=r(c * K))
                assert p["clamped"] == [] and p["frames"] == r(c * K) and p["achieved"] == [r(c * x) for x in xs], (c, K, xs, p)
                n += 1
    assert n > 30000


def test_check_duration_and_check_timing():
    from chatterbox_amd import ops
    assert ops.seconds_to_frames(0.05) == 3 and ops.seconds_to_frames(0.03) == 2 and ops.seconds_to_frames(3.2) == 160 and ops.seconds_to_frames(0.45) == 23
    assert ops.check_duration(None, 3) is None and ops.check_duration([None, None], 2) is None
    assert ops.check_duration(3.2, 2) == [160, 160] and ops.check_duration([0.02, None, 80], 3) == [1, None, 4000] and ops.check_duration((1,), 1) == [50]
    for bad, err in ((True, TypeError), ("1", TypeError), ([1.0, "1"], TypeError), ([1.0, False], TypeError), (torch.tensor([1.0, 1.2]), TypeError),
                     (float("nan"), ValueError), (float("inf"), ValueError), (0.019, ValueError), (80.01, ValueError), (-1.0, ValueError), ([1.0], ValueError),
                     ([1.0, 1.0, 1.0], ValueError)):
        with pytest.raises(err, match="duration"):
            ops.check_duration(bad, 2)
    assert ops.check_timing(None, 2) is None and ops.check_timing([None, [None, None]], 2) == [None, [None, None]]
    assert ops.check_timing([[0.0, None, 0.5, 0.5], None], 2) == [[0, None, 25, 25], None] and ops.check_timing(([0.45],), 1) == [[23]]
    for bad, err in ((1.0, TypeError), ([1.0, 2.0], TypeError), ([[True], None], TypeError), ([["1"], None], TypeError), ([[0.5, 0.4], None], ValueError),
                     ([[0.5, None, 0.4], None], ValueError), ([[-0.1], None], ValueError), ([[float("nan")], None], ValueError), ([[81.0], None], ValueError),
                     ([[0.1]], ValueError), ([[0.1], None, None], ValueError)):
        with pytest.raises(err, match="timing"):
            ops.check_timing(bad, 2)


def test_check_delivery_takes_warp_and_refuses_the_combinations_that_are_not_built():
    from chatterbox_amd import engine as E
    assert E.Delivery.OPTIONS[-1] == "warp" and E.check_delivery(2).warp is None and E.check_delivery(2, warp=[None, None]).warp is None
    assert "warp" not in E.check_delivery(2, warp=[None, None]).kw()
    d = E.check_delivery(2, warp=[None, dict(frames=7)], format=dict(sample_rate=16000, encoding="f32"), loudness=-20.0)
    assert d.warp == [None, dict(frames=7)] and d.kw()["warp"] == d.warp
    assert E.check_delivery(1, warp=[dict(anchors=[(2, 3), [4, 9]])]).warp == [dict(anchors=[(2, 3), (4, 9)], end=None)]
    for other, kw in (("speed", dict(speed=1.25)), ("pitch", dict(pitch=2.0)), ("pauses", dict(pauses=dict(keep=[3, 3], db=40.0, fade=48))),
                      ("join", dict(join=dict(gaps=[0, 0], trim_db=None, pad_frames=0, fade=0, first=True, last=True)))):
        with pytest.raises(ValueError, match=rf"(?s){other}.*warp"):
            E.check_delivery(2, warp=[dict(frames=7), None], **kw)
    for bad, err in ((dict(frames=7), TypeError), ([dict(frames=7)], ValueError), ([dict(frames=0), None], ValueError), ([dict(frames=1.5), None], ValueError),
                     ([dict(frame=3), None], ValueError), ([dict(anchors=[(3, 1), (2, 2)]), None], ValueError), ([dict(anchors=[(1.5, 1)]), None], TypeError),
                     ([dict(anchors=[(1, 2)], end=0), None], ValueError), ([7, None], ValueError)):
        with pytest.raises(err, match="warp"):
            E.check_delivery(2, warp=bad)
    job = dict(text_tokens=[torch.zeros(3), torch.zeros(2)], t3_conds=None, gen_ref=None)
    assert E._checked_job(dict(job, warp=[None, dict(frames=9)]))["warp"] == [None, dict(frames=9)] and "warp" not in E._checked_job(dict(job, warp=[None, None]))
    with pytest.raises(ValueError, match="anchors"):
        E._checked_job(dict(job, warp=[None, dict(anchors=[(2, 3)], end=None)]))


# ----------------------------------------------------------------------------- C ABI
def test_mel_time_warp_entry_point_is_declared_exported_and_bound():
    from chatterbox_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "cbx.h")).read()
    lib = ctypes.CDLL(os.path.join(ROOT, "chatterbox_amd", "libcbx_hip.so"))
    assert re.search(r"^int cbx_mel_time_warp_f32\(", hdr, re.M) and hasattr(lib, "cbx_mel_time_warp_f32") and "cbx_mel_time_warp_f32" in _lib._SIGS
    assert "#define CBX_ABI_VERSION 16" in hdr and _lib.lib.cbx_abi_version() == 16, "a new function only: no version step"
    src = open(os.path.join(ROOT, "chatterbox_amd", "csrc", "mel_warp.hip")).read()
    assert "s3gen.py:289" in src and "cbx_mel_taps_at" in src and "cbx_mel_blend_store" in src, "the taps and the blend are mel_speed.hip's, shared through cbx_common.h"
    assert "cbx_mel_taps_at" in open(os.path.join(ROOT, "chatterbox_amd", "csrc", "mel_speed.hip")).read()


def _descriptor_errors(lib):
    """Every refused descriptor returns -22 with a message, before any launch (host buffers: a launch of the product library on them would fault)."""
    f = lib.cbx_mel_time_warp_f32   # (bound by _lib._SIGS on both handles)
    buf, tab, ints = (ctypes.c_float * 64)(), (ctypes.c_double * 2)(0.0, 1.25), (ctypes.c_int * 3)(0, 4, 3)
    off, no_seg, beyond, neg = ((ctypes.c_int * 2)(*v) for v in ((0, 1), (0, 0), (0, 2), (-1, 1)))
    a = ctypes.addressof
    good = [a(buf), 32, 8, 4, a(ints) + 4, a(off), 1, a(ints), a(tab), a(tab) + 8, a(buf) + 128, 32, 8, 4, a(ints) + 8, 1, 8, None]
    for i, bad in ((0, None), (5, None), (7, None), (8, None), (9, None), (10, None), (14, None), (16, 0), (16, -3), (1, 7), (2, 7), (11, 7), (12, 7), (15, 65), (15, -1),
                   (3, -1), (13, -1), (6, 0), (6, -1), (5, a(no_seg)), (5, a(beyond)), (5, a(neg))):
        args = list(good)
        args[i] = bad
        assert f(*args) == -22 and b"mel_time_warp" in lib.cbx_last_error(), (i, bad)
    for i in (15, 13):   # B = 0, T_out = 0: nothing to do, no launch
        args = list(good)
        args[i] = 0
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


def _tables():
    """name -> (tables, out_lens) for rows of (1, 7, 8) frames"""
    per7, o7 = W.per_output_frame(7, 0.75)
    per8, o8 = W.per_output_frame(8, 1.25)
    return {
        "one_segment": ([[(0, 0.0, 0.9)], [(0, 0.0, 1.25)], [(0, 0.0, 0.5)]], [1, 5, 16]),
        "two_segments_0.5_2.0": ([[(0, 0.0, 0.5), (1, 0.5, 2.0)], [(0, 0.0, 0.5), (6, 3.0, 2.0)], [(0, 0.0, 0.5), (8, 4.0, 2.0)]], [2, 8, 10]),
        "one_segment_per_output_frame": ([[(0, 0.0, 1.0)], per7, per8], [1, o7, o8]),
    }


@FORMS
@pytest.mark.parametrize("name", ["one_segment", "two_segments_0.5_2.0", "one_segment_per_output_frame"])
def test_mel_time_warp_on_the_emulator(emu, name, strided):
    """B = 3, rows of 1, 7 and 8 frames inside T_in = 8: both forms of the kernel against the fp64 restatement; NaN beyond in_lens (and in the pad columns of the
    strided run), a sentinel in the output's pad columns and extra frames."""
    from chatterbox_amd import ops
    tables, O = _tables()[name]
    W.check_launch(ops, CPU, IN_LENS, tables, O, T_IN, strided)


@FORMS
def test_a_malformed_table_leaves_every_output_finite_and_every_sentinel_intact(emu, strided):
    """Decreasing seg_o, a negative rate, a NaN rate, an infinite and a NaN edge: memory safety does not depend on the table -- every output is a blend of valid
    frames (finite, within max|mel|) or zero, pad columns and extra frames keep their sentinel, nothing beyond in_lens is read (it holds NaN)."""
    from chatterbox_amd import ops
    nan, inf = float("nan"), float("inf")
    tables = [[(5, 0.0, -1.0), (3, nan, 1.0), (0, 2.0, nan)], [(0, 0.0, nan), (4, -inf, 1.0), (2, 1e300, -1e300), (9, inf, 0.5)], [(0, nan, nan), (3, 1e9, 1e9), (1, 3.0, 0.0)]]
    W.check_launch(ops, CPU, IN_LENS, tables, [4, 11, 9], T_IN, strided, finite_only=True)


@FORMS
@pytest.mark.parametrize("s", RATES)
def test_one_segment_tables_equal_mel_time_scale_bit_for_bit(emu, s, strided, C=80):
    from chatterbox_amd import ops
    mel = S.log_mel((3, T_IN, C), seed=7)
    O = [S.out_len(m, s) for m in IN_LENS]
    if strided:
        big = torch.full((3, T_IN, C + 3), float("nan"))
        big[:, :, :C] = mel
        mel = big[:, :, :C]
    a, al = ops.mel_time_warp(mel, [[(0, 0.0, s)]] * 3, in_lens=list(IN_LENS))     # out_lens derived: the last segment runs to the row's end, rounded
    b, bl = ops.mel_time_scale(mel, [s] * 3, in_lens=list(IN_LENS))
    want = [max(1, int(math.floor(m / s + 0.5))) for m in IN_LENS]
    assert al.tolist() == want, "derived out_lens: round((M - a) / s), what warp_plan's frames is for a plan over M"
    n = [min(x, y) for x, y in zip(want, O)]
    assert bl.tolist() == O and all(torch.equal(a[r, : n[r]], b[r, : n[r]]) for r in range(3)), f"s = {s}"
    a, al = ops.mel_time_warp(mel, [[(0, 0.0, s)]] * 3, in_lens=list(IN_LENS), out_lens=O)
    assert al.tolist() == O and torch.equal(a, b), f"s = {s}: a one-segment warp must reproduce the stretch's bits"


def test_emulated_entry_refuses_the_same_descriptors_and_clamps_out_lens(emu):
    from chatterbox_amd import ops
    _descriptor_errors(emu)
    mel = S.log_mel((1, 8, 80), seed=5)
    buf = torch.full((2, 4, 80), 777.0)
    tab, ints, off = torch.tensor([0.0, 1.25], dtype=torch.float64), torch.tensor([0, 8, 6], dtype=torch.int32), (ctypes.c_int * 2)(0, 1)   # out_lens 6 > T_out 4
    assert emu.cbx_mel_time_warp_f32(mel.data_ptr(), 640, 80, 8, ints.data_ptr() + 4, ctypes.addressof(off), 1, ints.data_ptr(), tab.data_ptr(), tab.data_ptr() + 8,
                                     buf.data_ptr(), 320, 80, 4, ints.data_ptr() + 8, 1, 80, None) == 0
    assert np.abs(buf[0].double().numpy() - W.reference(mel[0].numpy(), 8, 4, [(0, 0.0, 1.25)])).max() <= 4 * S.U * float(mel.abs().max())
    assert bool((buf[1] == 777.0).all()), "out_lens > T_out must not overrun the output"
    out, ol = ops.mel_time_warp(mel, [[(0, 0.0, 1.0)]])            # in_lens None: every row has T_in frames; rate 1 is the identity map
    assert ol.tolist() == [8] and torch.equal(out, mel)
    for bad in (dict(tables=[[(0, 0.0, 1.0)]] * 2), dict(tables=[[]]), dict(tables=[[(0, 0.0, 1.0)]], in_lens=[9]),
                dict(tables=[[(0, 0.0, 0.5)]], out=torch.zeros(1, 15, 80))):
        with pytest.raises(ValueError, match="mel_time_warp"):
            ops.mel_time_warp(mel, **bad)


# ----------------------------------------------------------------------------- the public classes over recording engines (nothing is launched)
DURS = [1.0, None, None, 0.5, 3.21]   # (by length the plan pairs requests 1 + 2, which have none)


def _jobs(calls):
    return [j for kind, kw in calls for j in (kw["jobs"] if kind == "pipelined" else [kw])]


@pytest.mark.parametrize("cls_name,extra", [("ChatterboxTTS", 2), ("ChatterboxMultilingualTTS", 2), ("ChatterboxTurboTTS", 0)])
@pytest.mark.parametrize("max_batch", [None, 2])
def test_durations_follow_their_requests_through_the_batch_plan(cls_name, extra, max_batch):
    from chatterbox_amd import api
    eng = _FakeEngine() if cls_name != "ChatterboxTurboTTS" else _FakeSerialEngine()
    m = _tts(getattr(api, cls_name), eng)
    m.max_batch = max_batch
    texts = ["x" * (n - 1) + "." for n in LENS]
    args = (texts, "en") if cls_name == "ChatterboxMultilingualTTS" else (texts,)
    out = m.generate_batch(*args, duration=DURS, seeds=list(range(5)))
    assert [int(w[0, 0]) for w in out] == [n + extra for n in LENS], "waveforms come back in the caller's order"
    jobs = _jobs(eng.calls)
    assert [len(j["text_tokens"]) for j in jobs] == ([4, 1] if max_batch is None else [2, 2, 1])
    warp_of_len = {n + extra: (None if d is None else dict(frames=int(math.floor(50 * d + 0.5)))) for n, d in zip(LENS, DURS)}
    for j in jobs:
        want = [warp_of_len[int(t.numel())] for t in j["text_tokens"]]
        assert j.get("warp") == (None if all(w is None for w in want) else want), "a sub-batch carries warp only when one of ITS requests uses it, in its row order"
        assert "words" not in j and "speed" not in j
    if max_batch == 2:
        assert sum("warp" in j for j in jobs) == 2 and any("warp" not in j for j in jobs)
    assert m.last_fit == [None] * 5, "(the recording engine reports no fit)"
    plain = _FakeEngine() if cls_name != "ChatterboxTurboTTS" else _FakeSerialEngine()
    p = _tts(getattr(api, cls_name), plain)
    p.max_batch = max_batch
    p.generate_batch(*args, seeds=list(range(5)))
    for none in (None, [None] * 5):
        eng.calls.clear()
        m.generate_batch(*args, seeds=list(range(5)), duration=none)   # nothing warped: exactly the recorded keywords of a call without the argument
        assert str(eng.calls) == str(plain.calls) and _sub_batches(eng.calls)
    eng.calls.clear()
    m.generate_batch(*args, duration=2.0)   # a number: the same length for every request
    assert all(j["warp"] == [dict(frames=100)] * len(j["text_tokens"]) for j in _jobs(eng.calls))


@pytest.mark.parametrize("cls_name", ["ChatterboxTTS", "ChatterboxMultilingualTTS", "ChatterboxTurboTTS"])
def test_duration_arguments_are_validated_before_the_engine_is_called(cls_name):
    from chatterbox_amd import api
    eng = _FakeEngine()
    m = _tts(getattr(api, cls_name), eng)
    texts = ["aaaa.", "bb.", "cccccc."]
    lang = ("en",) if cls_name == "ChatterboxMultilingualTTS" else ()
    blang = (["en"] * 3,) if lang else ()
    bad = ((True, TypeError), ("1", TypeError), (float("nan"), ValueError), (0.01, ValueError), (80.5, ValueError))
    for v, err in bad + (([1.0, 1.2], ValueError), ([1.0, 1.2, 0.9, 1.0], ValueError), ([1.0, "1", 1.0], TypeError)):
        with pytest.raises(err, match="duration"):
            m.generate_batch(texts, *blang, duration=v)
    for v, err in bad + (([1.0], TypeError),):
        with pytest.raises(err, match="duration"):
            m.generate("aaaa.", *lang, duration=v)
    for other in (dict(speed=1.25), dict(pitch=2.0), dict(max_pause=0.2)):
        with pytest.raises(ValueError, match=rf"duration together with {list(other)[0]}"):
            m.generate("aaaa.", *lang, duration=1.0, **other)
        with pytest.raises(ValueError, match=rf"duration together with {list(other)[0]}"):
            m.generate_batch(texts, *blang, duration=[1.0, None, None], **other)
    if cls_name == "ChatterboxTurboTTS":
        with pytest.raises(TypeError, match="timing"):
            m.generate("aaaa.", timing=[0.1])
    for meth in ("generate_long", "generate_stream"):
        with pytest.raises(TypeError, match="duration"):
            getattr(m, meth)("aaaa.", *lang, duration=1.0)
    assert eng.calls == []
    m.generate("aaaa.", *lang, duration=1.25, seed=3)
    assert eng.calls[-1][0] == "synthesize" and eng.calls[-1][1]["warp"] == [dict(frames=63)] and eng.calls[-1][1]["seeds"] == [3], "floor(62.5 + 0.5), not round()"
    m.generate("aaaa.", *lang)
    assert "warp" not in eng.calls[-1][1], "without duration the engine call is exactly the one without the argument"


def test_vc_durations_follow_their_requests_and_are_validated():
    from chatterbox_amd import api, synth

    class Voc:
        def __init__(self):
            self.calls, self.last_fit = [], None

        def vocode(self, toks, refs, **kw):
            self.calls.append(([int(t.numel()) for t in toks], kw))
            w = kw.get("warp") or [None] * len(toks)
            self.last_fit = [None if x is None else dict(target=x["frames"], frames=min(x["frames"], 4 * t.numel()), rate=(1.0, 1.0),
                                                         clamped=["end"] if x["frames"] > 4 * t.numel() else [], table=[]) for x, t in zip(w, toks)]
            return [torch.full((2,), float(t.numel())) for t in toks], None

    vc = api.ChatterboxVC.__new__(api.ChatterboxVC)
    vc.engine, vc.device, vc.ref_dict, vc.analyzer, vc.watermarker = Voc(), CPU, synth.s3gen_ref(n_prompt_tokens=8), None, None
    vc.MAX_BATCH = 2
    toks = [synth.speech_tokens(n) for n in (30, 10, 20)]
    for v, err in (([1.0, 1.2], ValueError), (100.0, ValueError), ([1.0, 1.0, "1"], TypeError), (True, TypeError)):
        with pytest.raises(err, match="duration"):
            vc.generate_batch(s3_tokens=toks, duration=v)
    with pytest.raises(ValueError, match="duration together with speed"):
        vc.generate(s3_tokens=toks[0], duration=1.0, speed=1.25)
    with pytest.raises(TypeError, match="timing"):
        vc.generate(s3_tokens=toks[0], timing=[0.1])
    assert vc.engine.calls == []
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        out = vc.generate_batch(s3_tokens=toks, duration=[1.0, 0.5, None])
    assert [int(w[0, 0]) for w in out] == [30, 10, 20]
    assert [(l, kw.get("warp")) for l, kw in vc.engine.calls] == [([10, 20], [dict(frames=25), None]), ([30], [dict(frames=50)])]
    assert [None if f is None else f["target"] for f in vc.last_fit] == [50, 25, None], "last_fit is in the caller's order"
    vc.engine.calls.clear()
    with pytest.warns(UserWarning, match="request"):
        vc.generate(s3_tokens=toks[1], duration=1.5)     # 75 frames of 10 tokens: the stand-in reports a clamp
    assert vc.last_fit[0]["clamped"] == ["end"]
    vc.generate(s3_tokens=toks[1])
    assert vc.engine.calls[0][1] == dict(warp=[dict(frames=75)]) and vc.engine.calls[1][1] == {}


def test_timing_runs_serially_with_words_and_maps_words_to_their_first_tokens():
    m = _model()
    assert m.words("Hi yo, a.") == ["Hi", "yo,", "a."]
    wav = m.generate("Hi yo, a.", seed=3, timing=[None, 0.3, 0.51], duration=1.0)
    assert torch.is_tensor(wav), "timing alone does not change what the call returns"
    kind, kw = m.engine.calls[-1]
    # engine tokens: [START] H i _ y o , _ a . [STOP]; the words begin at tokens 1, 4 and 8
    assert kind == "synthesize" and kw["words"] == dict(heads=None)
    assert kw["warp"] == [dict(starts=[None, None, None, None, 15, None, None, None, 26, None, None], end=50)]
    m.generate("Hi yo, a.", seed=3, timing=[0.0, None, None])
    assert m.engine.calls[-1][1]["warp"] == [dict(starts=[None, 0] + [None] * 9, end=None)]
    n = len(m.engine.calls)
    for bad in ([0.1, 0.2], [0.1, 0.2, 0.3, 0.4], []):
        with pytest.raises(ValueError, match=r"timing: \d entries for 3 words"):
            m.generate("Hi yo, a.", timing=bad)
    for bad, err in (([0.3, 0.2, 0.4], ValueError), ([0.1, "x", 0.3], TypeError), (0.5, TypeError), ([0.1, 0.2, 90.0], ValueError)):
        with pytest.raises(err, match="timing"):
            m.generate("Hi yo, a.", timing=bad)
    for other in (dict(speed=1.25), dict(pitch=2.0), dict(max_pause=0.2)):
        with pytest.raises(ValueError, match=rf"timing together with {list(other)[0]}"):
            m.generate("Hi yo, a.", timing=[None, 0.3, 0.5], **other)
    assert len(m.engine.calls) == n, "a refused call never reaches the engine"
    m.generate("Hi yo, a.", seed=3, timing=[None, None, None])
    assert "warp" not in m.engine.calls[-1][1] and "words" not in m.engine.calls[-1][1], "no entry with a time: the call without the argument"
    with pytest.raises(ValueError, match=r"timing: 2 entries for 3 words"):
        m.generate("Hi yo, a.", timing=[None, None])
    bare = _tts(type(m), _WordsEngine())   # test_seeded_rng_host's tokenizer: no pieces
    with pytest.raises(ValueError, match="pieces"):
        bare.generate("Hi.", timing=[0.1])
    with pytest.raises(ValueError, match="pieces"):
        bare.words("Hi.")


def test_batch_timing_runs_the_serial_schedule_and_follows_its_requests():
    m = _model("ChatterboxMultilingualTTS")
    m.max_batch = 2
    texts = ["Hi yo, a.", "A.", "Hi yo."]
    assert m.words(texts[2], "en") == ["Hi", "yo."]
    out = m.generate_batch(texts, "en", seeds=[1, 2, 3], timing=[[None, 0.3, 0.5], None, [None, 0.2]], duration=[None, 1.0, None])
    assert all(torch.is_tensor(w) for w in out)
    assert [k for k, _ in m.engine.calls] == ["synthesize", "synthesize"], "timing implies the alignment pass: the sub-batches run the serial schedule"
    by_len = {}
    for _, kw in m.engine.calls:
        assert kw["words"] == dict(heads=None)
        for t, w in zip(kw["text_tokens"], kw["warp"]):
            by_len[int(t.numel())] = w
    assert by_len == {11: dict(starts=[None, None, None, None, 15, None, None, None, 25, None, None], end=None), 4: dict(frames=50),
                      8: dict(starts=[None, None, None, None, 10, None, None, None], end=None)}
    with pytest.raises(ValueError, match=r"timing\[2\]: 3 entries for 2 words"):
        m.generate_batch(texts, "en", timing=[None, None, [0.1, 0.2, 0.3]])
    assert len(m.engine.calls) == 2


def test_words_of_a_warped_utterance_go_through_the_time_map():
    """With timing= and word_times= in one call the returned words are the achieved ones: the alignment entry carries the row's table, and a boundary at token
    frame f lies at ops.warp_place(table, 2 f) * 480 -- exactly the target at an anchor."""
    from chatterbox_amd import ops

    class Eng(_WordsEngine):
        last_fit = None

        def synthesize(self, text_tokens, t3_conds, gen_ref, **kw):
            wavs, st, al = super().synthesize(text_tokens, t3_conds, gen_ref, **kw)
            self.last_fit = []
            for a, w, t in zip(al, kw["warp"], text_tokens):
                K = 4 * t.numel()
                p = ops.warp_plan(K, [(2 * f[0], s) for f, s in zip(a["frames"], w["starts"]) if s is not None], end=w["end"])
                a["table"] = p["table"]
                self.last_fit.append(dict(target=w["end"], frames=p["frames"], rate=(0.5, 2.0), clamped=p["clamped"], achieved=p["achieved"], table=p["table"]))
            return [torch.zeros(480 * f["frames"]) for f in self.last_fit], st, al

    m = _model(engine=Eng())
    # tokens [START] H i _ y o . [STOP]: "Hi" begins at token 1 = frame 2 = mel frame 4, "yo." at token 4 = frame 8 = mel frame 16
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        wav, words = m.generate("Hi yo.", seed=3, timing=[0.1, 0.5], word_times=True, duration=1.0)
    assert wav.shape[-1] == 50 * 480 and m.last_fit[0]["clamped"] == [] and m.last_fit[0]["achieved"] == [5, 25]
    assert [w["text"] for w in words] == ["Hi", "yo."] and [w["start"] for w in words] == [5 * 480, 25 * 480] and words[0]["stop"] == 25 * 480
    assert words[1]["stop"] == int(math.floor(ops.warp_place(m.last_fit[0]["table"], 28) * 480 + 0.5)) <= 50 * 480
    with pytest.warns(UserWarning, match="clamped"):
        wav, words = m.generate("Hi yo.", seed=3, timing=[0.02, 0.04], word_times=True)
    assert m.last_fit[0]["clamped"] == [0, 1] and [w["start"] for w in words] == [2 * 480, 8 * 480], "4 frames in at least 2, 12 more in at least 6"


# ----------------------------------------------------------------------------- ChatterboxEngine.vocode over stand-in stages
def test_vocode_warp_rule_on_a_recording_engine(monkeypatch):
    """ChatterboxEngine.vocode over stand-in stages on the CPU: with warp= the flow's mel goes through ONE ops.mel_time_warp call (and no ops.mel_time_scale call)
    over M_b = 2 n_b - short_b frames -- warped rows by ops.warp_plan over K_b, plain rows by the rate-1 table over M_b --, the vocoder gets the warped mel with
    lens = frames, the returned mel is the flow's, row b's waveform is frames_b * 480 samples, and last_fit says what was planned -- also with the last token
    dropped.  warp=None and all-None make no such call."""
    from chatterbox_amd import engine, ops, synth
    eng = engine.ChatterboxEngine.__new__(engine.ChatterboxEngine)
    eng.dev, eng.last_timing, seen = CPU, {}, {}
    eng.flow = type("Flow", (), {"precision": 1, "inference": lambda self, tok, lens, ref, **kw: torch.ones(tok.shape[0], 2 * tok.shape[1], 80)})()

    def hift_inference(mel, lens=None, **kw):
        seen.update(mel=mel, lens=lens)
        return torch.zeros(mel.shape[0], 480 * mel.shape[1]), None
    eng.hift = type("Hift", (), {"precision": 1, "inference": staticmethod(hift_inference)})()
    calls = []

    def fake_warp(mel, tables, in_lens=None, out=None, out_lens=None):
        calls.append((tuple(mel.shape), [list(t) for t in tables], list(in_lens), list(out_lens)))
        return torch.zeros(mel.shape[0], max(out_lens), 80), torch.tensor(out_lens, dtype=torch.int32)

    def no_scale(*a, **k):
        raise AssertionError("vocode(warp=) must not call ops.mel_time_scale")
    monkeypatch.setattr(ops, "mel_time_warp", fake_warp)
    monkeypatch.setattr(ops, "mel_time_scale", no_scale)
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: None)
    ref = synth.s3gen_ref(n_prompt_tokens=6)
    st = [synth.speech_tokens(n, seed=k) for k, n in enumerate((12, 5, 9))]
    for drop in (False, True):
        base, mel0 = eng.vocode(st, ref, drop_last_token=drop)
        assert calls == [] and seen["mel"] is mel0 and eng.last_fit is None
        same, _ = eng.vocode(st, ref, drop_last_token=drop, warp=[None, None, None])
        assert calls == [] and [w.numel() for w in same] == [w.numel() for w in base]
        K = [w.numel() // 480 for w in base]
        assert K == ([22, 8, 16] if drop else [24, 10, 18])
        # row 0: a duration that fits (rate K / 30); row 1: plain; row 2: anchors (4 -> 6, 10 -> 9), one beyond K cut to K (which closes the plan: the end at 30 is missed)
        warp = [dict(frames=30), None, dict(anchors=[(4, 6), (10, 9), (40, 20)], end=30)]
        wavs, mel = eng.vocode(st, ref, drop_last_token=drop, warp=warp)
        p2 = ops.warp_plan(K[2], [(4, 6), (10, 9), (K[2], 20)], end=30)
        assert p2["frames"] == 20 and p2["clamped"] == ["end"], "an anchor at the row's end closes the plan"
        assert calls == [((3, 24, 80), [[(0, 0.0, K[0] / 30)], [(0, 0.0, 1.0)], p2["table"]], [24, 10, 18], [30, 10, 20])] and mel.shape == (3, 24, 80)
        assert seen["mel"].shape == (3, 30, 80) and seen["lens"].tolist() == [30, 10, 20]
        assert [w.numel() for w in wavs] == [480 * 30, 480 * K[1], 480 * 20], "the plain row keeps the length of the call without warp"
        fit = eng.last_fit
        assert fit[1] is None and fit[0] == dict(target=30, frames=30, rate=(K[0] / 30, K[0] / 30), clamped=[], table=[(0, 0.0, K[0] / 30)])
        assert fit[2]["target"] == 30 and fit[2]["frames"] == 20 and fit[2]["achieved"] == [6, 9, 20] and fit[2]["clamped"] == ["end"] and fit[2]["table"] == p2["table"]
        calls.clear()
        wavs, _ = eng.vocode(st, ref, drop_last_token=drop, warp=[dict(frames=3), None, dict(frames=100)])   # both clamps: ceil(K / 2) and 2 K frames
        assert [w.numel() // 480 for w in wavs] == [K[0] // 2, K[1], 2 * K[2]] and [f and f["clamped"] for f in eng.last_fit] == [["end"], None, ["end"]]
        assert eng.last_fit[0]["rate"] == (2.0, 2.0) and eng.last_fit[2]["rate"] == (0.5, 0.5)
        calls.clear()
        for other in (dict(speed=1.25), dict(pitch=1.0), dict(pauses=[3, 3, 3])):
            with pytest.raises(ValueError, match="warp"):
                eng.vocode(st, ref, drop_last_token=drop, warp=warp, **other)
        assert calls == []
