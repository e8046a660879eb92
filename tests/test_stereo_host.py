"""Host tests (no GPU) of stereo dialogue: the three entries of wave_stereo.hip on the SIMT emulator against the restatements of stereo_common.py (the pan mix
bit for bit), their refusals on the product library and on the emulator, ops.pan_gains / ops.check_pan, the pan= argument of generate_dialogue over the
recording engines of the dialogue host tests (nothing is launched), and pan=None as the call without the argument."""
import ctypes
import inspect
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

import stereo_common as S  # noqa: E402
from test_wave_join_host import KINDS, _jobs  # noqa: E402  (read-only import)
from test_wave_mix_host import SCRIPT, STARTS, TOTAL, _lang_kw, _Mark, _model, _norm, _record, _voices  # noqa: E402  (read-only import: the recording engines)

CPU = torch.device("cpu")
ENTRIES = {"cbx_wave_pan_mix_f32": 17, "cbx_wave_loudness_ch_f32": 14, "cbx_wave_limit_ch_f32": 19}


# ----------------------------------------------------------------------------- C ABI
def test_the_entries_are_declared_exported_bound_emulated_and_documented_without_a_version_step():
    from chatterbox_amd import _lib, ops
    import harness
    hdr = open(os.path.join(ROOT, "include", "cbx.h")).read()
    lib = ctypes.CDLL(os.path.join(ROOT, "chatterbox_amd", "libcbx_hip.so"))
    emu = harness.load_emu()
    for entry, nargs in ENTRIES.items():
        assert re.search(rf"^int {entry}\(", hdr, re.M) and hasattr(lib, entry) and entry in _lib._SIGS and hasattr(emu, entry), entry
        assert len(_lib._SIGS[entry][0]) == len(re.search(rf"^int {entry}\((.*?)\);", hdr, re.M | re.S).group(1).split(",")) == nargs, entry
    assert "#define CBX_ABI_VERSION 16" in hdr and _lib.lib.cbx_abi_version() == 16 and _lib.ABI_VERSION == 16, "new functions only: no version step"
    block = hdr[hdr.index("---- stereo dialogue"): hdr.index("---- music bed")]
    assert "ASCENDING r" in block and "one rounded multiply per plane" in block and "e_s = E_(0,s) + E_(1,s)" in block and "maximum over the channels" in block
    assert all(s in block for s in ("cbx_wave_mix_f32's bits in both planes", "L == R bit for bit", "plane of zeros", "C = 1 is cbx_wave_loudness_f32 bit for bit",
                                    "C = 1 is cbx_wave_limit_f32 bit for bit", "lowers the other by the same g", "-22 before any launch, nothing written"))
    src = open(os.path.join(ROOT, "chatterbox_amd", "csrc", "wave_stereo.hip")).read()
    assert "tts.py:272" in src and "__global__" not in src and "atomic" not in src, "the three entries hold no kernel of their own"
    assert f"WM_TILE = {ops.WAVE_MIX_TILE}" in open(os.path.join(ROOT, "chatterbox_amd", "csrc", "wave_mix.hip")).read(), "the one mixer kernel's tile"
    for doc, words in (("README.md", ("pan=",)), ("DESIGN.md", ("DIALOGUE_PAN_SPREAD", "cbx_wave_limit_ch_f32")), ("INTEGRATION.md", tuple(ENTRIES))):
        text = open(os.path.join(ROOT, doc)).read()
        assert all(w in text for w in words), doc
    assert all(callable(getattr(ops, n)) for n in ("wave_pan_mix", "wave_loudness_ch", "wave_limit_ch", "pan_gains", "check_pan"))


def test_the_product_library_refuses_bad_descriptors_before_any_launch():
    from chatterbox_amd import _lib, ops
    S.check_pan_refusals(_lib.lib, ops, CPU, None, run_good=False)
    S.check_loud_refusals(_lib.lib, ops, CPU, None, run_good=False)
    S.check_limit_refusals(_lib.lib, ops, CPU, None, run_good=False)


# ----------------------------------------------------------------------------- the kernels on the SIMT emulator
@pytest.fixture(scope="module")
def emu():
    import build_emu
    if not os.path.exists(build_emu.CLANG):
        pytest.skip("ROCm's clang++ (x86 host compiler of the emulator build) is not installed")
    import harness
    with harness.emulated() as lib:
        yield lib


@pytest.mark.parametrize("check", ["pan_mix", "loudness_ch", "limit_ch"])
def test_a_kernel_against_its_restatement(emu, check):
    from chatterbox_amd import ops
    getattr(S, f"check_{check}")(ops)


@pytest.mark.parametrize("check", ["pan", "loud", "limit"])
def test_the_emulated_entry_refuses_the_same_descriptors_and_runs_the_good_one(emu, check):
    from chatterbox_amd import ops
    getattr(S, f"check_{check}_refusals")(emu, ops, CPU, None)


def test_the_wrappers_check_their_arguments(emu):
    from chatterbox_amd import ops
    x = torch.from_numpy(S.M.noise(100, 1))
    out = torch.full((2, 120), 7.0)
    assert ops.wave_pan_mix([x[:0]], [5], [0], [(1.0, 1.0)], out) is out and float(out.abs().max()) == 0.0, "empty rows alone: zeros, no launch"
    with pytest.raises(ValueError, match="pan pairs"):
        ops.wave_pan_mix([x[:50], x[50:]], [0, 60], [0, 0], [(1.0, 1.0)], out)
    with pytest.raises(Exception, match="wave_pan_mix"):
        ops.wave_pan_mix([x[:50]], [0], [0], [(1.0, float("nan"))], out)
    with pytest.raises(ValueError, match="channels"):
        ops.wave_loudness_ch([x[:50], x[50:]], channels=3)
    with pytest.raises(ValueError, match="whole number"):
        ops.wave_limit_ch([x[:50]], -1.0)
    with pytest.raises(ValueError, match="different lengths"):
        ops.wave_loudness_ch([x[:50], x[50:99]])
    with pytest.raises(ValueError, match="targets"):
        ops.wave_loudness_ch([x[:50], x[50:]], [-23.0, -23.0])


# ----------------------------------------------------------------------------- the pan law
def test_pan_gains_end_points_centre_and_power():
    from chatterbox_amd import ops
    assert ops.pan_gains(-1) == (1.0, 0.0) and ops.pan_gains(1.0) == (0.0, 1.0), "the end points are exact by construction"
    l, r = ops.pan_gains(0)
    assert l == r == float(np.float32(np.sqrt(0.5)))
    for p in (-0.9, -0.3, 0.1, 0.3, 0.75):
        l, r = ops.pan_gains(p)
        th = (p + 1.0) * np.pi / 4.0
        assert l == float(np.float32(np.cos(th))) and r == float(np.float32(np.sin(th))), "fp64, rounded to fp32 once"
        assert abs(l * l + r * r - 1.0) < 2e-7 and (l > r) == (p < 0)
        assert ops.pan_gains(-p) == (r, l) or abs(ops.pan_gains(-p)[0] - r) < 1e-7
    assert inspect.signature(ops.wave_mix).parameters.keys() == {"rows", "starts", "flags", "out", "gain", "gain_idx", "fade", "accumulate"}, "the existing wrappers keep their signatures"


def test_check_pan():
    from chatterbox_amd import ops
    assert ops.check_pan(0) == 0.0 and ops.check_pan(-1) == -1.0 and ops.check_pan(0.25) == 0.25
    for bad, err in ((True, TypeError), ("0", TypeError), (None, TypeError), ([0.0], TypeError), (1.01, ValueError), (-2, ValueError), (float("nan"), ValueError),
                     (float("inf"), ValueError)):
        with pytest.raises(err, match="pan"):
            ops.check_pan(bad)
        with pytest.raises(err):
            ops.pan_gains(bad)


# ----------------------------------------------------------------------------- generate_dialogue(pan=) over the recording engines (nothing is launched)
def _record_stereo(monkeypatch, log):
    from chatterbox_amd import ops
    _record(monkeypatch, log)

    def pan_mix(rows, starts, flags, pan, out, gain=None, gain_idx=None, fade=240, accumulate=False):
        log.append(("pan_mix", dict(n=[int(r.numel()) for r in rows], starts=list(starts), flags=list(flags), pan=[tuple(p) for p in pan], gain=gain, gain_idx=gain_idx,
                                    fade=fade, accumulate=accumulate)))
        res = S.pan_oracle([r.numpy() for r in rows], starts, flags, pan, out.shape[1], None if gain is None else gain.tolist(), gain_idx, fade,
                           prev=out.numpy().copy() if accumulate else None)
        return out.copy_(torch.from_numpy(res))

    def loudness_ch(rows, target=None, ceiling=1.0, fs=24000, channels=2):
        log.append(("loudness_ch", [r.clone() for r in rows], target, ceiling, channels))
        return torch.tensor([[-30.0, 0.5, 2.0, 9.0]], dtype=torch.float64), torch.tensor([2.0])

    def limit_ch(rows, ceilings_db, gain=None, look=120, out=None, channels=2):
        log.append(("limit_ch", [r.clone() for r in rows], ceilings_db, gain, channels))
        for o, r in zip(out, rows):
            o.copy_(r * 0.5)
        return out, "limit stats"
    monkeypatch.setattr(ops, "wave_pan_mix", pan_mix)
    monkeypatch.setattr(ops, "wave_loudness_ch", loudness_ch)
    monkeypatch.setattr(ops, "wave_limit_ch", limit_ch)
    monkeypatch.setattr(ops, "wave_gain", lambda rows, gain: log.append(("gain", [r.clone() for r in rows], gain)) or rows)
    monkeypatch.setattr(ops, "wave_format", lambda rows, fmt: log.append(("format", [r.clone() for r in rows], fmt)) or [torch.zeros(3, dtype=torch.int16) for _ in rows])


@pytest.mark.parametrize("cls_name,extra,lang", KINDS)
def test_pan_places_the_voices_and_the_finish_is_one_visit_over_two_planes(cls_name, extra, lang, monkeypatch):
    from chatterbox_amd import api, ops
    m, eng = _model(cls_name)
    voices = _voices()
    log = []
    _record_stereo(monkeypatch, log)
    mono = m.generate_dialogue(SCRIPT, voices, **_lang_kw(lang), max_chars=14, seed=11)
    assert m.last_pan is None and mono.shape == (1, TOTAL)
    log.clear()
    wav, seg = m.generate_dialogue(SCRIPT, voices, **_lang_kw(lang), max_chars=14, seed=11, pan={"a": -1, "b": 0.5}, return_segments=True)
    assert [e[0] for e in log] == ["pan_mix"] and log[0][1]["starts"] == STARTS and log[0][1]["accumulate"] is False and log[0][1]["gain"] is None
    ga, gb, g0 = ops.pan_gains(-1), ops.pan_gains(0.5), ops.pan_gains(0)
    assert log[0][1]["pan"] == [ga, ga, gb, ga, g0], "a voice not named sits at 0"
    assert wav.shape == (2, TOTAL) and wav.dtype == torch.float32
    assert [(s["start"], s["stop"]) for s in seg] == [(a, a + 3840) for a in STARTS], "per-channel sample positions: the mono call's numbers"
    assert not wav[1, : STARTS[2]].any() and torch.equal(wav[0, :3840], mono[0, :3840]), "voice a is hard left: the right plane is silent where only a speaks"
    assert m.last_pan == [dict(voice="a", position=-1.0, left=1.0, right=0.0), dict(voice="b", position=0.5, left=gb[0], right=gb[1]),
                          dict(voice=None, position=0.0, left=g0[0], right=g0[1])]
    # pan=True: three voices spread over [-0.3, 0.3] in order of first appearance; a turn's own pan= overrides its voice's place
    log.clear()
    script = SCRIPT[:3] + [dict(voice=None, text="Kk llll mmmm.", pan=0.9)]
    m.generate_dialogue(script, voices, **_lang_kw(lang), max_chars=14, seed=11, pan=True)
    assert [p["position"] for p in m.last_pan] == [-api.DIALOGUE_PAN_SPREAD, 0.0, api.DIALOGUE_PAN_SPREAD] and api.DIALOGUE_PAN_SPREAD == 0.3
    assert log[0][1]["pan"] == [ops.pan_gains(-0.3)] * 2 + [ops.pan_gains(0.0), ops.pan_gains(-0.3), ops.pan_gains(0.9)]
    m.generate_dialogue([("a", "Aaaa.")], voices, **_lang_kw(lang), pan=True)
    assert [p["position"] for p in m.last_pan] == [0.0], "one voice sits at 0"
    # the whole finish: balance over the mono rows, pan mix, the two-channel meter, the linked limiter, the watermark per channel, one format call, one copy
    log.clear()
    m.watermarker = _Mark(log)
    wav = m.generate_dialogue(SCRIPT, voices, **_lang_kw(lang), max_chars=14, seed=11, balance=-20, loudness=-19, true_peak=-1.5, encoding="s16", pan=True)
    assert [e[0] for e in log] == ["loudness", "pan_mix", "loudness_ch", "limit_ch", "watermark", "watermark", "format"]
    assert log[0][2] == [-20.0] * 3 and log[1][1]["gain_idx"] == [0, 0, 1, 0, 2], "balance= meters each voice's MONO rows, unchanged"
    assert log[2][2] == [-19.0] and log[2][3] is None and log[2][4] == 2 and len(log[2][1]) == 2, "the two planes as ONE signal; the full gain where the limiter follows"
    assert log[3][2] == [-1.5] and torch.equal(log[3][3], torch.tensor([2.0])) and log[3][4] == 2
    assert len(log[6][1]) == 2 and log[6][1][0].numel() == TOTAL and wav.shape == (2, 3) and wav.dtype == torch.int16 and eng.last_limit == "limit stats"
    assert all(not {"loudness", "true_peak", "format"} & set(j) for j in _jobs(eng.calls))
    log.clear()
    m.watermarker = None
    wav = m.generate_dialogue(SCRIPT, voices, **_lang_kw(lang), max_chars=14, loudness=-19, pan=True)
    assert [e[0] for e in log] == ["pan_mix", "loudness_ch", "gain"] and log[1][3] == 1.0, "no ceiling: the gain is limited to a sample peak of 1.0 over both channels"
    assert torch.equal(log[2][2], torch.tensor([2.0, 2.0])) and wav.shape == (2, TOTAL)


def test_a_stereo_script_of_more_than_64_chunks_is_mixed_in_launches_of_64(monkeypatch):
    m, eng = _model("ChatterboxTTS", max_batch=4)
    log = []
    _record_stereo(monkeypatch, log)
    wav = m.generate_dialogue([(None, "Aa.")] * 70, turn_pause=0.0, pan=True)
    assert [(e[1]["accumulate"], len(e[1]["n"])) for e in log] == [(False, 64), (True, 6)] and wav.shape == (2, 70 * 3840)
    assert torch.equal(wav[0], wav[1]) and float(wav[0, 64 * 3840 + 1000]) == float(np.float32(5.0) * np.float32(np.sqrt(0.5)))


@pytest.mark.parametrize("cls_name,extra,lang", KINDS)
def test_bad_pan_arguments_raise_at_the_call_before_the_engine_is_touched(cls_name, extra, lang, monkeypatch):
    from chatterbox_amd import api
    m, eng = _model(cls_name)
    voices = _voices()
    monkeypatch.setattr(m, "_analyse", lambda *a, **k: pytest.fail("the voice analysis is not touched"))
    bad = [(dict(pan={"a": 1.5}), ValueError, "pan"), (dict(pan={"a": float("nan")}), ValueError, "pan"), (dict(pan={"a": True}), TypeError, "pan"),
           (dict(pan={"a": "left"}), TypeError, "pan"), (dict(pan={"zz": 0.0}), ValueError, "zz"), (dict(pan={"b": 0.0}), ValueError, "b"), (dict(pan=0.5), TypeError, "pan"),
           (dict(pan=[0.0]), TypeError, "pan"), (dict(pan="wide"), TypeError, "pan"),
           (dict(turns=[dict(voice="a", text="x.", pan=2)], pan=True), ValueError, "pan"), (dict(turns=[dict(voice="a", text="x.", pan=False)], pan=True), TypeError, "pan"),
           (dict(turns=[dict(voice="a", text="x.", pan=0.5)]), ValueError, "stereo call")]
    for over, err, match in bad:
        kw = dict(dict(turns=[("a", "Aaaa.")]), **_lang_kw(lang), **over)
        with pytest.raises(err, match=match):
            m.generate_dialogue(kw.pop("turns"), voices, **kw)
    with pytest.raises(ValueError, match=r"bed=.*pan="):
        m.generate_dialogue([("a", "Aaaa.")], voices, **_lang_kw(lang), pan=True, bed=(torch.zeros(24000), 24000))
    assert eng.calls == []
    for cls in (api.ChatterboxTTS, api.ChatterboxMultilingualTTS, api.ChatterboxTurboTTS):
        sig = inspect.signature(cls.generate_dialogue).parameters
        assert sig["pan"].default is None and sig["pan"].kind is inspect.Parameter.KEYWORD_ONLY
        assert all("pan" not in inspect.signature(getattr(cls, n)).parameters for n in ("generate", "generate_batch", "generate_long", "generate_long_stream", "generate_stream"))
    assert "UNMEASURED" in api.ChatterboxTTS.generate_dialogue.__doc__ and "DIALOGUE_PAN_SPREAD" in api.ChatterboxTTS.generate_dialogue.__doc__


@pytest.mark.parametrize("cls_name,extra,lang", KINDS)
def test_pan_none_records_the_engine_and_device_calls_of_the_call_without_the_argument(cls_name, extra, lang, monkeypatch):
    m, eng = _model(cls_name)
    log = []
    _record_stereo(monkeypatch, log)

    def run(**kw):
        eng.calls.clear()
        log.clear()
        wav = m.generate_dialogue(SCRIPT, _voices(), **_lang_kw(lang), max_chars=14, seed=5, balance=True, loudness=-19, true_peak=-1.5, encoding="s16", **kw)
        return _norm(eng.calls), _norm([(e[0],) + tuple(e[1:4]) for e in log]), wav
    calls, steps, wav = run()
    calls_n, steps_n, wav_n = run(pan=None)
    assert calls == calls_n and steps == steps_n and torch.equal(wav, wav_n) and wav_n.shape[0] == 1 and m.last_pan is None
    assert [s[0] for s in steps] == ["loudness", "mix", "loudness", "limit", "format"], "the mono finish, launch for launch"
    calls_s, steps_s, _ = run(pan=True)
    assert calls_s == calls, "pan= changes the finish alone: the engines see the same jobs"
