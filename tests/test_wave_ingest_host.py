"""CPU (-m "not gpu"): audio in -- the filter design of any pair of rates against scipy.signal.firwin, the fp64 restatement against scipy.signal.resample_poly, the
G.711 expansion against the committed encode tables, cbx_wave_ingest and cbx_wave_trim_edges_f32 on the SIMT emulator against the oracle (wave_ingest_common.py:
decode and mixdown exactness, the bound, lengths, alignments and paddings, sentinels, refusals), their C ABI, the RIFF reader against scipy.io.wavfile and load_wav,
ops.check_audio_in, the trim rule against frontend.trim_silence, and the plumbing of the raw input form and of `audio_in` through the four public classes over the
recording engines of test_seeded_rng_host.py (read-only import; nothing is launched there)."""
import ctypes
import os
import re
import struct
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, os.path.join(HERE, "simt")):
    if p not in sys.path:
        sys.path.insert(0, p)

import wave_ingest_common as C  # noqa: E402
from test_seeded_rng_host import _FakeSerialEngine, _tts  # noqa: E402  (read-only import: the recording engines)

CPU = torch.device("cpu")
RESAMPLED = [p for p in C.PAIRS if p[0] != p[1]]


# ----------------------------------------------------------------------------- the definition
@pytest.mark.parametrize("rate_in,rate_out", RESAMPLED)
def test_the_design_of_a_pair_is_scipys_and_the_table_is_its_phases(rate_in, rate_out):
    """fp64, as test_wave_format_host.py argues: 1e-13 of the largest tap is orders above the roundings of either evaluation and six below the table's fp32"""
    from chatterbox_amd import ops
    U, D, hl, h = C.scipy_design(rate_in, rate_out)
    f = ops.resample_filter(rate_in, rate_out)
    assert (f["U"], f["D"], f["hl"]) == (U, D, hl) and f["T"] == -(-(2 * hl + 1) // U) == C.taps(rate_in, rate_out)
    assert f["h"].dtype == np.float64 and f["h"].shape == h.shape and np.abs(f["h"] - h).max() <= 1e-13 * np.abs(h).max()
    tab = f["tab"]
    assert tab.dtype == np.float32 and tab.shape == (U, f["T"]) and tab.flags["C_CONTIGUOUS"]
    i = np.arange(U)[:, None] + U * np.arange(f["T"])[None, :]
    assert np.array_equal(tab, np.where(i <= 2 * hl, f["h"][np.minimum(i, 2 * hl)], 0.0).astype(np.float32))
    assert ops.resampled_len(1931, rate_in, rate_out) == C.out_len(1931, rate_in, rate_out) and ops.resampled_len(0, rate_in, rate_out) == 0


def test_the_new_design_generalises_wave_filter_and_leaves_it_alone():
    from chatterbox_amd import ops
    for rate in ops.WAVE_RATES:
        a, b = ops.wave_filter(rate), ops.resample_filter(24000, rate)
        assert (a["U"], a["D"], a["hl"], a["T"]) == (b["U"], b["D"], b["hl"], b["T"]) and np.array_equal(a["tab"], b["tab"]) and np.array_equal(a["h"], b["h"])
    with pytest.raises(ValueError, match="sample_rate"):
        ops.wave_filter(11025)
    f = ops.resample_filter(16000, 16000)
    assert (f["U"], f["D"], f["hl"], f["T"]) == (1, 1, 0, 1) and ops.resampled_len(777, 16000, 16000) == 777


def test_every_rate_of_the_issue_fits_the_caps_and_others_are_refused_by_the_wrapper():
    from chatterbox_amd import ops
    hdr = open(os.path.join(ROOT, "include", "cbx.h")).read()
    assert f"#define CBX_WAVE_INGEST_MAX_SPAN {ops.WAVE_INGEST_MAX_SPAN}" in hdr and f"#define CBX_WAVE_INGEST_MAX_TAB {ops.WAVE_INGEST_MAX_TAB}" in hdr
    assert ops.WAVE_IN_RATES == C.IN_RATES
    spans, tabs = [], []
    for ri in C.IN_RATES:
        for ro in (16000, 24000):
            f = ops.resample_filter(ri, ro)
            spans.append(255 * f["D"] // f["U"] + f["T"] + 1), tabs.append(f["U"] * f["T"])
    assert max(spans) == 1652 <= ops.WAVE_INGEST_MAX_SPAN and max(tabs) == 640 * 21 <= ops.WAVE_INGEST_MAX_TAB
    for ri, ro in ((16001, 16000), (192000, 8000), (7919, 24000)):
        with pytest.raises(ValueError, match="no conversion"):
            ops.resample_filter(ri, ro)
    for ri, ro, err in ((True, 16000, TypeError), (44100.0, 16000, TypeError), (0, 16000, ValueError), (16000, -1, ValueError)):
        with pytest.raises(err, match="rate_"):
            ops.resample_filter(ri, ro)


@pytest.mark.parametrize("rate_in,rate_out", RESAMPLED)
def test_the_restatement_is_resample_poly(rate_in, rate_out):
    from scipy.signal import resample_poly
    from chatterbox_amd import ops
    U, D = C.ratio(rate_in, rate_out)
    for n in (1, 7, 479, 480, 1931):
        x = np.random.default_rng(n).uniform(-0.99, 0.99, n)
        y64 = resample_poly(x, U, D)
        for h in (None, ops.resample_filter(rate_in, rate_out)["h"]):   # scipy's design, and the product's
            y, S = C.restate(x, rate_in, rate_out, h)
            assert y.shape == y64.shape == (C.out_len(n, rate_in, rate_out),) and np.abs(y - y64).max() <= 1e-12, (rate_in, rate_out, n)
            assert np.all(S >= np.abs(y) - 1e-12)


def test_the_g711_expansion_is_pinned_against_the_committed_encode_tables():
    C.check_g711_expansion_is_pinned()


def test_mixdown_is_numpys_mean_up_to_seven_channels():
    """load_wav's data.mean(axis=1) bit for bit for C <= 7; at 8 NumPy sums pairwise and the rule of include/cbx.h is the definition"""
    from chatterbox_amd import frontend
    rng = np.random.default_rng(5)
    for ch in range(1, 8):
        data = rng.uniform(-1, 1, (4001, ch)).astype(np.float32)
        got = frontend.decode_pcm(data, "f32", ch)
        assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), data.mean(axis=1).astype(np.float32).view(np.uint32)), ch
    one = np.array([-0.0, 1.5, np.float32(1e-40)], np.float32)
    assert np.array_equal(frontend.decode_pcm(one, "f32", 1).view(np.uint32), one.view(np.uint32)), "one channel: the bits"


def test_the_cases_the_shapes_are_chosen_for_are_what_they_claim():
    C.what_the_sets_cover()


# ----------------------------------------------------------------------------- C ABI
def test_entry_points_are_declared_exported_and_bound():
    from chatterbox_amd import _lib, ops
    hdr = open(os.path.join(ROOT, "include", "cbx.h")).read()
    lib = ctypes.CDLL(os.path.join(ROOT, "chatterbox_amd", "libcbx_hip.so"))
    for name in ("cbx_wave_ingest", "cbx_wave_trim_edges_f32"):
        assert re.search(rf"^int {name}\(", hdr, re.M) and hasattr(lib, name) and name in _lib._SIGS
        assert len(_lib._SIGS[name][0]) == len(re.search(rf"^int {name}\((.*?)\);", hdr, re.M | re.S).group(1).split(","))
    assert "#define CBX_ABI_VERSION 16" in hdr and _lib.lib.cbx_abi_version() == 16 and _lib.ABI_VERSION == 16, "new functions only: no version step"
    src = open(os.path.join(ROOT, "chatterbox_amd", "csrc", "wave_ingest.hip")).read()
    assert "frontend.load_wav" in hdr and "frontend.load_wav" in src and "librosa.effects.trim" in src
    for k, enc in enumerate(ops.WAVE_IN_ENCODINGS):
        assert f"#define CBX_WAVE_IN_{enc.upper()} {k}" in hdr
    assert ops.WAVE_IN_ENCODINGS == C.ENCODINGS and ops.WAVE_IN_SAMPLE_BYTES == C.SAMPLE_BYTES
    assert callable(ops.wave_ingest) and callable(ops.wave_trim_edges) and callable(ops.check_audio_in) and callable(ops.resample_filter)


def test_descriptor_errors_return_a_status_and_a_message():
    """the product library on host buffers: every refusal comes before a launch"""
    from chatterbox_amd import _lib, ops
    C.check_refusals(_lib.lib, ops, CPU, None, run_good=False)
    z = torch.zeros(8)
    e = torch.zeros(2, dtype=torch.int32)
    ws = torch.zeros(4, dtype=torch.float64)
    off, ln, neg = (ctypes.c_long * 1)(0), (ctypes.c_int * 1)(8), (ctypes.c_int * 1)(-1)
    a = ctypes.addressof
    good = [z.data_ptr(), a(off), a(ln), 1, 0.01, e.data_ptr(), ws.data_ptr(), 4, None]
    for i, v in ((0, None), (1, None), (2, None), (5, None), (6, None), (3, 0), (3, 65), (2, a(neg)), (4, -1.0), (4, float("inf")), (4, float("nan")), (7, 0)):
        args = list(good)
        args[i] = v
        assert _lib.lib.cbx_wave_trim_edges_f32(*args) == -22 and b"wave_trim_edges" in _lib.lib.cbx_last_error(), (i, v)


# ----------------------------------------------------------------------------- the kernels on the SIMT emulator
@pytest.fixture(scope="module")
def emu():
    import build_emu
    if not os.path.exists(build_emu.CLANG):
        pytest.skip("ROCm's clang++ (x86 host compiler of the emulator build) is not installed")
    import harness
    with harness.emulated() as lib:
        yield lib


@pytest.mark.parametrize("rate_in,rate_out", C.PAIRS)
@pytest.mark.parametrize("enc", C.ENCODINGS)
def test_wave_ingest_on_the_emulator(emu, enc, rate_in, rate_out):
    """set A at every channel count, 16-byte aligned and at two shifts of the rows; the 1-frame row stands in for the several-workgroup row of the GPU test"""
    from chatterbox_amd import ops
    C.check_ingest(ops, CPU, "A", enc, rate_in, rate_out, alignments=("aligned", 5))
    C.check_ingest(ops, CPU, "b", enc, rate_in, rate_out, alignments=(15,), channels=(1, 8))


def test_every_misalignment_and_a_row_of_several_workgroups_on_the_emulator(emu):
    from chatterbox_amd import ops
    for enc in C.ENCODINGS:
        C.check_ingest(ops, CPU, "A", enc, 24000, 16000, channels=(3,))
    C.check_ingest(ops, CPU, "B", "s24", 44100, 16000, alignments=(5,), channels=(2,))


@pytest.mark.parametrize("rate_in", [r for r in C.IN_RATES if r != 16000])
def test_every_source_rate_of_the_issue_converts_to_both_analysis_rates_on_the_emulator(emu, rate_in):
    from chatterbox_amd import ops
    for rate_out in (16000, 24000):
        if rate_in != rate_out:
            C.check_ingest(ops, CPU, "A", "s16", rate_in, rate_out, alignments=(5,), channels=(2,))


def test_typed_rows_are_the_bytes_they_hold_on_the_emulator(emu):
    """an int16 / int32 / float32 row gives the bits of the uint8 view of the same memory; a typed row must carry its own encoding"""
    from chatterbox_amd import ops
    for enc, dt in (("s16", torch.int16), ("s32", torch.int32), ("f32", torch.float32)):
        raw = torch.from_numpy(np.frombuffer(C.raw_row(enc, 2, 480, 1), np.uint8).copy())
        a = ops.wave_ingest([raw], enc, 2, 44100, 16000)[0]
        b = ops.wave_ingest([raw.view(dt)], enc, 2, 44100, 16000)[0]
        assert torch.equal(a, b) and a.numel() == C.out_len(480, 44100, 16000)
    with pytest.raises(TypeError, match="cannot hold"):
        ops.wave_ingest([torch.zeros(8, dtype=torch.int16)], "s32", 1, 16000, 16000)
    with pytest.raises(ValueError, match="whole number of frames"):
        ops.wave_ingest([torch.zeros(7, dtype=torch.uint8)], "s16", 2, 16000, 16000)
    with pytest.raises(ValueError, match="different allocations"):
        ops.wave_ingest([torch.zeros(8, dtype=torch.uint8), torch.zeros(8, dtype=torch.uint8)], "u8", 1, 8000, 16000)
    with pytest.raises(ValueError, match="encoding"):
        ops.wave_ingest([torch.zeros(8, dtype=torch.uint8)], "pcm", 1, 8000, 16000)
    with pytest.raises(ValueError, match="channels"):
        ops.wave_ingest([torch.zeros(9, dtype=torch.uint8)], "u8", 9, 8000, 16000)
    with pytest.raises(ValueError, match="no conversion"):
        ops.wave_ingest([torch.zeros(8, dtype=torch.uint8)], "u8", 1, 16001, 16000)


def test_nothing_is_written_outside_the_rows_on_the_emulator(emu):
    from chatterbox_amd import ops
    for enc, ch, ri, ro in (("mulaw", 1, 8000, 24000), ("s24", 3, 44100, 16000), ("f32", 8, 16000, 16000), ("s16", 2, 48000, 16000)):
        C.check_sentinels(ops, CPU, enc, ch, ri, ro)


def test_emulated_entry_refuses_the_same_descriptors_and_runs_the_good_one(emu):
    from chatterbox_amd import ops
    C.check_refusals(emu, ops, CPU, None)


@pytest.mark.parametrize("kind", C.TRIM_CASES)
def test_the_trim_rule_is_trim_silence(kind):
    C.check_trim_rule(kind)


def test_trim_edges_on_the_emulator(emu):
    from chatterbox_amd import ops
    C.check_trim(ops, CPU)
    assert ops.wave_trim_edges([torch.zeros(3000)], 0.0).tolist() == [[0, 0]], "top_db = 0: no frame is above the loudest"


@pytest.mark.parametrize("lengths", C.TRIM_SEAMS, ids=lambda t: "-".join(map(str, t)))
def test_trim_edges_at_the_block_seams_on_the_emulator(emu, lengths):
    from chatterbox_amd import ops
    C.check_trim_seams(ops, CPU, lengths)


# ----------------------------------------------------------------------------- the RIFF reader
def _chunk(cid, body):
    return cid + struct.pack("<I", len(body)) + body + (b"\0" if len(body) & 1 else b"")


def _riff(chunks):
    body = b"WAVE" + b"".join(chunks)
    return b"RIFF" + struct.pack("<I", len(body)) + body


def _fmt(tag, ch, rate, bits, ext=None):
    base = struct.pack("<HHIIHH", 0xFFFE if ext else tag, ch, rate, rate * ch * bits // 8, ch * bits // 8, bits)
    if ext:
        return base + struct.pack("<HHI", 22, bits, 0) + struct.pack("<H", tag) + b"\x00\x00\x00\x00\x10\x00\x80\x00\x00\xAA\x00\x38\x9B\x71"
    return base + (struct.pack("<H", 0) if tag != 1 else b"")


@pytest.mark.parametrize("enc,dtype", [("u8", np.uint8), ("s16", np.int16), ("s32", np.int32), ("f32", np.float32)])
def test_the_riff_reader_and_the_decode_are_load_wav_at_the_files_own_rate(tmp_path, enc, dtype):
    from scipy.io import wavfile
    from chatterbox_amd import frontend
    rng = np.random.default_rng(3)
    for ch in (1, 2, 3, 7):
        n = 1001
        data = rng.uniform(-1, 1, (n, ch)).astype(np.float32) if enc == "f32" else rng.integers(np.iinfo(dtype).min, np.iinfo(dtype).max + 1, (n, ch)).astype(dtype)
        path = tmp_path / f"{enc}_{ch}.wav"
        wavfile.write(str(path), 22050, data[:, 0] if ch == 1 else data)
        r = frontend.read_riff(path)
        assert (r["rate"], r["encoding"], r["channels"]) == (22050, enc, ch) and r["data"] == data.tobytes()
        ref, _ = frontend.load_wav(path, 22050)
        got = frontend.decode_pcm(r["data"], enc, ch)
        assert got.dtype == ref.dtype == np.float32 and np.array_equal(got.view(np.uint32), ref.view(np.uint32)), (enc, ch)


def test_the_riff_reader_on_hand_assembled_headers(tmp_path):
    from chatterbox_amd import frontend
    s24, g711 = C.raw_row("s24", 2, 333, 1), C.raw_row("mulaw", 1, 777, 2)   # (777 bytes: an odd-sized data chunk, padded)
    cases = {
        "s24": (_riff([_chunk(b"fmt ", _fmt(1, 2, 48000, 24)), _chunk(b"data", s24)]), dict(data=s24, rate=48000, encoding="s24", channels=2)),
        "mulaw": (_riff([_chunk(b"fmt ", _fmt(7, 1, 8000, 8)), _chunk(b"fact", struct.pack("<I", 777)), _chunk(b"data", g711)]), dict(data=g711, rate=8000, encoding="mulaw", channels=1)),
        "alaw": (_riff([_chunk(b"fmt ", _fmt(6, 1, 8000, 8)), _chunk(b"data", g711)]), dict(data=g711, rate=8000, encoding="alaw", channels=1)),
        "ext": (_riff([_chunk(b"fmt ", _fmt(1, 2, 44100, 24, ext=True)), _chunk(b"data", s24)]), dict(data=s24, rate=44100, encoding="s24", channels=2)),
        "ext_float": (_riff([_chunk(b"fmt ", _fmt(3, 1, 16000, 32, ext=True)), _chunk(b"data", s24[:1996])]), dict(data=s24[:1996], rate=16000, encoding="f32", channels=1)),
        "odd_chunk_first": (_riff([_chunk(b"LIST", b"abc"), _chunk(b"fmt ", _fmt(1, 1, 16000, 16)), _chunk(b"junk", b"x" * 5), _chunk(b"data", g711[:776]), _chunk(b"id3 ", b"zz")]),
                            dict(data=g711[:776], rate=16000, encoding="s16", channels=1)),
        "data_first": (_riff([_chunk(b"data", g711), _chunk(b"fmt ", _fmt(7, 1, 8000, 8))]), dict(data=g711, rate=8000, encoding="mulaw", channels=1)),
        "ragged": (_riff([_chunk(b"fmt ", _fmt(1, 2, 8000, 16)), _chunk(b"data", g711)]), dict(data=g711[:776], rate=8000, encoding="s16", channels=2)),
    }
    for name, (blob, want) in cases.items():
        path = tmp_path / (name + ".wav")
        path.write_bytes(blob)
        assert frontend.read_riff(path) == want, name
    with pytest.raises(ValueError):
        frontend.load_wav(tmp_path / "mulaw.wav", 8000)   # what the host path cannot open
    for name, blob in (("not", b"RIFX" + b"\0" * 40), ("nofmt", _riff([_chunk(b"data", g711)])), ("adpcm", _riff([_chunk(b"fmt ", _fmt(2, 1, 8000, 4)), _chunk(b"data", g711)])),
                       ("s12", _riff([_chunk(b"fmt ", _fmt(1, 1, 8000, 12)), _chunk(b"data", g711)])), ("ch9", _riff([_chunk(b"fmt ", _fmt(1, 9, 8000, 16)), _chunk(b"data", g711)]))):
        path = tmp_path / (name + ".wav")
        path.write_bytes(blob)
        with pytest.raises(ValueError, match=name + ".wav"):
            frontend.read_riff(path)


# ----------------------------------------------------------------------------- check_audio_in
def test_check_audio_in():
    from chatterbox_amd import ops
    assert ops.check_audio_in("a.wav") == dict(kind="path", path="a.wav") and ops.check_audio_in(b"a.wav")["kind"] == "path"
    w = np.zeros(8, np.float32)
    p = ops.check_audio_in((w, 16000))
    assert p["kind"] == "pair" and p["wav"] is w and p["rate"] == 16000 and ops.check_audio_in([w, np.int64(8000)])["rate"] == 8000
    raw = bytes(24)
    for data in (raw, bytearray(raw), memoryview(raw), np.zeros(24, np.uint8), torch.zeros(24, dtype=torch.uint8)):
        for enc in C.ENCODINGS:
            a = ops.check_audio_in((data, 8000, enc))
            assert a["kind"] == "raw" and a["frames"] == 24 // C.SAMPLE_BYTES[enc] and a["channels"] == 1 and a["encoding"] == enc and a["data"] is data
        assert ops.check_audio_in((data, 8000, "s16", 2))["frames"] == 6 and ops.check_audio_in((data, 8000, "s24", 8))["frames"] == 1
    assert ops.check_audio_in((np.zeros((5, 2), np.int16), 44100, "s16", 2))["frames"] == 5
    assert ops.check_audio_in((torch.zeros(6, dtype=torch.int32), 44100, "s32", 3))["frames"] == 2 and ops.check_audio_in((np.zeros(6, np.float32), 44100, "f32"))["frames"] == 6
    bad = [(3, TypeError, "audio"), ((w,), TypeError, "audio"), ((w, 1, "f32", 1, 0), TypeError, "audio"), ((w, 16000.0), TypeError, "sample_rate"), ((w, True), TypeError, "sample_rate"),
           ((w, 0), ValueError, "sample_rate"), ((raw, 8000, 7), TypeError, "encoding"), ((raw, 8000, "pcm"), ValueError, "encoding"), ((raw, 8000, "s16", 2.0), TypeError, "channels"),
           ((raw, 8000, "s16", True), TypeError, "channels"), ((raw, 8000, "s16", 0), ValueError, "channels"), ((raw, 8000, "s16", 9), ValueError, "channels"),
           (("text", 8000, "s16"), TypeError, "data"), ((np.zeros(4, np.float64), 8000, "f32"), TypeError, "dtype"), ((np.zeros(4, np.int16), 8000, "mulaw"), ValueError, "holds the encoding"),
           ((np.zeros(4, np.float32), 8000, "s32"), ValueError, "holds the encoding"), ((bytes(7), 8000, "s16"), ValueError, "whole number of frames"),
           ((bytes(8), 8000, "s24"), ValueError, "whole number of frames"), ((bytes(12), 8000, "s16", 4), ValueError, "whole number of frames")]
    for value, err, name in bad:
        with pytest.raises(err, match=name):
            ops.check_audio_in(value)


# ----------------------------------------------------------------------------- plumbing over recording stand-ins (nothing is launched)
class _Part:
    available = True

    def __init__(self, log, name, result):
        self.log, self.name, self.result = log, name, result

    def __call__(self, *a, **k):
        self.log.append((self.name, a, k))
        return self.result


class _RecAnalyzer:
    """records what the public classes ask of a PromptAnalyzer"""
    ENC_COND_LEN, DEC_COND_LEN = 6 * 16000, 10 * 24000

    def __init__(self):
        from chatterbox_amd import synth
        self.log, self.audio_in = [], "host"
        self.tokenizer = _Part(self.log, "tokenizer", (torch.arange(5)[None], torch.tensor([5])))
        self.speaker_encoder, self.ve = _Part(self.log, "xvec", None), object()
        self.ref = synth.s3gen_ref(n_prompt_tokens=8)

    def embed_ref(self, wav, sr):
        self.log.append(("embed_ref", np.asarray(wav).copy(), sr))
        return self.ref

    def embed_ref_staged(self, w24, w16):
        self.log.append(("embed_ref_staged", w24, w16))
        return self.ref

    def t3_prompt(self, w16, plen, enc_cond_len=None, ve_wav=None):
        self.log.append(("t3_prompt", w16, plen, enc_cond_len, ve_wav))
        return torch.zeros(1, 256), torch.zeros(1, 3, dtype=torch.long)

    def stage(self, audio, **kw):
        self.log.append(("stage", audio, kw))
        return dict(w24="w24", ref24="ref24", ref16="ref16", w16="w16", ve16="ve16", edges=(0, 1))

    def ingest(self, audios, rate_out):
        self.log.append(("ingest", list(audios), rate_out))
        return [f"w{k}" for k in range(len(audios))]


MULAW = (C.raw_row("mulaw", 1, 8000, 1), 8000, "mulaw")
STEREO = (np.frombuffer(C.raw_row("s16", 2, 4410, 2), np.int16).copy(), 44100, "s16", 2)


def _vc():
    from chatterbox_amd import api
    vc = api.ChatterboxVC.__new__(api.ChatterboxVC)
    vc.engine, vc.ref_dict, vc.watermarker, vc.analyzer, vc.device = _FakeSerialEngine(), {}, None, _RecAnalyzer(), CPU
    vc.engine.vocode = lambda toks, ref, **kw: (vc.engine.calls.append(("vocode", dict(tokens=toks, ref=ref, **kw))) or [torch.ones(3) for _ in toks], None)
    return vc


def test_audio_in_is_host_by_default_checked_and_mirrored_on_the_four_classes():
    from chatterbox_amd import api, frontend
    assert frontend.PromptAnalyzer.AUDIO_IN == ("host", "device")
    for cls in (api.ChatterboxTTS, api.ChatterboxMultilingualTTS, api.ChatterboxTurboTTS):
        m = _tts(cls, _FakeSerialEngine())
        assert m.audio_in == "host"          # (no analyzer: the switch is kept on the instance)
        m.audio_in = "device"
        assert m.audio_in == "device"
        m.analyzer = _RecAnalyzer()
        assert m.audio_in == "host"
        m.audio_in = "device"
        assert m.analyzer.audio_in == "device" and m.audio_in == "device"
        for bad, err in (("gpu", ValueError), ("", ValueError), (None, TypeError), (1, TypeError)):
            with pytest.raises(err, match="audio_in"):
                m.audio_in = bad
        assert m.audio_in == "device"
    vc = _vc()
    assert vc.audio_in == "host"
    vc.audio_in = "device"
    assert vc.analyzer.audio_in == "device"


def test_host_mode_decodes_the_raw_form_and_then_treats_it_as_a_pair():
    """the triple reaches the analysis as the resampled decode: what the pair (decode_pcm(data), rate) gives, bit for bit"""
    from chatterbox_amd import api, frontend
    for triple in (MULAW, STEREO, list(MULAW)):
        enc, ch = triple[2], (triple[3] if len(triple) == 4 else 1)
        x = frontend.decode_pcm(triple[0], enc, ch)
        for sr in (24000, 16000):
            assert np.array_equal(api._load_wave(triple, sr), frontend.resample(x, triple[1], sr))
    with pytest.raises(ValueError, match="encoding"):
        api._load_wave((b"", 8000, "pcm"), 16000)
    vc = _vc()
    vc.generate(audio=STEREO, seed=1)
    (name, a, k), = vc.analyzer.log
    w16 = frontend.resample(frontend.decode_pcm(STEREO[0], "s16", 2), 44100, 16000)
    assert name == "tokenizer" and torch.equal(a[0], torch.from_numpy(w16)) and vc.engine.calls[0][1]["tokens"][0].tolist() == [0, 1, 2, 3, 4]
    vc.analyzer.log.clear()
    vc.set_target_voice(MULAW)
    (name, wav, sr), = vc.analyzer.log
    assert name == "embed_ref" and sr == 24000 and np.array_equal(wav, frontend.resample(frontend.decode_pcm(MULAW[0], "mulaw", 1), 8000, 24000)[: vc.DEC_COND_LEN])


@pytest.mark.parametrize("cls_name,lang,kw", [("ChatterboxTTS", (), {}), ("ChatterboxMultilingualTTS", ("en",), {}), ("ChatterboxTurboTTS", (), dict(norm_loudness=False))])
def test_device_mode_hands_the_input_to_the_analyzer_as_it_is(cls_name, lang, kw):
    from chatterbox_amd import api
    m = _tts(getattr(api, cls_name), _FakeSerialEngine())
    m.analyzer = an = _RecAnalyzer()
    m.audio_in = "device"
    m.generate("aaaa.", *lang, audio_prompt_path=MULAW, **kw)
    assert [e[0] for e in an.log] == ["stage", "embed_ref_staged", "t3_prompt"]
    stage, emb, t3 = an.log
    assert stage[1] is MULAW and stage[2]["t3"] is True and stage[2]["norm"] is None and stage[2]["min_seconds"] == (5.0 if cls_name == "ChatterboxTurboTTS" else None)
    assert emb[1:] == ("ref24", "ref16") and t3[1] == "w16" and t3[2] == m.PROMPT_LEN and t3[4] == "ve16"
    an.log.clear()
    out = m.generate_batch(["x.", "yy.", "zzz."], *lang, audio_prompt_paths=[MULAW, STEREO, MULAW], **kw)
    assert len(out) == 3 and [e[1] for e in an.log if e[0] == "stage"] == [MULAW, STEREO], "equal prompts of one call are analysed once, by identity"
    if cls_name == "ChatterboxTurboTTS":
        an.log.clear()
        m.prepare_conditionals(STEREO, norm_loudness="device")
        assert callable(an.log[0][2]["norm"])
        with pytest.raises(ValueError, match="norm_loudness"):
            m.prepare_conditionals(STEREO, norm_loudness="host")
    m.audio_in = "host"
    an.log.clear()
    with pytest.raises(TypeError, match="audio"):
        m.prepare_conditionals((b"", 8000, "mulaw", 1, 2), **kw)
    assert an.log == []


def test_vc_device_mode_ingests_sources_together_and_tokenises_them_one_by_one():
    vc = _vc()
    vc.audio_in = "device"
    an = vc.analyzer
    vc.generate(audio=STEREO, seed=1)
    assert [e[0] for e in an.log] == ["ingest", "tokenizer"] and an.log[0][1] == [STEREO] and an.log[0][2] == 16000 and an.log[1][1] == ("w0",)
    an.log.clear()
    out = vc.generate_batch(audios=[STEREO, MULAW, "a.wav"], seeds=[1, 2, 3])
    assert len(out) == 3 and [e[0] for e in an.log] == ["ingest", "tokenizer", "tokenizer", "tokenizer"]
    assert an.log[0][1] == [STEREO, MULAW, "a.wav"] and [e[1] for e in an.log[1:]] == [("w0",), ("w1",), ("w2",)]
    an.log.clear()
    vc.set_target_voice(MULAW)
    assert [e[0] for e in an.log] == ["stage", "embed_ref_staged"] and an.log[0][1] is MULAW and an.log[0][2] == dict(dec_cond_len=vc.DEC_COND_LEN)


def test_the_analyzer_groups_sources_by_rate_encoding_and_channels(monkeypatch):
    """PromptAnalyzer.ingest over a recording ops.wave_ingest: one call per (rate, encoding, channels), the rows views of one buffer that hold the sources' bytes on
    16-byte boundaries, the results back in the caller's order; a rate over the caps raises before any call"""
    from chatterbox_amd import frontend, ops
    an = frontend.PromptAnalyzer.__new__(frontend.PromptAnalyzer)
    an.dev = CPU
    calls = []

    def rec(rows, enc, ch, ri, ro):
        calls.append((rows, enc, ch, ri, ro))
        return [f"{enc}{ri}#{k}" for k in range(len(rows))]

    monkeypatch.setattr(ops, "wave_ingest", rec)
    pair = (np.arange(10, dtype=np.float64) / 16, 22050)
    f32 = (torch.arange(6, dtype=torch.float32), 22050)
    other = (C.raw_row("mulaw", 1, 33, 7), 8000, "mulaw", 1)
    out = an.ingest([MULAW, STEREO, pair, other, f32], 16000)
    assert out == ["mulaw8000#0", "s1644100#0", "f3222050#0", "mulaw8000#1", "f3222050#1"]
    assert [(c[1], c[2], c[3], c[4], len(c[0])) for c in calls] == [("mulaw", 1, 8000, 16000, 2), ("s16", 2, 44100, 16000, 1), ("f32", 1, 22050, 16000, 2)]
    rows = calls[0][0]
    assert rows[0].numpy().tobytes() == MULAW[0] and rows[1].numpy().tobytes() == other[0] and rows[0].dtype == torch.uint8
    assert len({w.untyped_storage().data_ptr() for w in rows}) == 1 and all((w.data_ptr() - rows[0].untyped_storage().data_ptr()) % 16 == 0 for w in rows)
    assert calls[1][0][0].dtype == torch.int16 and torch.equal(calls[1][0][0], torch.from_numpy(STEREO[0]))
    assert calls[2][0][0].dtype == torch.float32 and calls[2][0][0].tolist() == (np.arange(10) / 16).tolist() and calls[2][0][1].tolist() == list(range(6))
    calls.clear()
    with pytest.raises(ValueError, match="no conversion"):
        an.ingest([MULAW, (b"\0" * 4, 16001, "s16")], 16000)
    assert calls == []
