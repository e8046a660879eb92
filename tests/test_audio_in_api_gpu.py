"""GPU (-m gpu): audio in through the public API on synthetic few-layer models -- the raw input form (data, sample_rate, encoding[, channels]) and the `audio_in`
switch.  Device mode is compared EXACTLY with host mode fed the device's own waveform (the plumbing adds nothing); every stage of the device chain meets the kernel
tests' derived bound against the fp64 chain applied to that stage's actual input, and the analysis outputs are bit for bit the four engines' on the staged
tensors; a G.711 WAV opens in device mode; batch grouping does not change a bit; the default mode is the call through frontend.load_wav.  How many S3 prompt tokens
differ between the modes is printed, not asserted (FSQ indices flip under any rounding-level change of the input).  The kernel-level tests are in
test_turbo_stream_wave_ingest_kernels_gpu.py."""
import os
import struct
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import test_seeded_api_gpu as A  # noqa: E402  (read-only import: the recording wrapper, the stand-in tokenizer)
import wave_format_common as F  # noqa: E402
import wave_ingest_common as C  # noqa: E402

pytestmark = pytest.mark.gpu


def _s16(x):
    return np.clip(np.rint(np.asarray(x, np.float64) * 32767.0), -32768, 32767).astype("<i2")


@pytest.fixture(scope="module")
def inputs():
    """1.5 s sources: 44.1 kHz stereo s16 (the channels differ), 8 kHz mu-law, 22.05 kHz f32 mono, 48 kHz 24-bit -- and a 1.6 s prompt with silence at both ends"""
    from chatterbox_amd import synth
    a, b = synth.prompt_wav(1.5, 44100, seed=1).numpy(), synth.prompt_wav(1.5, 44100, seed=2).numpy()
    stereo = np.stack([_s16(0.8 * a), _s16(0.5 * b)], 1)
    mu = F.g711_tables()["mulaw"][_s16(synth.prompt_wav(1.5, 8000, seed=3).numpy()).astype(np.int32) + 32768]
    f32 = synth.prompt_wav(1.5, 22050, seed=4).numpy().astype(np.float32)
    v = (np.asarray(synth.prompt_wav(1.5, 48000, seed=5).numpy(), np.float64) * (2 ** 23 - 1)).astype(np.int64) & 0xFFFFFF
    s24 = np.stack([v & 0xFF, (v >> 8) & 0xFF, (v >> 16) & 0xFF], 1).astype(np.uint8).tobytes()
    p = synth.prompt_wav(1.6, 22050, seed=6).numpy()
    p[:6000] *= 1e-4
    p[-5000:] *= 1e-4
    return dict(stereo=(stereo.tobytes(), 44100, "s16", 2), stereo_array=(stereo, 44100, "s16", 2), mulaw=(mu.tobytes(), 8000, "mulaw"), f32=(f32, 22050, "f32"),
                s24=(s24, 48000, "s24", 1), prompt=(_s16(p).tobytes(), 22050, "s16"))


@pytest.fixture(scope="module")
def vc(dev):
    from chatterbox_amd import api
    m = api.ChatterboxVC.from_synthetic(dev, tokenizer_layers=1)
    m.watermarker = None
    return m


@pytest.fixture(scope="module")
def tts(dev):
    from chatterbox_amd import api
    m = api.ChatterboxTTS.from_synthetic(dev, t3_layers=2, with_prompt_nets=True, tokenizer_layers=1)
    m.tokenizer = A._Tok(api.ChatterboxTTS._TEXT_VOCAB)
    A._bound_and_record(m.engine, "max_new_tokens")
    m.watermarker = None
    return m


def _mode(m, mode):
    m.audio_in = mode
    return m


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b)


def test_device_mode_is_host_mode_fed_the_device_waveform(dev, vc, inputs):
    from chatterbox_amd import ops
    data, rate, enc, ch = inputs["stereo"]
    try:
        got = _mode(vc, "device").generate(audio=inputs["stereo"], seed=1)
        with torch.cuda.device(dev):
            w16 = ops.wave_ingest([torch.frombuffer(bytearray(data), dtype=torch.uint8).to(dev)], enc, ch, rate, 16000)[0].cpu().numpy()
        assert w16.dtype == np.float32 and w16.shape == (C.out_len(len(data) // 4, 44100, 16000),)
        want = _mode(vc, "host").generate(audio=(w16, 16000), seed=1)
        assert got.dtype == torch.float32 and got.shape[1] > 24000 and _same(got, want), "the plumbing adds nothing"
        assert _same(_mode(vc, "device").generate(audio=inputs["stereo_array"], seed=1), got), "an int16 array is the bytes it holds"
        x = C.decode(data, enc, ch)
        print(f"44100 stereo s16 -> 16000: worst |y - y64| / bound = {C.check_bound(w16, x, 44100, 16000, 'vc source'):.3f}")
    finally:
        vc.audio_in = "host"


def test_the_raw_form_works_in_both_modes(vc, inputs):
    """mu-law 8 kHz in, mu-law 8 kHz out: on the parent commit the triple is rejected and `audio_in` does not exist"""
    from chatterbox_amd import frontend
    outs = {}
    try:
        for mode in ("host", "device"):
            w = _mode(vc, mode).generate(audio=inputs["mulaw"], seed=2, sample_rate=8000, encoding="mulaw")
            assert w.dtype == torch.uint8 and w.dim() == 2 and w.shape[0] == 1 and w.shape[1] > 8000 and w.device.type == "cpu"
            outs[mode] = w
    finally:
        vc.audio_in = "host"
    assert outs["host"].shape == outs["device"].shape
    x = frontend.decode_pcm(inputs["mulaw"][0], "mulaw", 1)
    assert _same(outs["host"], vc.generate(audio=(x, 8000), seed=2, sample_rate=8000, encoding="mulaw")), "host mode: the decode, then a pair"


def test_the_default_is_the_call_through_load_wav(vc, tmp_path):
    from scipy.io import wavfile
    from chatterbox_amd import frontend, synth
    path = tmp_path / "src.wav"
    wavfile.write(path, 22050, _s16(synth.prompt_wav(1.2, 22050, seed=9).numpy()))
    assert vc.audio_in == "host" and vc.analyzer.audio_in == "host"
    got = vc.generate(audio=str(path), seed=3)
    assert _same(got, vc.generate(audio=(frontend.load_wav(path, 16000)[0], 16000), seed=3))
    assert _same(got, vc.generate(audio=(frontend.load_wav(path, 22050)[0], 22050), seed=3))


def _g711_wav(path, codes, tag, rate=8000):
    fmt = struct.pack("<HHIIHHH", tag, 1, rate, rate, 1, 8, 0)
    body = b"WAVE" + b"fmt " + struct.pack("<I", len(fmt)) + fmt + b"fact" + struct.pack("<II", 4, len(codes)) + b"data" + struct.pack("<I", len(codes)) + codes + b"\0" * (len(codes) & 1)
    path.write_bytes(b"RIFF" + struct.pack("<I", len(body)) + body)
    return str(path)


def test_a_g711_wav_path_opens_in_device_mode(vc, inputs, tmp_path):
    from chatterbox_amd import frontend
    path = _g711_wav(tmp_path / "call.wav", inputs["mulaw"][0], 7)
    with pytest.raises(ValueError):
        frontend.load_wav(path, 16000)
    try:
        got = _mode(vc, "device").generate(audio=path, seed=4)
        assert _same(got, vc.generate(audio=inputs["mulaw"], seed=4)), "a path is its data chunk's bytes"
        s24 = vc.generate(audio=inputs["s24"], seed=4)
        assert s24.shape[1] > 24000 and torch.isfinite(s24).all()
    finally:
        vc.audio_in = "host"


def test_batch_grouping_is_bit_neutral(vc, inputs):
    """Mixed rates and encodings, two sources of one group among them: per request the bits of the single device-mode call with the same seed.
    What the grouping can change is the waveform the tokeniser sees, so the S3 tokens every request is vocoded from are compared exactly at the default MAX_BATCH
    (one device batch of six), and the audio exactly with device batches of one (MAX_BATCH = 1: the sources are still ingested together, group by group).  At
    B > 1 the flow and the vocoder themselves are not bit-equal to their B = 1 form -- test_batch_api_gpu.py::test_vc_generate_batch_equals_single_generates
    states that tolerance for s3_tokens= input, before any audio input exists -- so there the audio is held to that tolerance.  Measured on the MI355X, one batch
    of six against six single calls: tokens identical, waveform RMSE 3.0e-05 .. 1.6e-04 (TOL_WAV_E2E_8S = 6.5e-04), not bit-equal; batches of one: bit-equal."""
    from test_baseline_shapes_gpu import TOL_WAV_E2E_8S
    names = ["stereo", "mulaw", "f32", "mulaw", "stereo_array", "s24"]
    seeds = [11, 12, 13, 14, 15, 16]
    vocode, seen, max_batch = vc.engine.vocode, [], vc.MAX_BATCH

    def recording(tokens, ref, **kw):
        seen.extend(zip(kw["seeds"], (t.tolist() for t in tokens)))
        return vocode(tokens, ref, **kw)

    try:
        _mode(vc, "device")
        vc.engine.vocode = recording
        batch = vc.generate_batch(audios=[inputs[n] for n in names], seeds=seeds)
        assert len(seen) == 6
        in_batch = dict(seen)
        seen.clear()
        single = [vc.generate(audio=inputs[n], seed=s) for n, s in zip(names, seeds)]
        assert dict(seen) == in_batch and in_batch[12] == in_batch[14] and in_batch[11] == in_batch[15], "the tokens of a request do not depend on its group"
        for n, w, one in zip(names, batch, single):
            err = float((w.double() - one.double()).pow(2).mean().sqrt())
            print(f"{n}: one batch of six against the single call: RMSE {err:.3e} (tolerance {TOL_WAV_E2E_8S:.1e}), bit-equal: {_same(w, one)}")
            assert w.shape == one.shape and err <= TOL_WAV_E2E_8S, n
        vc.MAX_BATCH = 1
        for n, w, one in zip(names, vc.generate_batch(audios=[inputs[n] for n in names], seeds=seeds), single):
            assert _same(w, one), n
    finally:
        vc.audio_in, vc.engine.vocode, vc.MAX_BATCH = "host", vocode, max_batch


def _bound(y, x, ri, ro, what):
    return C.check_bound(y.cpu().numpy(), x, ri, ro, what)


def test_the_stages_meet_their_bound_and_the_outputs_are_the_engines_own(dev, tts, vc, inputs):
    from chatterbox_amd import frontend
    audio = inputs["prompt"]
    an, ref0 = tts.analyzer, vc.ref_dict
    try:
        _mode(tts, "device")
        with torch.cuda.device(dev):
            st = an.stage(audio, t3=True)
            x = C.decode(audio[0], "s16", 1)
            w24, w16 = st["w24"].cpu().numpy(), st["w16"].cpu().numpy()
            worst = [_bound(st["w24"], x, 22050, 24000, "w24"), _bound(st["w16"], w24, 24000, 16000, "w16"),
                     _bound(st["ref16"], st["ref24"].cpu().numpy(), 24000, 16000, "ref16")]
            print("stages, worst |y - y64| / bound: w24 %.3f, w16 %.3f, ref16 %.3f" % tuple(worst))
            assert torch.equal(st["ref24"], st["w24"][: an.DEC_COND_LEN])
            edges = frontend.trim_edges_rule(w16, 20.0)
            assert st["edges"] == edges and 0 < edges[0] < edges[1] < len(w16) and torch.equal(st["ve16"], st["w16"][edges[0]: edges[1]])
            print(f"trim: margin {C.trim_margin_db(w16):.3f} dB, kept {edges} of {len(w16)}")
            tts.prepare_conditionals(audio, exaggeration=0.5)
            c = tts.conds
            feat = an.mel(st["ref24"])[None]
            tok, _ = an.tokenizer(st["ref16"])
            tok = tok[:, : feat.shape[1] // 2]
            assert _same(c.gen["prompt_feat"], feat) and _same(c.gen["prompt_token"], tok.to(dev)) and _same(c.gen["embedding"], an.speaker_encoder.inference(st["ref16"]))
            ptok, _ = an.tokenizer(st["w16"][: an.ENC_COND_LEN], max_len=tts.PROMPT_LEN)
            spk = an.ve.inference(an.ve.melspectrogram(st["ve16"]), rate=1.3)
            assert _same(c.t3.cond_prompt_speech_tokens, ptok.to(dev)) and _same(c.t3.speaker_emb.cpu(), spk.cpu()[None])
            assert _same(an.ve.embeds_from_wavs([st["w16"]]), spk.cpu()[None]), "embeds_from_wavs trims a device waveform on the device"
        dev_tok = c.gen["prompt_token"].cpu()
        _mode(tts, "host").prepare_conditionals(audio, exaggeration=0.5)
        host_tok = tts.conds.gen["prompt_token"].cpu()
        assert host_tok.shape == dev_tok.shape
        print(f"S3 prompt tokens that differ between host and device mode: {int((host_tok != dev_tok).sum())} of {host_tok.numel()}")
        w = _mode(tts, "device").generate("aaaa bbbb.", audio_prompt_path=audio, seed=5)
        assert w.dim() == 2 and torch.isfinite(w).all()
        # the target voice of a conversion: embed_ref on the staged tensors
        _mode(vc, "device")
        with torch.cuda.device(dev):
            sv = vc.analyzer.stage(inputs["f32"], dec_cond_len=vc.DEC_COND_LEN)
            _bound(sv["w24"], inputs["f32"][0], 22050, 24000, "vc w24"), _bound(sv["ref16"], sv["ref24"].cpu().numpy(), 24000, 16000, "vc ref16")
            vc.set_target_voice(inputs["f32"])
            want = vc.analyzer.embed_ref_staged(sv["ref24"], sv["ref16"])
        for k in ("prompt_feat", "prompt_token", "embedding"):
            assert _same(vc.ref_dict[k], want[k]), k
    finally:
        tts.audio_in = vc.audio_in = "host"
        vc.ref_dict = ref0
