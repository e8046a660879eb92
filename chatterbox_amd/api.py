"""Drop-in boundary: the reference's Python class API on top of the MI355X engines.

`ChatterboxTTS` (reference tts.py:106), `ChatterboxMultilingualTTS` (mtl_tts.py:155), `ChatterboxVC` (vc.py:16) keep
the reference names, signatures, defaults, return convention (CPU float tensor (1, n_samples) at `.sr` = 24 kHz) and
error behaviour (ValueError for an unknown language / model alias, assert when no voice is prepared).  Checkpoints
are read in the reference's own file and state-dict layout.  `ChatterboxTurboTTS` (tts_turbo.py:111) covers the Turbo / Nano GPT-2
backbone.  Voice-prompt analysis (`prepare_conditionals`, `ChatterboxVC.set_target_voice`, `ChatterboxVC.generate(audio)`) runs on
the device through chatterbox_amd/frontend.py (S3 tokenizer, CAMPPlus, voice encoder, 24 kHz mel); it needs the `tokenizer.*` /
`speaker_encoder.*` tensors of the S3Gen checkpoint and `ve.safetensors`, and fails with a clear message when a checkpoint lacks
them.  The watermarker (third-party `perth`) is applied only if importable -- parity is defined on the pre-watermark waveform;
Turbo's `norm_loudness` needs `pyloudnorm` and is skipped with a warning when that is missing (as the reference does on error); norm_loudness="device" uses this
project's own meter instead.
"""
import contextlib
import math
import os
from dataclasses import dataclass
from pathlib import Path
from typing import Optional

import torch

from . import ops, synth
from .engine import ChatterboxEngine, S3GenEngine, TurboEngine, frame_sample
from .text import CJK_LANGUAGES, EnTokenizer, MTLTokenizer, default_max_chars, punc_norm, punc_norm_en, punc_norm_turbo, split_text, word_groups

S3GEN_SR, S3_SR = 24000, 16000
REPO_ID = "ResembleAI/chatterbox"
DEFAULT_MULTILINGUAL_T3_MODEL = "t3_mtl23ls_v2.safetensors"
MULTILINGUAL_T3_MODELS = {"v2": "t3_mtl23ls_v2.safetensors", "t3_mtl23ls_v2": "t3_mtl23ls_v2.safetensors",
                          "v3": "t3_mtl23ls_v3.safetensors", "t3_mtl23ls_v3": "t3_mtl23ls_v3.safetensors"}
SUPPORTED_LANGUAGES = {
    "ar": "Arabic", "da": "Danish", "de": "German", "el": "Greek", "en": "English", "es": "Spanish", "fi": "Finnish",
    "fr": "French", "he": "Hebrew", "hi": "Hindi", "it": "Italian", "ja": "Japanese", "ko": "Korean", "ms": "Malay",
    "nl": "Dutch", "no": "Norwegian", "pl": "Polish", "pt": "Portuguese", "ru": "Russian", "sv": "Swedish",
    "sw": "Swahili", "tr": "Turkish", "zh": "Chinese"}


def _resolve_multilingual_t3_model(t3_model):
    if t3_model is None:
        return DEFAULT_MULTILINGUAL_T3_MODEL
    if t3_model in MULTILINGUAL_T3_MODELS:
        return MULTILINGUAL_T3_MODELS[t3_model]
    if t3_model.endswith(".safetensors"):
        return t3_model
    raise ValueError(f"Unknown multilingual T3 model '{t3_model}'. Expected one of {sorted(MULTILINGUAL_T3_MODELS)} "
                     f"or a .safetensors filename.")


@dataclass
class T3Cond:
    """Same fields as the reference dataclass (models/t3/modules/cond_enc.py:12-22)."""
    speaker_emb: torch.Tensor
    clap_emb: Optional[torch.Tensor] = None
    cond_prompt_speech_tokens: Optional[torch.Tensor] = None
    cond_prompt_speech_emb: Optional[torch.Tensor] = None
    emotion_adv: Optional[torch.Tensor] = 0.5

    def to(self, *, device=None, dtype=None):
        for k, v in self.__dict__.items():
            if torch.is_tensor(v):
                setattr(self, k, v.to(device=device, dtype=dtype if v.is_floating_point() else None))
        return self

    def as_dict(self):
        return dict(speaker_emb=self.speaker_emb, cond_prompt_speech_tokens=self.cond_prompt_speech_tokens,
                    emotion_adv=self.emotion_adv)


@dataclass
class Conditionals:
    """`conds.pt` = torch.save(dict(t3=T3Cond.__dict__, gen=dict)) (reference tts.py:64-103); this is also exactly the
    payload that dist.broadcast_conditionals ships to the other ranks."""
    t3: T3Cond
    gen: dict

    def to(self, device):
        self.t3 = self.t3.to(device=device)
        self.gen = {k: (v.to(device) if torch.is_tensor(v) else v) for k, v in self.gen.items()}
        return self

    def save(self, fpath):
        if str(fpath).endswith(".safetensors"):  # pickle-free container (formats.py); conds.pt stays the reference's torch pickle
            from . import formats
            return formats.save_conds(self, fpath)
        torch.save(dict(t3=self.t3.__dict__, gen=self.gen), fpath)

    @classmethod
    def load(cls, fpath, map_location="cpu"):
        if str(fpath).endswith(".safetensors"):
            from . import formats
            return formats.load_conds(fpath, map_location)
        kw = torch.load(fpath, map_location=torch.device(map_location) if isinstance(map_location, str) else map_location,
                        weights_only=True)
        return cls(T3Cond(**kw["t3"]), kw["gen"])


def _load_state(path):
    path = str(path)
    if path.endswith(".safetensors"):
        from .formats import read_safetensors
        sd = read_safetensors(path)  # zero-copy views of one memory map (no host copy before the H2D transfer)
    else:
        sd = torch.load(path, map_location="cpu", weights_only=True)
    if "model" in sd and not torch.is_tensor(sd["model"]):  # `{"model": [state]}` wrapper (reference tts.py:146-147)
        sd = sd["model"][0]
    return sd


def _make_analyzer(s3gen_sd, ve_sd, device):
    from .frontend import PromptAnalyzer
    return PromptAnalyzer(s3gen_sd, ve_sd, device)


def _norm_loudness(wav, sr, target_lufs=-27.0):
    """Gain a waveform to `target_lufs` integrated loudness (reference ChatterboxTurboTTS.norm_loudness, tts_turbo.py:223-239): needs the
    third-party `pyloudnorm`; on any error the reference prints a warning and carries on with the input, and so does this."""
    try:
        import numpy as np
        import pyloudnorm as ln
        gain = 10.0 ** ((target_lufs - ln.Meter(sr).integrated_loudness(wav)) / 20.0)
        if np.isfinite(gain) and gain > 0.0:
            wav = wav * gain
    except Exception as e:
        print(f"Warning: Error in norm_loudness, skipping: {e}")
    return wav


def _norm_loudness_device(wav, device, target_lufs=-27.0):
    """_norm_loudness without pyloudnorm: the 24 kHz prompt goes to the device, cbx_wave_loudness_f32 measures it (ITU-R BS.1770-4 as include/cbx.h states it: whole
    400 ms blocks only, where pyloudnorm may add a partial one) and cbx_wave_gain_f32 gains it to `target_lufs`; no peak ceiling, as the reference applies none.  A
    silent prompt or one shorter than 0.4 s comes back as it is."""
    import numpy as np
    dev = torch.device(device)
    with (torch.cuda.device(dev) if dev.type == "cuda" else contextlib.nullcontext()):
        w = torch.from_numpy(np.ascontiguousarray(wav, dtype=np.float32)).to(dev, copy=True)  # (the gain is applied in place: never to the caller's array)
        ops.wave_normalize([w], [float(target_lufs)], ceiling=None, fs=S3GEN_SR)
        return w.cpu().numpy()


def _load_wave(wav, sr):
    """A file path, a (waveform, sample_rate) pair or a (data, sample_rate, encoding[, channels]) tuple -> the waveform at rate `sr` (a float32 array), on the host
    (audio_in = "host").  The raw form is decoded and mixed down by frontend.decode_pcm and then treated as a pair."""
    from . import frontend as fe
    if isinstance(wav, (tuple, list)) and len(wav) != 2:
        a = ops.check_audio_in(wav)
        wav = (fe.decode_pcm(a["data"], a["encoding"], a["channels"]), a["rate"])
    return fe.resample(wav[0], wav[1], sr) if isinstance(wav, (tuple, list)) else fe.load_wav(wav, sr)[0]


def _check_audio_in_mode(value):
    if not isinstance(value, str):
        raise TypeError(f"audio_in: expected 'host' or 'device', got {type(value).__name__}")
    if value not in ("host", "device"):
        raise ValueError(f"audio_in = {value!r}: expected 'host' or 'device'")
    return value


def _prepare_conditionals(analyzer, wav, exaggeration, prompt_len, device, min_seconds=None, norm_loudness=False, enc_cond_len=None):
    """The common body of prepare_conditionals (tts.py:182-206, mtl_tts.py:253-277, tts_turbo.py:241-270).  `wav`: a file path, a
    (waveform, sample_rate) pair or raw samples (data, sample_rate, encoding[, channels]) (ops.check_audio_in).  analyzer.audio_in = "device": the same stages
    with the waveform on the device (_prepare_conditionals_device)."""
    from . import frontend as fe
    if analyzer is None or not analyzer.tokenizer.available or not analyzer.speaker_encoder.available or analyzer.ve is None:
        raise RuntimeError("voice-prompt analysis needs the `tokenizer.*` and `speaker_encoder.*` tensors of the S3Gen checkpoint and "
                           "ve.safetensors; this model was built without them -- load a prepared voice with Conditionals.load('conds.pt')")
    if getattr(analyzer, "audio_in", "host") == "device":
        return _prepare_conditionals_device(analyzer, wav, exaggeration, prompt_len, device, min_seconds, norm_loudness, enc_cond_len)
    w24 = _load_wave(wav, S3GEN_SR)
    if min_seconds is not None:
        assert len(w24) / S3GEN_SR > min_seconds, "Audio prompt must be longer than 5 seconds!"
    if isinstance(norm_loudness, str):
        if norm_loudness != "device":
            raise ValueError(f"norm_loudness = {norm_loudness!r}: expected True, False or 'device'")
        w24 = _norm_loudness_device(w24, device)
    elif norm_loudness:
        w24 = _norm_loudness(w24, S3GEN_SR)
    w16 = fe.resample(w24, S3GEN_SR, S3_SR)
    gen = analyzer.embed_ref(w24[: analyzer.DEC_COND_LEN], S3GEN_SR)
    spk, ptoks = analyzer.t3_prompt(w16, prompt_len, enc_cond_len=enc_cond_len)
    t3 = T3Cond(speaker_emb=spk, cond_prompt_speech_tokens=ptoks, emotion_adv=exaggeration * torch.ones(1, 1, 1)).to(device=device)
    return Conditionals(t3, {k: (v.to(device) if torch.is_tensor(v) else v) for k, v in gen.items()})


def _prepare_conditionals_device(analyzer, wav, exaggeration, prompt_len, device, min_seconds, norm_loudness, enc_cond_len):
    """_prepare_conditionals with audio_in = "device": the same stages in the same order (PromptAnalyzer.stage), the waveform on the device from the upload of its
    raw bytes on.  norm_loudness="device" gains the 24 kHz waveform in place where it is; True (pyloudnorm) is a round trip through the host."""
    if isinstance(norm_loudness, str) and norm_loudness != "device":
        raise ValueError(f"norm_loudness = {norm_loudness!r}: expected True, False or 'device'")

    def norm(w24):
        if isinstance(norm_loudness, str):
            ops.wave_normalize([w24], [-27.0], ceiling=None, fs=S3GEN_SR)
            return w24
        return torch.from_numpy(_norm_loudness(w24.cpu().numpy(), S3GEN_SR).astype("float32")).to(w24.device)
    st = analyzer.stage(wav, t3=True, norm=norm if norm_loudness else None, min_seconds=min_seconds)
    gen = analyzer.embed_ref_staged(st["ref24"], st["ref16"])
    spk, ptoks = analyzer.t3_prompt(st["w16"], prompt_len, enc_cond_len=enc_cond_len, ve_wav=st["ve16"])
    t3 = T3Cond(speaker_emb=spk, cond_prompt_speech_tokens=ptoks, emotion_adv=exaggeration * torch.ones(1, 1, 1)).to(device=device)
    return Conditionals(t3, {k: (v.to(device) if torch.is_tensor(v) else v) for k, v in gen.items()})


def _watermarker():
    try:
        import perth
        return perth.PerthImplicitWatermarker()
    except Exception:
        return None


def _stream_kw(first_chunk, chunk, chunk_growth, lookahead, fade, overlap, window=None, speed=None):
    """The round-schedule arguments of generate_stream, passed through to the engine's synthesize_stream.  `window` and `speed` are checked here, when
    generate_stream is CALLED (the engine's generator would raise at the first next() only); the window against the rate (engine.check_stream_window).
    speed 1.0 / None adds no keyword: the engine call is then exactly the one without it."""
    from .engine import check_stream_window
    speed_kw = _stream_speed_kw(speed)
    return dict(first_chunk=first_chunk, chunk=chunk, chunk_growth=chunk_growth, lookahead=lookahead, fade=fade, overlap=overlap,
                window=check_stream_window(window, fade, speed_kw.get("speed")), **speed_kw)


PAUSE_FADE = 240  # samples of cross-fade over a shortened pause: fixed


def _pauses(max_pause, pause_db, B=1, one=False):
    """`max_pause` and `pause_db` as the engines' pauses= dict (ops.check_pauses), or None when no request has a max_pause: the engine call is then exactly the one
    without it.  max_pause: None, or seconds in [0.04, 60] -- a silence inside the utterance that is longer is shortened to round(max_pause * 50) frames of 480
    samples; generate_batch (one=False): a number for every request or a sequence of B numbers / Nones.  pause_db: ONE finite number >= 0 for the call, the decibels
    below the utterance's loudest frame at or under which a frame counts as silence.  TypeError / ValueError before anything is launched."""
    import math
    import numbers
    is_num = lambda v: isinstance(v, numbers.Real) and not isinstance(v, bool)
    if not is_num(pause_db):
        raise TypeError(f"pause_db: expected a number, got {type(pause_db).__name__}")
    if not math.isfinite(pause_db) or pause_db < 0.0:
        raise ValueError(f"pause_db = {pause_db}: expected a finite number >= 0")
    if isinstance(max_pause, (list, tuple)):
        if one:
            raise TypeError(f"max_pause: expected None or a number of seconds, got a {type(max_pause).__name__}")
        if len(max_pause) != B:
            raise ValueError(f"max_pause: {len(max_pause)} entries for {B} requests")
        vals = list(max_pause)
    else:
        vals = [max_pause] * B
    keep = []
    for v in vals:
        if v is None:
            keep.append(0)
            continue
        if not is_num(v):
            raise TypeError(f"max_pause: expected None or a number of seconds, got {type(v).__name__}")
        if not math.isfinite(v) or not 0.04 <= v <= 60.0:
            raise ValueError(f"max_pause = {v}: expected None or a number of seconds in [0.04, 60]")
        keep.append(int(round(float(v) * 50.0)))
    return dict(keep=keep, db=float(pause_db), fade=PAUSE_FADE) if any(keep) else None


def _request_seeds(seed, B=1, one=True, generator=None):
    """`seed` of a method that takes ONE request (None or an int in [0, 2^64)) or `seeds` of generate_batch (None, an int for every request or a sequence of B ints;
    not together with a generator) -> a list of B ints, or None.  TypeError / ValueError before anything is launched."""
    if not one:
        return ops.request_seeds(seed, B, generator)
    if seed is None:
        return None
    if isinstance(seed, bool) or not isinstance(seed, int):
        raise TypeError(f"seed: expected an int, got {type(seed).__name__}")
    return ops.check_seeds(seed, 1, "seed")


class _Options:
    """The delivery options of ONE public call for its B requests, built from the public arguments and validated when the method is CALLED, generators included --
    in one order for every method: the format (sample_rate, encoding), word_times, seed / seeds (with the generator), speed, loudness, true_peak, bed, max_pause / pause_db, pitch
    with the speed x pitch rule (ops.check_speed_pitch), guard.  one=True: the method serves one request (generate, generate_long, ...): a sequence for
    loudness, true_peak, max_pause or pitch is then a TypeError.  segments=False (generate_long without return_segments): word_times is refused, its words travel in the
    segments.  Holds fmt (ops.check_format's dict), words (_word_times' mode), seeds, speed, loud, peak (ops.check_true_peak's dBTP ceilings), pitch (B entries each), pz (_pauses' dict), guard (the
    engines' dict) -- each None when no request uses it -- and the generator; kw(idx) turns them into the engines' keywords.
    duration / timing (the timing control; checked last): dur holds ops.check_duration's B target lengths in frames / Nones, timing ops.check_timing's B lists of
    word starts in frames / Nones; either is refused together with speed, pitch or max_pause (ValueError naming both).  timing needs the text: bind(tokens) --
    called by the model once the requests are tokenised, before anything is launched -- checks the number of entries against the words of each request
    (_TTS._word_groups) and turns them into one start per text token (`starts`), which kw(idx) hands to the engine."""

    def __init__(self, model, B=1, one=True, *, seeds=None, generator=None, speed=None, sample_rate=None, encoding=None, loudness=None, max_pause=None, pause_db=40.0,
                 pitch=None, word_times=False, guard=None, segments=True, duration=None, timing=None, true_peak=None, bed=None):
        self.model, self.one, self.generator = model, one, generator
        self.fmt = ops.check_format(sample_rate, encoding)
        self.words = None if word_times is None or word_times is False else model._word_mode(word_times, max_pause)
        if self.words is not None and not segments:
            raise ValueError("word_times without return_segments: the words of generate_long travel in its segments")
        self.seeds = _request_seeds(seeds, B, one, generator)
        self.speed = ops.check_speed(speed, B)
        if one and isinstance(loudness, (list, tuple)):
            raise TypeError(f"loudness: expected None or a number, got a {type(loudness).__name__}")
        self.loud = ops.check_loudness(loudness, B)
        if one and isinstance(true_peak, (list, tuple)):
            raise TypeError(f"true_peak: expected None or a number of dBTP, got a {type(true_peak).__name__}")
        self.peak = ops.check_true_peak(true_peak, B)
        self.bed = ops.check_bed(bed)  # (generate_dialogue / generate_long: the plan of the music bed, or None; it never travels in a job)
        self.pz = _pauses(max_pause, pause_db, B, one)
        if one and isinstance(pitch, (list, tuple)):
            raise TypeError(f"pitch: expected None or a number of semitones, got a {type(pitch).__name__}")
        self.pitch = ops.check_pitch(pitch, B)
        ops.check_speed_pitch(self.speed, self.pitch, B)
        self.guard = None if guard is None or guard is False else model._guard(guard)
        if one and isinstance(duration, (list, tuple)):
            raise TypeError(f"duration: expected None or a number of seconds, got a {type(duration).__name__}")
        self.dur = ops.check_duration(duration, B)
        self.timing = ops.check_timing([timing] if one and timing is not None else timing, B)
        self.starts = None
        if self.timing is not None and not hasattr(getattr(model, "tokenizer", None), "pieces"):
            raise ValueError("timing needs a tokenizer with pieces(ids) to group text tokens into words (model.words(text) names them)")
        for mine, on in (("duration", self.dur), ("timing", self.timing)):
            for other, v in (("speed", self.speed), ("pitch", self.pitch), ("max_pause", self.pz)):
                if on is not None and v is not None:
                    raise ValueError(f"{mine} together with {other}: the time map fixes when things happen; combining it with {other} is not built -- give one of the two")

    @property
    def warped(self):
        return self.dur is not None or self.timing is not None

    def bind(self, tokens):
        """The requests' engine tokens (B 1-D id tensors) -> self, with timing turned into `starts`: per request None or one output frame / None per TEXT TOKEN
        (word i's start at its first token).  A wrong number of entries is a ValueError -- before anything is launched."""
        if self.timing is None:
            return self
        self.starts = []
        for b, (row, tok) in enumerate(zip(self.timing, tokens)):
            if row is None:
                self.starts.append(None)
                continue
            groups, texts = self.model._word_groups(tok)
            if len(row) != len(groups):
                raise ValueError(f"timing{'' if self.one else f'[{b}]'}: {len(row)} entries for {len(groups)} words {texts!r} (model.words(text) lists them)")
            per_token = [None] * int(tok.numel())
            for (a, _), t in zip(groups, row):
                per_token[a] = t
            self.starts.append(None if all(t is None for t in row) else per_token)
        if all(st is None for st in self.starts):  # no word of any request has a time: the call without the argument
            self.timing = self.starts = None
        return self

    def warp_kw(self, idx):
        """The engines' warp= list over the requests `idx`, or None when none of them is warped"""
        if not self.warped:
            return None
        assert self.timing is None or self.starts is not None, "timing: bind(tokens) comes first"
        out = []
        for i in idx:
            d, st = None if self.dur is None else self.dur[i], None if self.starts is None else self.starts[i]
            out.append(dict(starts=st, end=d) if st is not None else (None if d is None else dict(frames=d)))
        return None if all(w is None for w in out) else out

    def kw(self, idx, chunks=False):
        """The engines' keywords of a call or job over the requests `idx`, the call without an option being exactly the call before there was one: seeds and speed
        are present when given at all; loudness, true_peak, pauses and pitch only when a request in idx uses them; the format unless a watermarker is loaded (it works on the
        24 kHz fp32 waveform: the conversion then follows it, in _finish); words and guard, one setting for the call, with the model's align_heads.
        chunks=True (long form): idx are chunks of the ONE request.  Every chunk carries the request's options, chunk k the seed chunk_seed(seed, k); loudness,
        true_peak and the format are held back from the jobs -- the assembled whole is normalised, limited and converted once."""
        rows = (lambda v: [v[0]] * len(idx)) if chunks else (lambda v: _pick(v, idx))
        kw = {}
        if self.seeds is not None:
            kw["seeds"] = [chunk_seed(self.seeds[0], k) for k in idx] if chunks else rows(self.seeds)
        if self.speed is not None:
            kw["speed"] = rows(self.speed)
        if self.loud is not None and not chunks and any(v is not None for v in rows(self.loud)):
            kw["loudness"] = self.loud[0] if self.one else rows(self.loud)
        if self.peak is not None and not chunks and any(v is not None for v in rows(self.peak)):
            kw["true_peak"] = self.peak[0] if self.one else rows(self.peak)
        if self.pz is not None and any(rows(self.pz["keep"])):
            kw["pauses"] = dict(self.pz, keep=rows(self.pz["keep"]))
        if self.pitch is not None and any(rows(self.pitch)):
            kw["pitch"] = rows(self.pitch)
        if self.fmt is not None and not chunks and self.model.watermarker is None:
            kw["format"] = self.fmt
        if self.words is not None or self.timing is not None:  # (timing implies the alignment pass: one setting for the call)
            kw["words"] = dict(heads=self.model.align_heads)
        if self.guard is not None:
            kw["guard"] = self.guard
        if not chunks and self.warp_kw(idx) is not None:
            kw["warp"] = self.warp_kw(idx)
        return kw


def _stream_speed_kw(speed):
    """generate_stream's `speed` as the engines' speed= keyword: ONE number in [0.5, 2.0] for the stream ({} at 1.0 / None).  TypeError / ValueError
    (engine.check_stream_speed) before anything is launched."""
    from .engine import check_stream_speed
    speed = check_stream_speed(speed)
    return {} if speed is None else dict(speed=speed)



# ---------------------------------------------------------------------------------------------------------------- generate_batch: host-side plumbing
def _per_request(value, B, name, one):
    """A per-request argument as a list of B.  `one` names the types that are ONE entry of this argument (a path, a Conditionals, a language id, ...): such a value,
    or None, serves every request; anything else must be a list or tuple of exactly B entries (ValueError before anything is launched).  A (waveform, sample_rate)
    pair is an entry, never the whole argument: it goes inside a list."""
    if value is None or isinstance(value, one):
        return [value] * B
    if not isinstance(value, (list, tuple)):
        raise TypeError(f"{name}: expected {' / '.join(t.__name__ for t in one)} or a list of {B}, got {type(value).__name__}")
    if len(value) != B:
        raise ValueError(f"{name}: {len(value)} entries for {B} requests")
    return list(value)


_PATH = (str, bytes, os.PathLike)


# ---------------------------------------------------------------------------------------------------------------- generate_long: host-side plumbing
CHUNK_SEED_STEP = 0x9E3779B97F4A7C15  # 2^64 / golden ratio: consecutive chunks get seeds that are far apart


def chunk_seed(seed, k):
    """The seed of chunk k of a seeded generate_long call: (seed + k * 0x9E3779B97F4A7C15) mod 2^64.  Chunk 0 uses `seed` itself, so a one-chunk text draws as
    generate(seed=) does."""
    return (int(seed) + int(k) * CHUNK_SEED_STEP) % (1 << 64)


def _long_args(max_chars, pause, paragraph_pause, trim_db, trim_pad, join_fade, seed, speed, cjk):
    """generate_long's own arguments, validated when the method is CALLED (TypeError / ValueError before anything is launched) -> dict(max_chars, pause,
    paragraph_pause, trim_db, trim_pad, join_fade, seed, speed: a float, or None at 1.0)."""
    import math
    import numbers
    is_int = lambda v: isinstance(v, int) and not isinstance(v, bool)
    is_num = lambda v: isinstance(v, numbers.Real) and not isinstance(v, bool)
    if max_chars is None:
        max_chars = default_max_chars(cjk)
    if not is_int(max_chars):
        raise TypeError(f"max_chars: expected None or an int, got {type(max_chars).__name__}")
    if max_chars < 1:
        raise ValueError(f"max_chars = {max_chars}: expected an int >= 1")
    for name, v in (("pause", pause), ("paragraph_pause", paragraph_pause)):
        if not is_num(v):
            raise TypeError(f"{name}: expected a number of seconds, got {type(v).__name__}")
        if not math.isfinite(v) or not 0.0 <= v <= 60.0:
            raise ValueError(f"{name} = {v}: expected a finite number of seconds in [0, 60]")
    if trim_db is not None:
        if not is_num(trim_db):
            raise TypeError(f"trim_db: expected None or a number, got {type(trim_db).__name__}")
        if not math.isfinite(trim_db) or trim_db < 0.0:
            raise ValueError(f"trim_db = {trim_db}: expected None or a finite number >= 0")
        trim_db = float(trim_db)
    for name, v in (("trim_pad", trim_pad), ("join_fade", join_fade)):
        if not is_int(v):
            raise TypeError(f"{name}: expected an int, got {type(v).__name__}")
        if not 0 <= v <= 1 << 20:
            raise ValueError(f"{name} = {v}: expected an int in [0, 2^20]")
    seed, speed = _request_seeds(seed), ops.check_speed(speed, 1)
    return dict(max_chars=max_chars, pause=float(pause), paragraph_pause=float(paragraph_pause), trim_db=trim_db, trim_pad=trim_pad, join_fade=join_fade,
                seed=None if seed is None else seed[0], speed=None if speed is None else speed[0])


def _long_numbers(**params):
    """generate_long's sampling arguments: one finite number each for the whole text (TypeError / ValueError before anything is launched)"""
    import math
    import numbers
    for name, v in params.items():
        if not isinstance(v, numbers.Real) or isinstance(v, bool):
            raise TypeError(f"{name}: expected a number, got {type(v).__name__}")
        if not math.isfinite(v):
            raise ValueError(f"{name} = {v}: expected a finite number")


def _long_stream_args(first_batch, batch_growth):
    """generate_long_stream's own arguments, validated when the method is CALLED -> (first_batch: None or an int >= 1, batch_growth: a finite float >= 1)"""
    import math
    import numbers
    if first_batch is not None:
        if not isinstance(first_batch, int) or isinstance(first_batch, bool):
            raise TypeError(f"first_batch: expected None or an int, got {type(first_batch).__name__}")
        if first_batch < 1:
            raise ValueError(f"first_batch = {first_batch}: expected None or an int >= 1")
    if not isinstance(batch_growth, numbers.Real) or isinstance(batch_growth, bool):
        raise TypeError(f"batch_growth: expected a number, got {type(batch_growth).__name__}")
    if not math.isfinite(batch_growth) or batch_growth < 1.0:
        raise ValueError(f"batch_growth = {batch_growth}: expected a finite number >= 1")
    return first_batch, float(batch_growth)


def _long_jobs(chunks, max_batch, a, sizes=None):
    """long_plan / long_stream_plan: the chunks in text order, cut into consecutive groups of `sizes` (an iterable of group sizes, each clipped to
    [1, min(max_batch, 64)]; None: every group is that step) and each group as a job."""
    import itertools
    step = max(1, min(int(max_batch), ops.WAVE_JOIN_MAX_ROWS))
    rate = 1.0 if a["speed"] is None else a["speed"]
    gap = lambda para_end: int(round((a["paragraph_pause"] if para_end else a["pause"]) * S3GEN_SR / rate))
    groups, lo = [], 0
    for size in itertools.repeat(step) if sizes is None else sizes:
        if lo >= len(chunks):
            break
        size = max(1, min(int(size), step))
        groups.append(list(range(lo, min(lo + size, len(chunks)))))
        lo += size
    jobs = []
    for g, idx in enumerate(groups):
        job = dict(chunks=idx, join=dict(gaps=[gap(chunks[k][1]) for k in idx], trim_db=a["trim_db"], pad_frames=a["trim_pad"], fade=a["join_fade"], first=g == 0,
                                         last=g == len(groups) - 1))
        if a["seed"] is not None:
            job["seeds"] = [chunk_seed(a["seed"], k) for k in idx]
        if a["speed"] is not None:
            job["speed"] = [a["speed"]] * len(idx)
        jobs.append(job)
    return jobs


def long_plan(chunks, max_batch, a):
    """The jobs of a generate_long call, WITHOUT their tokens and voices: chunks = split_text's list, a = _long_args' dict.  Chunks keep the text's order (no length
    sort: a piece is a run of consecutive chunks) and are cut into consecutive device batches of at most max_batch (and at most 64, the join's row limit).  Per job:
    dict(chunks=[indices], join=the engines' join dict, seeds=[...] if seeded, speed=[...] if not 1.0) -- the seeds and speeds _Options.kw(chunks=True) gives the
    engine jobs, next to the other options.  The gap behind a chunk is round(pause * 24000 / speed)
    samples, paragraph_pause behind a paragraph's last chunk; the first job carries first=True, the last one last=True."""
    return _long_jobs(chunks, max_batch, a)


def long_stream_plan(chunks, max_batch, a, first_batch=1, batch_growth=2.0):
    """The jobs of a generate_long_stream call: long_plan's, with device batches that start small so that the first piece comes early.  With
    step = min(max_batch, 64) the group sizes are s_0 = min(first_batch, step), s_(g+1) = min(step, max(s_g, ceil(s_g * batch_growth))); chunks stay in text order,
    and gaps, first / last, chunk seeds and speed are exactly long_plan's.  first_batch=None IS long_plan."""
    import math
    if first_batch is None:
        return long_plan(chunks, max_batch, a)
    step = max(1, min(int(max_batch), ops.WAVE_JOIN_MAX_ROWS))

    def sizes():
        size = min(int(first_batch), step)
        while True:
            yield size
            size = min(step, max(size, math.ceil(size * batch_growth)))
    return _long_jobs(chunks, max_batch, a, sizes())


# ---------------------------------------------------------------------------------------------------------------- generate_dialogue: host-side plumbing
DIALOGUE_TURN_PAUSE = 0.3   # seconds between two turns: an UNMEASURED default -- nobody has tuned it on trained weights
DIALOGUE_BALANCE = -23.0    # balance=True: the LUFS level every voice is brought to (EBU R 128's programme level): an UNMEASURED default
DIALOGUE_GAP = 60.0         # |gap| and |turn_pause| of a turn, seconds
DIALOGUE_TURN_KEYS = ("voice", "text", "gap", "speed", "pitch", "exaggeration", "pan")
DIALOGUE_PAN_SPREAD = 0.3   # pan=True: the distinct voices are spread evenly over [-0.3, +0.3]: an UNMEASURED default -- nobody has tuned it by listening
DIALOGUE_MAX_VOICES = ops.WAVE_JOIN_MAX_ROWS   # the meter of balance= takes one row per voice


def _dialogue_gap(v, name):
    import numbers
    if not isinstance(v, numbers.Real) or isinstance(v, bool):
        raise TypeError(f"{name}: expected a number of seconds, got {type(v).__name__}")
    if not math.isfinite(v) or not -DIALOGUE_GAP <= v <= DIALOGUE_GAP:
        raise ValueError(f"{name} = {v}: expected a finite number of seconds in [-{DIALOGUE_GAP:g}, {DIALOGUE_GAP:g}] (negative: the turn starts that long before "
                         "the front of the conversation)")
    return float(v)


def _dialogue_balance(balance):
    """balance= of generate_dialogue -> None, or the LUFS level every voice is brought to (True: DIALOGUE_BALANCE)"""
    if balance is None or balance is False:
        return None
    if balance is True:
        return DIALOGUE_BALANCE
    if isinstance(balance, (list, tuple)):
        raise TypeError(f"balance: expected None, True or a number of LUFS, got a {type(balance).__name__}")
    return ops.check_loudness(balance, 1, "balance")[0]


def _dialogue_pan(pan, ts, keys, bed=None):
    """pan= of generate_dialogue -> None (mono: today's call), or dict(voices=[position per distinct voice, in the order of `keys`], rows=[position per turn]).
    pan: None; True (the distinct voices spread evenly over [-DIALOGUE_PAN_SPREAD, +DIALOGUE_PAN_SPREAD] in order of first appearance, one voice at 0); or a dict
    voice key -> position in [-1, 1] (a voice not named sits at 0; a key that no turn uses is a ValueError).  A turn's own pan= overrides its voice's place for that
    turn, and needs pan= on the call.  Raised when the method is called: TypeError for wrong types and bools where a number belongs, ValueError for the rest."""
    if pan is None or pan is False:
        for t, turn in enumerate(ts):
            if turn["pan"] is not None:
                raise ValueError(f"turns[{t}]: pan: a turn is placed only in a stereo call; pass pan=True or pan={{voice: position}} to generate_dialogue")
        return None
    if bed is not None:
        raise ValueError("bed= together with pan= is not built: a stereo bed needs a linked ducking kernel and an ingest that keeps the channels")
    if pan is True:
        V = len(keys)
        place = [0.0 if V == 1 else -DIALOGUE_PAN_SPREAD + 2.0 * DIALOGUE_PAN_SPREAD * v / (V - 1) for v in range(V)]
    elif isinstance(pan, dict):
        for k, v in pan.items():
            try:
                known = k in keys
            except TypeError:
                known = False
            if not known:
                raise ValueError(f"pan: voice {k!r} speaks no turn of the script ({sorted(map(repr, keys))})")
            ops.check_pan(v, f"pan[{k!r}]")
        place = [ops.check_pan(pan.get(k, 0.0), f"pan[{k!r}]") for k in keys]
    else:
        raise TypeError(f"pan: expected None, True or a dict of voice key -> position in [-1, 1], got {type(pan).__name__}")
    return dict(voices=place, rows=[place[keys.index(t["voice"])] if t["pan"] is None else t["pan"] for t in ts])


def _dialogue_turns(turns, voices, turn_pause, exaggeration, language_id=None, multilingual=False):
    """generate_dialogue's script, validated when the method is CALLED (TypeError: wrong types, unknown dict keys, a bool where a number belongs, `turns` not a
    list; ValueError: values out of range or not finite, an unknown voice key, empty text) -> one dict(voice, text, gap, speed, pitch, exaggeration, language_id)
    per turn: speed a float (1.0: none), pitch a float (0.0: none), language_id lower case or None."""
    if not isinstance(turns, list):
        raise TypeError(f"turns: expected a list of (voice, text) pairs or dicts, got {type(turns).__name__}")
    if not turns:
        raise ValueError("turns: expected at least one turn")
    if voices is not None and not isinstance(voices, dict):
        raise TypeError(f"voices: expected None or a dict of voice key -> Conditionals / voice prompt, got {type(voices).__name__}")
    turn_pause = _dialogue_gap(turn_pause, "turn_pause")
    keys = DIALOGUE_TURN_KEYS + (("language_id",) if multilingual else ())
    out = []
    for t, turn in enumerate(turns):
        name = f"turns[{t}]"
        if isinstance(turn, dict):
            extra = set(turn) - set(keys)
            if extra or "text" not in turn:
                raise TypeError(f"{name}: keys {sorted(map(str, turn))}: `text` is required, the others are {[k for k in keys if k != 'text']}")
            turn = dict(turn)
        elif isinstance(turn, (tuple, list)) and len(turn) == 2:
            turn = dict(voice=turn[0], text=turn[1])
        else:
            raise TypeError(f"{name}: expected a (voice, text) pair or a dict with {keys}, got {type(turn).__name__}")
        voice, text = turn.get("voice"), turn["text"]
        if not isinstance(text, str):
            raise TypeError(f"{name}: text: expected a str, got {type(text).__name__}")
        if not text.strip():
            raise ValueError(f"{name}: text is empty")
        if voice is not None:
            try:
                known = voices is not None and voice in voices
            except TypeError:
                raise TypeError(f"{name}: voice: expected None or a key of `voices`, got {type(voice).__name__}") from None
            if not known:
                raise ValueError(f"{name}: voice {voice!r} is not a key of `voices` ({sorted(map(repr, voices or {}))})")
        gap = turn_pause if turn.get("gap") is None else _dialogue_gap(turn["gap"], f"{name}: gap")
        for key in ("speed", "pitch"):
            if isinstance(turn.get(key), (list, tuple)):
                raise TypeError(f"{name}: {key}: expected None or a number, got a {type(turn[key]).__name__}")
        speed, pitch = ops.check_speed(turn.get("speed"), 1, f"{name}: speed"), ops.check_pitch(turn.get("pitch"), 1, f"{name}: pitch")
        try:
            ops.check_speed_pitch(speed, pitch, 1)
        except ValueError as e:
            raise ValueError(f"{name}: {e}") from None
        place = None if turn.get("pan") is None else ops.check_pan(turn["pan"], f"{name}: pan")
        ex = exaggeration if turn.get("exaggeration") is None else turn["exaggeration"]
        _long_numbers(**{f"{name}: exaggeration": ex})
        lid = language_id
        if multilingual and turn.get("language_id") is not None:
            if not isinstance(turn["language_id"], str):
                raise TypeError(f"{name}: language_id: expected a str, got {type(turn['language_id']).__name__}")
            lid = _language(turn["language_id"], f" (turn {t})")
        out.append(dict(voice=voice, text=text, gap=gap, speed=1.0 if speed is None else speed[0], pitch=0.0 if pitch is None else pitch[0], exaggeration=ex,
                        language_id=lid, pan=place))
    return out


def dialogue_plan(turns, max_batch, a):
    """The rows and jobs of a generate_dialogue call, WITHOUT their tokens and voices.  turns: one dict(chunks=split_text's list of the turn's text, gap=seconds
    before the turn, speed=, pitch=) per turn (speed / pitch may be missing: 1.0 / 0.0); a: _long_args' dict.  The rows are the chunks in script order; chunk k,
    counted over the whole script, is seeded with chunk_seed(seed, k).  Returns dict(rows, jobs):
    rows[k] = dict(turn, text, after): `after` is ops.mix_layout's signed count of samples behind the row -- round(pause * 24000 / speed) behind an inner chunk
      of a turn (paragraph_pause behind a paragraph's last chunk; the turn's speed, as long_plan computes it), round(gap * 24000) of the NEXT turn behind a
      turn's last chunk (not scaled by speed; negative: an overlap), 0 behind the last row of all;
    jobs: the rows cut into consecutive device batches of at most max_batch (and at most 64), no length sort, as long_plan cuts them; per job dict(chunks=[row
      indices], join=the engines' join dict, seeds=[...] if seeded, speed=[...] if any row of the SCRIPT is scaled, pitch=[...] if a row of the job is
      transposed).  The join has zero gaps and no fade, first = last = True: a job's piece is its trimmed rows back to back, and the mixer places and fades them."""
    rows = []
    for t, turn in enumerate(turns):
        rate = float(turn.get("speed") or 1.0)
        for c, (text, para_end) in enumerate(turn["chunks"]):
            if c + 1 < len(turn["chunks"]):
                after = int(round((a["paragraph_pause"] if para_end else a["pause"]) * S3GEN_SR / rate))
            else:
                after = int(round(turns[t + 1]["gap"] * S3GEN_SR)) if t + 1 < len(turns) else 0
            rows.append(dict(turn=t, text=text, after=after, speed=rate, pitch=float(turn.get("pitch") or 0.0)))
    step = max(1, min(int(max_batch), ops.WAVE_JOIN_MAX_ROWS))
    scaled = any(r["speed"] != 1.0 for r in rows)
    jobs = []
    for lo in range(0, len(rows), step):
        idx = list(range(lo, min(lo + step, len(rows))))
        job = dict(chunks=idx, join=dict(gaps=[0] * len(idx), trim_db=a["trim_db"], pad_frames=a["trim_pad"], fade=0, first=True, last=True))
        if a["seed"] is not None:
            job["seeds"] = [chunk_seed(a["seed"], k) for k in idx]
        if scaled:
            job["speed"] = [rows[k]["speed"] for k in idx]
        if any(rows[k]["pitch"] for k in idx):
            job["pitch"] = [rows[k]["pitch"] for k in idx]
        jobs.append(job)
    return dict(rows=[dict(turn=r["turn"], text=r["text"], after=r["after"]) for r in rows], jobs=jobs)


# T3 cond dicts of a voice, kept while its T3Cond lives (generate_batch): id(T3Cond) -> [emotion tensor the entry was built from, its value, {exaggeration: dict}]
_T3_DICTS = {}


def _t3_dict(t3, exaggeration):
    """The cond dict of voice `t3` at `exaggeration`: one dict over the voice's own tensors at its own exaggeration, else with the emotion tensor `generate` would
    build.  The same dict from call to call, so the engines' voice-prefix cache (which matches tensors by identity) hits; dropped when the voice is garbage."""
    import weakref
    ent = _T3_DICTS.get(id(t3))
    if ent is None or ent[0] is not t3.emotion_adv:  # first sight of this voice (or its emotion was replaced): read its value once
        if ent is None:
            weakref.finalize(t3, _T3_DICTS.pop, id(t3), None)
        own = None if t3.emotion_adv is None else float(torch.as_tensor(t3.emotion_adv).reshape(-1)[0])
        ent = _T3_DICTS[id(t3)] = [t3.emotion_adv, own, {}]
    key = None if (ent[1] is None or ent[1] == float(exaggeration)) else float(exaggeration)
    d = ent[2].get(key)
    if d is None or d["speaker_emb"] is not t3.speaker_emb or d["cond_prompt_speech_tokens"] is not t3.cond_prompt_speech_tokens:  # (T3Cond.to() replaces tensors)
        d = ent[2][key] = t3.as_dict() if key is None else dict(t3.as_dict(), emotion_adv=key * torch.ones(1, 1, 1))
    return d


def batch_plan(lengths, max_batch):
    """Execution order of a batch: requests sorted by length (stable), cut into consecutive sub-batches of at most `max_batch`; each sub-batch is a list of the
    caller's indices.  Neighbours in length share a sub-batch, which keeps the padding of the prefill and of the flow down."""
    assert max_batch >= 1
    order = sorted(range(len(lengths)), key=lambda i: (lengths[i], i))
    return [order[lo:lo + max_batch] for lo in range(0, len(order), max_batch)]


def _batch_of(texts):
    """generate_batch's texts as a list of B >= 1: one str is a batch of one"""
    texts = [texts] if isinstance(texts, str) else list(texts)
    assert len(texts) >= 1, "empty batch"
    return texts


def _sampling_lists(B, **params):
    from .t3 import per_utterance
    return {k: per_utterance(v, B, k) for k, v in params.items()}


def _one_or_list(items):
    """One object when every request uses the very same one (the engines' single-voice path), else the list."""
    return items[0] if all(it is items[0] for it in items) else list(items)


def _pick(lst, idx):
    return [lst[i] for i in idx]


def _voice_key(wav):
    """What makes two voice prompts of one call the same prompt: a path by its name, a (waveform, sample_rate) pair by identity."""
    return os.fspath(wav) if isinstance(wav, _PATH) else id(wav)


def _analysed_once(requests, analyse):
    """analyse(wav, *rest) for every (wav, *rest) of `requests`, in their order; requests that are equal (_voice_key, and equal rest) are analysed once per call and
    share the result."""
    done, out = {}, []
    for wav, *rest in requests:
        key = (_voice_key(wav), *rest)
        if key not in done:
            done[key] = analyse(wav, *rest)
        out.append(done[key])
    return out


_NO_VOICE = "Please `prepare_conditionals` first or specify `audio_prompt_path`"


WORD_TIMES_PAUSE = ("max_pause together with word_times: the pause step's cut map is data on the device, and mapping word boundaries through it is not built "
                    "-- ask for one of the two")


def _word_times(word_times, max_pause=None):
    """word_times of generate / generate_batch / generate_long -> None (False / None: the call without the argument), "words" (True / "words") or "tokens"."""
    if word_times is None or word_times is False:
        return None
    mode = "words" if word_times is True else word_times
    if mode not in ("words", "tokens"):
        raise ValueError(f'word_times: expected False, True, "words" or "tokens", got {word_times!r}')
    pauses = max_pause if isinstance(max_pause, (list, tuple)) else [max_pause]
    if any(v is not None for v in pauses):
        raise ValueError(WORD_TIMES_PAUSE)
    return mode


def _no_true_peak(method, true_peak):
    """generate_long_stream lists true_peak only because its signature is generate_long's plus the ramp; anything but None is refused as an argument the method
    does not take"""
    if true_peak is not None:
        raise TypeError(f"{method}() does not take true_peak: a running limiter needs a look-ahead carried from piece to piece, which is not built -- use "
                        "generate_long(true_peak=...)")


def _no_bed(method, bed):
    """generate_long_stream lists bed only because its signature is generate_long's plus the ramp; anything but None is refused as an argument the method does
    not take"""
    if bed is not None:
        raise TypeError(f"{method}() does not take bed: ducking looks ahead of every word over the WHOLE signal, and a running form carried from piece to piece "
                        "is not built -- use generate_long(bed=...)")


def _no_word_times(method, word_times):
    """generate_long_stream lists word_times only because its signature is generate_long's plus the ramp; anything but False / None is refused as an argument the
    method does not take"""
    if word_times is not None and word_times is not False:
        raise TypeError(f"{method}() does not take word_times: a stream has no finished token sequence for the alignment pass to read -- use generate_long("
                        "return_segments=True, word_times=...)")


class _Finish:
    """The epilogue of every public method that returns audio, and the `audio_in` switch of every method that takes audio."""
    sr = S3GEN_SR
    last_bed = None  # of the last generate_dialogue / generate_long call: None, or with bed= dict(gain, speech_lufs, bed_lufs, ducked, frames, peak)
    last_fit = None  # per request of the last call with duration= / timing=, in the caller's order: None (a plain request) or the engine's fit report

    def _take_fit(self, reports, who):
        """model.last_fit = the engine's fit reports (engine._fit_report) in the caller's order; one UserWarning names the requests whose targets were not met"""
        self.last_fit = reports
        odd = [(i, r) for i, r in enumerate(reports) if r is not None and r["clamped"]]
        if odd:
            import warnings
            warnings.warn(f"{who}: the time map of request(s) " + ", ".join(f"{i} (asked {r['target']} frames, got {r['frames']}; missed: {r['clamped']})" for i, r in odd)
                          + " was clamped to rates in [0.5, 2.0]: nothing is padded or cut (model.last_fit has the plan)", UserWarning, stacklevel=3)

    @property
    def audio_in(self):
        """Where audio inputs (voice prompts, conversion sources, target voices) are decoded, mixed down, resampled and trimmed: "host" (the default: NumPy / SciPy
        in fp64, every call as it always was) or "device" (the raw bytes are uploaded; cbx_wave_ingest and cbx_wave_trim_edges_f32 do it in fp32, so results differ
        from host mode in rounding).  It lives on the analyzer (frontend.PromptAnalyzer.audio_in)."""
        return getattr(self.analyzer, "audio_in", "host") if self.analyzer is not None else getattr(self, "_audio_in", "host")

    @audio_in.setter
    def audio_in(self, value):
        value = _check_audio_in_mode(value)
        if self.analyzer is not None:
            self.analyzer.audio_in = value
        else:
            self._audio_in = value

    def _finish(self, wav, fmt=None, converted=True, loud=None, peak=None, bed=None):
        """A device waveform as the reference returns it: CPU float32 (1, n), watermarked if a watermarker is loaded.
        fmt (ops.check_format's dict; None: exactly the above): the (1, n) CPU tensor at fmt's rate in fmt's encoding.  Without a watermarker the engine was given the
        format and `wav` is the converted audio already (converted=True): one copy to the host.  With one -- or when the caller kept the format from the engine
        (converted=False: generate_long) -- `wav` is 24 kHz fp32 and goes through the chain (_chain): it is watermarked on the host as ever, then converted on the device.
        loud (a LUFS target), peak (a ceiling in dBTP), bed ((plan, source) of _bed_source) -- generate_long's: the chain's steps ahead of the watermark, over the
        24 kHz waveform as ONE signal, in the same visit to the device."""
        if fmt is not None and converted and self.watermarker is None:
            return wav.detach().cpu().unsqueeze(0)
        return self._chain(wav.detach().float(), fmt, loud, peak, bed).unsqueeze(0)

    def _device_scope(self):
        dev = torch.device(self.engine.dev)
        return dev, (torch.cuda.device(dev) if dev.type == "cuda" else contextlib.nullcontext())

    def _chain(self, w, fmt=None, loud=None, peak=None, bed=None):
        """THE finishing chain of generate_long and generate_dialogue.  w: 24 kHz fp32, 1-D or planar (2, n), on the host or on the device.  In this order:
          the bed (bed: (plan, source) of _bed_source; _lay_bed; mono only) -- the meter and the limiter then see speech plus bed;
          loudness and true peak over the whole as ONE signal.  With a ceiling (peak, dBTP) the meter gives the FULL gain to the target (loud, LUFS; no gain
            without one) and the limiter takes it as its pre-gain; without a ceiling the gain is capped at a sample peak of 1.0 and applied in place.  Mono:
            ops.wave_loudness, ops.wave_limit, ops.wave_normalize.  Two planes, linked: ops.wave_loudness_ch, ops.wave_limit_ch, and ops.wave_gain with the one
            gain for both.  The stats stay on the device as engine.last_loudness / engine.last_limit;
          the watermark on the host, per channel, if a watermarker is loaded;
          the format (_to_format) and the one copy to the host; then model.last_bed (_take_bed).
        Nothing is uploaded before a step needs the device, and what is there stays there: without a watermarker a call makes ONE visit, with one the round trip
        to the host lies between the limiter and the format.  Returns the CPU tensor, 1-D or (2, n') as w was."""
        stereo = w.dim() == 2
        rows = (lambda t: [t[0], t[1]]) if stereo else (lambda t: [t])
        if bed is not None or loud is not None or peak is not None:
            dev, scope = self._device_scope()
            with scope:
                w = w.to(dev).contiguous()
                if bed is not None:
                    w = self._lay_bed(w, *bed)
                if peak is not None:
                    pre = None
                    if loud is not None:
                        self.engine.last_loudness, pre = (ops.wave_loudness_ch if stereo else ops.wave_loudness)(rows(w), [float(loud)], None)
                    if stereo:
                        lim = torch.empty_like(w)
                        _, self.engine.last_limit = ops.wave_limit_ch(rows(w), [float(peak)], gain=pre, out=rows(lim))
                        w = lim
                    else:
                        out, self.engine.last_limit = ops.wave_limit(rows(w), [float(peak)], gain=pre)
                        w = out[0]
                elif loud is not None and stereo:
                    self.engine.last_loudness, g1 = ops.wave_loudness_ch(rows(w), [float(loud)], 1.0)
                    ops.wave_gain(rows(w), g1.repeat(2))
                elif loud is not None:
                    self.engine.last_loudness = ops.wave_normalize(rows(w), [float(loud)])
        if self.watermarker is not None:
            mark = lambda x: torch.from_numpy(self.watermarker.apply_watermark(x, sample_rate=self.sr))
            host = w.cpu().numpy()
            w = torch.stack([mark(host[c]) for c in range(2)]) if stereo else mark(host)
        w = w.cpu() if fmt is None else self._to_format(w, fmt)
        if bed is not None:
            self._take_bed()
        return w

    def _to_format(self, w, fmt):
        """The chain's format step: 24 kHz fp32, 1-D or planar (2, n), on the host or already on the device -> ONE ops.wave_format launch (the planes as two
        rows), then the copy to the host"""
        dev, scope = self._device_scope()
        with scope:
            w = w.to(dev)
            out = ops.wave_format([w[0], w[1]] if w.dim() == 2 else [w], fmt)
            return (torch.stack(out) if w.dim() == 2 else out[0]).cpu()

    def _bed_source(self, plan):
        """The source of a music bed (plan: ops.check_bed's) at 24 kHz mono, brought there as a voice prompt is: a float32 host array (audio_in = "host":
        _load_wave) or a 1-D fp32 device tensor (audio_in = "device": PromptAnalyzer.ingest, ops.wave_ingest).  Read when the method is called, before the engine
        runs.  ValueError naming `bed` for an empty source and for one that cannot loop (no longer than twice the cross-fade)."""
        import numpy as np
        if self.audio_in == "device":
            from types import SimpleNamespace
            from .frontend import PromptAnalyzer
            # (ingest reads its analyzer's device alone: a model built without the prompt networks lends it the engine's)
            who = self.analyzer if self.analyzer is not None else SimpleNamespace(dev=torch.device(self.engine.dev), raw_form=PromptAnalyzer.raw_form)
            src = PromptAnalyzer.ingest(who, [plan["audio"]], S3GEN_SR)[0]
            nb = int(src.numel())
        else:
            src = np.ascontiguousarray(_load_wave(plan["audio"], S3GEN_SR), dtype=np.float32).reshape(-1)
            nb = int(src.size)
        if nb == 0:
            raise ValueError("bed: the audio is empty")
        if plan["loop"] and nb <= 2 * plan["xf"]:
            raise ValueError(f"bed: a source of {nb} samples at 24 kHz cannot loop with a cross-fade of {plan['xf']} samples (loop_fade): it must be longer than twice that")
        return src

    def _lay_bed(self, w, plan, src):
        """The bed step on the device, inside the caller's scope and visit: w (1-D fp32, the finished speech) -> speech over the ducked bed (ops.bed_len(n, plan)
        samples).  Two measure-only ops.wave_loudness calls -- the speech as it is, the bed over its whole source -- feed ops.wave_duck_level, whose gain
        ops.wave_duck applies.  Nothing is synchronised: the numbers of model.last_bed wait on the device (_take_bed)."""
        b = src if torch.is_tensor(src) else torch.from_numpy(src).to(w.device)
        silent = lambda: torch.tensor([[float("-inf"), 0.0, 1.0, 0.0]], dtype=torch.float64).to(w.device)
        ss = ops.wave_loudness([w], None, None)[0] if w.numel() else silent()
        sb = ops.wave_loudness([b], None, None)[0]
        out, st = ops.wave_duck([w], [b], plan, gain=ops.wave_duck_level(ss, sb, plan["level"]))
        self._bed_numbers = torch.cat([st.reshape(-1), ss[0, :1], sb[0, :1]])
        return out[0]

    def _take_bed(self):
        """model.last_bed from the six numbers _lay_bed left on the device: one small copy beside the audio's"""
        g, ducked, frames, peak, ls, lb = self._bed_numbers.cpu().tolist()
        self._bed_numbers = None
        self.last_bed = dict(gain=g, speech_lufs=ls, bed_lufs=lb, ducked=int(ducked), frames=int(frames), peak=peak)

    def _stream_pieces(self, rounds, fmt):
        """The pieces of generate_stream from an engine stream's rounds: (1, n) CPU tensors, empty ones left out.  With a format and a watermarker every piece is
        watermarked as 24 kHz fp32 and then goes through an ops.WaveFormatStream held here, so the pieces add up to the conversion of the whole."""
        conv = None
        for r in rounds:
            w = r["wavs"][0]
            if fmt is None or self.watermarker is None:
                if w.numel():
                    yield self._finish(w, fmt)
                continue
            final = bool(r["final"][0])
            if not (w.numel() or final):
                continue
            dev, scope = self._device_scope()
            w = w.detach().float().cpu()
            if w.numel():
                w = torch.from_numpy(self.watermarker.apply_watermark(w.numpy(), sample_rate=self.sr))
            with scope:
                conv = conv or ops.WaveFormatStream(1, fmt, dev)
                out = conv.push([w.to(dev)], [final])[0].cpu()
            if out.numel():
                yield out.unsqueeze(0)


class _TTS(_Finish):
    """The host side of the three TTS classes: the voice of a request, the device batches of generate_batch and generate_long, the pieces of generate_stream.  A
    backbone says how it differs in a few hooks: _text_ids (text -> tokenizer ids), _engine_tokens (ids -> what its engine takes), _synth_kw (the fixed keywords of
    its engine calls), N_DRAWS, PROMPT_LEN / ANALYSIS_KW (voice-prompt analysis), _set_exaggeration and _warn_ignored.
    Only engine, tokenizer, device, analyzer, watermarker and conds are read from the instance (plus model_label on Turbo)."""
    ENC_COND_LEN, DEC_COND_LEN = 6 * S3_SR, 10 * S3GEN_SR
    PROMPT_LEN = 150    # T3Config.speech_cond_prompt_len
    ANALYSIS_KW = {}    # further keywords of the voice-prompt analysis (_prepare_conditionals)
    max_batch = None    # utterances per device batch of generate_batch / generate_long (None: the T3 engine's MAX_BATCH)
    align_heads = None  # (layer, head) pairs the alignment pass of word_times= reads (None: T3Engine.ALIGN_HEADS, an UNMEASURED default)

    def __init__(self, engine, tokenizer, device, conds: Optional[Conditionals] = None, analyzer=None):
        self.engine, self.tokenizer, self.device, self.conds = engine, tokenizer, device, conds
        # the sub-batches of generate_batch / generate_long stay ONE T3 call and one vocoder call each (engine.synthesize_pipelined pairs the T3 of consecutive
        # jobs by default): a request's draws, reports and first audio are defined per sub-batch here, and a pair would make the first sub-batch wait for the second
        if getattr(engine, "t3_pair", False):
            engine.t3_pair = False
        self.analyzer = analyzer  # frontend.PromptAnalyzer (S3 tokenizer + CAMPPlus + voice encoder + 24 kHz mel) or None
        self.t3, self.s3gen, self.ve = engine.t3, engine, (analyzer.ve if analyzer is not None else None)
        self.watermarker = _watermarker()

    # ------------------------------------------------------------------------------------------------------------ the voice
    def _analyse(self, wav, exaggeration, **kw):
        return _prepare_conditionals(self.analyzer, wav, exaggeration, self.PROMPT_LEN, self.device, **self.ANALYSIS_KW, **kw)

    def _use_voice(self, audio_prompt_path, exaggeration, **prepare_kw):
        """The voice prologue of generate, generate_stream and generate_long: a given prompt is analysed into self.conds, else self.conds must be there; then the
        exaggeration of the request (a backbone without emotion conditioning ignores it)."""
        if audio_prompt_path:
            self.prepare_conditionals(audio_prompt_path, exaggeration=exaggeration, **prepare_kw)
        else:
            assert self.conds is not None, _NO_VOICE
        self._set_exaggeration(exaggeration)

    def _warn_ignored(self, *values):
        """cfg_weight, exaggeration and min_p of a request (of every request of a batch), for a backbone that does not support them to warn about."""

    def _voices_of_batch(self, B, audio_prompt_paths, conds, exaggeration, **analyse_kw):
        """One Conditionals per request: analysed from `audio_prompt_paths` (equal paths once per call), taken from `conds`, or self.conds.  Never writes self.conds."""
        if audio_prompt_paths is not None and conds is not None:
            raise ValueError("give audio_prompt_paths or conds, not both")
        if audio_prompt_paths is not None:
            paths = _per_request(audio_prompt_paths, B, "audio_prompt_paths", _PATH)
            return _analysed_once(zip(paths, exaggeration), lambda wav, ex: self._analyse(wav, ex, **analyse_kw))
        out = _per_request(conds, B, "conds", (Conditionals,)) if conds is not None else [self.conds] * B
        assert all(c is not None for c in out), _NO_VOICE
        return out

    # ------------------------------------------------------------------------------------------------------------ word timestamps
    def _word_mode(self, word_times, max_pause=None):
        """_word_times, and what the mode needs from this model: "words" a tokenizer with pieces(ids) (text.MTLTokenizer.pieces)"""
        mode = _word_times(word_times, max_pause)
        if mode == "words" and not hasattr(self.tokenizer, "pieces"):
            raise ValueError('word_times="words" needs a tokenizer with pieces(ids) to group text tokens into words; word_times="tokens" does not')
        return mode

    def _words_of(self, mode, tokens, al, place):
        """The words of one utterance: dict(text, start, stop, tokens=(a, b), frames=(f0, f1)) in text order.  tokens: the engine's 1-D text ids; al: its entry of
        synthesize(words=)'s alignment; place(s): a 24 kHz sample of the utterance's own waveform -> a sample of what the caller receives (clipping included).
        A word begins where its first token's frames begin and ends where the next word begins -- frames of spaces and control tokens go to the word in front
        of them --, the last one where its last token's frames end: start / stop are nondecreasing and stop of one word is start of the next.
        mode "tokens": every text token is a word (text: its piece, or its id where the tokenizer has no pieces)."""
        ids = [int(i) for i in tokens.view(-1).tolist()]
        pieces = self.tokenizer.pieces(ids) if hasattr(self.tokenizer, "pieces") else [str(i) for i in ids]
        space = getattr(self.tokenizer, "SPACE", "[SPACE]")
        groups = [(i, i + 1) for i in range(len(ids))] if mode == "tokens" else word_groups(pieces, space)
        if not groups:
            return []
        fr = al["frames"]
        if al.get("table") is not None:  # a warped utterance: token frame f is mel frame 2 f, which the map places (exactly on the target at an anchor)
            at = lambda f: int(place(int(math.floor(ops.warp_place(al["table"], 2 * f) * 480 + 0.5))))
        else:
            at = lambda f: int(place(frame_sample(f, al["speed"], al["pitch"])))
        starts = [at(fr[a][0]) for a, _ in groups]
        stops = starts[1:] + [max(starts[-1], at(fr[groups[-1][1] - 1][1]))]
        return [dict(text="".join(pieces[a:b]).replace(space, " ").strip() if mode == "words" else pieces[a], start=s0, stop=s1, tokens=(a, b),
                     frames=(fr[a][0], fr[b - 1][1])) for (a, b), s0, s1 in zip(groups, starts, stops)]

    def _word_groups(self, tokens):
        """The engine's 1-D text ids -> ([(a, b) token range per word], [the word strings]) exactly as word_times="words" groups and names them"""
        ids = [int(i) for i in tokens.view(-1).tolist()]
        pieces = self.tokenizer.pieces(ids)
        space = getattr(self.tokenizer, "SPACE", "[SPACE]")
        groups = word_groups(pieces, space)
        return groups, ["".join(pieces[a:b]).replace(space, " ").strip() for a, b in groups]

    def words(self, text, language_id=None):
        """The words of `text` as word_times="words" groups them (text.word_groups over the tokenizer's pieces), as strings in text order: what `timing=` takes one
        entry for.  Nothing is launched."""
        if not hasattr(self.tokenizer, "pieces"):
            raise ValueError("words() needs a tokenizer with pieces(ids)")
        return self._word_groups(self._engine_tokens(self._text_ids(text, language_id)))[1]

    @staticmethod
    def _place(n_out, fmt):
        """_words_of's place for a waveform returned whole: through the format's rate (ops.formatted_len, as segments go), clipped to its n_out samples"""
        return lambda s: min(n_out, s if fmt is None else ops.formatted_len(s, fmt["sample_rate"]))

    # ------------------------------------------------------------------------------------------------------------ the alignment guard
    last_guard = None  # per request of the last guarded call, in the caller's order: T3Engine.collect's report

    def _guard(self, guard):
        """guard= of generate / generate_batch / generate_long / generate_long_stream (None / False, the call without the argument, never gets here) -> the
        engine's dict: True is T3Engine.GUARD_DEFAULTS with this model's align_heads, a dict overrides single keys; an unknown key is a ValueError.  The values
        are checked by the engine, before anything is launched."""
        from .t3 import T3Engine
        if guard is not True and not isinstance(guard, dict):
            raise ValueError(f"guard: expected None, True or a dict of {sorted(T3Engine.GUARD_DEFAULTS)}, got {guard!r}")
        over = {} if guard is True else dict(guard)
        if set(over) - set(T3Engine.GUARD_DEFAULTS):
            raise ValueError(f"guard: unknown key(s) {sorted(set(over) - set(T3Engine.GUARD_DEFAULTS))} (known: {sorted(T3Engine.GUARD_DEFAULTS)})")
        g = dict(T3Engine.GUARD_DEFAULTS, heads=self.align_heads, **over) if "heads" not in over else dict(T3Engine.GUARD_DEFAULTS, **over)
        check = getattr(getattr(self.engine, "t3", None), "check_guard", None)
        return g if check is None else check(g)

    def _take_guard(self, reports, who):
        """model.last_guard = the reports in the caller's order; one UserWarning names the requests that did not end by a sampled end-of-speech token"""
        self.last_guard = reports
        odd = [(i, r["reason"]) for i, r in enumerate(reports) if r is not None and r["reason"] != "eos"]
        if odd:
            import warnings
            warnings.warn(f"{who}: the alignment guard ended request(s) " + ", ".join(f"{i} by {why!r}" for i, why in odd) + " (tail / repeat / run: end of speech "
                          "was forced; length: the speech-token budget was spent)", UserWarning, stacklevel=3)

    # ------------------------------------------------------------------------------------------------------------ one utterance
    def _generate(self, text_ids, opts=None, **kw):
        """generate() behind its argument handling: tokenizer ids -> the finished waveform (opts.words: and its words).  opts: the call's _Options (None: no
        option); kw: sampling arguments, and _synth_kw's if they are to differ.  With a guard last_guard is the request's report."""
        opts = opts or _Options(self)
        tokens = self._engine_tokens(text_ids)
        opts.bind([tokens])
        res = self.engine.synthesize([tokens], self.conds.t3.as_dict(), self.conds.gen, **dict(self._synth_kw(), **kw), **opts.kw([0]))
        if opts.guard is not None:
            self._take_guard(list(self.engine.last_guard), "generate")
        if opts.warped:
            self._take_fit(list(getattr(self.engine, "last_fit", None) or [None]), "generate")
        wav = self._finish(res[0][0], opts.fmt)
        return wav if opts.words is None else (wav, self._words_of(opts.words, tokens, res[2][0], self._place(wav.shape[-1], opts.fmt)))

    def _generate_stream(self, text_ids, stream_kw, opts, **samp):
        """generate_stream() behind its argument handling; of opts a stream takes the seed and the format, its speed travels in stream_kw (_stream_kw)"""
        return self._stream_pieces(self.engine.synthesize_stream([self._engine_tokens(text_ids)], self.conds.t3.as_dict(), self.conds.gen, **self._synth_kw(), **stream_kw,
                                                                 **samp, **opts.kw([0])), opts.fmt)

    # ------------------------------------------------------------------------------------------------------------ device batches
    def _run_jobs(self, jobs, synth_kw):
        """(wavs or joined piece, speech tokens) of every job, in order: several jobs run the throughput schedule (synthesize_pipelined) where the engine has one;
        one job, or an engine without it, the serial schedule (synthesize), one job after the other -- also a call whose jobs carry `words` (word timestamps:
        the alignment pass runs between T3 and the vocoder of the serial schedule; such a call gives up the T3 / flow overlap), whose results are synthesize's
        3-tuples."""
        if len(jobs) > 1 and hasattr(self.engine, "synthesize_pipelined") and not any(job.get("words") is not None for job in jobs):
            results = self.engine.synthesize_pipelined(jobs, **synth_kw)
            try:
                for r in results:
                    yield r[0], r[1]
            finally:  # closed with this generator (generate_long_stream): the engine's own `finally` runs now, not when the garbage is collected
                getattr(results, "close", lambda: None)()
            return
        for job in jobs:
            job = dict(job)
            args = [job.pop(k) for k in ("text_tokens", "t3_conds", "gen_ref")]
            yield self.engine.synthesize(*args, **synth_kw, **job)

    def _generate_batch(self, texts, language_ids, audio_prompt_paths, conds, samp, unsampled, opts, **analyse_kw):
        """generate_batch behind its signature and its _Options: validation of the other per-request arguments, then the voices, then tokenisation, then the
        device work.  samp: the sampling arguments the engine takes; unsampled: those it does not -- exaggeration, which picks the voice's cond dict, and what the
        backbone ignores."""
        B = len(texts)
        langs = self._languages(language_ids, B)
        samp = _sampling_lists(B, **samp)
        unsampled = _sampling_lists(B, **unsampled)
        self._warn_ignored(*(v for vals in unsampled.values() for v in vals))
        voices = self._voices_of_batch(B, audio_prompt_paths, conds, unsampled["exaggeration"], **analyse_kw)
        tokens = [self._engine_tokens(self._text_ids(t, lid)) for t, lid in zip(texts, langs)]
        return self._run_batch(tokens, voices, unsampled["exaggeration"], samp, opts.bind(tokens))

    def _languages(self, language_ids, B):
        return [None] * B

    def _run_batch(self, tokens, voices, exaggeration, samp, opts):
        """Sub-batches of at most max_batch requests in order of text length (_run_jobs: one runs the serial schedule, several the throughput schedule).  Returns the
        finished waveforms in the caller's order.  Every option travels with its request (opts.kw(idx): a request's draws, rate, level, pauses and pitch do not
        depend on the sub-batch or the row it lands in, and a job carries an option only when one of its requests uses it).  With word_times every job carries
        `words`, the sub-batches then run the serial schedule one after the other (_run_jobs), and the result is a list of (waveform, words).  With a guard every
        job carries it, one setting for the call; last_guard holds the reports in the caller's order."""
        dicts = [_t3_dict(c.t3, ex) for c, ex in zip(voices, exaggeration)]
        plan = batch_plan([int(t.numel()) for t in tokens], int(self.max_batch or self.engine.t3.MAX_BATCH))
        jobs = []
        for idx in plan:
            job = dict(text_tokens=_pick(tokens, idx), t3_conds=_one_or_list(_pick(dicts, idx)), gen_ref=_one_or_list([voices[i].gen for i in idx]),
                       **{k: _pick(v, idx) for k, v in samp.items()})
            if opts.generator is not None:  # repeatable: the sampling draws of every sub-batch come from the generator, in execution order
                job["uniforms"] = torch.rand(len(idx), self.N_DRAWS, device=self.engine.dev, generator=opts.generator)
                job["generator"] = opts.generator
            jobs.append(dict(job, **opts.kw(idx)))
        out, reports, fits = [None] * len(tokens), [None] * len(tokens), [None] * len(tokens)
        for idx, res in zip(plan, self._run_jobs(jobs, self._synth_kw(batch=True))):
            if opts.guard is not None:
                for i, r in zip(idx, self.engine.last_guard):
                    reports[i] = r
            if opts.warp_kw(idx) is not None:
                for i, r in zip(idx, getattr(self.engine, "last_fit", None) or [None] * len(idx)):
                    fits[i] = r
            for r, (i, w) in enumerate(zip(idx, res[0])):
                out[i] = self._finish(w, opts.fmt)
                if opts.words is not None:
                    out[i] = (out[i], self._words_of(opts.words, tokens[i], res[2][r], self._place(out[i].shape[-1], opts.fmt)))
        if opts.guard is not None:
            self._take_guard(reports, "generate_batch")
        if opts.warped:
            self._take_fit(fits, "generate_batch")
        return out

    def _generate_long(self, text, language_id, audio_prompt_path, a, return_segments, samp, unsampled, opts, ramp=None, **prepare_kw):
        """generate_long behind its signature, its _Options and _long_args: the remaining checks, the voice as generate() prepares it, then _run_long.  samp /
        unsampled: as _generate_batch takes them, one number each.  ramp (_long_stream_args' pair): generate_long_stream -- the same checks and the same voice,
        all of it when the method is CALLED, then the generator of _stream_long."""
        if not isinstance(text, str):
            raise TypeError(f"text: expected a str, got {type(text).__name__}")
        _long_numbers(**unsampled, **samp)
        if ramp is None:
            self.last_bed = None
            opts.bed_source = None if opts.bed is None else self._bed_source(opts.bed)  # (read ahead of the voice analysis: a bad source costs nothing)
        self._use_voice(audio_prompt_path, unsampled["exaggeration"], **prepare_kw)
        self._warn_ignored(*unsampled.values())
        tokenize = lambda chunk: self._engine_tokens(self._text_ids(chunk, language_id))
        if ramp is not None:
            return self._stream_long(*self._long_work(text, a, tokenize, samp, opts, ramp), a, return_segments, opts)
        return self._run_long(text, a, tokenize, samp, return_segments, opts)

    def _long_work(self, text, a, tokenize, samp, opts, ramp=None):
        """(chunks, plan, engine jobs) of a long-form call: split, tokenise (`tokenize(chunk)` -> the engine's 1-D id tensor), long_plan -- long_stream_plan with
        a ramp (first_batch, batch_growth); a job carries its chunks' options (opts.kw(chunks=True): loudness and the format are held back for the whole)"""
        chunks = split_text(text, a["max_chars"])
        tokens = [tokenize(c) for c, _ in chunks]
        max_batch = int(self.max_batch or self.engine.t3.MAX_BATCH)
        plan = long_plan(chunks, max_batch, a) if ramp is None else long_stream_plan(chunks, max_batch, a, *ramp)
        t3, gen = self.conds.t3.as_dict(), self.conds.gen
        jobs = [dict(text_tokens=_pick(tokens, p["chunks"]), t3_conds=t3, gen_ref=gen, **samp, join=p["join"], **opts.kw(p["chunks"], chunks=True)) for p in plan]
        return chunks, plan, jobs

    @staticmethod
    def _long_segments(chunks, p, piece, st, base):
        """The segment records of one joined piece that begins at sample `base` of the whole"""
        out = []
        for r, k in enumerate(p["chunks"]):
            a0, b0 = piece["edges"][r]
            out.append(dict(text=chunks[k][0], start=base + piece["offsets"][r], stop=base + piece["offsets"][r] + (b0 - a0), src_start=a0, src_stop=b0,
                            tokens=None if st is None else st[r], truncated=bool(piece["truncated"][r])))
        return out

    @staticmethod
    def _warn_truncated(who, truncated, max_chars):
        cut = [k for k, t in enumerate(truncated) if t]
        if cut:
            import logging
            logging.getLogger(__name__).warning("%s: chunk(s) %s of %d reached the speech-token budget without an end-of-speech token and are cut "
                                                "off; use a smaller max_chars (now %d)", who, cut, len(truncated), max_chars)

    def _run_long(self, text, a, tokenize, samp, return_segments, opts):
        """generate_long behind its validation: split, tokenise (`tokenize(chunk)` -> the engine's 1-D id tensor), run the jobs of long_plan (_run_jobs), concatenate
        the joined pieces on the host, watermark the whole once.  opts.fmt: the engine jobs do not carry it -- the concatenated 24 kHz waveform is converted once, in
        _finish (host -> device -> host; no converter state travels through the joined pieces on the device), and the segments' start / stop become output samples,
        ceil(s U / D), so the last stop is the length; src_start / src_stop stay 24 kHz samples.  opts.loud (the LUFS target or None): the engine jobs do not carry it
        either -- the concatenated waveform is measured and gained as ONE signal in _finish, ahead of the watermark, so the chunks keep their relative level; opts.peak
        (the dBTP ceiling or None) likewise: the whole is limited once, behind that gain.  opts.bed (ops.check_bed's plan or None): its source was read before the
        voice analysis (_generate_long: opts.bed_source), the bed is laid under the whole in _finish's visit ahead of the meter, and segments and words begin `lead` samples later."""
        bed = None if opts.bed is None else (opts.bed, opts.bed_source)
        chunks, plan, jobs = self._long_work(text, a, tokenize, samp, opts)
        fmt, pieces, segments, base = opts.fmt, [], [], 0 if bed is None else opts.bed["lead"]  # (the speech begins `lead` samples into the result)
        fl = (lambda v: v) if fmt is None else (lambda v: ops.formatted_len(v, fmt["sample_rate"]))
        for p, job, res in zip(plan, jobs, self._run_jobs(jobs, self._synth_kw())):
            piece, st = res[0], res[1]
            pieces.append(piece["wav"].detach().float().cpu())
            assert pieces[-1].numel() == piece["total"], "a joined piece and its layout record disagree"
            segs = self._long_segments(chunks, p, piece, st, base)
            if opts.guard is not None:  # the alignment guard's report of every chunk travels in its segment
                for seg, r in zip(segs, self.engine.last_guard):
                    seg["guard"] = r
            if opts.words is not None:  # a word of chunk r: its samples clipped to the kept part [src_start, src_stop), shifted to the segment's start
                for r, seg in enumerate(segs):
                    place = lambda v, seg=seg: fl(seg["start"] + min(max(v, seg["src_start"]), seg["src_stop"]) - seg["src_start"])
                    seg["words"] = self._words_of(opts.words, job["text_tokens"][r], res[2][r], place)
            segments += segs
            base += piece["total"]
        self._warn_truncated("generate_long", [s["truncated"] for s in segments], a["max_chars"])
        if opts.guard is not None:
            self._take_guard([s["guard"] for s in segments], "generate_long")
        wav = self._finish(torch.cat(pieces), fmt, converted=False, loud=None if opts.loud is None else opts.loud[0], peak=None if opts.peak is None else opts.peak[0], bed=bed)
        if fmt is not None:
            for seg in segments:
                seg.update(start=ops.formatted_len(seg["start"], fmt["sample_rate"]), stop=ops.formatted_len(seg["stop"], fmt["sample_rate"]))
        return (wav, segments) if return_segments else wav

    # ------------------------------------------------------------------------------------------------------------ dialogue
    last_balance = None  # per voice of the last generate_dialogue(balance=) call, in order of first appearance: dict(voice, lufs, peak, gain, blocks); else None

    last_pan = None      # per voice of the last generate_dialogue(pan=) call, in order of first appearance: dict(voice, position, left, right); else None

    def _generate_dialogue(self, turns, voices, turn_pause, balance, a, return_segments, samp, unsampled, opts, language_id=None, multilingual=False, pan=None,
                           **analyse_kw):
        """generate_dialogue behind its signature, its _Options (format, loudness, true_peak, guard: the finish and the guard) and _long_args: the script's
        validation, the voices (each distinct prompt analysed once; self.conds is never written), the chunks of every turn, dialogue_plan's jobs through _run_jobs,
        then _mix_dialogue.  samp / unsampled: as _generate_long takes them, one number each."""
        ts = _dialogue_turns(turns, voices, turn_pause, unsampled["exaggeration"], language_id, multilingual)
        level = _dialogue_balance(balance)
        _long_numbers(**unsampled, **samp)
        self.last_bed = self.last_pan = None
        keys = list(dict.fromkeys(t["voice"] for t in ts))  # the distinct voices in order of first appearance (None: the model's own)
        place = _dialogue_pan(pan, ts, keys, opts.bed)
        bed = None if opts.bed is None else (opts.bed, self._bed_source(opts.bed))
        if level is not None and len(keys) > DIALOGUE_MAX_VOICES:
            raise ValueError(f"balance: {len(keys)} distinct voices, the meter takes at most {DIALOGUE_MAX_VOICES}")
        assert self.conds is not None or None not in keys, _NO_VOICE
        self._warn_ignored(*unsampled.values(), *(t["exaggeration"] for t in ts))
        given = [None if k is None else voices[k] for k in keys]
        prompts = [(g, unsampled["exaggeration"]) for g in given if g is not None and not isinstance(g, Conditionals)]
        analysed = iter(_analysed_once(prompts, lambda wav, ex: self._analyse(wav, ex, **analyse_kw)))
        conds = [self.conds if g is None else (g if isinstance(g, Conditionals) else next(analysed)) for g in given]
        for t in ts:
            t["chunks"] = split_text(t["text"], a["max_chars"])
        plan = dialogue_plan(ts, int(self.max_batch or self.engine.t3.MAX_BATCH), a)
        turn_of = [r["turn"] for r in plan["rows"]]
        tokens = [self._engine_tokens(self._text_ids(r["text"], ts[r["turn"]]["language_id"])) for r in plan["rows"]]
        row_voice = [keys.index(ts[t]["voice"]) for t in turn_of]
        dicts = [_t3_dict(conds[v].t3, ts[t]["exaggeration"]) for v, t in zip(row_voice, turn_of)]
        jobs = []
        for p in plan["jobs"]:
            idx = p["chunks"]
            job = dict(text_tokens=_pick(tokens, idx), t3_conds=_one_or_list(_pick(dicts, idx)), gen_ref=_one_or_list([conds[row_voice[k]].gen for k in idx]), **samp,
                       **{k: v for k, v in p.items() if k != "chunks"})
            if opts.guard is not None:
                job["guard"] = opts.guard
            jobs.append(job)
        pieces, recs, truncated, reports = [], [], [], []
        for p, res in zip(plan["jobs"], self._run_jobs(jobs, self._synth_kw())):
            piece = res[0]
            pieces.append(piece["wav"].detach().float().cpu())
            assert pieces[-1].numel() == piece["total"], "a joined piece and its layout record disagree"
            recs.append(piece)
            truncated += [bool(v) for v in piece["truncated"]]
            if opts.guard is not None:
                reports += list(self.engine.last_guard)
        self._warn_truncated("generate_dialogue", truncated, a["max_chars"])
        if opts.guard is not None:
            self._take_guard(reports, "generate_dialogue")
        wav, starts, kept = self._mix_dialogue(pieces, recs, [r["after"] for r in plan["rows"]], row_voice, keys, level, a["join_fade"], opts, bed,
                                               None if place is None else [ops.pan_gains(place["rows"][t]) for t in turn_of])
        if place is not None:
            self.last_pan = [dict(voice=k, position=p, left=g[0], right=g[1]) for k, p in zip(keys, place["voices"]) for g in [ops.pan_gains(p)]]
        if bed is not None:  # the speech begins `lead` samples into the result
            starts = [v + opts.bed["lead"] for v in starts]
        if not return_segments:
            return wav
        fl = (lambda v: v) if opts.fmt is None else (lambda v: ops.formatted_len(v, opts.fmt["sample_rate"]))
        segments = []
        for k, (r, (a0, b0)) in enumerate(zip(plan["rows"], kept)):
            seg = dict(turn=r["turn"], voice=ts[r["turn"]]["voice"], text=r["text"], start=fl(starts[k]), stop=fl(starts[k] + b0 - a0), src_start=a0, src_stop=b0,
                       truncated=truncated[k])
            if opts.guard is not None:
                seg["guard"] = reports[k]
            segments.append(seg)
        return wav, segments

    @staticmethod
    def _dialogue_layout(recs, after):
        """The rows of a conversation from the jobs' records -> (kept (src_start, src_stop) per row, their lengths, ops.mix_layout's starts and total, the fade
        flags: every row fades in and out except the very first row's start and the very last row's end where nothing was trimmed there)."""
        kept = [e for rec in recs for e in rec["edges"]]
        lengths = [b0 - a0 for a0, b0 in kept]
        starts, total = ops.mix_layout(lengths, after)
        flags = [3] * len(kept)
        if kept[0][0] == 0:
            flags[0] &= ~1
        if kept[-1][1] == recs[-1]["n"][-1]:
            flags[-1] &= ~2
        return kept, lengths, starts, total, flags

    @staticmethod
    def _dialogue_upload(pieces, recs, lengths, row_voice, keys, level, dev):
        """The upload of the finish: every piece into its slice of ONE allocation, so that a launch may take rows of several pieces -> (the rows as views of it,
        and with a balance level the meter's (V, 4) stats and (V,) gains over every voice's rows packed back to back, else None, None)."""
        cuts = [0]
        for w in pieces:
            cuts.append(cuts[-1] + int(w.numel()))
        up = torch.empty(max(1, cuts[-1]), dtype=torch.float32, device=dev)
        for g, w in enumerate(pieces):
            up[cuts[g]: cuts[g + 1]].copy_(w)
        flat = [up[cuts[g] + off: cuts[g] + off + (b0 - a0)] for g, rec in enumerate(recs) for off, (a0, b0) in zip(rec["offsets"], rec["edges"])]
        gain = stats = None
        if level is not None:
            order = [k for v in range(len(keys)) for k in range(len(flat)) if row_voice[k] == v]
            packed = torch.cat([flat[k] for k in order])
            ends = [sum(lengths[k] for k in order if row_voice[k] < v) for v in range(len(keys) + 1)]
            stats, gain = ops.wave_loudness([packed[ends[v]: ends[v + 1]] for v in range(len(keys))], [level] * len(keys), 1.0)
        return flat, stats, gain

    def _mix_dialogue(self, pieces, recs, after, row_voice, keys, level, fade, opts, bed=None, pan=None):
        """The finish of generate_dialogue, ONE visit to the device for the whole conversation: the jobs' pieces (host tensors: each the job's trimmed rows back to
        back; recs: their records of offsets and edges) are uploaded into ONE allocation, ops.mix_layout over the kept lengths places the rows, the meter of
        balance= reads every voice's MONO rows packed back to back (torch.cat: copies, no arithmetic; ONE ops.wave_loudness over the V voices, ceiling 1.0 -> the (V,)
        gain vector the rows index through gain_idx), and the mixer sums the rows -- ONE launch for up to 64 rows, whatever pieces they came in; a longer script
        in launches of 64, the first writing every sample and the others accumulating.  pan None: ops.wave_mix into a (total,) buffer.  pan (the (left, right)
        gains of every row: ops.pan_gains of its turn's place): ops.wave_pan_mix into a planar (2, total) buffer.  Then the chain (_chain), whose order is
        _finish's because it is the same code: the music bed (bed: (plan, source) or None, mono only; the mix is measured before the bed, the bed over its whole
        source), loudness over the result as ONE signal, true_peak, the watermark on the host if a watermarker is loaded, the format, the one copy to the host.
        (One launch per PIECE would also be the definition's values, but an accumulating launch adds to the +0.0 its predecessor left: a row that begins with
        -0.0 samples -- the vocoder's do -- would differ from generate_long's bits in the sign of those zeros.  With one allocation a script of up to 64 chunks
        is one launch and has no such seam.)  Every row fades in and out over `fade` samples except the very first row's start and the very last row's end where
        nothing was trimmed there (the join's first / last rule).  Returns (the CPU tensor, (1, n) or planar (2, n), the rows' starts in 24 kHz samples, their
        kept (src_start, src_stop))."""
        kept, lengths, starts, total, flags = self._dialogue_layout(recs, after)
        fmt, loud, peak = opts.fmt, None if opts.loud is None else opts.loud[0], None if opts.peak is None else opts.peak[0]
        self.last_balance = None
        if total == 0 and bed is None:
            w = self._finish(torch.zeros(0), fmt, converted=False)
            return (w if pan is None else torch.cat([w, w])), starts, kept
        dev, scope = self._device_scope()
        with scope:
            flat, stats, gain = self._dialogue_upload(pieces, recs, lengths, row_voice, keys, level, dev)
            out = torch.empty(*(() if pan is None else (2,)), total, dtype=torch.float32, device=dev)
            for lo in range(0, len(flat), ops.WAVE_JOIN_MAX_ROWS):
                hi = min(lo + ops.WAVE_JOIN_MAX_ROWS, len(flat))
                kw = dict(gain=gain, gain_idx=None if gain is None else row_voice[lo:hi], fade=fade, accumulate=lo > 0)
                if pan is not None:
                    ops.wave_pan_mix(flat[lo:hi], starts[lo:hi], flags[lo:hi], pan[lo:hi], out, **kw)
                elif total:
                    ops.wave_mix(flat[lo:hi], starts[lo:hi], flags[lo:hi], out, **kw)
            w = self._chain(out, fmt, loud, peak, bed)
            if stats is not None:
                self.last_balance = [dict(voice=k, lufs=s[0], peak=s[1], gain=s[2], blocks=int(s[3])) for k, s in zip(keys, stats.cpu().tolist())]
        return (w.unsqueeze(0) if pan is None else w), starts, kept

    def _stream_long(self, chunks, plan, jobs, a, return_segments, opts):
        """generate_long_stream behind its validation, a generator: the jobs run through _run_jobs -- while the consumer holds piece k the throughput schedule has
        the T3 of pieces k + 1 and k + 2 in flight --, and every joined piece is finished and yielded as it leaves the device.  Per piece, in this order:
        loudness (opts.loud: upload, ONE ops.WaveLoudnessStream held here measures pieces 0 .. k, ops.wave_gain with its gain, ceiling 1.0; engine.last_loudness = the
        latest stats), the watermark if a watermarker is loaded, the format (ONE ops.WaveFormatStream held here, final on the last piece; the engine jobs do not
        carry it).  With neither a piece costs what generate_long's costs: one copy to the host.  Closing the generator closes _run_jobs, and with it the
        engine's synthesize_pipelined (its `finally` returns the T3 engines)."""
        dev, scope = self._device_scope()
        run = self._run_jobs(jobs, self._synth_kw())
        fmt, loud = opts.fmt, None if opts.loud is None else opts.loud[0]
        meter = conv = None
        base, truncated, reports = 0, [], []
        try:
            for g, (p, (piece, st)) in enumerate(zip(plan, run)):
                wav = piece["wav"].detach().float().cpu()
                assert wav.numel() == piece["total"], "a joined piece and its layout record disagree"
                segments = self._long_segments(chunks, p, piece, st, base)
                if opts.guard is not None:  # the reports so far, in text order; a piece's own travel in its segments
                    for seg, r in zip(segments, self.engine.last_guard):
                        seg["guard"] = r
                    reports += [s["guard"] for s in segments]
                base += piece["total"]
                truncated += [s["truncated"] for s in segments]
                on_dev = None  # the piece on the device, while the host copy `wav` is the same samples
                if loud is not None and wav.numel():
                    with scope:
                        on_dev = wav.to(dev).contiguous()
                        meter = meter or ops.WaveLoudnessStream(1, dev)
                        stats, gain = meter.push([on_dev], [float(loud)], 1.0)
                        ops.wave_gain([on_dev], gain)
                        self.engine.last_loudness = stats
                        wav = on_dev.cpu()
                if self.watermarker is not None and wav.numel():
                    wav, on_dev = torch.from_numpy(self.watermarker.apply_watermark(wav.numpy(), sample_rate=self.sr)), None
                if fmt is not None:
                    with scope:
                        conv = conv or ops.WaveFormatStream(1, fmt, dev)
                        wav = conv.push([wav.to(dev) if on_dev is None else on_dev], [g == len(plan) - 1])[0].cpu()
                    for seg in segments:
                        seg.update(start=ops.formatted_len(seg["start"], fmt["sample_rate"]), stop=ops.formatted_len(seg["stop"], fmt["sample_rate"]))
                if wav.numel() or (return_segments and segments):
                    yield (wav.unsqueeze(0), segments) if return_segments else wav.unsqueeze(0)
        finally:
            run.close()
            self._warn_truncated("generate_long_stream", truncated, a["max_chars"])
            if opts.guard is not None:
                self._take_guard(reports, "generate_long_stream")


class _LlamaTTS(_TTS):
    """The two classes on the Llama T3: text ids wrapped in start / end-of-text, CFG, min_p and an emotion scalar in the voice."""
    N_DRAWS = 1000             # sampling draws of an utterance: max_new_tokens
    DROP_LAST_TOKEN = False    # the multilingual path drops the last token's 40 ms (mtl_tts.py:348-352)

    def prepare_conditionals(self, wav_fpath, exaggeration=0.5):
        """reference tts.py:182-206 / mtl_tts.py:253-277: waveform file -> self.conds."""
        self.conds = self._analyse(wav_fpath, exaggeration)

    def _set_exaggeration(self, exaggeration):
        cur = float(torch.as_tensor(self.conds.t3.emotion_adv).reshape(-1)[0])
        if float(exaggeration) != cur:
            c = self.conds.t3
            self.conds.t3 = T3Cond(speaker_emb=c.speaker_emb, cond_prompt_speech_tokens=c.cond_prompt_speech_tokens,
                                   emotion_adv=exaggeration * torch.ones(1, 1, 1))

    def _engine_tokens(self, text_ids):
        sot, eot = 255, 0
        return torch.cat([torch.tensor([sot]), text_ids.view(-1).long().cpu(), torch.tensor([eot])])

    def _synth_kw(self, batch=False):
        return dict(max_new_tokens=1000, drop_last_token=self.DROP_LAST_TOKEN)

    @classmethod
    def from_synthetic(cls, device="cuda", seed=0, t3_layers=30, **kw):
        """Seeded random-init model in the reference checkpoint layout + a synthetic voice (no network / no checkpoints)."""
        eng = ChatterboxEngine(synth.t3_state_dict(t3_layers, seed, text_vocab=cls._TEXT_VOCAB), synth.s3gen_state_dict(seed),
                               device, n_t3_layers=t3_layers)
        c = synth.t3_cond()
        conds = Conditionals(T3Cond(**c), synth.s3gen_ref())
        analyzer = None
        if kw.get("with_prompt_nets"):  # synthetic S3 tokenizer / CAMPPlus / voice encoder so that prepare_conditionals runs end to end
            nl = kw.get("tokenizer_layers", 6)
            analyzer = _make_analyzer(dict(synth.s3tokenizer_state_dict(seed, n_layer=nl), **synth.campplus_state_dict(seed)),
                                      synth.voice_encoder_state_dict(seed), device)
        return cls(eng, None, device, conds, analyzer)


class ChatterboxTTS(_LlamaTTS):
    _TEXT_VOCAB = 704

    @classmethod
    def from_local(cls, ckpt_dir, device):
        d = Path(ckpt_dir)
        s3 = _load_state(d / "s3gen.safetensors")
        eng = ChatterboxEngine(_load_state(d / "t3_cfg.safetensors"), s3, device)
        conds = Conditionals.load(d / "conds.pt") if (d / "conds.pt").exists() else None
        ve = _load_state(d / "ve.safetensors") if (d / "ve.safetensors").exists() else None
        return cls(eng, EnTokenizer(d / "tokenizer.json"), device, conds, _make_analyzer(s3, ve, device))

    @classmethod
    def from_pretrained(cls, device):
        from huggingface_hub import hf_hub_download
        for f in ("ve.safetensors", "t3_cfg.safetensors", "s3gen.safetensors", "tokenizer.json", "conds.pt"):
            local = hf_hub_download(repo_id=REPO_ID, filename=f)
        return cls.from_local(Path(local).parent, device)

    def _text_ids(self, text, language_id=None):
        return self.tokenizer.text_to_tokens(punc_norm_en(text))

    def generate(self, text, repetition_penalty=1.2, min_p=0.05, top_p=1.0, audio_prompt_path=None, exaggeration=0.5,
                 cfg_weight=0.5, temperature=0.8, seed=None, speed=1.0, sample_rate=None, encoding=None, loudness=None, max_pause=None, pause_db=40.0, pitch=None,
                 word_times=False, guard=None, duration=None, timing=None, true_peak=None):
        """seed (None, or an int in [0, 2^64)): every random draw of this request -- sampling, flow noise, vocoder phase and noise -- is a function of the seed
        alone (no torch RNG is consumed), and is the one generate_batch(seeds=) gives the request in any batch.
        speed (a number in [0.5, 2.0]): the speaking rate, 1.25 = 25 % faster, at unchanged pitch -- the mel is interpolated along time between the flow decoder and
        the vocoder (ChatterboxEngine.vocode(speed=)).  With a seed the tokens do not depend on it; the result has max(1, floor(K / speed)) * 480 samples where
        speed 1.0 gives K * 480.
        sample_rate (None / 24000, or 8000, 16000, 22050, 32000, 44100, 48000) and encoding (None / "f32", "s16", "mulaw", "alaw"): the delivery format.  The
        result is then the (1, n) CPU tensor of float32, int16 (PCM16) or uint8 (G.711) at that rate, n = ceil(n24 U / D) -- resampled as
        scipy.signal.resample_poly does (frontend.resample's definition; its default filter, no dither) and encoded by ONE launch on the device, ahead of the only
        copy to the host (ops.wave_format); with a watermarker loaded, after the watermark.  `.sr` stays 24000.  The defaults are the call without the arguments.
        loudness (None, or a number in [-50, -5]): the target integrated loudness in LUFS (ITU-R BS.1770-4, e.g. -16 for podcasts, -23 for broadcast).  The
        waveform is measured and multiplied by the gain that brings it to the target on the device, behind the vocoder and ahead of the format conversion and the
        only copy to the host (ops.wave_normalize); the gain is limited so that no sample exceeds a peak of 1.0, so a quiet target is met exactly and a loud one
        may fall short.  A silent result and one shorter than 0.4 s are returned as they are.  None is the call without the argument.
        true_peak (None, or a ceiling in [-20, 0] dBTP, e.g. -1 for EBU R 128 and the streaming platforms): the true-peak limiter.  The peak of the 4-times
        oversampled waveform -- the values between the samples that a D/A converter or a rate conversion reconstructs -- is held under the ceiling by a
        look-ahead gain envelope of 5 ms on the device (ops.wave_limit), behind the loudness step and ahead of the pauses, the format conversion and the only
        copy to the host.  Together with `loudness` the gain to the target is applied in full (the sample-peak limit of 1.0 gives way to the limiter), so a loud
        target is met up to what the limiter removes: the loudness is not measured again and can end slightly below the target.  It changes no length: word
        times and segments are untouched.  The ceiling holds for the 24 kHz fp32 signal; a later rate conversion or a host watermark can move peaks slightly --
        that is what the headroom below 0 dBTP is for.  engine.last_limit keeps {true peak before, least gain, samples gained down, samples over the ceiling}.
        generate_batch: a number or one number / None per request, travelling with its request like loudness.  generate_long: the assembled whole is limited
        once, behind its loudness step.  The streams do not take the argument: a running limiter needs a carried look-ahead (generate_long_stream lists it, as it
        lists word_times, because its signature is generate_long's plus the ramp, and refuses anything but None with a TypeError).  The look-ahead and the window are
        UNMEASURED choices.  None is the call without the argument.
        max_pause (None, or seconds in [0.04, 60]) and pause_db (a finite number >= 0, default 40): pause control.  A silence INSIDE the utterance -- a run of
        480-sample frames whose mean square is pause_db decibels or more below the loudest frame's, between two frames that are not -- that is longer than
        round(max_pause * 50) frames is shortened to that many, on the device (ops.wave_squeeze), behind the loudness step and ahead of the format conversion and
        the only copy to the host; the cut is cross-faded over 240 samples.  Silence at the two ends is not touched.  The result is shorter by 480 samples per
        removed frame; engine.last_pauses keeps the record.  With a watermarker the watermark sees the shortened signal.  pause_db = 40 is trim_db's default, an
        UNMEASURED choice.  generate_batch: max_pause is a number or one number / None per request and travels with its request like speed; pause_db is one number
        for the call.  generate_long: every chunk is shortened ahead of the join; a segment's [start, stop) holds the chunk's kept, shortened samples, and
        [src_start, src_stop) count samples of the shortened chunk.  generate_stream does not take the arguments: a pause's end is not known inside a round.
        pitch (None, or semitones in [-12, 12]; 0 is None): pitch control.  With r = 2^(pitch / 12) the mel is stretched at speed / r instead of speed -- that
        rate must lie in [0.5, 2.0], else a ValueError that names both arguments --, the vocoder runs on it, and one launch on the device (ops.wave_pitch) reads the
        waveform back at a step of r samples, ahead of the loudness step, the pauses, the format conversion and the only copy to the host: the result has exactly
        the length of the call without `pitch`, every frequency multiplied by r.  The formants move WITH the pitch (varispeed with the duration restored): two or
        three semitones keep the voice, an octave does not.  The range and the filter are UNMEASURED choices.  generate_batch: a number or
        one number / None per request, travelling with its request like speed.  generate_long: every chunk is transposed ahead of the join; the gaps do not
        change.  generate_stream does not take the argument.
        word_times (False; True or "words"; "tokens"): word timestamps.  The call returns (wav, words), words a list of dict(text, start, stop, tokens=(a, b),
        frames=(f0, f1)) in text order: the word is text tokens [a, b) of the request (start / end-of-text included in the count), spoken over the speech tokens
        [f0, f1) and the samples [start, stop) of the returned waveform -- nondecreasing, stop of one word is start of the next, everything clipped to the
        waveform's length; with `speed`, `pitch` and `sample_rate` the boundaries are mapped as the audio is.  "tokens": one entry per text token, no grouping.
        The times come from T3's own attention: after the tokens are sampled, one teacher-forced pass over the request reads how much attention a few heads
        (align_heads; T3Engine.ALIGN_HEADS) put on each text token while each speech token was sampled, and a monotonic path through that is cut at the word
        boundaries (T3Engine.align).  WHICH heads align is an UNMEASURED default taken from the reference project's analyser: nobody has
        checked it on trained weights here.  Not together with max_pause (ValueError).  generate_batch: one flag for the call, a list of (wav, words); the
        sub-batches of such a call run one after the other, without the T3 / flow overlap.  generate_long: with return_segments=True every segment gains `words`
        in samples of the joined result, clipped to the segment.  generate_stream, generate_long_stream, ChatterboxTurboTTS and ChatterboxVC do not take it.
        guard (None; True, or a dict that overrides single keys of T3Engine.GUARD_DEFAULTS -- heads, back, ahead, end_tokens, tail, repeat, repeat_skip,
        token_run, hold_eos, min_text; an unknown key is a ValueError): the alignment guard, a bound on how the request ENDS.  T3 sometimes never samples its
        end-of-speech token -- it trails off into noise, repeats a phrase, sits on one token -- or samples it in the middle of the sentence.  With the guard, every
        token step also reads, on the device, how much attention a few heads (`heads`; default align_heads / T3Engine.ALIGN_HEADS) put on each text token,
        follows the text position, bans end-of-speech until the position has reached the last end_tokens text tokens (hold_eos, for texts of min_text tokens or
        more), and forces it once the attention has stayed on the last tokens (`tail`), has gone back to earlier text (`repeat`) or the last token_run sampled
        tokens are one token (`run`) (include/cbx.h cbx_guard_update_f32).  last_guard is then the list of reports, dict(reason: "eos",
        "tail", "repeat", "run" or "length"; tokens, fired_at, completed_at, position, text_tokens) per request in the caller's order, and one UserWarning names
        the requests that did not end by a sampled end-of-speech token.  The defaults follow what is publicly described of the reference project's analyser and are
        UNMEASURED here: nobody has run them on trained weights with these kernels, and with the wrong heads hold_eos can itself keep a request running to the
        token budget.  Opt-in; None is the call without the argument, launch for launch.  generate_batch: one setting for the call.  generate_long /
        generate_long_stream: every chunk is guarded, with return_segments its report travels in its segment as `guard`.  generate_stream, ChatterboxTurboTTS and
        ChatterboxVC do not take the argument: round streams and the GPT-2 backbone are not built.
        duration (None, or seconds in [0.02, 80]): timing control, the length.  The number of speech tokens is known before the flow runs, so the K mel frames
        the plain call would return are fitted into O = floor(50 duration + 0.5) frames by ONE launch between the flow and the vocoder (ops.mel_time_warp,
        cbx_mel_time_warp_f32) that stretches the mel at rate K / O; the F0 predictor runs on the stretched mel, so the pitch is kept, and T3 and its tokens do
        not depend on it.  The result has exactly O * 480 samples at 24 kHz whenever K / O lies in [0.5, 2.0] (then through sample_rate= / encoding= as ever);
        otherwise the rate is held at the bound, the result has the length that gives -- nothing is padded or cut --, a UserWarning names the request and
        model.last_fit[b] = dict(target, frames, rate=(min, max), clamped, table) says so.  Not together with speed, pitch or max_pause (ValueError); not on the
        streams or generate_long.  generate_batch: a number, or one number / None per request.
        timing (None, or a list with one entry per word of the text -- model.words(text) lists them --, each None or the word's START in seconds, nondecreasing):
        timing control, the words.  Honoured on the 20 ms frame grid: after T3 the alignment pass of word_times= says at which mel frame x_i word i begins, and the
        anchors (x_i, floor(50 t_i + 0.5)) become a piecewise-linear time map (ops.warp_plan) applied by the same one launch; every segment's rate is held in
        [0.5, 2.0], so a target that needs more is met as closely as the bound allows (UserWarning, last_fit[b]["clamped"] / ["achieved"]) and a later word still
        aims at its own target.  A word that begins at frame 0 cannot be moved (there is nothing in front of it to stretch: no lead-in silence is inserted).
        duration= may be given with it and fixes the end.  It implies the alignment pass, so the call runs the serial schedule, and it inherits that pass's
        UNMEASURED default ALIGN_HEADS exactly as word_times= does: nobody has checked on trained weights here that those heads track the words.  With word_times=
        in the same call the returned words are the achieved ones, mapped through the time map (ops.warp_place).  A wrong number of entries is a ValueError
        before anything is launched.  generate_batch: a list of such lists / Nones.  Not on Turbo (its GPT-2 backbone has no alignment pass) or voice conversion.
        This is the statement of `seed`, `speed`, `sample_rate`, `encoding`, `loudness`, `max_pause`, `pause_db`, `pitch`, `word_times`, `guard`, `duration` and `timing` for every method
        of every class of this module; the others say only what differs."""
        opts = _Options(self, seeds=seed, speed=speed, sample_rate=sample_rate, encoding=encoding, loudness=loudness, true_peak=true_peak, max_pause=max_pause, pause_db=pause_db, pitch=pitch, word_times=word_times, guard=guard, duration=duration, timing=timing)
        self._use_voice(audio_prompt_path, exaggeration)
        return self._generate(self._text_ids(text), opts, temperature=temperature, cfg_weight=cfg_weight, repetition_penalty=repetition_penalty, min_p=min_p, top_p=top_p)

    def generate_long(self, text, repetition_penalty=1.2, min_p=0.05, top_p=1.0, audio_prompt_path=None, exaggeration=0.5, cfg_weight=0.5, temperature=0.8,
                      max_chars=None, pause=0.15, paragraph_pause=0.4, trim_db=40.0, trim_pad=2, join_fade=240, seed=None, speed=1.0, return_segments=False, sample_rate=None, encoding=None, loudness=None, max_pause=None, pause_db=40.0, pitch=None,
                      word_times=False, guard=None, true_peak=None, bed=None):
        """generate() for a text of ANY length: the reference stops at 1000 speech tokens (40 s) and cuts a longer text off.  The text is split into chunks of at
        most max_chars characters at paragraph, sentence and clause boundaries (text.split_text), the chunks are synthesised in text order as device batches
        (one: synthesize; several: the throughput schedule where the engine has it), and each batch's waveforms are trimmed of their leading / trailing silence and
        joined ON THE DEVICE (ChatterboxEngine.vocode(join=)): a batch leaves the device as one piece in one copy.  Returns the (1, n) CPU tensor at `.sr`; the
        watermarker, if loaded, is applied once to the whole.
        max_chars (None: 300, or 100 for zh / ja / ko), pause / paragraph_pause (seconds of silence behind a chunk / behind a paragraph's last chunk, divided by
        speed), trim_db (a frame of 480 samples is silence when its mean square is that many dB below the chunk's loudest frame; None: no trimming), trim_pad
        (frames kept on either side), join_fade (samples of linear fade at every seam): UNMEASURED defaults -- nobody has tuned them with trained weights.
        seed: chunk k draws from chunk_seed(seed, k), chunk 0 from `seed` itself; without one the call draws as generate_batch does.  speed: generate()'s.
        return_segments=True: also a list of dict(text, start, stop, src_start, src_stop, tokens, truncated) per chunk -- [start, stop) are its samples in the
        result (usable for captions), [src_start, src_stop) the part of its own waveform that was kept.  A chunk whose T3 spent the token budget without an
        end-of-speech token is `truncated`; one warning names them.  Every argument is checked before anything is launched; self.conds is written only as
        generate() writes it (audio_prompt_path).
        sample_rate, encoding: generate()'s; the whole waveform is converted once, after the watermark, and the segments' [start, stop) are then samples of the
        converted result (ceil(s U / D)) while [src_start, src_stop) stay 24 kHz samples.
        loudness: generate()'s, of the WHOLE assembled waveform measured as one signal (pauses included), so the chunks keep their relative level: one gain for
        all of it, limited to a sample peak of 1.0, applied on the device ahead of the watermark and the conversion.
        word_times: generate()'s, with return_segments=True (without: ValueError): every segment gains `words`, its chunk's words shifted into the joined result
        through the segment's start / src_start and clipped to [start, stop); the device batches of such a call run one after the other.
        bed: generate_dialogue()'s music bed under the whole assembled waveform, in the visit to the device that loudness and true_peak make; segments and words
        begin `lead` seconds later."""
        opts = _Options(self, seeds=seed, speed=speed, sample_rate=sample_rate, encoding=encoding, loudness=loudness, true_peak=true_peak, max_pause=max_pause, pause_db=pause_db, pitch=pitch, word_times=word_times, guard=guard, segments=return_segments, bed=bed)
        a = _long_args(max_chars, pause, paragraph_pause, trim_db, trim_pad, join_fade, seed, speed, False)
        samp = dict(temperature=temperature, cfg_weight=cfg_weight, repetition_penalty=repetition_penalty, min_p=min_p, top_p=top_p)
        return self._generate_long(text, None, audio_prompt_path, a, return_segments, samp, dict(exaggeration=exaggeration), opts)

    def generate_dialogue(self, turns, voices=None, *, turn_pause=DIALOGUE_TURN_PAUSE, balance=None, return_segments=False, max_chars=None, pause=0.15,
                          paragraph_pause=0.4, trim_db=40.0, trim_pad=2, join_fade=240, repetition_penalty=1.2, min_p=0.05, top_p=1.0, exaggeration=0.5,
                          cfg_weight=0.5, temperature=0.8, seed=None, sample_rate=None, encoding=None, loudness=None, true_peak=None, guard=None, bed=None, pan=None):
        """A conversation: a script whose turns are spoken by different voices, delivered as ONE waveform.  The reference has no counterpart: it returns one
        utterance of one voice.  turns: a non-empty list of (voice, text) pairs or dicts dict(voice=, text=, gap=, speed=, pitch=, exaggeration=); voice is a key
        of `voices` or None (the model's current conds); `voices` maps a key to a Conditionals or to anything audio_prompt_path= takes (each distinct prompt is
        analysed once per call; self.conds is never written).  gap: seconds before this turn, a finite number in [-60, 60], default turn_pause; a NEGATIVE gap
        starts the turn that long before the front of the conversation -- the next speaker comes in before the last one has finished, a "mm-hm" lies over the
        other voice (clipped at the start of the conversation; the first turn's gap is not used; not scaled by speed).  speed, pitch, exaggeration: generate()'s,
        per turn, travelling with the turn's chunks as generate_batch's per-request values do.
        Every turn's text is split as generate_long splits it (max_chars; pause / paragraph_pause between a turn's own chunks, divided by the turn's speed); the
        chunks run in script order as device batches of mixed voices (no length sort), chunk k of the whole script seeded with chunk_seed(seed, k); each batch is
        trimmed on the device (trim_db, trim_pad) and leaves it as one piece.  The finish is ONE more visit to the device: the pieces are uploaded, every chunk is
        placed (ops.mix_layout), faded over join_fade samples and SUMMED into the conversation by cbx_wave_mix_f32 (ops.wave_mix: rows that overlap are added in
        script order, bit for bit reproducible), then loudness (the mix as ONE signal), true_peak, the watermark, sample_rate / encoding: generate_long's, in its
        order.  A one-voice script with non-negative gaps is generate_long's result bit for bit.
        balance (None; True: -23 LUFS; or a number in [-50, -5]): two cloned voices seldom have the same level -- every voice's chunks, packed back to back, are
        measured by ONE launch of the BS.1770-4 meter and each voice gets the one gain that brings it to that level (sample peak limited to 1.0; a voice shorter
        than 0.4 s keeps gain 1, the meter's own rule), applied inside the mixer.  More than 64 distinct voices with balance is a ValueError.  model.last_balance
        then holds dict(voice, lufs, peak, gain, blocks) per voice in order of first appearance (else None).
        return_segments=True: also one dict per chunk with turn, voice, text, start, stop, src_start, src_stop, truncated (and guard with a guard): [start, stop)
        in samples of the returned waveform (through the format's rate as generate_long maps them; overlapping chunks overlap in these numbers), [src_start,
        src_stop) the kept part of the chunk's own waveform.  Truncated chunks get generate_long's single warning.
        Everything is validated when the method is called, before the engine or the voice analysis is touched: TypeError for wrong types, unknown dict keys, a
        bool where a number belongs and `turns` not a list; ValueError for out-of-range or non-finite values, an unknown voice key and empty text.
        bed (None; an audio input -- whatever audio_prompt_path= takes: a path, a (waveform, sample_rate) pair or raw (data, rate, encoding[, channels]) --; or a
        dict with `audio` plus overrides of ops.BED_DEFAULTS): background music or room tone under the conversation, pulled down while someone talks.  The source
        is brought to 24 kHz mono as a voice prompt is (model.audio_in), looped with a cross-fade if it is shorter than the programme (loop, loop_fade), faded in
        and out (fade_in, fade_out), and may play alone before and after the speech (lead, tail).  Its level is `level` LU relative to the speech (default -12:
        two readings of the BS.1770-4 meter, the mix before the bed and the bed over its whole source); while a 10 ms frame of speech peaks above `threshold`
        dBFS the bed is `duck` dB lower, from `pre` seconds before a word until `post` seconds after it, every transition taking `ramp` seconds -- the whole
        signal is known, so the bed is down BEFORE the word (cbx_wave_duck_f32, ops.wave_duck; include/cbx.h states the definition).  Order of the finish: mix,
        bed, loudness, true_peak, the watermark, sample_rate / encoding: meter and limiter see speech plus bed.  Without loudness= / true_peak= the sum is NOT
        bounded -- speech near full scale plus the bed can pass 1.0 --: true_peak=-1 is recommended with a bed.  With return_segments the records begin `lead`
        seconds later.  model.last_bed then holds dict(gain, speech_lufs, bed_lufs, ducked, frames, peak) -- the linear gain applied to the bed, the two
        readings, the 10 ms frames the bed was down for, all frames, the sample peak of the sum (else None).  bed=None is the call without the argument.  Every
        default of ops.BED_DEFAULTS is an UNMEASURED choice: nobody has tuned them by listening.
        pan (None; True; or a dict voice key -> position in [-1, 1], -1 hard left, 0 the centre, +1 hard right): a STEREO programme, each voice at a place in the
        image.  A voice the dict does not name sits at 0, a key that speaks no turn is a ValueError; True spreads the distinct voices evenly over
        [-DIALOGUE_PAN_SPREAD, +DIALOGUE_PAN_SPREAD] = [-0.3, 0.3] in order of first appearance (one voice: 0); a turn's dict may carry pan= and overrides its
        voice's place for that turn.  The constant-power law (ops.pan_gains: left = cos, right = sin of (p + 1) pi / 4) keeps a voice's power wherever it sits.
        The finish stays ONE visit to the device: balance= still meters each voice's mono rows; cbx_wave_pan_mix_f32 sums the rows into two planes, reading every
        sample once; loudness= reads the two planes as one signal (cbx_wave_loudness_ch_f32: BS.1770-4 gates on the SUM of the channels' block energies);
        true_peak= is the LINKED limiter (cbx_wave_limit_ch_f32: one gain envelope for both channels, so a peak on one side does not move the image); the
        watermark is applied per channel; sample_rate= / encoding= convert both planes in one launch.  The result is a planar (2, n) tensor in every encoding;
        the segments' numbers are per-channel sample positions, those of the mono call.  model.last_pan then holds dict(voice, position, left, right) per voice
        in order of first appearance (else None).  pan=None is the call without the argument, launch for launch.  bed= together with pan= is a ValueError: a
        stereo bed is not built.  DIALOGUE_PAN_SPREAD = 0.3 is an UNMEASURED default: nobody has tuned it by listening.
        turn_pause = 0.3 s and balance=True -> -23 LUFS are UNMEASURED defaults: nobody has tuned them with trained weights.  Not taken:
        streaming, word_times, max_pause, duration / timing, a stereo bed, more than two channels or interleaved output, more than one bed or a bed that changes
        per turn; ChatterboxVC has no such method.
        This is the contract of generate_dialogue of the three TTS classes; the others say only what differs."""
        opts = _Options(self, seeds=seed, sample_rate=sample_rate, encoding=encoding, loudness=loudness, true_peak=true_peak, guard=guard, bed=bed)
        a = _long_args(max_chars, pause, paragraph_pause, trim_db, trim_pad, join_fade, seed, 1.0, False)
        samp = dict(temperature=temperature, cfg_weight=cfg_weight, repetition_penalty=repetition_penalty, min_p=min_p, top_p=top_p)
        return self._generate_dialogue(turns, voices, turn_pause, balance, a, return_segments, samp, dict(exaggeration=exaggeration), opts, pan=pan)

    def generate_long_stream(self, text, repetition_penalty=1.2, min_p=0.05, top_p=1.0, audio_prompt_path=None, exaggeration=0.5, cfg_weight=0.5, temperature=0.8,
                             max_chars=None, pause=0.15, paragraph_pause=0.4, trim_db=40.0, trim_pad=2, join_fade=240, seed=None, speed=1.0, return_segments=False,
                             sample_rate=None, encoding=None, loudness=None, max_pause=None, pause_db=40.0, pitch=None, word_times=False, guard=None, true_peak=None, bed=None,
                             first_batch=1, batch_growth=2.0):
        """generate_long() in pieces: a generator of (1, n) CPU tensors, one per device batch as it leaves the device (empty pieces left out); concatenated along
        dim 1 they are the long-form result.  Every argument of generate_long with its meaning and default, plus the ramp of the device batches:
        first_batch (None, or an int >= 1) and batch_growth (a finite number >= 1): the batches hold s_0 = min(first_batch, step) chunks, then
        s_(g+1) = min(step, max(s_g, ceil(s_g * batch_growth))), step = min(max_batch, 64) (long_stream_plan), so the first piece is one chunk's work and the
        later ones fill the device.  first_batch=None is generate_long's own plan: the pieces then concatenate to generate_long bit for bit (same seed).  The
        defaults 1 / 2.0 are UNMEASURED choices.  Everything is validated, and the voice prepared, when this method is CALLED, not at the first next().
        While the consumer holds piece k the throughput schedule has the T3 of the next two batches in flight; closing the generator early returns the engines at
        once.  The truncation warning is issued once, when the stream ends.
        return_segments=True: (wav, segments) per piece, `segments` the records of that piece's chunks with generate_long's keys; start / stop count samples of the
        whole stream.
        loudness: piece k is multiplied by the gain the one-shot meter gives for pieces 0 .. k of the ungained signal, limited to a sample peak of 1.0 -- the
        "integrated so far" reading of a live meter (ops.WaveLoudnessStream: bit for bit ops.wave_loudness of the concatenation).  The step between two gains falls
        at a piece boundary, where the join left a pause of zeros followed by a fade-in, so it makes no click; with pause=0 or join_fade=0 it DOES fall on signal.
        A first piece under 0.4 s, or a silent one, gets gain 1.  The result is not generate_long(loudness=)'s, which knows the whole signal -- except for a text of
        one piece.  The watermarker, if loaded, is applied per piece, as generate_stream does.
        sample_rate, encoding: every piece goes through ONE ops.WaveFormatStream, so the pieces add up to the conversion of the whole bit for bit.  A piece that is
        not the last holds the resampling filter's tail back: a segment's last samples may arrive with the NEXT piece.
        word_times: NOT taken -- it stands in the signature only because that is generate_long's plus the ramp; anything but False is a TypeError: a stream has
        no finished token sequence for the alignment pass.  true_peak and bed likewise: anything but None is a TypeError (a running limiter and a running bed
        are not built)."""
        _no_word_times("generate_long_stream", word_times)
        _no_true_peak("generate_long_stream", true_peak)
        _no_bed("generate_long_stream", bed)
        opts = _Options(self, seeds=seed, speed=speed, sample_rate=sample_rate, encoding=encoding, loudness=loudness, max_pause=max_pause, pause_db=pause_db, pitch=pitch, guard=guard)
        a = _long_args(max_chars, pause, paragraph_pause, trim_db, trim_pad, join_fade, seed, speed, False)
        ramp = _long_stream_args(first_batch, batch_growth)
        samp = dict(temperature=temperature, cfg_weight=cfg_weight, repetition_penalty=repetition_penalty, min_p=min_p, top_p=top_p)
        return self._generate_long(text, None, audio_prompt_path, a, return_segments, samp, dict(exaggeration=exaggeration), opts, ramp)

    def generate_batch(self, texts, audio_prompt_paths=None, conds=None, exaggeration=0.5, cfg_weight=0.5, temperature=0.8, repetition_penalty=1.2,
                       min_p=0.05, top_p=1.0, generator=None, seeds=None, speed=1.0, sample_rate=None, encoding=None, loudness=None, max_pause=None, pause_db=40.0, pitch=None,
                       word_times=False, guard=None, duration=None, timing=None, true_peak=None):
        """generate() for B requests in one call: a list of B CPU float32 tensors (1, n_b) at `.sr`, in the caller's order, each what generate() returns for that
        request.  Voice per request: `audio_prompt_paths` (one, or a list of B; equal paths are analysed once) or `conds` (one Conditionals, or a list of B);
        neither: self.conds.  exaggeration .. top_p: a float or a sequence of B (a wrong length raises ValueError before anything is launched).  generator: a
        torch.Generator on the model's device makes the call repeatable (None: the global RNG).  More requests than the device batch run as sub-batches in order
        of text length through the throughput schedule.  Never overwrites self.conds.
        seeds (None, an int for every request, or a sequence of B ints in [0, 2^64); not together with a generator): request b's random draws depend on seeds[b]
        alone -- not on the other requests, its row, the sub-batch split or the order of calls -- and are those of generate(seed=seeds[b]).  Its tokens and audio
        then agree with that call's as far as batched and single arithmetic agree: the kernels pick their forms by row count, so this is not bit equality.
        speed (a number for every request, or a sequence of B numbers in [0.5, 2.0]; None entries are 1.0): request b's speaking rate, generate(speed=)'s; it
        travels with its request through the sub-batches like its seed.  sample_rate, encoding: generate()'s, ONE format for the call (checked first).
        loudness (None, a number for every request, or a sequence of B numbers / Nones in [-50, -5]): request b's LUFS target, generate(loudness=)'s; a None entry
        leaves that request as it is; it travels with its request through the sub-batches like its speed.
        This is the contract of generate_batch of every class of this module; the others say only what differs."""
        texts = _batch_of(texts)
        opts = _Options(self, len(texts), False, seeds=seeds, generator=generator, speed=speed, sample_rate=sample_rate, encoding=encoding, loudness=loudness, true_peak=true_peak, max_pause=max_pause, pause_db=pause_db, pitch=pitch, word_times=word_times, guard=guard, duration=duration, timing=timing)
        samp = dict(temperature=temperature, cfg_weight=cfg_weight, repetition_penalty=repetition_penalty, min_p=min_p, top_p=top_p)
        return self._generate_batch(texts, None, audio_prompt_paths, conds, samp, dict(exaggeration=exaggeration), opts)

    def generate_stream(self, text, repetition_penalty=1.2, min_p=0.05, top_p=1.0, audio_prompt_path=None, exaggeration=0.5,
                        cfg_weight=0.5, temperature=0.8, first_chunk=25, chunk=50, chunk_growth=1.0, lookahead=3, fade=480, overlap=True, window=None, seed=None, sample_rate=None, encoding=None, speed=1.0):
        """generate() in pieces (the engine's synthesize_stream): a generator of CPU float32 tensors (1, n) at `.sr`, the first after
        `first_chunk` tokens; concatenated along dim 1 they give the utterance.  If a watermarker is loaded it is applied to each piece.
        window (None: every round re-synthesises the utterance so far): tokens of left context of a round of bounded cost (synthesize_stream).
        seed: generate()'s.  speed (a number in [0.5, 2.0]): generate(speed=)'s speaking rate -- the pieces add up to the length generate(speed=) returns;
        checked, with the window it asks for (engine.check_stream_window), when this is called.  sample_rate, encoding: generate()'s -- every round's new samples
        are converted ahead of the round's copy to the host (one ops.WaveFormatStream for the stream); the pieces add up to the conversion of the whole utterance.
        This is the contract of generate_stream of the three TTS classes; the others say only what differs."""
        opts = _Options(self, seeds=seed, sample_rate=sample_rate, encoding=encoding)
        self._use_voice(audio_prompt_path, exaggeration)
        return self._generate_stream(self._text_ids(text), _stream_kw(first_chunk, chunk, chunk_growth, lookahead, fade, overlap, window, speed), opts, temperature=temperature,
                                     cfg_weight=cfg_weight, repetition_penalty=repetition_penalty, min_p=min_p, top_p=top_p)


def _language(language_id, request=""):
    """A language id as the tokenizer takes it: lower case, or None for none.  An unknown one is the reference's ValueError (mtl_tts.py); `request` names the
    request of a batch it belongs to."""
    if language_id and language_id.lower() not in SUPPORTED_LANGUAGES:
        raise ValueError(f"Unsupported language_id '{language_id}'{request}. Supported languages: {', '.join(SUPPORTED_LANGUAGES)}")
    return language_id.lower() if language_id else None


class ChatterboxMultilingualTTS(_LlamaTTS):
    _TEXT_VOCAB = 2454
    DROP_LAST_TOKEN = True

    @classmethod
    def get_supported_languages(cls):
        return SUPPORTED_LANGUAGES.copy()

    @classmethod
    def from_local(cls, ckpt_dir, device, t3_model=None):
        d = Path(ckpt_dir)
        t3_file = _resolve_multilingual_t3_model(t3_model)
        s3 = _load_state(d / "s3gen.pt")
        eng = ChatterboxEngine(_load_state(d / t3_file), s3, device)
        conds = Conditionals.load(d / "conds.pt") if (d / "conds.pt").exists() else None
        ve = _load_state(d / "ve.pt") if (d / "ve.pt").exists() else None
        return cls(eng, MTLTokenizer(d / "grapheme_mtl_merged_expanded_v1.json"), device, conds, _make_analyzer(s3, ve, device))

    @classmethod
    def from_pretrained(cls, device, t3_model=None):
        from huggingface_hub import snapshot_download
        t3_file = _resolve_multilingual_t3_model(t3_model)
        d = snapshot_download(repo_id=REPO_ID, repo_type="model", revision="main", token=os.getenv("HF_TOKEN"),
                              allow_patterns=["ve.pt", t3_file, "s3gen.pt", "grapheme_mtl_merged_expanded_v1.json", "conds.pt",
                                              "Cangjie5_TC.json"])
        return cls.from_local(d, device, t3_model=t3_model)

    def _text_ids(self, text, language_id=None):
        """language_id: checked and lower case already (_language)"""
        return self.tokenizer.text_to_tokens(punc_norm(text), language_id=language_id)

    def _languages(self, language_ids, B):
        langs = _per_request(language_ids, B, "language_ids", (str,))
        return [_language(lid, f" (request {k})") for k, lid in enumerate(langs)]

    def generate(self, text, language_id, audio_prompt_path=None, exaggeration=0.5, cfg_weight=0.5, temperature=0.8,
                 repetition_penalty=1.2, min_p=0.05, top_p=1.0, seed=None, speed=1.0, sample_rate=None, encoding=None, loudness=None, max_pause=None, pause_db=40.0, pitch=None,
                 word_times=False, guard=None, duration=None, timing=None, true_peak=None):
        """ChatterboxTTS.generate in the language `language_id` (ValueError for one that is not in SUPPORTED_LANGUAGES; None: no language token); the last
        token's 40 ms are dropped as the reference does.  seed, speed, sample_rate, encoding, loudness, word_times, guard: as there."""
        opts = _Options(self, seeds=seed, speed=speed, sample_rate=sample_rate, encoding=encoding, loudness=loudness, true_peak=true_peak, max_pause=max_pause, pause_db=pause_db, pitch=pitch, word_times=word_times, guard=guard, duration=duration, timing=timing)
        lid = _language(language_id)
        self._use_voice(audio_prompt_path, exaggeration)
        return self._generate(self._text_ids(text, lid), opts, temperature=temperature, cfg_weight=cfg_weight, repetition_penalty=repetition_penalty, min_p=min_p, top_p=top_p)

    def generate_long(self, text, language_id, audio_prompt_path=None, exaggeration=0.5, cfg_weight=0.5, temperature=0.8, repetition_penalty=1.2, min_p=0.05,
                      top_p=1.0, max_chars=None, pause=0.15, paragraph_pause=0.4, trim_db=40.0, trim_pad=2, join_fade=240, seed=None, speed=1.0,
                      return_segments=False, sample_rate=None, encoding=None, loudness=None, max_pause=None, pause_db=40.0, pitch=None, word_times=False,
                      guard=None, true_peak=None, bed=None):
        """ChatterboxTTS.generate_long with generate()'s language_id; max_chars=None is 100 for zh / ja / ko and 300 otherwise."""
        opts = _Options(self, seeds=seed, speed=speed, sample_rate=sample_rate, encoding=encoding, loudness=loudness, true_peak=true_peak, max_pause=max_pause, pause_db=pause_db, pitch=pitch, word_times=word_times, guard=guard, segments=return_segments, bed=bed)
        lid = _language(language_id)
        a = _long_args(max_chars, pause, paragraph_pause, trim_db, trim_pad, join_fade, seed, speed, lid in CJK_LANGUAGES)
        samp = dict(temperature=temperature, cfg_weight=cfg_weight, repetition_penalty=repetition_penalty, min_p=min_p, top_p=top_p)
        return self._generate_long(text, lid, audio_prompt_path, a, return_segments, samp, dict(exaggeration=exaggeration), opts)

    def generate_dialogue(self, turns, voices=None, *, language_id=None, turn_pause=DIALOGUE_TURN_PAUSE, balance=None, return_segments=False, max_chars=None,
                          pause=0.15, paragraph_pause=0.4, trim_db=40.0, trim_pad=2, join_fade=240, exaggeration=0.5, cfg_weight=0.5, temperature=0.8,
                          repetition_penalty=1.2, min_p=0.05, top_p=1.0, seed=None, sample_rate=None, encoding=None, loudness=None, true_peak=None, guard=None, bed=None,
                          pan=None):
        """ChatterboxTTS.generate_dialogue with generate()'s language_id for the call and, as a further key of a turn's dict, per turn (default: the call's);
        max_chars=None is 100 when the call's language is zh / ja / ko and 300 otherwise."""
        opts = _Options(self, seeds=seed, sample_rate=sample_rate, encoding=encoding, loudness=loudness, true_peak=true_peak, guard=guard, bed=bed)
        if language_id is not None and not isinstance(language_id, str):
            raise TypeError(f"language_id: expected None or a str, got {type(language_id).__name__}")
        lid = _language(language_id)
        a = _long_args(max_chars, pause, paragraph_pause, trim_db, trim_pad, join_fade, seed, 1.0, lid in CJK_LANGUAGES)
        samp = dict(temperature=temperature, cfg_weight=cfg_weight, repetition_penalty=repetition_penalty, min_p=min_p, top_p=top_p)
        return self._generate_dialogue(turns, voices, turn_pause, balance, a, return_segments, samp, dict(exaggeration=exaggeration), opts, lid, True, pan=pan)

    def generate_long_stream(self, text, language_id, audio_prompt_path=None, exaggeration=0.5, cfg_weight=0.5, temperature=0.8, repetition_penalty=1.2, min_p=0.05,
                             top_p=1.0, max_chars=None, pause=0.15, paragraph_pause=0.4, trim_db=40.0, trim_pad=2, join_fade=240, seed=None, speed=1.0,
                             return_segments=False, sample_rate=None, encoding=None, loudness=None, max_pause=None, pause_db=40.0, pitch=None, word_times=False, guard=None,
                             true_peak=None, bed=None, first_batch=1, batch_growth=2.0):
        """ChatterboxTTS.generate_long_stream with generate()'s language_id; max_chars=None is 100 for zh / ja / ko and 300 otherwise."""
        _no_word_times("generate_long_stream", word_times)
        _no_true_peak("generate_long_stream", true_peak)
        _no_bed("generate_long_stream", bed)
        opts = _Options(self, seeds=seed, speed=speed, sample_rate=sample_rate, encoding=encoding, loudness=loudness, max_pause=max_pause, pause_db=pause_db, pitch=pitch, guard=guard)
        lid = _language(language_id)
        a = _long_args(max_chars, pause, paragraph_pause, trim_db, trim_pad, join_fade, seed, speed, lid in CJK_LANGUAGES)
        ramp = _long_stream_args(first_batch, batch_growth)
        samp = dict(temperature=temperature, cfg_weight=cfg_weight, repetition_penalty=repetition_penalty, min_p=min_p, top_p=top_p)
        return self._generate_long(text, lid, audio_prompt_path, a, return_segments, samp, dict(exaggeration=exaggeration), opts, ramp)

    def generate_batch(self, texts, language_ids, audio_prompt_paths=None, conds=None, exaggeration=0.5, cfg_weight=0.5, temperature=0.8,
                       repetition_penalty=1.2, min_p=0.05, top_p=1.0, generator=None, seeds=None, speed=1.0, sample_rate=None, encoding=None, loudness=None, max_pause=None, pause_db=40.0, pitch=None,
                       word_times=False, guard=None, duration=None, timing=None, true_peak=None):
        """ChatterboxTTS.generate_batch with a language per request: `language_ids` one id or a list of B, each validated as generate() does (after seeds and
        speed, before the sampling arguments)."""
        texts = _batch_of(texts)
        opts = _Options(self, len(texts), False, seeds=seeds, generator=generator, speed=speed, sample_rate=sample_rate, encoding=encoding, loudness=loudness, true_peak=true_peak, max_pause=max_pause, pause_db=pause_db, pitch=pitch, word_times=word_times, guard=guard, duration=duration, timing=timing)
        samp = dict(temperature=temperature, cfg_weight=cfg_weight, repetition_penalty=repetition_penalty, min_p=min_p, top_p=top_p)
        return self._generate_batch(texts, language_ids, audio_prompt_paths, conds, samp, dict(exaggeration=exaggeration), opts)

    def generate_stream(self, text, language_id, audio_prompt_path=None, exaggeration=0.5, cfg_weight=0.5, temperature=0.8,
                        repetition_penalty=1.2, min_p=0.05, top_p=1.0, first_chunk=25, chunk=50, chunk_growth=1.0, lookahead=3, fade=480, overlap=True, window=None,
                        seed=None, sample_rate=None, encoding=None, speed=1.0):
        """ChatterboxTTS.generate_stream with generate()'s language_id."""
        opts = _Options(self, seeds=seed, sample_rate=sample_rate, encoding=encoding)
        lid = _language(language_id)
        self._use_voice(audio_prompt_path, exaggeration)
        return self._generate_stream(self._text_ids(text, lid), _stream_kw(first_chunk, chunk, chunk_growth, lookahead, fade, overlap, window, speed), opts,
                                     temperature=temperature, cfg_weight=cfg_weight, repetition_penalty=repetition_penalty, min_p=min_p, top_p=top_p)


class ChatterboxTurboTTS(_TTS):
    """Reference tts_turbo.py:111-320: GPT2-medium (Turbo) or GPT2-small (Nano) T3, meanflow S3Gen, GPT-2 BPE tokenizer.  CFG, min_p and exaggeration are not
    supported by this backbone: the arguments are there for the reference's signatures and ignored with its warning.  The engine has no throughput schedule: the
    device batches of generate_batch and generate_long run one after the other."""
    ENC_COND_LEN = 15 * S3_SR  # tts_turbo.py:112-113: the T3 prompt covers up to 15 s (375 tokens)
    PROMPT_LEN = 375
    ANALYSIS_KW = dict(min_seconds=5.0, enc_cond_len=ENC_COND_LEN)
    N_DRAWS = 1001  # T3 can sample max_gen_len + 1 tokens

    def __init__(self, engine, tokenizer, device, conds=None, model_label="Turbo", analyzer=None):
        super().__init__(engine, tokenizer, device, conds, analyzer)
        self.model_label = model_label

    @classmethod
    def from_local(cls, ckpt_dir, device, nano=False):
        d = Path(ckpt_dir)
        t3_sd = _load_state(d / ("t3_nano_v1.safetensors" if nano else "t3_turbo_v1.safetensors"))
        t3_sd.pop("tfmr.wte.weight", None)  # present in the file, unused (reference deletes it after loading, tts_turbo.py:167)
        s3 = _load_state(d / "s3gen_meanflow.safetensors")
        eng = TurboEngine(t3_sd, s3, device)
        ve = _load_state(d / "ve.safetensors") if (d / "ve.safetensors").exists() else None
        from transformers import AutoTokenizer
        tok = AutoTokenizer.from_pretrained(str(d))
        if tok.pad_token is None:
            tok.pad_token = tok.eos_token
        conds = Conditionals.load(d / "conds.pt") if (d / "conds.pt").exists() else None
        return cls(eng, tok, device, conds, "Nano" if nano else "Turbo", _make_analyzer(s3, ve, device))

    @classmethod
    def from_pretrained(cls, device, nano=False):
        from huggingface_hub import snapshot_download
        d = snapshot_download(repo_id="ResembleAI/chatterbox-nano" if nano else "ResembleAI/chatterbox-turbo", token=os.getenv("HF_TOKEN"),
                              allow_patterns=["*.safetensors", "*.json", "*.txt", "*.pt", "*.model"])
        return cls.from_local(d, device, nano=nano)

    @classmethod
    def from_synthetic(cls, device="cuda", seed=0, nano=False, t3_layers=None):
        dmodel, layers = (768, 12) if nano else (1024, 24)
        layers = t3_layers or layers
        eng = TurboEngine(synth.t3_turbo_state_dict(layers, dmodel, seed), synth.s3gen_state_dict(seed, meanflow=True), device,
                          n_t3_layers=layers)
        c = synth.t3_cond(prompt_len=375)
        return cls(eng, None, device, Conditionals(T3Cond(speaker_emb=c["speaker_emb"], cond_prompt_speech_tokens=c["cond_prompt_speech_tokens"],
                                                          emotion_adv=None), synth.s3gen_ref()), "Nano" if nano else "Turbo")

    def norm_loudness(self, wav, sr, target_lufs=-27):
        return _norm_loudness(wav, sr, target_lufs)

    def prepare_conditionals(self, wav_fpath, exaggeration=0.0, norm_loudness=True):
        """reference tts_turbo.py:241-270 (prompt > 5 s, optional loudness normalisation to -27 LUFS, 375 prompt tokens).  norm_loudness: True is the reference's
        (pyloudnorm on the host; skipped with its warning where that is missing), False none, "device" the same gain from this project's own BS.1770-4 meter on
        the device (_norm_loudness_device): no third-party dependency, no ceiling.  With self.audio_in = "device" the prompt is on the device already: "device"
        gains it in place there, True (pyloudnorm) copies the 24 kHz waveform to the host and back -- a host round trip."""
        self.conds = self._analyse(wav_fpath, exaggeration, norm_loudness=norm_loudness)

    def _set_exaggeration(self, exaggeration):
        """(no emotion conditioning on this backbone: the voice stays as it is)"""

    def _warn_ignored(self, *values):
        if any(v > 0.0 for v in values):
            import logging
            logging.getLogger(__name__).warning(f"CFG, min_p and exaggeration are not supported by the {self.model_label} version and will be ignored.")

    def _text_ids(self, text, language_id=None):
        return self.tokenizer(punc_norm_turbo(text), return_tensors="pt", padding=True, truncation=True).input_ids[0]

    def _engine_tokens(self, text_ids):
        return text_ids.view(-1).long().cpu()

    def _synth_kw(self, batch=False):
        """(generate_batch spells the token budget out; generate, generate_stream and generate_long leave it to the engine's default, the same 1000)"""
        return dict(max_gen_len=1000) if batch else {}

    def generate(self, text, repetition_penalty=1.2, min_p=0.00, top_p=0.95, audio_prompt_path=None, exaggeration=0.0, cfg_weight=0.0,
                 temperature=0.8, top_k=1000, norm_loudness=True, seed=None, speed=1.0, sample_rate=None, encoding=None, loudness=None, max_pause=None, pause_db=40.0, pitch=None, duration=None, true_peak=None):
        """reference tts_turbo.py:272-320.  norm_loudness: prepare_conditionals' (used with an audio_prompt_path).  seed, speed, sample_rate, encoding, loudness: as
        ChatterboxTTS.generate."""
        opts = _Options(self, seeds=seed, speed=speed, sample_rate=sample_rate, encoding=encoding, loudness=loudness, true_peak=true_peak, max_pause=max_pause, pause_db=pause_db, pitch=pitch, duration=duration)
        self._use_voice(audio_prompt_path, exaggeration, norm_loudness=norm_loudness)
        self._warn_ignored(cfg_weight, exaggeration, min_p)
        return self._generate(self._text_ids(text), opts, temperature=temperature, top_k=top_k, top_p=top_p, repetition_penalty=repetition_penalty)

    def generate_long(self, text, repetition_penalty=1.2, min_p=0.00, top_p=0.95, audio_prompt_path=None, exaggeration=0.0, cfg_weight=0.0, temperature=0.8,
                      top_k=1000, norm_loudness=True, max_chars=None, pause=0.15, paragraph_pause=0.4, trim_db=40.0, trim_pad=2, join_fade=240, seed=None, speed=1.0,
                      return_segments=False, sample_rate=None, encoding=None, loudness=None, max_pause=None, pause_db=40.0, pitch=None, true_peak=None, bed=None):
        """ChatterboxTTS.generate_long on the Turbo / Nano backbone (generate()'s sampling arguments; the batches run one after the other)."""
        opts = _Options(self, seeds=seed, speed=speed, sample_rate=sample_rate, encoding=encoding, loudness=loudness, true_peak=true_peak, max_pause=max_pause, pause_db=pause_db, pitch=pitch, bed=bed)
        a = _long_args(max_chars, pause, paragraph_pause, trim_db, trim_pad, join_fade, seed, speed, False)
        samp = dict(temperature=temperature, top_k=top_k, top_p=top_p, repetition_penalty=repetition_penalty)
        return self._generate_long(text, None, audio_prompt_path, a, return_segments, samp, dict(cfg_weight=cfg_weight, exaggeration=exaggeration, min_p=min_p), opts,
                                   norm_loudness=norm_loudness)

    def generate_dialogue(self, turns, voices=None, *, turn_pause=DIALOGUE_TURN_PAUSE, balance=None, return_segments=False, max_chars=None, pause=0.15,
                          paragraph_pause=0.4, trim_db=40.0, trim_pad=2, join_fade=240, repetition_penalty=1.2, min_p=0.00, top_p=0.95, exaggeration=0.0,
                          cfg_weight=0.0, temperature=0.8, top_k=1000, norm_loudness=True, seed=None, sample_rate=None, encoding=None, loudness=None,
                          true_peak=None, bed=None, pan=None):
        """ChatterboxTTS.generate_dialogue on the Turbo / Nano backbone (generate()'s sampling arguments; norm_loudness: prepare_conditionals', for the prompts in
        `voices`; the batches run one after the other; no guard on this backbone)."""
        opts = _Options(self, seeds=seed, sample_rate=sample_rate, encoding=encoding, loudness=loudness, true_peak=true_peak, bed=bed)
        a = _long_args(max_chars, pause, paragraph_pause, trim_db, trim_pad, join_fade, seed, 1.0, False)
        samp = dict(temperature=temperature, top_k=top_k, top_p=top_p, repetition_penalty=repetition_penalty)
        return self._generate_dialogue(turns, voices, turn_pause, balance, a, return_segments, samp, dict(cfg_weight=cfg_weight, exaggeration=exaggeration, min_p=min_p),
                                       opts, pan=pan, norm_loudness=norm_loudness)

    def generate_long_stream(self, text, repetition_penalty=1.2, min_p=0.00, top_p=0.95, audio_prompt_path=None, exaggeration=0.0, cfg_weight=0.0, temperature=0.8,
                             top_k=1000, norm_loudness=True, max_chars=None, pause=0.15, paragraph_pause=0.4, trim_db=40.0, trim_pad=2, join_fade=240, seed=None,
                             speed=1.0, return_segments=False, sample_rate=None, encoding=None, loudness=None, max_pause=None, pause_db=40.0, pitch=None, true_peak=None, bed=None, first_batch=1, batch_growth=2.0):
        """ChatterboxTTS.generate_long_stream on the Turbo / Nano backbone (generate()'s sampling arguments; the batches run one after the other, so a piece is
        yielded before the next batch starts)."""
        _no_true_peak("generate_long_stream", true_peak)
        _no_bed("generate_long_stream", bed)
        opts = _Options(self, seeds=seed, speed=speed, sample_rate=sample_rate, encoding=encoding, loudness=loudness, max_pause=max_pause, pause_db=pause_db, pitch=pitch)
        a = _long_args(max_chars, pause, paragraph_pause, trim_db, trim_pad, join_fade, seed, speed, False)
        ramp = _long_stream_args(first_batch, batch_growth)
        samp = dict(temperature=temperature, top_k=top_k, top_p=top_p, repetition_penalty=repetition_penalty)
        return self._generate_long(text, None, audio_prompt_path, a, return_segments, samp, dict(cfg_weight=cfg_weight, exaggeration=exaggeration, min_p=min_p), opts,
                                   ramp, norm_loudness=norm_loudness)

    def generate_batch(self, texts, audio_prompt_paths=None, conds=None, exaggeration=0.0, cfg_weight=0.0, temperature=0.8, repetition_penalty=1.2, min_p=0.00,
                       top_p=0.95, top_k=1000, norm_loudness=True, generator=None, seeds=None, speed=1.0, sample_rate=None, encoding=None, loudness=None, max_pause=None, pause_db=40.0, pitch=None, duration=None, true_peak=None):
        """generate() for B requests in one call (the contract of ChatterboxTTS.generate_batch; temperature, repetition_penalty, top_p, top_k: a number or a sequence
        of B).  CFG, min_p and exaggeration are ignored with generate()'s warning.  Sub-batches run one after the other."""
        texts = _batch_of(texts)
        opts = _Options(self, len(texts), False, seeds=seeds, generator=generator, speed=speed, sample_rate=sample_rate, encoding=encoding, loudness=loudness, true_peak=true_peak, max_pause=max_pause, pause_db=pause_db, pitch=pitch, duration=duration)
        samp = dict(temperature=temperature, top_k=top_k, top_p=top_p, repetition_penalty=repetition_penalty)
        return self._generate_batch(texts, None, audio_prompt_paths, conds, samp, dict(cfg_weight=cfg_weight, exaggeration=exaggeration, min_p=min_p), opts,
                                    norm_loudness=norm_loudness)

    def generate_stream(self, text, repetition_penalty=1.2, min_p=0.00, top_p=0.95, audio_prompt_path=None, exaggeration=0.0, cfg_weight=0.0,
                        temperature=0.8, top_k=1000, norm_loudness=True, first_chunk=25, chunk=50, chunk_growth=1.0, lookahead=3, fade=480, overlap=True, window=None,
                        seed=None, sample_rate=None, encoding=None, speed=1.0):
        """ChatterboxTTS.generate_stream on the Turbo / Nano backbone (TurboEngine.synthesize_stream; generate()'s sampling arguments)."""
        opts = _Options(self, seeds=seed, sample_rate=sample_rate, encoding=encoding)
        self._use_voice(audio_prompt_path, exaggeration, norm_loudness=norm_loudness)
        self._warn_ignored(cfg_weight, exaggeration, min_p)
        return self._generate_stream(self._text_ids(text), _stream_kw(first_chunk, chunk, chunk_growth, lookahead, fade, overlap, window, speed), opts, temperature=temperature,
                                     top_k=top_k, top_p=top_p, repetition_penalty=repetition_penalty)


class ChatterboxVC(_Finish):
    """Voice conversion (reference vc.py:16-104): S3 tokens of the source audio (S3 tokenizer on the device) -> S3Gen with the target
    voice -> HiFT.  `generate` also accepts the source as S3 tokens (`s3_tokens=`): the parity contract of config 5 starts at the token
    boundary because the tokenizer's arithmetic is third-party."""
    ENC_COND_LEN, DEC_COND_LEN = 6 * S3_SR, 10 * S3GEN_SR

    def __init__(self, engine, device, ref_dict=None, analyzer=None):
        self.engine, self.device, self.ref_dict, self.analyzer = engine, device, ref_dict, analyzer
        self.s3gen = engine
        self.watermarker = _watermarker()

    @staticmethod
    def _engine(s3, device):
        """The flow-and-vocoder engine of a voice conversion: no T3."""
        return S3GenEngine(s3, device)

    @classmethod
    def from_local(cls, ckpt_dir, device):
        d = Path(ckpt_dir)
        s3 = _load_state(d / "s3gen.safetensors")
        ref = Conditionals.load(d / "conds.pt").gen if (d / "conds.pt").exists() else None
        return cls(cls._engine(s3, device), device, ref, _make_analyzer(s3, None, device))

    @classmethod
    def from_pretrained(cls, device):
        """reference vc.py:61-74"""
        from huggingface_hub import hf_hub_download
        for f in ("s3gen.safetensors", "conds.pt"):
            local = hf_hub_download(repo_id=REPO_ID, filename=f)
        return cls.from_local(Path(local).parent, device)

    @classmethod
    def from_synthetic(cls, device="cuda", seed=0, tokenizer_layers=6):
        s3 = dict(synth.s3gen_state_dict(seed), **synth.s3tokenizer_state_dict(seed, n_layer=tokenizer_layers), **synth.campplus_state_dict(seed))
        return cls(cls._engine(s3, device), device, synth.s3gen_ref(), _make_analyzer(s3, None, device))

    def _need_analyzer(self):
        if self.analyzer is None or not self.analyzer.tokenizer.available or not self.analyzer.speaker_encoder.available:
            raise RuntimeError("this S3Gen checkpoint carries no `tokenizer.*` / `speaker_encoder.*` tensors: pass s3_tokens= and a prepared "
                               "ref_dict instead of waveforms")

    def _embed_ref(self, wav):
        """A target voice (a WAV path or a (waveform, sample_rate) pair) -> its S3Gen reference dict"""
        if self.audio_in == "device":
            st = self.analyzer.stage(wav, dec_cond_len=self.DEC_COND_LEN)
            return self.analyzer.embed_ref_staged(st["ref24"], st["ref16"])
        return self.analyzer.embed_ref(_load_wave(wav, S3GEN_SR)[: self.DEC_COND_LEN], S3GEN_SR)

    def _tokens_of(self, audio):
        """A source (a WAV path, a (waveform, sample_rate) pair or a raw (data, sample_rate, encoding[, channels]) tuple) -> its S3 tokens"""
        if self.audio_in == "device":
            return self.analyzer.tokenizer(self.analyzer.ingest([audio], S3_SR)[0])[0]
        return self.analyzer.tokenizer(torch.from_numpy(_load_wave(audio, S3_SR)))[0]

    def set_target_voice(self, wav_fpath):
        """reference vc.py:76-81"""
        self._need_analyzer()
        self.ref_dict = self._embed_ref(wav_fpath)

    def _source_tokens(self, audio, target_voice_path, s3_tokens):
        """The argument handling of generate (reference vc.py:83-104) -> the source's S3 tokens, 1-D on the host.  self.ref_dict is written only when a
        target_voice_path is given."""
        if target_voice_path:
            self.set_target_voice(target_voice_path)
        else:
            assert self.ref_dict is not None, "Please `prepare_conditionals` first or specify `target_voice_path`"
        if s3_tokens is None:
            self._need_analyzer()
            s3_tokens = self._tokens_of(audio)
        return torch.as_tensor(s3_tokens).view(-1).long().cpu()

    def generate(self, audio=None, target_voice_path=None, s3_tokens=None, seed=None, speed=1.0, sample_rate=None, encoding=None, loudness=None, max_pause=None, pause_db=40.0, pitch=None, duration=None, true_peak=None):
        """reference vc.py:83-104.  audio: a WAV path, a (waveform, sample_rate) pair or raw samples (data, sample_rate, encoding[, channels]) -- bytes or a uint8 /
        int16 / int32 / float32 array of interleaved frames in one of ops.WAVE_IN_ENCODINGS; with self.audio_in = "device" it is decoded and resampled on the device
        (a path then opens G.711 and 24-bit WAVs too).  seed, speed: as ChatterboxTTS.generate, where the draws of a conversion
        are the flow noise and the vocoder's phase and noise (there is no sampling), and the tokens are the source's.  sample_rate, encoding, loudness: as there.
        duration (None, or seconds in [0.02, 80]): ChatterboxTTS.generate(duration=)'s -- the conversion is fitted into that length; not with speed, pitch or
        max_pause; model.last_fit has the plan."""
        opts = _Options(self, seeds=seed, speed=speed, sample_rate=sample_rate, encoding=encoding, loudness=loudness, true_peak=true_peak, max_pause=max_pause, pause_db=pause_db, pitch=pitch, duration=duration)
        wavs, _ = self.engine.vocode([self._source_tokens(audio, target_voice_path, s3_tokens)], self.ref_dict, **opts.kw([0]))
        if opts.warped:
            self._take_fit(list(self.engine.last_fit), "generate")
        return self._finish(wavs[0], opts.fmt)

    def generate_stream(self, audio=None, target_voice_path=None, s3_tokens=None, first_chunk=25, chunk=50, chunk_growth=1.0, lookahead=3, fade=480, window=200, seed=None, sample_rate=None, encoding=None, speed=1.0):
        """generate() in pieces (the engine's vocode_stream): a generator of CPU float32 tensors (1, n) at `.sr`, the first after `first_chunk` tokens of
        the source; concatenated along dim 1 they give the conversion.  A round synthesises the target voice's prompt, `window` tokens of left context, the new
        chunk and the lookahead, so its cost does not grow with the length of the source (window=None: every round re-synthesises everything so far); the
        default 200 + chunk 50 is the 250-token round the flow is tuned at.  Arguments are checked and the source is tokenised when this is CALLED, as generate
        does; self.ref_dict is written only when target_voice_path is given.  The target voice's prompt must be a whole number of tokens (2 mel frames per
        prompt token).  If a watermarker is loaded it is applied to each piece.  seed: generate()'s; the noise of a windowed stream is then filled round by round.
        speed (a number in [0.5, 2.0]): generate(speed=)'s speaking rate at the bounded cost of a windowed round; the pieces add up to generate(speed=)'s length.
        sample_rate, encoding: as ChatterboxTTS.generate_stream."""
        from .engine import check_stream_window
        opts = _Options(self, seeds=seed, sample_rate=sample_rate, encoding=encoding)
        seed_kw = dict(opts.kw([0]), **_stream_speed_kw(speed))
        for name, v, lo in (("first_chunk", first_chunk, 1), ("chunk", chunk, 1), ("lookahead", lookahead, 0), ("fade", fade, 0)):
            if isinstance(v, bool) or not isinstance(v, int) or v < lo:
                raise ValueError(f"{name}={v!r}: expected an int >= {lo}")
        check_stream_window(window, fade, seed_kw.get("speed"))
        if not chunk_growth >= 1.0:
            raise ValueError(f"chunk_growth={chunk_growth!r}: expected a number >= 1")
        if audio is None and s3_tokens is None:
            raise ValueError("give audio or s3_tokens")
        toks = self._source_tokens(audio, target_voice_path, s3_tokens)
        if toks.numel() == 0:
            raise ValueError("the source has no S3 tokens")
        ref = self.ref_dict  # (the voice of THIS call: a later set_target_voice does not reach into a running stream)

        return self._stream_pieces(self.engine.vocode_stream([toks], ref, first_chunk=first_chunk, chunk=chunk, chunk_growth=chunk_growth, lookahead=lookahead,
                                                             fade=fade, window=window, **seed_kw), opts.fmt)

    MAX_BATCH = 8  # utterances per device batch of generate_batch (flow + vocoder activations grow with batch x length)

    def generate_batch(self, audios=None, target_voice_paths=None, ref_dicts=None, s3_tokens=None, seeds=None, speed=1.0, sample_rate=None, encoding=None, loudness=None, max_pause=None, pause_db=40.0, pitch=None, duration=None, true_peak=None):
        """generate() for B conversions in one call: `audios` (WAV paths, (waveform, sample_rate) pairs or raw (data, sample_rate, encoding[, channels]) tuples; with
        audio_in = "device" the sources of one (rate, encoding, channels) are uploaded and converted together) or `s3_tokens` (B id sequences); target voice per
        request from `target_voice_paths` (one, or a list of B; equal paths are analysed once) or `ref_dicts` (one S3Gen reference dict, or a list of B), neither:
        self.ref_dict.  Returns B CPU float32 tensors (1, n_b) at `.sr` in the caller's order; more than MAX_BATCH requests run as sub-batches in order of length.
        Never overwrites self.ref_dict.  seeds, speed: per request as ChatterboxTTS.generate_batch states them -- request b's noise is that of
        generate(seed=seeds[b]), its speaking rate generate(speed=speed[b])'s; sample_rate, encoding: one format for the call; loudness: a LUFS target for every
        request or one number / None per request, as there."""
        src = s3_tokens if s3_tokens is not None else audios
        assert src is not None, "give audios or s3_tokens"
        src = [src] if (isinstance(src, _PATH) or (torch.is_tensor(src) and src.dim() <= 1)) else list(src)
        B = len(src)
        assert B >= 1, "empty batch"
        opts = _Options(self, B, False, seeds=seeds, speed=speed, sample_rate=sample_rate, encoding=encoding, loudness=loudness, true_peak=true_peak, max_pause=max_pause, pause_db=pause_db, pitch=pitch, duration=duration)
        if target_voice_paths is not None and ref_dicts is not None:
            raise ValueError("give target_voice_paths or ref_dicts, not both")
        if target_voice_paths is not None:
            self._need_analyzer()
            refs = _analysed_once(((p,) for p in _per_request(target_voice_paths, B, "target_voice_paths", _PATH)), self._embed_ref)
        else:
            refs = _per_request(ref_dicts, B, "ref_dicts", (dict,)) if ref_dicts is not None else [self.ref_dict] * B
            assert all(r is not None for r in refs), "Please `prepare_conditionals` first or specify `target_voice_path`"
        if s3_tokens is None:
            self._need_analyzer()
            if self.audio_in == "device":  # the sources of one (rate, encoding, channels) share an upload and a launch; the tokeniser stays one source per pass
                src = [self.analyzer.tokenizer(w)[0] for w in self.analyzer.ingest(src, S3_SR)]
            else:
                src = [self._tokens_of(a) for a in src]
        toks = [torch.as_tensor(t).view(-1).long().cpu() for t in src]
        out, fits = [None] * B, [None] * B
        for idx in batch_plan([int(t.numel()) for t in toks], int(self.MAX_BATCH)):
            wavs, _ = self.engine.vocode(_pick(toks, idx), _one_or_list(_pick(refs, idx)), **opts.kw(idx))
            for i, w in zip(idx, wavs):
                out[i] = self._finish(w, opts.fmt)
            if opts.warp_kw(idx) is not None:
                for i, r in zip(idx, self.engine.last_fit):
                    fits[i] = r
        if opts.warped:
            self._take_fit(fits, "generate_batch")
        return out
