"""generate() = T3.inference -> S3Gen.flow_inference -> HiFT.inference for a BATCH of utterances on one MI355X.

Mirrors the body of `ChatterboxMultilingualTTS.generate` (reference mtl_tts.py:324-352) after text tokenisation:
speech tokens are stripped of SOS/EOS (`drop_invalid_tokens`, s3tokenizer/__init__.py:16-30), the flow + vocoder run
on the padded batch, and each waveform is cut to its own length (the multilingual path also drops the last
token's 40 ms, mtl_tts.py:348-352).
"""
import contextlib
import math
import os
import time
import warnings
from dataclasses import dataclass
from typing import Optional

import torch

from . import ops
from .hift import HiFTEngine
from .s3gen import FlowEngine
from .t3 import T3Engine, START_SPEECH, STOP_SPEECH

SPEECH_VOCAB = 6561
SAMPLES_PER_TOKEN = 960  # 24 kHz / 25 tokens per second


RANGE_TRIPS = 0  # S3Gen passes of this process that met an operand outside the fp16 range and were repeated at bf16x6 (bench.py reports it)


def _range_checked(eng, run, check=True):
    """S3Gen's default numerics (precision 16 = f16x3) need operands inside the fp16 range; a launch that meets one outside it raises a
    device flag (ops.enable_range_flag).  Then the result is not meaningful and the work is repeated at bf16x6, which has the fp32
    exponent range.  check=False: the caller looks at ops.range_flag_tripped() itself at its next synchronisation point."""
    out = run()
    if check and 16 in (eng.flow.precision, eng.hift.precision) and ops.range_flag_tripped():
        with _repeat_at_bf16x6(eng):
            out = run()
    return out


@contextlib.contextmanager
def _repeat_at_bf16x6(eng, what=""):
    """The repeat of S3Gen work whose f16x3 pass raised the range flag: one warning (`what` names the work if it is not the whole call), one count in RANGE_TRIPS,
    and inside the block every engine that runs at precision 16 runs at 6; the precisions are restored behind it, also when the repeat raises."""
    warnings.warn(f"an S3Gen operand exceeded the fp16 range: repeating flow matching + vocoder{what} at bf16x6")
    global RANGE_TRIPS
    RANGE_TRIPS += 1
    saved = eng.flow.precision, eng.hift.precision
    eng.flow.precision, eng.hift.precision = (6 if p == 16 else p for p in saved)
    try:
        yield
    finally:
        eng.flow.precision, eng.hift.precision = saved


def drop_invalid_tokens(x):
    """Strip [SOS ... EOS) and ids outside the S3 codebook (reference s3tokenizer/__init__.py:16-30, tts.py:260-262)."""
    x = x.view(-1)
    sos = (x == START_SPEECH).nonzero()
    s = int(sos[0]) + 1 if len(sos) else 0
    eos = (x == STOP_SPEECH).nonzero()
    e = int(eos[0]) if len(eos) else len(x)
    x = x[s:e]
    return x[x < SPEECH_VOCAB]


def _valid_tokens(toks):
    """What T3 sampled, per utterance, as the flow takes it: drop_invalid_tokens, and the single token 0 for an utterance of which nothing is left (flow and
    vocoder need a frame to work on)."""
    st = [drop_invalid_tokens(t) for t in toks]
    return [t if t.numel() > 0 else torch.zeros(1, dtype=torch.long) for t in st]


def _checked_job(job):
    """A job of synthesize_pipelined with its optional keys checked as synthesize checks its arguments (check_delivery: seeds not together with the job's
    generator, loudness and true_peak not together with a join, speed x pitch).  A join of None is dropped: from here on `"join" in job` says whether the job is joined;
    likewise a format that is None or the default (24 kHz fp32), a loudness that normalises no utterance, pauses that shorten no utterance, a pitch that
    transposes no utterance and a guard of None.  seeds and speed keep their key when the job has one."""
    if job.get("words") is not None:
        raise ValueError(WORDS_PIPELINED)
    d = check_delivery(len(job["text_tokens"]), **{k: job.get(k) for k in ("seeds", "generator", "speed") + Delivery.OPTIONS})
    if d.warp is not None and any(w is not None and "anchors" in w for w in d.warp):
        raise ValueError(WARP_PIPELINED)
    job = {k: v for k, v in job.items() if k not in Delivery.OPTIONS + ("words",) and not (k == "guard" and v is None)}
    job.update(d.kw())
    for k, v in (("seeds", d.seeds), ("speed", d.speed)):
        if job.get(k) is not None:
            job[k] = v
    return job


WORDS_PIPELINED = ("words: the alignment pass runs between T3 and the vocoder of the serial schedule only -- call synthesize(words=) per job "
                   "(synthesize_pipelined keeps two T3 states in flight; the pass inside that overlap is not built)")
WORDS_PAUSES = ("max_pause (pauses) together with word_times (words): the cut map of the pause step is data on the device; mapping word boundaries "
                "through it is not built")


WARP_PIPELINED = ("warp with anchors (timing): the anchors come from the alignment pass, which runs on the serial schedule only -- call synthesize(words=, warp=) "
                  "per job; a job of synthesize_pipelined takes a warp of the duration kind, dict(frames=)")
WARP_WITH = ("{0} together with duration / timing (warp): the time map fixes when things happen; combining it with {0} is not built -- "
             "give one of the two")


GUARD_BANS = "guard together with ban_eos / ban_from: both ban the end-of-speech token the guard must be able to force"


def check_words(words):
    """synthesize's words= argument: None, or dict(heads=None or a sequence of (layer, head) pairs) -> None or dict(heads=...)"""
    if words is None:
        return None
    if not isinstance(words, dict) or set(words) - {"heads"}:
        raise ValueError(f"words: expected None or dict(heads=...), got {words!r}")
    return dict(heads=words.get("heads"))


def valid_frame_counts(toks):
    """c[i] = how many of the sampled tokens toks[:i] the flow receives (drop_invalid_tokens), i = 0 .. len(toks): frame boundary i of the alignment -- which
    counts every sampled token -- is boundary c[i] of the waveform's tokens.  An invalid id in the middle shifts what follows."""
    x = toks.view(-1)
    sos, eos = (x == START_SPEECH).nonzero(), (x == STOP_SPEECH).nonzero()
    s = int(sos[0]) + 1 if len(sos) else 0
    e = int(eos[0]) if len(eos) else len(x)
    keep = (x < SPEECH_VOCAB)
    keep[:s] = False
    keep[e:] = False
    return [0] + torch.cumsum(keep.long(), 0).tolist()


def frame_sample(f, speed=None, pitch=None):
    """The 24 kHz sample at which token frame f (a count of valid speech tokens; 2 mel frames, 960 samples each at speed 1) begins in the waveform vocode(speed=,
    pitch=) returns: the first stretched mel frame j whose position x_j = stretch_position(j, s_eff) is at or beyond mel frame 2 f (s_eff = speed / 2^(pitch /
    12), the rate the mel is stretched at), times 480 -- and under a pitch, which reads that waveform back at a step of r = 2^(pitch / 12), divided by r.  Not
    clipped to the waveform's length: the caller does that."""
    s, r = float(speed or 1.0), (1.0 if not pitch else ops.pitch_ratio(pitch))
    s_eff = s / r
    j = 2 * int(f) if s_eff == 1.0 else _first_frame_at(2.0 * int(f), s_eff)
    pos = (SAMPLES_PER_TOKEN // 2) * j
    return pos if r == 1.0 else int(math.floor(pos / r + 0.5))


def check_warp(warp, B):
    """The `warp` option of an engine call for B utterances: None, or a list / tuple of B entries, each None (a plain row), dict(frames=O) -- fit the row into O >= 1
    mel frames of 480 samples (the duration kind) -- or dict(anchors=[(x, t), ...], end=O or None): input mel frame x (nondecreasing, >= 0) lands on output frame t,
    and the row ends at frame `end` (ops.warp_plan's arguments; x beyond the row's K frames is cut to K when the plan is made).  -> the list with every entry
    normalised, or None when no row is warped.  TypeError / ValueError before anything is launched."""
    import numbers
    if warp is None:
        return None
    if not isinstance(warp, (list, tuple)):
        raise TypeError(f"warp: expected None or a list of {B} entries (None, dict(frames=) or dict(anchors=, end=)), got {type(warp).__name__}")
    if len(warp) != B:
        raise ValueError(f"warp: {len(warp)} entries for {B} utterances")
    integer = lambda v: isinstance(v, numbers.Integral) and not isinstance(v, bool)
    out = []
    for b, w in enumerate(warp):
        if w is None:
            out.append(None)
            continue
        if not isinstance(w, dict) or set(w) not in ({"frames"}, {"anchors"}, {"anchors", "end"}):
            raise ValueError(f"warp[{b}]: expected None, dict(frames=) or dict(anchors=, end=), got {w!r}")
        end = w.get("frames", w.get("end"))
        if "frames" in w and end is None or end is not None and not (integer(end) and 1 <= end <= 2 * 4000):
            raise ValueError(f"warp[{b}]: a length of {end!r} frames (an int in [1, 8000])")
        if "frames" in w:
            out.append(dict(frames=int(end)))
            continue
        anchors, last = [], (0, 0)
        for k, a in enumerate(w["anchors"]):
            if not (isinstance(a, (list, tuple)) and len(a) == 2 and integer(a[0]) and integer(a[1])):
                raise TypeError(f"warp[{b}]: anchor {k} = {a!r}: expected (input frame, output frame) as two ints")
            if a[0] < last[0] or a[1] < last[1]:
                raise ValueError(f"warp[{b}]: anchor {k} = {tuple(a)} after {last}: both frames are nondecreasing and not negative")
            last = (int(a[0]), int(a[1]))
            anchors.append(last)
        out.append(dict(anchors=anchors, end=None if end is None else int(end)))
    return None if all(w is None for w in out) else out


LOUDNESS_JOIN = "loudness together with join: a long text is normalised as a whole, after its pieces are assembled (generate_long(loudness=))"
TRUE_PEAK_JOIN = "true_peak together with join: a long text is limited as a whole, after its pieces are assembled (generate_long(true_peak=))"


@dataclass(frozen=True)
class Delivery:
    """The delivery options of one engine call for B utterances, checked and normalised (check_delivery): seeds (B ints), speed (B floats), pitch (B semitones),
    rates (the B rates at which the mel is stretched: speed, or speed / 2^(pitch / 12) under a pitch), join (ops.check_join's dict), fmt (ops.check_format's
    dict), loud (B LUFS targets / Nones), pz (ops.check_pauses' dict), peak (B true-peak ceilings in dBTP / Nones).  Each is None when the option is off for every utterance -- the call is then, launch for
    launch, the call without it."""
    seeds: Optional[list] = None
    speed: Optional[list] = None
    pitch: Optional[list] = None
    rates: Optional[list] = None
    join: Optional[dict] = None
    fmt: Optional[dict] = None
    loud: Optional[list] = None
    pz: Optional[dict] = None
    peak: Optional[list] = None  # ops.check_true_peak's list: per utterance None or a ceiling in dBTP
    warp: Optional[list] = None  # check_warp's list: per utterance None, dict(frames=) or dict(anchors=, end=)
    OPTIONS = ("pitch", "join", "format", "loudness", "pauses", "true_peak", "warp")  # the keywords a call carries only when the option is on

    def kw(self):
        """The OPTIONS as the keywords of a downstream call (vocode, a job of synthesize_pipelined): a key is present only when its option is on.  seeds and speed
        are not among them: they travel as they were given."""
        return {k: v for k, v in zip(self.OPTIONS, (self.pitch, self.join, self.fmt, self.loud, self.pz, self.peak, self.warp)) if v is not None}


def check_delivery(B, *, seeds=None, generator=None, speed=None, pitch=None, join=None, format=None, loudness=None, pauses=None, true_peak=None, warp=None):
    """The one place where an engine entry (vocode, both synthesize methods, a job of synthesize_pipelined) checks its delivery options -> Delivery.  In this
    order: seeds (ops.request_seeds; not together with a generator), speed, pitch with the speed x pitch rule (ops.check_speed_pitch), join, format, loudness
    (not together with a join: LOUDNESS_JOIN), true_peak (ops.check_true_peak; not together with a join: TRUE_PEAK_JOIN), pauses, warp (check_warp; not together with speed, pitch, pauses or a join: WARP_WITH).  TypeError / ValueError
    before anything is launched; a checked value passes unchanged."""
    seeds = ops.request_seeds(seeds, B, generator)
    speed = ops.check_speed(speed, B)
    pitch = ops.check_pitch(pitch, B)
    eff = ops.check_speed_pitch(speed, pitch, B)
    join = ops.check_join(join, B)
    fmt = ops.check_format_arg(format)
    loud = ops.check_loudness(loudness, B)
    if loud is not None and join is not None:
        raise ValueError(LOUDNESS_JOIN)
    peak = ops.check_true_peak(true_peak, B)
    if peak is not None and join is not None:
        raise ValueError(TRUE_PEAK_JOIN)
    rates = speed if eff is None else (None if all(e == 1.0 for e in eff) else eff)
    pz = ops.check_pauses(pauses, B)
    warp = check_warp(warp, B)
    if warp is not None:
        for name, on in (("speed", speed), ("pitch", pitch), ("max_pause (pauses)", pz), ("join", join)):
            if on is not None:
                raise ValueError(WARP_WITH.format(name))
    return Delivery(seeds, speed, pitch, rates, join, fmt, loud, pz, peak, warp)


def _joined_on_host(out, rec, n, fmt, pauses, truncated):
    """What synthesize(join=) and a joined job of synthesize_pipelined return once the piece is readable on the host: ops.piece_on_host's dict, plus truncated and,
    with pauses, the record {n', pauses cut, frames removed, n} per chunk as lists"""
    return dict(ops.piece_on_host(out, rec, n, fmt), truncated=truncated, **({} if pauses is None else dict(pauses=pauses.tolist())))


def _fit_report(w, plan):
    """What last_fit keeps for a warped row: target (the frames asked for: dict(frames=)'s O, or `end` of an anchored row, None when that was left open), frames
    (the output length), rate = (min, max) over the plan's segments, clamped (ops.warp_plan's: the anchors that missed their frame, "end" for a missed length),
    table (the map itself, mel_time_warp's row), and for an anchored row achieved (the output frame of every anchor) and dropped."""
    rates = [s for _, _, s in plan["table"]]
    rep = dict(target=w.get("frames", w.get("end")), frames=plan["frames"], rate=(min(rates), max(rates)), clamped=list(plan["clamped"]), table=list(plan["table"]))
    if "anchors" in w:
        rep.update(achieved=list(plan["achieved"]), dropped=list(plan["dropped"]))
    return rep


class S3GenEngine:
    """The S3Gen half of every engine -- flow matching (FlowEngine) and vocoder (HiFTEngine) of one checkpoint on one device -- and what is built on the two alone:
    vocode, vocode_stream and the streams and kernel forms of the overlapped schedules.  On its own it is the engine of voice conversion (no T3);
    ChatterboxEngine and TurboEngine put their T3 in front of it."""
    t3 = None
    last_limit = None  # set by a call with true_peak= (S3GenEngine.__init__ states the layout)
    last_fit = None  # per utterance of the last vocode(warp=) call: None (a plain row) or _fit_report's dict; None after a call without warp

    def __init__(self, s3gen_sd, device="cuda", meanflow=False):
        self.dev = torch.device(device)
        self.flow = FlowEngine(s3gen_sd, self.dev, meanflow=meanflow)
        self.hift = HiFTEngine(s3gen_sd, self.dev)
        self.last_timing = {}
        self.last_loudness = None  # the (B, 4) float64 device tensor {L, peak, gain, blocks used} of the last call with loudness=; not synchronised
        self.last_limit = None  # the (B, 4) float64 device tensor {true peak, min g, samples with g < 1, samples over the ceiling} of the last call with true_peak=; not synchronised
        self.last_pauses = None  # the (B, 4) int32 device tensor {n', pauses cut, frames removed, n} of the last call with pauses=; not synchronised

    @ops.on_device
    @torch.inference_mode()
    def vocode(self, speech_tokens, gen_ref, z=None, phase=None, noise=None, n_cfm_timesteps=10, drop_last_token=False, sync=True, hift_stream=None,
               generator=None, seeds=None, speed=None, join=None, format=None, loudness=None, pauses=None, pitch=None, warp=None, true_peak=None):
        """S3Gen.inference for a list of 1-D token tensors (already valid ids).  Returns (list of 1-D wav tensors on
        device, mel (B, 2Nmax, 80) channel-last).  hift_stream (synthesize_pipelined): the vocoder runs on THAT stream behind an event, so the flow
        stream is free for the next batch's encoder + CFM; the returned waveforms belong to it.  generator: a torch.Generator on the engine's device for the flow / vocoder noise
        that is not injected (None: the global RNG).  seeds: None, or B ints in [0, 2^64) (an int: the same for every utterance) -- the noise that is not injected
        is then a function of the utterance's seed alone (ops.seeded_z / seeded_phase / seeded_noise: cbx_rng_fill_f32), whatever its row and the batch around it,
        and no torch RNG is consumed; not together with a generator.
        speed: None, a number or B numbers in [0.5, 2.0] (ops.check_speed; None entries are 1.0) -- the speaking rate.  None or all 1.0: exactly the call without
        it.  Otherwise the flow runs as ever and ONE ops.mel_time_scale launch stretches row b's M_b = 2 n_b - short_b valid mel frames to O_b =
        ops.scaled_len(M_b, speed[b]) (models/s3gen/s3gen.py:289 leaves this out); the vocoder runs on the stretched mel with lens = O_b, so the F0 predictor
        sees it and the pitch is kept.  Utterance b's waveform is max(1, floor(K_b / speed[b])) * 480 samples where the unscaled call returns K_b * 480.
        Noise and phase that are not injected are sized from the stretched mel; injected ones must have ITS shapes: phase (B, 9), noise
        (B, 9, 480 * max_b O_b).  z is the flow's and does not change.  The returned mel stays the unscaled flow mel.
        join (None: this call, launch for launch; else ops.check_join's dict(gaps=[B ints], trim_db=float|None, pad_frames=int, fade=int, first=bool, last=bool)):
        long-form synthesis -- the B utterances are consecutive chunks of one text, and two launches behind the vocoder, on the stream that owns the waveforms,
        trim each of its silence (cbx_wave_edges_f32; skipped with trim_db=None) and lay them out with their gaps and fades as ONE piece (cbx_wave_join_f32).  The
        call then returns (piece, mel), piece = ops.wave_join's dict on the device: the `out` buffer, its layout record and the edge table.  Nothing is synchronised
        for it; ops.piece_on_host reads it once it is on the host.
        format (None or the default: this call, launch for launch; else ops.check_format's dict(sample_rate=, encoding=)): the delivery format -- ONE
        ops.wave_format launch (cbx_wave_format_f32) behind the vocoder, on the stream that owns the waveforms, resamples the B cut waveforms and encodes them; the
        call returns them as views (float32, int16 or uint8) of one packed buffer, utterance b with ops.formatted_len(n_b, sample_rate) elements.  With a join the
        launch converts the joined piece instead: the join writes into a zeroed buffer, so converting all of it gives, in [0, formatted_len(total)), exactly the
        conversion of the piece's [0, total); the piece dict gains `formatted` (that buffer) and `format`; layout and edges stay in 24 kHz samples.
        loudness (None, or no utterance with a target: this call, launch for launch; else ops.check_loudness's list -- a number or B numbers / Nones in [-50, -5]
        LUFS): ops.wave_normalize behind the vocoder, on the stream that owns the waveforms -- the BS.1770-4 integrated loudness of each cut waveform (after the
        speed stretch has shaped it) is measured and the waveform multiplied in place by the gain that brings it to its target, limited so that no sample exceeds
        1.0; a None entry, a silent utterance and one shorter than 0.4 s keep their samples.  It runs ahead of the format launch, whose s16 / G.711 store therefore
        sees the normalised signal and does not clip.  The stats {L, peak, gain, blocks used} of the call stay on the device as self.last_loudness; nothing is
        synchronised.  Not together with a join (ValueError): a long text is normalised as a whole.
        true_peak (None, or no utterance with a ceiling: this call, launch for launch; else ops.check_true_peak's list -- a number or B numbers / Nones in [-20, 0]
        dBTP): the true-peak limiter -- ONE ops.wave_limit call (cbx_wave_limit_f32, two launches) behind pitch and loudness, on the stream that owns the
        waveforms, ahead of the pauses and the format launch, whose s16 / G.711 store therefore sees the limited signal: the 4-times oversampled peak of every row
        with a ceiling is held under it by a look-ahead gain envelope (include/cbx.h states the definition).  A row with a loudness target AND a ceiling gets the
        full gain to its target -- the sample-peak cap of 1.0 is the limiter's job there --; what the limiter removes is not measured again, so its loudness can
        end below the target.  A row without a ceiling is what the call without true_peak returns, bit for bit.  The stats {true peak, min g, samples with
        g < 1, samples over the ceiling} stay on the device as self.last_limit; nothing is synchronised.  It changes no length.  Not together with a join
        (ValueError): a long text is limited as a whole.
        pauses (None, or no utterance with a keep: this call, launch for launch; else ops.check_pauses' dict(keep=[B ints], db=, fade=)): the pause control --
        ops.wave_squeeze (cbx_wave_squeeze_f32) on the stream that owns the waveforms, behind the loudness step (which measures and gains the unshortened rows) and
        ahead of the join and / or the format launch: of every silence inside utterance b that is longer than keep[b] frames of 480 samples, keep[b] remain.  The
        new lengths n' exist on the device only (self.last_pauses keeps the record {n', pauses cut, frames removed, n}; not synchronised).  Without a join: with
        sync=True the record is read (one small copy) and the returned waveforms are cut to n' -- formatted ones to ops.formatted_len(n', rate): the conversion
        of a zero-tailed row is, in that range, the conversion of the exact-length row --; with sync=False the call returns dict(rows=, pauses=, format=) on the
        device, the rows still n long with zero tails, for ops.cut_pauses once the record is on the host.  With a join the three launches run in the order edges
        (on the original rows), squeeze (which maps the edge table), join (ops.wave_join(squeeze=)); the piece gains `pauses`, and its layout is in delivered
        samples already.
        pitch (None, or every entry None / 0: this call, launch for launch; else a number or B numbers / Nones in [-12, 12] semitones, ops.check_pitch): the pitch
        control.  With r_b = ops.pitch_ratio(pitch[b]) the ONE ops.mel_time_scale launch stretches row b at s_eff = speed[b] / r_b (ops.check_speed_pitch: in
        [0.5, 2.0], else a ValueError naming both arguments; a row without a pitch at its plain speed), the vocoder runs on that mel -- noise, phase and seeded
        draws sized from it exactly as speed= sizes them --, and ONE ops.wave_pitch launch (cbx_wave_pitch_f32) on the stream that owns the waveforms reads the
        cut rows, 480 scaled_len(K_b, s_eff) samples, at a step of r_b into 480 scaled_len(K_b, speed[b]) samples: the length of the call without a pitch,
        every frequency multiplied by r_b.  The formants move with the pitch.  The launch runs ahead of the loudness step, the pauses, the join and the format
        launch, which see its rows (views of one packed buffer; a row without a pitch is copied).
        warp (None, or no utterance with an entry: this call, launch for launch; else check_warp's list): the timing control.  Row b's entry is None, dict(frames=O)
        -- fit the K_b frames the plain call returns into O -- or dict(anchors=[(x, t), ...], end=O or None) -- mel frame x lands on output frame t.  ops.warp_plan
        turns it into a piecewise-linear map whose every rate lies in [0.5, 2.0] (a target that needs more is met as far as the bound allows: nothing is padded or
        cut), ONE ops.mel_time_warp launch (cbx_mel_time_warp_f32) in the place of the ops.mel_time_scale launch warps the flow's mel -- a plain row of the batch
        rides along on the one-segment rate-1 table, which copies it --, the vocoder runs on the warped mel with lens = frames, noise, phase and seeded draws sized
        from it as speed= sizes them, and row b comes back with frames_b * 480 samples.  self.last_fit keeps the plans (_fit_report).  Not together with speed,
        pitch, pauses or a join (ValueError naming both).  The returned mel stays the flow's."""
        B = len(speech_tokens)
        d = check_delivery(B, seeds=seeds, generator=generator, speed=speed, pitch=pitch, join=join, format=format, loudness=loudness, pauses=pauses, warp=warp, true_peak=true_peak)
        seeds, rates = d.seeds, d.rates
        ns = [int(t.numel()) for t in speech_tokens]
        Nmax = max(ns)
        tok = torch.zeros(B, Nmax, dtype=torch.long)
        for b, t in enumerate(speech_tokens):
            tok[b, : ns[b]] = t
        lens = torch.tensor(ns, dtype=torch.int32)
        same = all(n == Nmax for n in ns)
        refs = list(gen_ref) if isinstance(gen_ref, (list, tuple)) else [gen_ref] * B  # one voice for all, or one per utterance (s3gen.py:173-229)
        assert len(refs) == B, f"{len(refs)} voices for {B} utterances"
        shorts = [int(r["prompt_feat"].reshape(-1, 80).shape[0]) - 2 * int(r["prompt_token"].numel()) for r in refs]
        plans = None if d.warp is None else self._warp_plans(d.warp, ns, shorts, drop_last_token)
        self.last_fit = None if plans is None else [None if p is None else _fit_report(w, p) for w, p in zip(d.warp, plans)]

        def run():
            t0 = time.perf_counter()
            mel = self.flow.inference(tok.to(self.dev), lens.to(self.dev), gen_ref, z=z, n_steps=n_cfm_timesteps, generator=generator, seeds=seeds)
            if sync:  # per-stage wall times; the pipelined mode never blocks the host between stages
                torch.cuda.synchronize()
            t1 = time.perf_counter()
            # short_b > 0 only when the prompt mel has an odd frame more than 2 * prompt tokens (flow.py:170-195); per voice when the batch mixes voices
            if plans is not None:  # ONE launch: warped rows by their plans over the M_b valid frames, plain rows copied by the rate-1 table
                M = [2 * n - sh for n, sh in zip(ns, shorts)]
                vmel, mel_lens = ops.mel_time_warp(mel, [[(0, 0.0, 1.0)] if p is None else p["table"] for p in plans], in_lens=M,
                                                   out_lens=[m if p is None else p["frames"] for m, p in zip(M, plans)])
            elif rates is None:
                vmel, mel_lens = mel, None if same and len(set(shorts)) == 1 else (2 * lens - torch.tensor(shorts, dtype=torch.int32)).to(self.dev)
            else:  # the vocoder's input is the stretched mel; lens always: the rows differ
                vmel, mel_lens = ops.mel_time_scale(mel, rates, in_lens=[2 * n - sh for n, sh in zip(ns, shorts)])
            if hift_stream is not None:
                ev = torch.cuda.Event()
                ev.record()
                with torch.cuda.stream(hift_stream):
                    hift_stream.wait_event(ev)
                    vmel.record_stream(hift_stream)
                    if mel_lens is not None:
                        mel_lens.record_stream(hift_stream)
                    wav, _ = self.hift.inference(vmel, phase=phase, noise=noise, lens=mel_lens, fade=True, generator=generator, seeds=seeds)
            else:
                wav, _ = self.hift.inference(vmel, phase=phase, noise=noise, lens=mel_lens, fade=True, generator=generator, seeds=seeds)
            if sync:
                torch.cuda.synchronize()
            t2 = time.perf_counter()
            self.last_timing.update(flow_s=t1 - t0, hift_s=t2 - t1)
            return wav, mel

        wav, mel = _range_checked(self, run, check=sync)
        return self._deliver(wav, ns, shorts, d, drop_last_token, sync, hift_stream, plans), mel

    @staticmethod
    def _warp_plans(warp, ns, shorts, drop_last_token):
        """ops.warp_plan per warped row over K_b, the frames the plain call returns for it (the rule of _deliver); an anchor beyond K_b is cut to K_b"""
        plans = []
        for w, n, sh in zip(warp, ns, shorts):
            if w is None:
                plans.append(None)
                continue
            K = min(2 * (max(1, n - 1) if drop_last_token else n), 2 * n - sh)
            if "frames" in w:
                plans.append(ops.warp_plan(K, [], end=w["frames"]))
            else:
                plans.append(ops.warp_plan(K, [(min(x, K), t) for x, t in w["anchors"]], end=w["end"]))
        return plans

    def _deliver(self, wav, ns, shorts, d, drop_last_token, sync, hift_stream, plans=None):
        """The chain behind the vocoder, in the one order vocode's docstring states: cut the rows of the padded batch `wav`, pitch, loudness, then either edges +
        squeeze + join (ONE ops.wave_join call) or the squeeze alone, then the format; with a true_peak the loudness step and the limiter are _limit's.  Every launch lands on the stream that owns the waveforms: ONE stream
        scope, entered only when a step is on.  Returns the rows; the formatted views; with pauses the rows cut through ops.cut_pauses (sync=True) or
        dict(rows=, pauses=, format=) for the caller to cut (sync=False); with a join the piece dict, with `formatted` / `format` under a format."""
        HALF = SAMPLES_PER_TOKEN // 2
        out, plain = [], []
        for b, n in enumerate(ns):
            keep = max(1, n - 1) if drop_last_token else n
            frames = min(2 * keep, 2 * n - shorts[b])  # K_b: what the unscaled call returns, in mel frames of 480 samples
            if d.pitch is not None:
                plain.append(ops.scaled_len(frames, d.speed[b]) if d.speed is not None else frames)
            if d.rates is not None:
                frames = ops.scaled_len(frames, d.rates[b])
            if plans is not None and plans[b] is not None:
                frames = plans[b]["frames"]
            out.append(wav[b, : frames * HALF])
        if not d.kw():
            return out
        with (torch.cuda.stream(hift_stream) if hift_stream is not None else contextlib.nullcontext()):
            if d.pitch is not None:  # the source rows, read at a step of r_b into the lengths of the call without a pitch
                out = ops.wave_pitch(out, [ops.pitch_ratio(p) for p in d.pitch], [k * HALF for k in plain])
            if d.peak is not None:
                out = self._limit(out, d)
            elif d.loud is not None:
                self.last_loudness = ops.wave_normalize(out, d.loud)
            if d.join is not None:  # (a join that will be formatted writes into a zeroed buffer: converting all of it converts the piece)
                cap = sum(int(w.numel()) for w in out) + sum(d.join["gaps"])
                piece = ops.wave_join(out, **({} if d.pz is None else dict(squeeze=d.pz)), **({} if d.fmt is None else dict(out=torch.zeros(max(1, cap), device=wav.device))),
                                      **d.join)
                if d.pz is not None:
                    self.last_pauses = piece["pauses"]
                return piece if d.fmt is None else dict(piece, formatted=ops.wave_format([piece["out"]], d.fmt)[0], format=d.fmt)
            stats = None
            if d.pz is not None:
                sq = ops.wave_squeeze(out, d.pz["keep"], d.pz["db"], d.pz["fade"])
                out, stats = sq["rows"], sq["stats"]
                self.last_pauses = stats
            if d.fmt is not None:
                out = ops.wave_format(out, d.fmt)
            if stats is None:
                return out
            return ops.cut_pauses(out, stats.cpu(), d.fmt) if sync else dict(rows=out, pauses=stats, format=d.fmt)

    def _limit(self, out, d):
        """The loudness step and the true-peak limiter of a batch in which a row has a ceiling.  A row with a target AND a ceiling gets the FULL gain to its target
        (the meter runs for it with ceiling=None; the limiter holds the peaks); a row with a target and no ceiling keeps the sample-peak cap of 1.0, and so the
        bits of the call without true_peak.  The meter runs once per kind of row that is present (ops.wave_loudness per group); its gain vector goes into the ONE
        limiter launch as the pre-gain, which every row of the batch passes -- a row without a ceiling is copied as x * gain, ops.wave_gain's bits, so
        ops.wave_gain is not launched.  last_loudness / last_limit keep the stats on the device."""
        gain = None
        if d.loud is not None:
            B = len(out)
            capped = [b for b in range(B) if d.loud[b] is not None and d.peak[b] is None]
            free = [b for b in range(B) if b not in capped]
            if not capped:
                self.last_loudness, gain = ops.wave_loudness(out, d.loud, None)
            else:
                self.last_loudness = torch.empty(B, 4, dtype=torch.float64, device=out[0].device)
                gain = torch.empty(B, dtype=torch.float32, device=out[0].device)
                for idx, ceiling in ((capped, 1.0), (free, None)):
                    if idx:
                        st, g = ops.wave_loudness([out[b] for b in idx], [d.loud[b] for b in idx], ceiling)
                        at = torch.tensor(idx, device=g.device)
                        self.last_loudness[at], gain[at] = st, g
        out, self.last_limit = ops.wave_limit(out, d.peak, gain=gain)
        return out

    def co_resident(self, on):
        """Both stages on (or off) the kernel forms whose workgroups can share a CU with the other stage's (T3Engine.co_resident, FlowEngine.co_resident)."""
        if self.t3 is not None and hasattr(self.t3, "co_resident"):
            self.t3.co_resident(on)
        self.flow.co_resident(on)

    def _pipeline_streams(self, priorities=(-1, 0)):
        """The T3 / flow streams of the overlapped schedules (created once; HIP priorities: measured, no effect either way)."""
        if not hasattr(self, "_s_t3"):
            pt3, pvoc = priorities
            self._s_t3 = torch.cuda.Stream(device=self.dev, priority=pt3)
            self._s_t3x = [self._s_t3] + [torch.cuda.Stream(device=self.dev, priority=pt3) for _ in range(2)]  # one per T3 state in flight
            self._s_voc = torch.cuda.Stream(device=self.dev, priority=pvoc)

    @torch.inference_mode()
    def vocode_stream(self, speech_tokens, gen_ref, *, first_chunk=25, chunk=50, chunk_growth=1.0, lookahead=3, fade=480, window=None, z=None, phase=None,
                      noise=None, n_cfm_timesteps=10, drop_last_token=False, seeds=None, speed=None, format=None):
        """vocode() in rounds: the schedule, the yields and the `window` of synthesize_stream with a list of B 1-D token tensors (valid ids; lengths may differ) in
        place of T3 -- round r synthesises the first n_r tokens of every utterance (stream_token_schedule over the longest), utterance b is final once
        n_r >= N_b.  No T3 is touched: this is the streaming form of voice conversion (the engine ChatterboxVC builds has none), where every token exists up
        front and the input can be arbitrarily long -- give a `window`.  gen_ref: one voice with a whole-token prompt.  seeds: as vocode(seeds=); with a window the
        noise is filled round by round (_stream_rounds).  speed: None or ONE number in [0.5, 2.0] -- the speaking rate of vocode(speed=), as synthesize_stream(speed=)
        takes it: utterance b's pieces add up to the length vocode(speed=) returns.  format: vocode(format=)'s dict, as synthesize_stream(format=) takes it."""
        check_stream_window(window, fade, check_stream_speed(speed))
        seeds = ops.check_seeds(seeds, len(speech_tokens))
        format = ops.check_format_arg(format)
        pin = self.dev if self.dev.index is not None else torch.device("cuda", torch.cuda.current_device())
        torch.cuda.set_device(pin)  # (a generator cannot hold a device guard across yields)
        toks = [torch.as_tensor(t).view(-1).long().cpu() for t in speech_tokens]
        assert toks and all(t.numel() > 0 for t in toks), "vocode_stream: every utterance needs at least one token"
        lens = [int(t.numel()) for t in toks]
        self.co_resident(False)
        one_round, closed = _stream_rounds(self, len(toks), gen_ref, n_tokens=max(lens), round_tokens=lambda ts, fin: ts, lookahead=lookahead, fade=fade, z=z,
                                           phase=phase, noise=noise, n_cfm_timesteps=n_cfm_timesteps, drop_last_token=drop_last_token, window=window, seeds=seeds, speed=speed,
                                           format=format)
        for n_r in stream_token_schedule(max(lens), first_chunk, chunk, lookahead, chunk_growth):
            yield one_round([t[:n_r] for t in toks], [n_r >= n for n in lens], n_r >= max(lens))
            if all(closed):
                return


class ChatterboxEngine(S3GenEngine):
    last_guard = None  # the alignment guard's per-utterance report of the last guarded synthesize() call / synthesize_pipelined job yielded
    t3_pair = True     # synthesize_pipelined(t3_pair=None): pair the T3 of jobs 2p and 2p + 1 (the public classes of api.py switch it off for their sub-batches)

    def __init__(self, t3_sd, s3gen_sd, device="cuda", n_t3_layers=None, meanflow=False, t3_weights=None):
        self.dev = torch.device(device)
        self.t3_weights = t3_weights  # None / "fp32" (parity path) or "bf16" (opt-in: decode weight images rounded to bf16)
        self.t3 = self._build_t3(t3_sd, n_t3_layers)  # (T3 first, then flow and vocoder: the order in which the engines have always taken their device memory)
        super().__init__(s3gen_sd, device, meanflow=meanflow)

    def _build_t3(self, t3_sd, n_layers):
        """CBX_PACK_CACHE=<dir>: keep the packed device layout of the T3 weights (4 GB: row-major + lane-ordered GEMV images) on disk,
        keyed by a fingerprint of the checkpoint, and map it straight to the device on later starts (formats.py)."""
        cache = os.environ.get("CBX_PACK_CACHE")
        if not cache:
            return T3Engine(t3_sd, self.dev, n_layers=n_layers, weight_dtype=self.t3_weights)
        from . import formats
        fp = formats.fingerprint(t3_sd) + f"-L{n_layers}"
        path = os.path.join(cache, f"t3_{fp}.cbxpack")
        kind = formats.packed_kind("t3-llama-" + os.environ.get("CBX_T3_DECODE", "v2") + "-" + (self.t3_weights or os.environ.get("CBX_T3_WEIGHTS", "fp32"))
                                   + f"-ht{int(bool(T3Engine._TUNE.get('half_tiles')))}")  # the half-tile images are part of the packed set
        t = formats.load_packed(path, fp, kind)
        if t is not None:
            return T3Engine.from_packed(t, self.dev)
        eng = T3Engine(t3_sd, self.dev, n_layers=n_layers, weight_dtype=self.t3_weights)
        os.makedirs(cache, exist_ok=True)
        formats.save_packed(eng.export_packed(), path, fp, kind)
        return eng

    @ops.on_device
    @torch.inference_mode()
    def synthesize(self, text_tokens, t3_conds, gen_ref, *, max_new_tokens=1000, temperature=0.8, top_p=1.0, min_p=0.05,
                   repetition_penalty=1.2, cfg_weight=0.5, uniforms=None, ban_eos=False, ban_from=0, z=None, phase=None,
                   noise=None, n_cfm_timesteps=10, drop_last_token=True, generator=None, seeds=None, speed=None, join=None, format=None, loudness=None, pauses=None, pitch=None,
                   words=None, guard=None, warp=None, true_peak=None):
        """Full hot path for B utterances.  Returns (wavs: list of 1-D device tensors, speech_tokens: list).  t3_conds / gen_ref: one voice or a list of B;
        temperature, top_p, min_p, repetition_penalty, cfg_weight: a scalar or a sequence of B; generator: torch.Generator (device) for every draw that is not injected.
        seeds: None, or B ints in [0, 2^64) (an int: the same for every utterance): every draw of utterance b that is not injected depends on seeds[b] alone
        (T3Engine.generate(seeds=), vocode(seeds=)); not together with a generator.
        speed: None, a number or B numbers in [0.5, 2.0]: the speaking rate of vocode(speed=); T3 and its tokens do not depend on it.
        join: None, or vocode(join=)'s dict -- the B utterances are consecutive chunks of one text; the call then returns (piece, speech_tokens) with piece =
        ops.piece_on_host's dict (wav = the joined piece on the device, offsets, total, edges, n) plus truncated = [B bools: T3 spent its budget without EOS].
        format: None, or vocode(format=)'s dict -- the waveforms (the joined piece's `wav`) come back at that sample rate in that encoding.
        loudness: None, a number or B numbers / Nones in [-50, -5] LUFS -- vocode(loudness=): every utterance with a target is brought to it on the device (sample
        peak limited to 1.0); not together with a join.
        true_peak: None, a number or B numbers / Nones in [-20, 0] dBTP -- vocode(true_peak=): every utterance with a ceiling is limited to it on the device, behind
        the loudness step (which then applies its full gain); not together with a join.
        pauses: None, or vocode(pauses=)'s dict / list -- silences inside an utterance longer than its keep are shortened on the device; the waveforms come back cut
        to their new lengths, a joined piece gains `pauses` = the record {n', pauses cut, frames removed, n} per chunk as lists.
        pitch: None, a number or B numbers / Nones in [-12, 12] semitones -- vocode(pitch=): utterance b comes back transposed by pitch[b] at the length speed[b]
        alone gives it; T3 and its tokens do not depend on it.  speed / 2^(pitch / 12) outside [0.5, 2.0] is a ValueError before anything is launched.
        words: None, or dict(heads=None or (layer, head) pairs) -- word timestamps: T3Engine.align runs between T3 and the vocoder, on the state the tokens came
        from, and the call returns (wavs, speech_tokens, alignment): per utterance dict(frames = [(f0, f1) per text token]: the token is spoken over the valid
        speech tokens [f0, f1) (valid_frame_counts: the tokens the flow receives; 960 samples each at speed 1), n_frames, speed, pitch -- what frame_sample needs
        to turn a frame into a sample of wavs[b]).  Not together with pauses; at most T3Engine.MAX_BATCH utterances.  Without it the call is launch for launch
        the one it always was.
        guard: None, or T3Engine.generate(guard=)'s dict -- the alignment guard inside the token step (it holds EOS back until the text has been spoken and
        forces it when the alignment says the utterance is over); last_guard is then the per-utterance report (T3Engine.collect).  Not with ban_eos / ban_from.
        warp: None, or vocode(warp=)'s list -- the timing control; T3 and its tokens do not depend on it.  An entry dict(frames=O) fits the utterance into O mel
        frames.  With words= an entry may instead be dict(starts=[one output frame or None per TEXT TOKEN], end=O or None): once t3.align has said where every
        text token begins, token i with a start becomes the anchor (2 c[f0_i], starts[i]) -- its first mel frame lands on that output frame --, and the
        alignment entry of the utterance gains `table`, the map its boundaries go through (ops.warp_place); without words= such an entry is a ValueError.
        last_fit is vocode's."""
        starts = None
        if warp is not None and isinstance(warp, (list, tuple)) and any(isinstance(w, dict) and "starts" in w for w in warp):
            if words is None:
                raise ValueError("warp with starts: the anchors come from the alignment pass -- give words= as well")
            starts = [w if isinstance(w, dict) and "starts" in w else None for w in warp]
            for b, w in enumerate(starts):
                if w is not None and (set(w) - {"starts", "end"} or len(w["starts"]) != int(text_tokens[b].numel())):
                    raise ValueError(f"warp[{b}]: dict(starts=, end=) with one start / None per text token ({int(text_tokens[b].numel())}), got {w!r}")
            # checked as anchors at the frames they will at least have (x is known only after the alignment): the targets alone
            warp = [w if s is None else dict(anchors=[(0, t) for t in s["starts"] if t is not None], end=s.get("end")) for w, s in zip(warp, starts)]
        if guard is not None:
            guard = self.t3.check_guard(guard)
            if ban_eos or ban_from > 0:
                raise ValueError(GUARD_BANS)
        words = check_words(words)
        if words is not None:
            if pauses is not None and ops.check_pauses(pauses, len(text_tokens)) is not None:
                raise ValueError(WORDS_PAUSES)
            if len(text_tokens) > self.t3.MAX_BATCH:
                raise ValueError(f"words: {len(text_tokens)} utterances (at most {self.t3.MAX_BATCH}: the pass runs on the state of ONE device batch)")
            self.t3.check_align_heads(words["heads"])
        d = check_delivery(len(text_tokens), seeds=seeds, generator=generator, speed=speed, pitch=pitch, join=join, format=format, loudness=loudness, pauses=pauses,
                           warp=warp, true_peak=true_peak)
        seeds = d.seeds
        self.co_resident(False)  # the serial schedule runs every kernel on its fastest-alone form (a no-op unless synthesize_pipelined ran before)
        t0 = time.perf_counter()
        toks = self.t3.generate(t3_conds, text_tokens, max_new_tokens=max_new_tokens, temperature=temperature, top_p=top_p,
                   min_p=min_p, repetition_penalty=repetition_penalty, cfg_weight=cfg_weight, uniforms=uniforms,
                   ban_eos=ban_eos, ban_from=ban_from, generator=generator, seeds=seeds, **({} if guard is None else dict(guard=guard)))
        self.last_guard = None if guard is None else self.t3.last_guard
        torch.cuda.synchronize()
        self.last_timing = dict(t3_s=time.perf_counter() - t0)
        st = _valid_tokens(toks)
        alignment = None
        if words is not None:
            t1 = time.perf_counter()
            spans = self.t3.align(text_tokens, toks, align_heads=words["heads"])
            alignment = []
            for b, (sp, t) in enumerate(zip(spans, toks)):
                c = valid_frame_counts(t)
                alignment.append(dict(frames=[(c[f0], c[f1]) for f0, f1 in sp.tolist()], n_frames=c[-1], speed=None if d.speed is None else d.speed[b],
                                      pitch=None if d.pitch is None else d.pitch[b]))
            self.last_timing["align_s"] = time.perf_counter() - t1
        vkw = d.kw()
        if starts is not None:  # word i's first mel frame, 2 c[f0_i], lands on its target
            vkw["warp"] = [w if s is None else dict(anchors=[(2 * f[0], t) for f, t in zip(a["frames"], s["starts"]) if t is not None], end=s.get("end"))
                           for w, s, a in zip(d.warp, starts, alignment)]
        wavs, _ = self.vocode(st, gen_ref, z=z, phase=phase, noise=noise, n_cfm_timesteps=n_cfm_timesteps,
                              drop_last_token=drop_last_token, generator=generator, seeds=seeds, speed=d.speed, **vkw)
        if alignment is not None and self.last_fit is not None:
            for a, fit in zip(alignment, self.last_fit):
                if fit is not None:
                    a["table"] = fit["table"]  # (frame_sample is for unwarped rows: a warped row's boundaries go through ops.warp_place(table, 2 f) * 480)
        if d.join is not None:  # (the record's copy waits for the two launches behind the vocoder)
            wavs = _joined_on_host(wavs.get("formatted", wavs["out"]), wavs["rec"], wavs["n"], d.fmt, wavs.get("pauses"), self._truncated(toks))
        self.last_timing["total_s"] = time.perf_counter() - t0
        return (wavs, st) if alignment is None else (wavs, st, alignment)

    @staticmethod
    def _truncated(toks):
        """Per utterance of a joined piece: T3 spent its budget without sampling an end-of-speech token (generate keeps a sampled one in `toks`)."""
        return [not bool((t == STOP_SPEECH).any()) for t in toks]
    @torch.inference_mode()
    def synthesize_pipelined(self, jobs, co_resident=True, host_threads=True, t3_in_flight=2, stream_priorities=(-1, 0), t3_pair=None, **kw):
        """Throughput mode for a stream of batches: T3 of batch k+1 runs on a high-priority HIP stream WHILE the flow
        matching + vocoder of batch k run on a second stream.  jobs: list of dicts(text_tokens=[...], t3_conds=..., gen_ref=...); yields
        (wavs, tokens, latency_s) per job in order.  Results are identical to synthesize() called per job.  A job may carry sampling parameters of its own
        (temperature, top_p, min_p, repetition_penalty, cfg_weight: scalar or one per utterance; they override **kw for that job) and a `generator` for the flow / vocoder noise that is not injected (the
        sampling draws of a repeatable job are injected as `uniforms`: T3 is enqueued by another host thread), or `seeds` (one int per utterance, or one int for all:
        every draw of the job that is not injected, as synthesize(seeds=); not together with a generator), or `speed` (a number or one per utterance: vocode(speed=)),
        or `format` (vocode(format=)'s dict: the job's audio is converted on the device ahead of its copies, which then carry the encoded samples),
        or `loudness` (vocode(loudness=): a number or one number / None per utterance; the meter and the gain run behind the vocoder on its stream; not with a join),
        or `pitch` (vocode(pitch=): a number or one number / None per utterance, semitones; the launch runs behind the vocoder on its stream),
        or `true_peak` (vocode(true_peak=): a number or one number / None per utterance, dBTP; the limiter runs behind the vocoder on its stream; not with a join),
        or `warp` (vocode(warp=)'s list, entries of the duration kind -- None or dict(frames=) -- only: anchors need the alignment pass of the serial schedule,
        WARP_PIPELINED; engine.last_fit is the job's report while the job is the one just yielded),
        or `guard` (T3Engine.generate(guard=)'s dict: the job's T3 runs with the alignment guard inside its token step, in whichever of the two T3 states it
        lands; engine.last_guard is the job's report while the job is the one just yielded; not with ban_eos / ban_from),
        or `pauses` (vocode(pauses=)'s dict / list: the squeeze runs behind the vocoder on its stream; its record of the new lengths travels to the host as one more
        small pinned copy behind the same event, and the waveforms are cut after it: no host synchronisation is added),
        or `join` (vocode(join=)'s dict: the job's utterances are consecutive chunks of one text; `wavs` is then synthesize(join=)'s piece dict with `wav` on the host.
        The two launches run behind the vocoder on its stream, the piece leaves the device as ONE pinned copy plus one of its small records where a job without
        it makes one copy per utterance, and it is sliced after the event this schedule waits for anyway: no host synchronisation is added).

        What makes the two stages actually overlap (round 5, profiles/r05_overlap_*; none of it changes a result):
          * co_resident: a chain of small dependent kernels keeps its pace beside chip-filling kernels of another stream only if its workgroups FIT
            on the CUs beside theirs (scripts/micro/concur.hip: 1.0x when they fit, 6-7x slower when every launch has to wait for workgroups to retire).
            The CFM runs its plane GEMMs / attention on one-workgroup-per-CU forms (8 waves x <= 120 VGPRs + 96 KiB LDS; 4 waves x 200 VGPRs), the
            decode step on launches of <= 8 waves x <= 128 VGPRs; the decode kernels raise their wave priority (s_setprio 3).
          * host_threads: the decode loop is 250 hipGraph launches of 153 kernel nodes -- ~0.6 ms of HOST time each, invisible in the serial schedule
            (the GPU needs 1.1 ms per token) but 150-180 ms per batch in front of the flow's own ~130 ms of launches when one thread enqueues both
            (scripts/overlap_probe.py: the flow started 180 ms late).  The T3 enqueue runs on a second host thread (graph launches and the ctypes
            calls of the C stage seams release the GIL).
        t3_pair (host_threads only; None: the engine's t3_pair attribute -- True --, unless CBX_T3_PAIR=0 in the environment): jobs 2p and 2p + 1 decode as ONE T3Engine.generate call of up to 32 rows --
        two row tiles per launch, every decode launch streams its weights once for both jobs and each row is bit for bit what its own 16-row launch gives
        (T3Engine._packed_rows); t3_in_flight such calls are in flight.  A pair forms when the two jobs' rows sum to <= 32, neither
        carries a guard, and both inject uniforms, or neither does and both or neither carry seeds; sampling parameters, uniforms and seeds reach the rows of their
        own job.  The pair's tokens are split per job: flow + vocoder of job 2p, then of job 2p + 1, beside the next pair's T3.  Any other job, and the last of an
        odd count, runs alone as before; the yield order, the per-job results, last_guard and last_fit are unchanged (the first audio of job 2p waits for the
        pair's T3).  False: today's schedule, call for call."""
        import threading
        jobs = [_checked_job(job) for job in jobs]
        for job in jobs:  # `guard` (T3Engine.generate(guard=)'s dict): the job's T3 runs guarded, in either slot; engine.last_guard is its report when the job is yielded
            if "guard" in job:
                job["guard"] = self.t3.check_guard(job["guard"])
                if kw.get("ban_eos") or kw.get("ban_from", 0) > 0:
                    raise ValueError(GUARD_BANS)
        torch.cuda.set_device(self.dev)  # a generator cannot hold a device guard across yields: pin the device for the caller
        self._pipeline_streams(stream_priorities)
        t3_kw = {k: kw[k] for k in ("max_new_tokens", "temperature", "top_p", "min_p", "repetition_penalty", "cfg_weight", "ban_eos",
                                    "ban_from") if k in kw}
        job_kw = lambda job: dict(t3_kw, **{k: job[k] for k in ("temperature", "top_p", "min_p", "repetition_penalty", "cfg_weight", "guard") if k in job})
        self.co_resident(bool(co_resident))
        # the CFM solve as two half-batch chains (FlowEngine.two_chain_schedule): measured in this form of the schedule only -- 320.3 -> 313.4 ms per batch,
        # three alternating pairs (profiles/r09_cfm_two_chains_headline_ab.jsonl); alone the flow loses 2 % with it, so every other caller keeps one chain
        self.flow.two_chain_schedule = bool(co_resident) and bool(host_threads)
        # ... and the flow + vocoder stream carries the co-resident ATTRIBUTE: its LayerNorm / split-GEMM launches (encoder, vocoder) keep to one or two
        # workgroups per CU as well (cbx_set_stream_coresident; no effect on results)
        from ._lib import check, lib
        # (with TWO T3 batches in flight the flow stream is the critical one and T3 has slack: capping its short LayerNorm launches costs more than the
        # decode chains gain -- 217.2x with the attribute, 220.8x without, same box; it stays on for t3_in_flight = 1)
        attr = bool(co_resident) and t3_in_flight < 2
        check(lib.cbx_set_stream_coresident(self._s_voc.cuda_stream, int(attr)), "cbx_set_stream_coresident")
        torch.cuda.synchronize()

        def enqueue_t3(job, box):
            try:
                torch.cuda.set_device(self.dev)
                with torch.inference_mode(), torch.cuda.stream(self._s_t3):
                    box["handle"] = self.t3.generate(job["t3_conds"], job["text_tokens"], async_mode=True, uniforms=job.get("uniforms"), seeds=job.get("seeds"), **job_kw(job))
            except BaseException as e:  # re-raised by the consumer thread
                box["error"] = e

        def vocode_job(job, st):
            """flow + vocoder of a job on the CURRENT stream, not synchronised -> its device waveforms, or its joined piece on the device (a job without a join: vocode
            is called exactly as before there was one)"""
            wavs, _ = self.vocode(st, job["gen_ref"], z=job.get("z"), phase=job.get("phase"), noise=job.get("noise"), generator=job.get("generator"), seeds=job.get("seeds"),
                                  speed=job.get("speed"), n_cfm_timesteps=kw.get("n_cfm_timesteps", 10), drop_last_token=kw.get("drop_last_token", True), sync=False,
                                  **({k: job[k] for k in ("join", "format", "loudness", "pauses", "pitch", "warp", "true_peak") if k in job}))
            if "warp" in job:
                job["_fit"] = self.last_fit  # (the job's own dict, _checked_job's copy: the report travels with it to the yield)
            return wavs

        def to_host(job, wavs, pinned):
            """The D2H copies of a job's audio on the CURRENT stream.  pinned=False: blocking copies, which return when the audio is on the host.  pinned=True: copies
            into pinned buffers that are only enqueued -- read them behind an event.  A joined piece is ONE copy plus one of its small record (-> the arguments of
            ops.piece_on_host), any other job one copy per utterance."""
            copy = (lambda w: torch.empty(w.shape, dtype=w.dtype, pin_memory=True).copy_(w, non_blocking=True)) if pinned else (lambda w: w.cpu())
            if "join" in job:
                return copy(wavs.get("formatted", wavs["out"])), copy(wavs["rec"]), wavs["n"], job.get("format"), copy(wavs["pauses"]) if "pauses" in job else None
            if "pauses" in job:  # (the rows are still n long; the record that cuts them travels the same way)
                return [copy(w) for w in wavs["rows"]], copy(wavs["pauses"]), wavs["format"]
            return [copy(w) for w in wavs]

        def result_of(job, host, toks):
            """What a job yields as `wavs` once `host` is readable: the waveforms, or the joined piece as its record lays it out, which also says which chunks spent
            T3's budget without EOS"""
            if "join" in job:
                return _joined_on_host(*host, self._truncated(toks))
            return ops.cut_pauses(*host) if "pauses" in job else host

        if not host_threads:  # round 4's form: one host thread enqueues T3(k + 1), then flow + vocoder(k)
            try:
                pending = None  # (job, speech tokens, t_start)
                for k in range(len(jobs) + 1):
                    box = {}
                    if k < len(jobs):
                        t_start = time.perf_counter()
                        enqueue_t3(jobs[k], box)
                        if "error" in box:
                            raise box["error"]
                    if pending is not None:
                        job, st, t0, raw, rep = pending
                        with torch.cuda.stream(self._s_voc):  # (the copies block: this returns when the batch's audio is on the host)
                            host = _range_checked(self, lambda: to_host(job, vocode_job(job, st), pinned=False))
                        self.last_guard, self.last_fit = rep, job.get("_fit")
                        yield result_of(job, host, raw), st, time.perf_counter() - t0
                    pending = None
                    if "handle" in box:
                        with torch.cuda.stream(self._s_t3):
                            raw = self.t3.collect(box["handle"])
                        pending = (jobs[k], _valid_tokens(raw), t_start, raw, self.t3.last_guard if "guard" in jobs[k] else None)
            finally:
                torch.cuda.synchronize()
                self.co_resident(False)
                self.flow.two_chain_schedule = False
            return

        # ---- two host threads, two T3 states: the worker enqueues T3(k) into state k % 2 as soon as batch k - 2's tokens were collected, so the T3 stream
        #      runs T3(0), T3(1), ... back to back (the Python prologue of a generate() call -- conditioning, embeddings, ~10 ms -- and the per-batch host
        #      round trip are off its critical path); this thread waits for T3(k)'s END EVENT on the vocoder stream, fetches its tokens there (a copy on the
        #      T3 stream would queue behind T3(k + 1)) and enqueues flow + vocoder(k) beside T3(k + 1).
        import queue
        n_t3 = max(1, min(3, int(t3_in_flight)))
        q, stop = queue.Queue(), threading.Event()
        n_slots = max(2, n_t3)
        slot_free = [threading.Semaphore(1) for _ in range(n_slots)]
        if t3_pair is None:
            t3_pair = bool(self.t3_pair) and os.environ.get("CBX_T3_PAIR", "1") != "0"
        # units of T3 work: [k] (a job alone: generate() exactly as before) or [2p, 2p + 1] (one paired call)
        units, k = [], 0
        while k < len(jobs):
            pair = None
            if t3_pair and k % 2 == 0 and k + 1 < len(jobs):
                pair = _paired_t3_call(jobs[k], jobs[k + 1], job_kw(jobs[k]), job_kw(jobs[k + 1]), int(kw.get("max_new_tokens", 1000)))
            units.append(([k, k + 1], pair) if pair is not None else ([k], None))
            k += len(units[-1][0])
        # (paired calls keep the t3_in_flight chains: measured on one MI355X, headline command, two 32-row chains 249.8 audio-s/wall-s against 231.2 for the
        # unpaired schedule and 233.8 for ONE 32-row chain beside the flow with the co-resident stream attribute on -- profiles/r07_pair_schedule_ab.jsonl)

        def worker():
            try:
                torch.cuda.set_device(self.dev)
                for u, (ks, pair) in enumerate(units):
                    slot_free[u % n_slots].acquire()
                    if stop.is_set():
                        return
                    t_start = time.perf_counter()
                    job = jobs[ks[0]]
                    with torch.inference_mode(), torch.cuda.stream(self._s_t3x[u % n_t3]):
                        if pair is None:
                            h = self.t3.generate(job["t3_conds"], job["text_tokens"], async_mode=True, uniforms=job.get("uniforms"), seeds=job.get("seeds"), slot=u % n_slots, **job_kw(job))
                        else:
                            pkw = dict(pair)
                            h = self.t3.generate(pkw.pop("conds"), pkw.pop("text_tokens"), async_mode=True, slot=u % n_slots, two_tile=True, **pkw)
                        ev = torch.cuda.Event()
                        ev.record()
                    q.put((h, ev, t_start))
            except BaseException as e:  # re-raised by the consumer thread
                q.put(e)

        # (the vocoder of batch k on a stream of its own was measured WORSE -- 208.9x against 226.3x, same box, profiles/r05_throughput_schedule_sweep.log: a
        # fourth stream of chip-filling work thrashes like a third decode chain does -- and is gone.)  Consecutive batches report fp16-range trips into
        # alternating flag words (ops.select_range_flag: a launch carries the word that was registered when it was ENQUEUED).
        import collections
        inflight = collections.deque()

        def start_voc(job, st, which):
            ops.select_range_flag(self.dev, which)
            with torch.cuda.stream(self._s_voc):
                host = to_host(job, vocode_job(job, st), pinned=True)  # read in finish(), behind the event
                ev = torch.cuda.Event()
                ev.record()
            return host, ev

        def finish(job, st, t0, host, ev, which, raw, rep):
            self.last_guard = rep  # (the guard's report of THIS job, taken when its tokens were collected)
            ev.synchronize()
            if 16 in (self.flow.precision, self.hift.precision) and ops.range_flag_tripped(self.dev, which):
                with _repeat_at_bf16x6(self, " of this batch"), torch.cuda.stream(self._s_voc):
                    host = to_host(job, vocode_job(job, st), pinned=False)  # (the repeat repeats the join)
            self.last_fit = job.get("_fit")  # (the fit report of THIS job: the vocoder of the next one may have been enqueued since)
            return result_of(job, host, raw), st, time.perf_counter() - t0

        th = threading.Thread(target=worker, name="cbx-t3-enqueue", daemon=True)
        th.start()
        try:
            for u, (ks, pair) in enumerate(units):
                item = q.get()
                if isinstance(item, BaseException):
                    raise item
                h, ev, t0 = item
                with torch.cuda.stream(self._s_voc):
                    self._s_voc.wait_event(ev)
                    toks_u = self.t3.collect(h)  # blocks this thread until this unit's T3 is done; the next unit's is already enqueued behind it
                    rep = self.t3.last_guard if "guard" in jobs[ks[0]] else None  # (a guarded job is never paired)
                slot_free[u % n_slots].release()
                lo = 0
                for k in ks:  # the pair's tokens go back to their jobs, in order
                    job = jobs[k]
                    toks = toks_u[lo:lo + len(job["text_tokens"])]
                    lo += len(job["text_tokens"])
                    st = _valid_tokens(toks)
                    host, evv = start_voc(job, st, k % 2)
                    inflight.append((job, st, t0, host, evv, k % 2, toks, rep))
                    yield finish(*inflight.popleft())
            while inflight:
                yield finish(*inflight.popleft())
        finally:
            stop.set()
            for sem in slot_free:
                sem.release()
            th.join()
            ops.select_range_flag(self.dev, 0)
            torch.cuda.synchronize()
            self.co_resident(False)  # callers of vocode() / flow.inference() / synthesize_stream() get the fastest-alone forms back
            self.flow.two_chain_schedule = False

    @torch.inference_mode()
    def synthesize_stream(self, text_tokens, t3_conds, gen_ref, *, first_chunk=25, chunk=50, chunk_growth=1.0, lookahead=3, fade=480, max_new_tokens=1000,
                          temperature=0.8, top_p=1.0, min_p=0.05, repetition_penalty=1.2, cfg_weight=0.5, uniforms=None, ban_eos=False,
                          ban_from=0, z=None, phase=None, noise=None, n_cfm_timesteps=10, drop_last_token=True, overlap=True, first_alone=True, run_ahead=2,
                          window=None, seeds=None, speed=None, format=None):
        """Chunked synthesis: first audio after `first_chunk` tokens instead of after the whole utterance.

        The reference is non-streaming; of its vestigial hooks only HiFT's `cache_source` works (hifigan.py:470-472) -- `finalize=False`
        (flow.py:170-171) raises a shape error there -- so the schedule is this build's own, with its own oracle
        (tests/test_stream_gpu.py restates it on the CPU oracle):
          * round r works on the first n_r tokens, n_0 = first_chunk + lookahead, n_r = n_{r-1} + chunk * chunk_growth^(r-1) (stream_token_schedule);
          * every round runs encoder + CFM over the tokens so far with the same noise realisation, masking the last 2 * lookahead mel frames of
            unfinished utterances (the encoder looks 3 tokens ahead), and HiFT with the previous round's source as `cache_source`
            (phase-continuous excitation);
          * new samples are emitted up to `fade` samples before the end of what the round could vocode; that tail is cross-faded (linear ramp)
            with the next round's re-synthesis of the same samples.
        The last round is a full synthesis: identical mel to synthesize() for the same noise.
        overlap (round 6, the default): the two stages of the SAME utterances run side by side -- a second host thread keeps the T3 decode going on
        its own high-priority stream (at most two rounds ahead of the vocoder; graph replays of the captured step), this thread waits for a round's
        tokens on the flow stream and runs that round's flow + vocoder there, both stages on their co-resident kernel forms (synthesize_pipelined).
        A round still sees exactly its n_r tokens, so every yielded sample is the one the serial form (overlap=False) yields.
        window (None: the schedule above): the left context, in tokens, of a round of BOUNDED cost -- a round then synthesises the voice prompt, `window`
        tokens in front of the first sample it has not emitted yet, the new chunk and the lookahead, whatever the round's number (_stream_rounds,
        stream_window_schedule); at least ceil((8000 + fade) / 960) tokens, else ValueError.  The last round is then no longer the full synthesis.
        seeds (None, an int, or B ints in [0, 2^64)): every draw that is not injected comes from its utterance's seed (synthesize(seeds=)); with a window, z and
        noise are then filled round by round and never for the whole budget (_stream_rounds).
        speed (None, or ONE number in [0.5, 2.0] for all utterances; None / 1.0: exactly the stream without it): the speaking rate of synthesize(speed=).  Every round
        stretches its mel (the window's, with a window) by one ops.mel_time_scale_window launch in front of the vocoder, and samples are counted in the stretched
        signal (_stream_rounds): utterance b's pieces add up to the length synthesize(speed=) returns, and with window=None the last round vocodes the very mel the
        one-shot call stretches.  An injected `noise` covers 480 * ops.scaled_len(2 n, speed) samples; a window must satisfy check_stream_window(window, fade, speed).
        format (None or the default: exactly the stream without it; else vocode(format=)'s dict): ONE ops.WaveFormatStream lives for the whole stream and every
        round's new samples of all open rows go through one push (one cbx_wave_format_f32 launch) ahead of the round's copy to the host, which then carries the
        encoded pieces; utterance b's pieces add up to ops.formatted_len of what the stream without it emits, and are bit for bit ops.wave_format of that.
        Yields dicts {wavs: [B CPU tensors of NEW samples], final: [B bools], n_tokens: [B], tokens: [B CPU tensors: the speech tokens the round vocoded]};
        concatenating an utterance's pieces gives its waveform."""
        t3_kw = dict(max_new_tokens=max_new_tokens, temperature=temperature, top_p=top_p, min_p=min_p, repetition_penalty=repetition_penalty,
                     cfg_weight=cfg_weight, uniforms=uniforms, ban_eos=ban_eos, ban_from=ban_from)

        yield from _synthesize_stream(self, text_tokens, t3_conds, gen_ref, n_budget=max_new_tokens, t3_kw=t3_kw, round_tokens=lambda toks, fin: _valid_tokens(toks), n_extra=0,
                                      first_chunk=first_chunk, chunk=chunk, chunk_growth=chunk_growth, lookahead=lookahead, fade=fade, z=z, phase=phase,
                                      noise=noise, n_cfm_timesteps=n_cfm_timesteps, drop_last_token=drop_last_token, overlap=overlap, first_alone=first_alone,
                                      run_ahead=run_ahead, window=window, seeds=seeds, speed=speed, format=format)


_T3_SAMPLING_DEFAULTS = dict(temperature=0.8, top_p=1.0, min_p=0.05, repetition_penalty=1.2, cfg_weight=0.5)  # T3Engine.generate's


def _paired_t3_call(job_a, job_b, kw_a, kw_b, max_new_tokens):
    """The keyword arguments of ONE T3Engine.generate call that decodes two jobs of synthesize_pipelined(t3_pair=True) -- utterances of job_a first --, or None when
    the two cannot share a call: more than 32 rows, a guard, or draws that one call cannot express (uniforms in one job only; seeds in one job only).  kw_a / kw_b:
    each job's own T3 keywords (the call's, overridden by the job's).  Everything that differs between the jobs travels per utterance."""
    na, nb = len(job_a["text_tokens"]), len(job_b["text_tokens"])
    if 2 * (na + nb) > 32 or "guard" in kw_a or "guard" in kw_b:
        return None
    ua, ub = job_a.get("uniforms"), job_b.get("uniforms")
    sa, sb = job_a.get("seeds"), job_b.get("seeds")
    if (ua is None) != (ub is None) or (ua is None and (sa is None) != (sb is None)):
        return None
    out = {k: v for k, v in kw_a.items() if k not in _T3_SAMPLING_DEFAULTS}
    if out != {k: v for k, v in kw_b.items() if k not in _T3_SAMPLING_DEFAULTS}:
        return None
    per_utt = lambda v, n: [float(x) for x in v] if isinstance(v, (list, tuple)) or torch.is_tensor(v) else [float(v)] * n
    for key, default in _T3_SAMPLING_DEFAULTS.items():
        if key in kw_a or key in kw_b:
            va, vb = per_utt(kw_a.get(key, default), na), per_utt(kw_b.get(key, default), nb)
            if len(va) != na or len(vb) != nb:
                return None  # (a wrong length: let the job's own call raise as it always did)
            out[key] = va + vb
    conds = lambda job, n: list(job["t3_conds"]) if isinstance(job["t3_conds"], (list, tuple)) else [job["t3_conds"]] * n
    out["conds"], out["text_tokens"] = conds(job_a, na) + conds(job_b, nb), list(job_a["text_tokens"]) + list(job_b["text_tokens"])
    if ua is not None:
        rows = lambda u, n: torch.as_tensor(u, dtype=torch.float32).reshape(n, -1)
        ua, ub = rows(ua, na), rows(ub, nb)
        if min(ua.shape[1], ub.shape[1]) < max_new_tokens:
            return None
        out["uniforms"] = torch.cat([ua[:, :max_new_tokens], ub[:, :max_new_tokens].to(ua.device)])
    elif sa is not None:
        ints = lambda v, n: [int(x) for x in v] if isinstance(v, (list, tuple)) or torch.is_tensor(v) else [int(v)] * n
        out["seeds"] = ints(sa, na) + ints(sb, nb)
    return out


def _stream_plan(n_tokens, done, exhausted, lookahead):
    """Per utterance: (final?, mel frames to hold back).  An utterance is final once its EOS was sampled or the step budget is spent;
    until then the encoder's `lookahead` tokens (2 mel frames each) are not vocoded yet."""
    fin = [bool(d) or exhausted for d in done]
    return fin, [0 if f else 2 * lookahead for f in fin]


def stream_token_schedule(n_tokens, first_chunk=25, chunk=50, lookahead=3, chunk_growth=1.0):
    """Tokens available to round 0, 1, 2, ... of synthesize_stream for an utterance of `n_tokens` sampled tokens: first_chunk + lookahead,
    then `chunk` more per round, each chunk `chunk_growth` times the previous one (1.0: constant chunks -- every round re-runs encoder + CFM
    over all tokens so far, so the total work grows with the number of rounds; a growth of 2 keeps the first-audio latency and bounds the
    total at about twice the one-shot synthesis)."""
    out, n, c = [], min(n_tokens, first_chunk + lookahead), float(chunk)
    while True:
        out.append(n)
        if n >= n_tokens:
            return out
        n = min(n_tokens, n + max(1, int(round(c))))
        c *= chunk_growth


STREAM_RECEPTIVE_FIELD = 8000  # samples of context the vocoder needs on the left of a sample (measured on the oracle: tests/test_stream_gpu.py)


def check_stream_speed(speed):
    """The speaking rate of a stream: None (also for 1.0: the stream is then exactly the one without the argument) or ONE float in [0.5, 2.0] for all its
    utterances (ops.check_speed).  A sequence is a TypeError: the rows of a stream share the window origin, so they share the rate."""
    if speed is None:
        return None
    if isinstance(speed, (list, tuple)):
        raise TypeError(f"speed: a stream takes one number for all its utterances, got a {type(speed).__name__}")
    v = ops.check_speed(speed, 1)
    return None if v is None else v[0]


def check_stream_window(window, fade, speed=None):
    """window=None (every round re-synthesises everything so far) or a left context in TOKENS that covers the vocoder's receptive field and the cross-fade:
    at least ceil((8000 + fade) / 960).  Anything else is a ValueError, raised before a launch.
    speed (None, or a rate != 1 in [0.5, 2.0]): the stream is stretched, and the context the vocoder sees is counted in STRETCHED frames.  With F =
    ceil((8000 + fade) / 480) frames, je = E // 480 the first frame not yet emitted whole, c = max(0, s - 1), ie = floor(x_je + c), a = ie // 2 - W and j0 the
    first frame with x_j0 >= 2a + 0.25 (stream_window_origin, stream_origin_frame; x_j = (j + 0.5) s - 0.5):
        je = (x_je + 0.5) / s - 0.5
        x_(j0 - 1) < 2a + 0.25   =>  j0 < (2a + 0.75) / s + 0.5
        2a <= x_je + c - 2W      =>  je - j0 > (2W - c - 0.25) / s - 1
    so 2W >= F s + c + 0.25 gives je - j0 > F - 1, i.e. 480 (je - j0) >= 8000 + fade, the invariant a round asserts whenever a > 0.  The bound asked for is
    ceil((F s + c + 0.5) / 2) -- 0.5 in place of 0.25 keeps the roundings of x_j in Python floats away from the edge -- and never less than the bound without a
    rate, so the flow sees no less context than an unscaled stream gives it."""
    if window is None:
        return None
    need = -(-(STREAM_RECEPTIVE_FIELD + int(fade)) // SAMPLES_PER_TOKEN)
    why = ""
    if speed is not None:
        F = -(-(STREAM_RECEPTIVE_FIELD + int(fade)) // (SAMPLES_PER_TOKEN // 2))
        need, why = max(need, int(math.ceil((F * float(speed) + max(0.0, float(speed) - 1.0) + 0.5) / 2.0))), f" at speed={speed}"
    if isinstance(window, bool) or not isinstance(window, int) or window < need:
        raise ValueError(f"window={window!r}: expected None or an int >= {need} tokens (the vocoder's receptive field of {STREAM_RECEPTIVE_FIELD} samples + fade={fade}{why})")
    return window


def stream_window_schedule(n_tokens, first_chunk=25, chunk=50, lookahead=3, chunk_growth=1.0, window=None, fade=480):
    """[(a_r, n_r), ...]: round r of a stream of an utterance of `n_tokens` tokens synthesises tokens [a_r, n_r).  n_r is stream_token_schedule's; with
    window=None every a_r is 0 (the work of a round grows with r), with window=W tokens a_r = max(0, E_r // 960 - W), E_r = the samples emitted before round r
    (all but the last `fade` of what round r - 1 could vocode): once the window slides a round is W + chunk + lookahead + 1 tokens long whatever r is
    (fade <= 960).  Pure host arithmetic: the engine computes the same a_r from what it has emitted.  (A stream at a speaking rate: stream_speed_schedule.)"""
    window = check_stream_window(window, fade)
    out, emitted = [], 0
    for n in stream_token_schedule(n_tokens, first_chunk, chunk, lookahead, chunk_growth):
        out.append((0 if window is None else max(0, emitted // SAMPLES_PER_TOKEN - window), n))
        final = n >= n_tokens
        avail = (SAMPLES_PER_TOKEN // 2) * (2 * n - (0 if final else 2 * lookahead))
        emitted = avail if final else max(emitted, avail - fade)
    return out


# ---- a stream at a speaking rate s: everything upstream of the stretch (tokens, flow, z, hold_back, the window origin a) stays in unscaled units; everything
# downstream (the vocoder's lens, noise columns, cache_source, the phase carry, emitted / end / avail, the tails, the emission's origin) is in absolute frames or
# samples of the STRETCHED signal.  Stretched frame j is cbx_mel_time_scale_f32's function of (j, s) alone.  Host and device evaluate x_j differently (two
# roundings here, one fused multiply-add there) and can disagree on floor(x_j) only when x_j is within an ulp of an integer:
#   * on the LEFT of a window the origin is chosen with a quarter frame of margin (stream_origin_frame), so the device never needs a tap left of it;
#   * on the RIGHT the disagreement is benign: there l is ~0 or ~1 and both readings blend to in[n] to within rounding (a frame the host calls ready while the
#     device's floor is one higher reads the last frame twice, clamped; the other way round the frame is just emitted one round later).
# Memory safety depends on neither: the kernel clamps every tap into the window (cbx_mel_time_scale_win_f32).
def stretch_position(j, s):
    """x_j = max(0, (j + 0.5) s - 0.5): where stretched frame j samples the unscaled mel"""
    return max(0.0, (j + 0.5) * s - 0.5)


def _first_frame_at(x0, s):
    """the smallest j >= 0 with x_j >= x0"""
    j = max(0, int(math.ceil((x0 + 0.5) / s - 0.5)))
    while j > 0 and stretch_position(j - 1, s) >= x0:
        j -= 1
    while stretch_position(j, s) < x0:
        j += 1
    return j


def stream_ready_frames(M_abs, s):
    """Stretched frames [0, R) a NON-FINAL round may vocode when unscaled frames [0, M_abs) exist: both taps of frame j exist, floor(x_j) + 1 <= M_abs - 1, i.e.
    x_j < M_abs - 1.  A frame that would clamp its right tap to the current end is not ready: it changes once more tokens arrive."""
    return 0 if M_abs < 2 else _first_frame_at(float(M_abs - 1), s)


def stream_round_frames(M_abs, s, final):
    """Stretched frames [0, R) that exist after a round over unscaled frames [0, M_abs): the ready ones, or all ops.scaled_len(M_abs, s) of a final round (whose
    last taps clamp to the end, as vocode(speed=) does)."""
    return ops.scaled_len(M_abs, s) if final else stream_ready_frames(M_abs, s)


def stream_origin_frame(a, s):
    """j0: the first stretched frame all of whose taps lie at or right of unscaled frame 2a, with a margin (x_j0 >= 2a + 0.25) that host / device rounding cannot
    cross; 0 when a == 0.  A windowed round's waveform starts at absolute stretched sample 480 j0."""
    return 0 if a == 0 else _first_frame_at(2 * a + 0.25, s)


def stream_window_origin(E, W, s):
    """The window origin a (tokens) of a round that has emitted E stretched samples: je = E // 480 is the first frame not emitted whole, ie = floor(x_je) its
    left tap, a = max(0, ie // 2 - W).  At s = 1 this is E // 960 - W.
    For s > 1 the position is advanced by c = s - 1 first, ie = floor(x_je + c): a stretched frame then steps over MORE than one unscaled frame, the emitted count
    trails what the last round held (M_abs = 2m frames: x_je >= 2m - 1 - s, fade <= 480) by up to 1 + s of them, and with ie = floor(x_je) a round at 1 < s < 2
    would at times be W + chunk + lookahead + 2 tokens long; with c, x_je + c >= 2m - 2, so ie // 2 >= m - 1 and a round is at most W + chunk + lookahead + 1 tokens
    at every rate, as without one (check_stream_window accounts for c).  1e-9 keeps a product that is an integer in exact arithmetic from rounding below it."""
    x = stretch_position(E // (SAMPLES_PER_TOKEN // 2), s) + max(0.0, s - 1.0)
    return max(0, int(math.floor(x + 1e-9)) // 2 - W)


def stream_speed_schedule(n_tokens, speed=None, first_chunk=25, chunk=50, lookahead=3, chunk_growth=1.0, window=None, fade=480, drop_last_token=False):
    """[(a_r, n_r, j0_r, E_r), ...] of a stream at speaking rate `speed`: round r synthesises tokens [a_r, n_r), its waveform starts at absolute stretched sample
    480 j0_r, and E_r stretched samples are emitted once it is done -- the arithmetic _stream_rounds runs, for one utterance that ends with its n_tokens-th token.
    speed None / 1.0: (a_r, n_r) are stream_window_schedule's, j0_r = 2 a_r.  The last E_r is 480 * ops.scaled_len(2 * keep, speed), what vocode(speed=) returns."""
    s = check_stream_speed(speed)
    W = check_stream_window(window, fade, s)
    HALF = SAMPLES_PER_TOKEN // 2
    out, emitted = [], 0
    for n in stream_token_schedule(n_tokens, first_chunk, chunk, lookahead, chunk_growth):
        final = n >= n_tokens
        M_abs = 2 * n - (0 if final else 2 * lookahead)
        keep = max(1, n - 1) if drop_last_token else n
        if s is None:
            a = 0 if W is None else max(0, emitted // SAMPLES_PER_TOKEN - W)
            j0, avail = 2 * a, HALF * (min(M_abs, 2 * keep) if final else M_abs)
        else:
            a = 0 if W is None else stream_window_origin(emitted, W, s)
            j0 = stream_origin_frame(a, s)
            avail = HALF * max(j0, stream_round_frames(M_abs, s, final))
            if final:
                avail = min(avail, HALF * ops.scaled_len(2 * keep, s))
        emitted = avail if final else max(emitted, avail - fade)
        out.append((a, n, j0, emitted))
    return out


def _stream_rounds(self, B, gen_ref, *, n_tokens, round_tokens, lookahead, fade, z, phase, noise, n_cfm_timesteps, drop_last_token, window, seeds=None, speed=None, format=None):
    """The state of one stream of B utterances and its round function: -> (one_round, closed flags).  one_round(toks, done, exhausted) runs flow + vocoder
    on the CURRENT stream and returns the dict the stream generators yield.  n_tokens: the most tokens an utterance can have (the default z / noise cover them).

    window=None: a round synthesises every token so far.  window=W (tokens; check_stream_window): a round synthesises the voice prompt and tokens [a, n) only,
    a = max(0, E // 960 - W) with E the samples already emitted (of the utterances still open) -- W tokens of left context in front of the first new sample:
      * the CFM noise of absolute frame t is z[:, 2P + t] in every round, the source noise of absolute sample q is noise[:, :, q];
      * the vocoder's excitation stays phase-continuous although the window does not start at sample 0: the source's phase scan starts from the previous
        round's cumulative cycles at the frame the window now begins (HiFTEngine.inference(cum_in=), cbx_hift_f0_source_carry), and the previous round's source
        from that sample on is the `cache_source`;
      * S3Gen's trim_fade belongs to sample 0: applied while a == 0 only;
      * emitted / end / avail stay ABSOLUTE samples of the utterance; the round's waveform starts at sample 960 a.  The emission (new samples, cross-fade
        with the kept tail, next tail) is one cbx_stream_emit_f32 launch and one D2H copy for all utterances.
    The cache keeps the source of the rows that go on (the window=None form keeps the shortest row's, finished rows included); with every a == 0 and no row
    finishing before the others the two forms yield the same bits.
    seeds (B ints or None): the z / phase / noise that is not injected comes from each utterance's seed (ops.seeded_*).  window=None: filled once, at the sizes of
    the unseeded defaults.  window=W: z and noise are NOT materialised for the whole budget -- a round fills the columns it reads (z frames [0, 2P) and
    [2(P + a), 2(P + a + Nk)), noise samples [o, o + 480 frames)), which are those of the full fill by construction (cbx_rng_fill_f32's col0).
    speed (None / 1.0: every launch and every bit of the stream without it; else ONE rate s for all rows, check_stream_speed): the flow runs as ever on tokens
    [a, n) and ONE ops.mel_time_scale_window launch per round stretches its mel -- absolute stretched frames [j0, R_b) from the window's unscaled frames
    [2a, 2a + frames_b), R_b = stream_round_frames (the ready frames of a row that goes on, all ops.scaled_len(2 n_b, s) of a final one), j0 =
    stream_origin_frame(a, s) (window=None: a = j0 = 0, the whole mel so far).  From there on every quantity is in frames / samples of the STRETCHED signal: the
    vocoder's lens, the noise columns [480 j0, ...), the cache and the phase carry (offset j0 - j0 of the last round), emitted / end / avail, the tails and the
    emission's origin 480 j0; a = stream_window_origin(E, W, s).  trim_fade while j0 == 0.  A final row's avail is 480 * ops.scaled_len(min(2 keep, 2 n), s),
    what vocode(speed=) returns.  Default noise is sized 480 * ops.scaled_len(2 n_tokens, s); an injected one must cover the stretched utterance; z is the
    flow's and does not change.
    format (None or the default: every launch of the stream without it; else ops.check_format's dict): the stream's ops.WaveFormatStream -- a round's new samples
    (after the cross-fade) of all rows go through ONE push, and the round's single copy to the host takes the packed, encoded buffer."""
    dev = self.dev
    fmt = ops.check_format_arg(format)
    wfs = None if fmt is None else ops.WaveFormatStream(B, fmt, dev)
    rate = check_stream_speed(speed)
    W = check_stream_window(window, fade, rate)
    P = gen_ref["prompt_token"].shape[-1]
    N = n_tokens
    HALF = SAMPLES_PER_TOKEN // 2  # samples per mel frame
    n_noise = SAMPLES_PER_TOKEN * N if rate is None else HALF * ops.scaled_len(2 * N, rate)  # samples of the longest (stretched) utterance
    assert gen_ref["prompt_feat"].shape[-2] == 2 * P, "chunked synthesis needs a whole-token prompt (embed_ref output trimmed to 2 frames per token)"
    per_round = seeds is not None and W is not None  # seeded and windowed: z / noise that is not injected is filled round by round (z_frames, noise_samples)
    if seeds is not None:
        if phase is None:
            phase = ops.seeded_phase(seeds, dev)
        if not per_round:
            z = ops.seeded_z(seeds, 2 * (P + N), dev) if z is None else z
            noise = ops.seeded_noise(seeds, n_noise, dev) if noise is None else noise
    else:
        if z is None:
            z = torch.randn(B, 2 * (P + N), 80, device=dev)
        if phase is None:
            phase = (torch.rand(B, 9, device=dev) * 2 - 1) * 3.141592653589793
            phase[:, 0] = 0
        if noise is None:
            noise = torch.randn(B, 9, n_noise, device=dev)
    z, phase, noise = None if z is None else z.to(dev), phase.to(dev).reshape(B, 9), None if noise is None else noise.to(dev)

    def z_frames(a, Nk):
        """CFM noise of the prompt's frames and of tokens [a, a + Nk): (B, 2 (P + Nk), 80)"""
        if z is not None:
            return z[:, : 2 * (P + Nk)] if a == 0 else torch.cat([z[:, : 2 * P], z[:, 2 * (P + a): 2 * (P + a + Nk)]], 1)
        if a == 0:
            return ops.seeded_z(seeds, 2 * (P + Nk), dev)
        return torch.cat([ops.seeded_z(seeds, 2 * P, dev), ops.seeded_z(seeds, 2 * Nk, dev, frame0=2 * (P + a))], 1)

    def noise_samples(o, n):
        """source noise of absolute samples [o, o + n): (B, 9, n)"""
        assert rate is None or noise is None or noise.shape[2] >= o + n, f"noise: {noise.shape[2]} samples, the stretched stream reads up to {o + n} (480 * ops.scaled_len(2 N, speed))"
        return noise[:, :, o: o + n] if noise is not None else ops.seeded_noise(seeds, n, dev, col0=o)

    emitted, tails, closed, cache = [0] * B, [None] * B, [False] * B, [None]
    ramp = torch.linspace(0.0, 1.0, fade + 2, device=dev)[1:-1]
    win = dict(a=0, j0=0, cum=None, tail_len=[0] * B, bufs=None, cur=0)  # window form: origin (tokens; vocoder frames) and phase scan of the last round, the kept tails (device, ping-pong)

    def one_round(toks, done, exhausted):
        """flow + vocoder over the tokens so far (window form: over the window) on the CURRENT stream -> the dict this generator yields"""
        fin, hold = _stream_plan([t.numel() for t in toks], done, exhausted, lookahead)
        st = round_tokens(toks, fin)
        ns = [int(t.numel()) for t in st]
        a, j0, cum_in, cache_src = 0, 0, None, cache[0]  # j0: the vocoder frame (480 samples) the round's waveform starts at
        if W is not None:
            live = [emitted[b] for b in range(B) if not closed[b]]
            if rate is None:
                a = max(0, min(live) // SAMPLES_PER_TOKEN - W) if live else win["a"]
                j0 = 2 * a
            else:
                a = stream_window_origin(min(live), W, rate) if live else win["a"]
                j0 = stream_origin_frame(a, rate)
                assert a == 0 or not live or HALF * (min(live) // HALF - j0) >= STREAM_RECEPTIVE_FIELD + fade, "the window is shorter than the vocoder's receptive field + fade"
            assert all(closed[b] or ns[b] > a for b in range(B)), "an open utterance ends left of the window"
            if win["cum"] is not None:  # continue the previous round's excitation from where this window begins
                d = j0 - win["j0"]
                assert 0 <= d < win["cum"].shape[2]
                cum_in = win["cum"][:, :, d].contiguous()
                cache_src = cache[0][:, HALF * d:] if cache[0] is not None and cache[0].shape[1] > HALF * d else None
        ws = st if a == 0 else [t[a:] if t.numel() > a else t.new_zeros(1) for t in st]  # (a finished utterance left of the window: one dummy token)
        wn = [int(t.numel()) for t in ws]
        Nk = max(wn)
        frames = [max(0, 2 * n - hb) for n, hb in zip(wn, hold)]
        mel_frames = frames  # the flow's frames of the window, unscaled
        if rate is not None:  # vocoder frames of the window: absolute stretched frames [j0, R_b); a row that finished earlier only rides along
            frames = [max(0, stream_round_frames(2 * a + f, rate, fin[b]) - j0) if f > 0 else 0 for b, f in enumerate(mel_frames)]
            cap = max([f for b, f in enumerate(frames) if not closed[b]], default=0)
            frames = [min(f, cap) if closed[b] else f for b, f in enumerate(frames)]
        out = [torch.zeros(0)] * B
        if max(frames) > 0:
            tok = torch.zeros(B, Nk, dtype=torch.long)
            for b, t in enumerate(ws):
                tok[b, : wn[b]] = t
            fl = torch.tensor(frames, dtype=torch.int32, device=dev) if rate is None else None
            o = HALF * j0  # absolute sample of wav[:, 0]

            def run():
                mel = self.flow.inference(tok.to(dev), torch.tensor(wn, dtype=torch.int32, device=dev), gen_ref, z=z_frames(a, Nk),
                                          n_steps=n_cfm_timesteps, hold_back=hold)
                lens = fl
                if rate is not None:  # the vocoder's input is the stretched window
                    mel, lens = ops.mel_time_scale_window(mel, rate, j0, 2 * a, mel_frames, frames)
                return self.hift.inference(mel, phase=phase, noise=noise_samples(o, HALF * mel.shape[1]), lens=lens, fade=j0 == 0,
                                           cache_source=cache_src, cum_in=cum_in)
            wav, src = _range_checked(self, run)

            def span(b):
                """(end, avail) of open row b, in absolute samples of its utterance: `avail` of them exist after this round (a final row: no more than the one-shot
                call returns), [emitted, end) leave now, and [end, avail) -- at most `fade` samples, none of a final row -- is the tail the next round cross-fades"""
                avail = o + HALF * frames[b]
                if fin[b]:
                    keep = max(1, ns[b] - 1) if drop_last_token else ns[b]
                    avail = min(avail, keep * SAMPLES_PER_TOKEN if rate is None else HALF * ops.scaled_len(2 * keep, rate))
                return (avail if fin[b] else max(emitted[b], avail - fade)), avail

            def formatted(rows):
                """one push of the round's new samples (views of one device tensor, None for a row that was closed before) -> the encoded pieces on the host"""
                wfs.push(rows, [fin[b] or rows[b] is None for b in range(B)])
                host = wfs.packed.cpu()
                return [host[s: s + c].clone() if c else out[b] for b, (s, c) in enumerate(wfs.spans)]

            if W is None:  # (o == 0: every round starts at sample 0)
                cache[0] = src[:, : HALF * min(frames)].clone() if min(frames) > 0 else None
                dnew = [None] * B
                for b in range(B):
                    if closed[b]:
                        continue
                    end, avail = span(b)
                    new = wav[b, emitted[b]: end].clone()
                    if tails[b] is not None and new.numel() > 0:
                        k = min(tails[b].numel(), new.numel())
                        new[:k] = tails[b][:k] * (1.0 - ramp[:k]) + new[:k] * ramp[:k]
                    tails[b] = None if fin[b] else wav[b, end: min(avail, end + fade)].clone()
                    emitted[b] = end
                    closed[b] = fin[b]
                    if wfs is None:
                        out[b] = new.cpu()
                    else:
                        dnew[b] = new
                if wfs is not None:  # the rows as views of one tensor
                    pack = torch.empty(B, max([0] + [w.numel() for w in dnew if w is not None]), device=dev)
                    for b, w in enumerate(dnew):
                        if w is not None:
                            pack[b, : w.numel()] = w
                    out = formatted([None if w is None else pack[b, : w.numel()] for b, w in enumerate(dnew)])
            else:
                go_on = [frames[b] for b in range(B) if not fin[b]]
                cache[0] = src[:, : HALF * min(go_on)].clone() if go_on and min(go_on) > 0 else None
                win.update(a=a, j0=j0, cum=self.hift.frame_cum)
                meta, news, nxt = torch.zeros(4, B, dtype=torch.int32), [0] * B, [0] * B
                was_closed = list(closed)
                for b in range(B):
                    if closed[b]:
                        meta[:3, b] = emitted[b]
                        continue
                    end, avail = span(b)
                    meta[:, b] = torch.tensor([emitted[b], end, avail, win["tail_len"][b]], dtype=torch.int32)
                    news[b], nxt[b] = max(0, end - emitted[b]), 0 if fin[b] else max(0, min(avail, end + fade) - end)
                    emitted[b] = end
                    closed[b] = fin[b]
                if fade and win["bufs"] is None:
                    win["bufs"] = [torch.zeros(B, fade, device=dev) for _ in range(2)]
                t_in, t_out = (win["bufs"][win["cur"]], win["bufs"][1 - win["cur"]]) if fade else (None, None)
                new = torch.empty(B, max(news), device=dev)
                ops.stream_emit(wav, o, meta.to(dev), t_in, ramp if fade else None, new, t_out)
                win.update(tail_len=nxt, cur=1 - win["cur"])
                if wfs is not None:
                    out = formatted([None if was_closed[b] else new[b, : news[b]] for b in range(B)])
                else:
                    host = new.cpu()
                    for b in range(B):
                        if news[b]:
                            out[b] = host[b, : news[b]].clone()
        return dict(wavs=out, final=list(fin), n_tokens=ns, tokens=st)

    return one_round, closed


def _synthesize_stream(self, text_tokens, t3_conds, gen_ref, *, n_budget, t3_kw, round_tokens, n_extra, first_chunk, chunk, chunk_growth, lookahead, fade, z,
                       phase, noise, n_cfm_timesteps, drop_last_token, overlap, first_alone, run_ahead, window=None, seeds=None, speed=None, format=None):
    """The round schedule of synthesize_stream for either backbone (ChatterboxEngine: Llama T3, TurboEngine: GPT-2 T3; both T3 engines offer the async
    generate / advance / peek protocol).  n_budget: tokens the T3 call can sample; t3_kw: its sampling arguments; round_tokens(toks, final flags) -> the
    valid speech tokens a round vocodes (never empty); n_extra: tokens round_tokens may add (the default z / noise cover n_budget + n_extra).
    window: None, or the left context in tokens of a bounded round (_stream_rounds).  seeds: None, an int or B ints -- the sampling draws (generate(seeds=))
    and the flow / vocoder noise (_stream_rounds) that are not injected.  speed: None or one rate for the stream (_stream_rounds(speed=)); T3 does not depend on it,
    so the serial and the overlapped schedule take it alike.  format: None or the stream's delivery format (_stream_rounds(format=))."""
    check_stream_window(window, fade, check_stream_speed(speed))
    seeds = ops.check_seeds(seeds, len(text_tokens))
    format = ops.check_format_arg(format)
    # (a generator cannot hold a device guard across yields: pin the device for the caller; "cuda" without an index = the current device)
    pin = self.dev if self.dev.index is not None else torch.device("cuda", torch.cuda.current_device())
    torch.cuda.set_device(pin)
    B, N = len(text_tokens), n_budget
    t3_kw = dict(t3_kw, async_mode=True, seeds=seeds)
    totals = stream_token_schedule(N, first_chunk, chunk, lookahead, chunk_growth)  # tokens decoded when round r starts
    one_round, closed = _stream_rounds(self, B, gen_ref, n_tokens=N + n_extra, round_tokens=round_tokens, lookahead=lookahead, fade=fade, z=z, phase=phase, noise=noise,
                                       n_cfm_timesteps=n_cfm_timesteps, drop_last_token=drop_last_token, window=window, seeds=seeds, speed=speed, format=format)
    if not overlap:  # the serial form of rounds 3-5: T3 waits while a round is synthesised
        h = self.t3.generate(t3_conds, text_tokens, run_steps=totals[0], **t3_kw)
        for r, n_r in enumerate(totals):
            toks, done = self.t3.peek(h)
            exhausted = h["next_i"] >= h["max_new_tokens"]
            yield one_round(toks, done, exhausted)
            if all(closed) or exhausted:
                return
            self.t3.advance(h, totals[r + 1] - n_r)
        return

    # ---- overlapped: T3 on its own stream + host thread, at most `ahead` rounds in front of the vocoder
    import queue
    import threading
    self._pipeline_streams()
    self.co_resident(True)
    torch.cuda.synchronize()
    # T3 run-ahead policy (round 6, measured: profiles/r06_streaming_*): the FIRST round's flow + vocoder decide the first-audio latency, so T3 does not
    # decode beside them (`first_alone`); once the first audio is out T3 may be up to `ahead` rounds in front of the vocoder
    ahead = max(1, int(run_ahead))
    q, stop, credit = queue.Queue(), threading.Event(), threading.Semaphore(1 if first_alone else ahead)

    def worker():
        try:
            torch.cuda.set_device(pin)
            h = None
            with torch.inference_mode(), torch.cuda.stream(self._s_t3):
                for r, n_r in enumerate(totals):
                    credit.acquire()
                    if stop.is_set():
                        return
                    if h is None:
                        h = self.t3.generate(t3_conds, text_tokens, run_steps=n_r, **t3_kw)
                    else:
                        self.t3.advance(h, n_r - totals[r - 1])
                    ev = torch.cuda.Event()
                    ev.record()
                    q.put((h, ev, n_r))
        except BaseException as e:  # re-raised by the consumer
            q.put(e)

    th = threading.Thread(target=worker, name="cbx-t3-stream", daemon=True)
    th.start()
    try:
        for r in range(len(totals)):
            item = q.get()
            if isinstance(item, BaseException):
                raise item
            h, ev, n_r = item
            # the FIRST round decides the first-audio latency and T3 is far ahead of what round 1 needs: its flow runs on the fastest-alone kernel forms (T3's
            # workgroups wait for CU slots meanwhile); from round 1 on both stages share the CUs on the co-resident forms
            self.flow.co_resident(r > 0 or not first_alone)
            with torch.cuda.stream(self._s_voc):  # (not held across the yield: the caller keeps its own current stream)
                self._s_voc.wait_event(ev)
                toks, done = self.t3.peek(h)  # synchronises THIS stream (behind the event); T3 may already be further: a round sees its n_r tokens
                done = [bool(d) and int(t.numel()) <= n_r for d, t in zip(done, toks)]
                toks = [t[:n_r] for t in toks]
                exhausted = n_r >= N
                res = one_round(toks, done, exhausted)
            for _ in range(ahead if (first_alone and r == 0) else 1):
                credit.release()
            yield res
            if all(closed) or exhausted:
                return
    finally:
        stop.set()
        for _ in range(ahead + 1):
            credit.release()
        th.join()
        torch.cuda.synchronize()
        self.co_resident(False)


S3GEN_SIL = 4299  # reference models/s3gen/const.py:2


class TurboEngine(S3GenEngine):
    """ChatterboxTurboTTS hot path (reference tts_turbo.py:298-317): GPT-2 T3 (no CFG) -> ids < 6561 + 3 silence tokens ->
    2-step meanflow S3Gen (no CFG) -> HiFT."""

    def __init__(self, t3_sd, s3gen_sd, device="cuda", n_t3_layers=None):
        from .t3_turbo import T3TurboEngine
        self.t3 = T3TurboEngine(t3_sd, torch.device(device), n_layers=n_t3_layers)  # (T3 first, as in ChatterboxEngine)
        super().__init__(s3gen_sd, device, meanflow=True)

    @ops.on_device
    @torch.inference_mode()
    def synthesize(self, text_tokens, t3_conds, gen_ref, *, max_gen_len=1000, temperature=0.8, top_k=1000, top_p=0.95,
                   repetition_penalty=1.2, uniforms=None, ban_eos=False, ban_from=0, z=None, phase=None, noise=None, generator=None, seeds=None, speed=None, join=None, format=None, loudness=None, pauses=None, pitch=None, warp=None, true_peak=None):
        """t3_conds / gen_ref: one voice or a list of B; temperature, top_k, top_p, repetition_penalty: a scalar or a sequence of B; generator: torch.Generator (device)
        for every draw that is not injected; seeds: None, an int or B ints in [0, 2^64) -- the per-utterance draws of ChatterboxEngine.synthesize(seeds=);
        speed: None, a number or B numbers in [0.5, 2.0] -- the speaking rate of vocode(speed=); join: None, or vocode(join=)'s dict -- the call then returns
        ChatterboxEngine.synthesize(join=)'s piece (truncated: T3 sampled all max_gen_len + 1 tokens without EOS); format: None, or vocode(format=)'s dict; loudness: None, or vocode(loudness=)'s targets (not with a join);
        pauses: None, or vocode(pauses=)'s dict / list, as ChatterboxEngine.synthesize(pauses=) returns its results; pitch: None, or vocode(pitch=)'s semitones,
        checked against speed before anything is launched as ChatterboxEngine.synthesize(pitch=) does; warp: None, or vocode(warp=)'s list with entries of the
        duration kind (None or dict(frames=)): anchors need an alignment pass, which the GPT-2 backbone does not have; true_peak: None, or vocode(true_peak=)'s
        ceilings in dBTP (not with a join)."""
        d = check_delivery(len(text_tokens), seeds=seeds, generator=generator, speed=speed, pitch=pitch, join=join, format=format, loudness=loudness, pauses=pauses,
                           warp=warp, true_peak=true_peak)
        if d.warp is not None and any(w is not None and "anchors" in w for w in d.warp):
            raise ValueError("warp with anchors (timing) on the Turbo engine: the alignment pass on the GPT-2 backbone is not built -- dict(frames=) only")
        seeds = d.seeds
        t0 = time.perf_counter()
        toks = self.t3.generate(t3_conds, text_tokens, max_gen_len=max_gen_len, temperature=temperature, top_k=top_k, top_p=top_p,
                                repetition_penalty=repetition_penalty, uniforms=uniforms, ban_eos=ban_eos, ban_from=ban_from, generator=generator, seeds=seeds)
        torch.cuda.synchronize()
        self.last_timing = dict(t3_s=time.perf_counter() - t0)
        sil = torch.full((3,), S3GEN_SIL, dtype=torch.long)
        st = [torch.cat([t[t < SPEECH_VOCAB], sil]) for t in toks]
        wavs, _ = self.vocode(st, gen_ref, z=z, phase=phase, noise=noise, n_cfm_timesteps=2, drop_last_token=False, generator=generator, seeds=seeds, speed=d.speed,
                              **d.kw())
        if d.join is not None:
            wavs = _joined_on_host(wavs.get("formatted", wavs["out"]), wavs["rec"], wavs["n"], d.fmt, wavs.get("pauses"), self._truncated(toks, max_gen_len))
        self.last_timing["total_s"] = time.perf_counter() - t0
        return wavs, st

    @staticmethod
    def _truncated(toks, max_gen_len):
        """Per utterance of a joined piece: T3 spent its budget without EOS (generate strips a sampled EOS: a chunk that still has max_gen_len + 1 tokens never
        sampled one)."""
        return [int(t.numel()) > max_gen_len for t in toks]

    @torch.inference_mode()
    def synthesize_stream(self, text_tokens, t3_conds, gen_ref, *, first_chunk=25, chunk=50, chunk_growth=1.0, lookahead=3, fade=480, max_gen_len=1000,
                          temperature=0.8, top_k=1000, top_p=0.95, repetition_penalty=1.2, uniforms=None, ban_eos=False, ban_from=0, z=None, phase=None,
                          noise=None, n_cfm_timesteps=2, drop_last_token=False, overlap=True, first_alone=True, run_ahead=2, window=None, seeds=None, speed=None, format=None):
        """Chunked synthesis of Turbo / Nano: the round schedule, yields and overlap / first_alone / run_ahead semantics of ChatterboxEngine.synthesize_stream
        around the GPT-2 T3 (chunked through T3TurboEngine.generate(async_mode=True) / advance / peek) and the 2-step meanflow flow.  A round vocodes the
        sampled ids < 6561; the FINAL round of an utterance appends the three S3GEN_SIL tokens exactly as synthesize() does and keeps every token
        (drop_last_token=False), non-final rounds carry no silence and hold back 2 * lookahead frames.  T3 can sample max_gen_len + 1 tokens: the default
        z / phase / noise cover that many plus the 3 silence tokens.  The last round is a full synthesis: identical mel to synthesize() for the same noise.
        window: the bounded-cost rounds of ChatterboxEngine.synthesize_stream; seeds: its per-utterance seeds; speed: its speaking rate (one number for the stream); format: its delivery format."""
        t3_kw = dict(max_gen_len=max_gen_len, temperature=temperature, top_k=top_k, top_p=top_p, repetition_penalty=repetition_penalty, uniforms=uniforms,
                     ban_eos=ban_eos, ban_from=ban_from)
        sil = torch.full((3,), S3GEN_SIL, dtype=torch.long)

        def round_tokens(toks, fin):
            st = [torch.cat([t[t < SPEECH_VOCAB], sil]) if f else t[t < SPEECH_VOCAB] for t, f in zip(toks, fin)]
            return [t if t.numel() > 0 else torch.zeros(1, dtype=torch.long) for t in st]

        yield from _synthesize_stream(self, text_tokens, t3_conds, gen_ref, n_budget=max_gen_len + 1, t3_kw=t3_kw, round_tokens=round_tokens, n_extra=3,
                                      first_chunk=first_chunk, chunk=chunk, chunk_growth=chunk_growth, lookahead=lookahead, fade=fade, z=z, phase=phase,
                                      noise=noise, n_cfm_timesteps=n_cfm_timesteps, drop_last_token=drop_last_token, overlap=overlap, first_alone=first_alone,
                                      run_ahead=run_ahead, window=window, seeds=seeds, speed=speed, format=format)
