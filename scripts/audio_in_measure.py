"""Audio in on the device against the host path, one process on one box, the modes ALTERNATING inside every repetition (synthetic weights: a 6-layer S3
tokenizer, a 2-layer T3 -- the front-end under test is the same whatever follows it):
  vc1   ChatterboxVC.generate(audio=path), a 60 s 44.1 kHz stereo s16 WAV
  vc4   ChatterboxVC.generate_batch(audios=[4 such files])
  tts   ChatterboxTTS.generate(text, audio_prompt_path=path), a 10 s 44.1 kHz stereo s16 prompt, 50 sampled tokens
Per case and mode: wall seconds of the call, and the seconds from the call to the first flow launch (the entry of the engine's vocode / synthesize: everything
before it is the input path -- decode, resample, trim, the analysis engines).  Prints one JSON line.  A checkout without `audio_in` (the parent commit) runs the
host mode alone, so the same script gives the baseline.

    python scripts/audio_in_measure.py [repetitions, default 5]
    python scripts/audio_in_measure.py kernel      # the ingest launch alone (60 s stereo s16 44100 -> 16000 and -> 24000, B = 1 and 4) and the trim, device events
"""
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, ".")
from chatterbox_amd import api, synth  # noqa: E402

dev = torch.device("cuda:0")


def stereo_s16(seconds, seed):
    a, b = synth.prompt_wav(seconds, 44100, seed=seed).numpy(), synth.prompt_wav(seconds, 44100, seed=seed + 1).numpy()
    return np.stack([np.rint(a * 32767 * 0.8), np.rint(b * 32767 * 0.5)], 1).astype(np.int16)


def kernel_only(reps=20):
    from chatterbox_amd import ops
    out = {}
    for B in (1, 4):
        raw = torch.from_numpy(np.stack([stereo_s16(60.0, 2 * b) for b in range(B)])).to(dev)   # (B, frames, 2) int16
        rows = [raw[b].view(-1) for b in range(B)]
        for rate in (16000, 24000):
            ops.wave_ingest(rows, "s16", 2, 44100, rate)
            torch.cuda.synchronize()
            us = []
            for _ in range(reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                ops.wave_ingest(rows, "s16", 2, 44100, rate)
                e1.record()
                torch.cuda.synchronize()
                us.append(e0.elapsed_time(e1) * 1e3)
            out[f"ingest_B{B}_44100x2_s16_to_{rate}"] = round(statistics.median(us), 1)
    w = ops.wave_ingest([raw[0].view(-1)], "s16", 2, 44100, 16000)
    ops.wave_trim_edges(w, 20.0)
    torch.cuda.synchronize()
    us = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ops.wave_trim_edges(w, 20.0)
        e1.record()
        torch.cuda.synchronize()
        us.append(e0.elapsed_time(e1) * 1e3)
    out["trim_edges_960000_samples"] = round(statistics.median(us), 1)
    print(json.dumps(dict(kernel_only_median_us_between_events=out, gpu=torch.cuda.get_device_name(0))), flush=True)


if len(sys.argv) > 1 and sys.argv[1] == "kernel":
    kernel_only()
    sys.exit(0)

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
from scipy.io import wavfile  # noqa: E402

tmp = tempfile.mkdtemp()
src = []
for k in range(4):
    src.append(os.path.join(tmp, f"src{k}.wav"))
    wavfile.write(src[-1], 44100, stereo_s16(60.0, 10 + 2 * k))
prompt = os.path.join(tmp, "prompt.wav")
wavfile.write(prompt, 44100, stereo_s16(10.0, 30))

vc = api.ChatterboxVC.from_synthetic(dev, tokenizer_layers=6)
tts = api.ChatterboxTTS.from_synthetic(dev, t3_layers=2, with_prompt_nets=True, tokenizer_layers=6)
vc.watermarker = tts.watermarker = None


class Tok:
    def text_to_tokens(self, text, language_id=None):
        return synth.text_tokens(30, seed=len(text), vocab=api.ChatterboxTTS._TEXT_VOCAB)[1:-1].int().unsqueeze(0)


tts.tokenizer = Tok()
gen = tts.engine.t3.generate
tts.engine.t3.generate = lambda conds, tt, **kw: gen(conds, tt, **dict(kw, max_new_tokens=50, ban_eos=True))
first = {}


def stamp(engine, name):
    fn = getattr(engine, name)

    def wrapped(*a, **kw):
        torch.cuda.synchronize()   # (everything the input path enqueued has run: the flow could start here)
        first.setdefault("t", time.perf_counter())
        return fn(*a, **kw)
    setattr(engine, name, wrapped)


stamp(vc.engine, "vocode")
stamp(tts.engine, "synthesize")
modes = ["host", "device"] if hasattr(vc, "audio_in") else ["host"]
CASES = dict(vc1=lambda: vc.generate(audio=src[0], seed=1), vc4=lambda: vc.generate_batch(audios=src, seeds=[1, 2, 3, 4]),
             tts=lambda: tts.generate("aaaa bbbb cccc.", audio_prompt_path=prompt, seed=1))


def set_mode(mode):
    if len(modes) > 1:
        vc.audio_in = tts.audio_in = mode


for mode in modes:
    set_mode(mode)
    for fn in CASES.values():
        fn()
wall = {c: {m: [] for m in modes} for c in CASES}
lead = {c: {m: [] for m in modes} for c in CASES}
for _ in range(reps):
    for c, fn in CASES.items():
        for mode in modes:
            set_mode(mode)
            first.clear()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            wall[c][mode].append(round(time.perf_counter() - t0, 4))
            lead[c][mode].append(round(first["t"] - t0, 4))
med = lambda d: {c: {m: round(statistics.median(t), 4) for m, t in v.items()} for c, v in d.items()}
spread = lambda d: {c: {m: round(max(t) - min(t), 4) for m, t in v.items()} for c, v in d.items()}
print(json.dumps(dict(modes=modes, wall_s=wall, to_first_flow_launch_s=lead, median_wall_s=med(wall), spread_wall_s=spread(wall), median_to_first_flow_launch_s=med(lead),
                      spread_to_first_flow_launch_s=spread(lead), gpu=torch.cuda.get_device_name(0))), flush=True)
