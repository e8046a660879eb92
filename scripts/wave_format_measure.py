"""Delivery formats on the configs[2] shape, one process on one box: eight requests (Multilingual, synthetic 30-layer weights, 64 text tokens, 250 sampled
tokens = 10 s each, 3 voices) through generate_batch, the variants ALTERNATING inside every repetition:
  i    the default format (24 kHz fp32; uses nothing newer than generate_batch, so it also runs from a checkout of the parent commit: `... i`)
  ii   the default followed by what a caller does today on the host, per utterance: frontend.resample (scipy.signal.resample_poly) to 48 kHz + a NumPy PCM16 quantise
  iii  sample_rate=8000, encoding="mulaw"
  iv   sample_rate=48000, encoding="s16"
Prints one JSON line: wall seconds per variant and repetition, and the bytes the variant's device-to-host copies carry (the elements returned times their size).

    python scripts/wave_format_measure.py [variants, default i,ii,iii,iv] [repetitions, default 5]
    python scripts/wave_format_measure.py kernel      # the conversion launch alone on 8 x 10 s (device events here; run it under rocprofv3 --kernel-trace --stats
                                                      # for the launch's own time)
"""
import json
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
from chatterbox_amd import api, frontend, synth  # noqa: E402

dev = torch.device("cuda:0")
FORMATS = dict(iii=dict(sample_rate=8000, encoding="mulaw"), iv=dict(sample_rate=48000, encoding="s16"))


def kernel_only(reps=20):
    from chatterbox_amd import ops
    wav = torch.rand(8, 240000, device=dev) * 1.98 - 0.99
    rows = [wav[b] for b in range(8)]
    out = {}
    for name, fmt in FORMATS.items():
        ops.wave_format(rows, fmt)
        torch.cuda.synchronize()
        us = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ops.wave_format(rows, fmt)
            e1.record()
            torch.cuda.synchronize()
            us.append(e0.elapsed_time(e1) * 1e3)
        out[name] = dict(format=fmt, median_us_between_events=round(statistics.median(us), 1))
    print(json.dumps(dict(kernel_only=out, rows=8, samples_per_row=240000, gpu=torch.cuda.get_device_name(0))), flush=True)


if len(sys.argv) > 1 and sys.argv[1] == "kernel":
    kernel_only()
    sys.exit(0)

variants = (sys.argv[1] if len(sys.argv) > 1 else "i,ii,iii,iv").split(",")
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
m = api.ChatterboxMultilingualTTS.from_synthetic(dev, t3_layers=30)


class Tok:
    def text_to_tokens(self, text, language_id=None):
        return synth.text_tokens(62, seed=len(text)).int().unsqueeze(0)   # + SOT / EOT = 64 text tokens


m.tokenizer = Tok()
gen = m.engine.t3.generate
m.engine.t3.generate = lambda conds, tt, **kw: gen(conds, tt, **dict(kw, max_new_tokens=250, ban_eos=True))
voices = [api.Conditionals(api.T3Cond(**synth.t3_cond(seed=s)), synth.s3gen_ref(seed=s)) for s in (11, 12, 13)]
conds = [voices[k % 3] for k in range(8)]
texts = ["x" * (10 + k) + "." for k in range(8)]


def host_path(wavs):
    """24 kHz fp32 on the host -> 48 kHz PCM16, per utterance"""
    out = []
    for w in wavs:
        y = frontend.resample(w[0].numpy(), 24000, 48000)
        out.append(np.clip(np.rint(y * np.float32(32768.0)), -32768, 32767).astype(np.int16))
    return out


def run(v):
    if v == "i":
        return m.generate_batch(texts, "en", conds=conds)
    if v == "ii":
        return host_path(m.generate_batch(texts, "en", conds=conds))
    return m.generate_batch(texts, "en", conds=conds, **FORMATS[v])


for v in variants:
    run(v)
secs, d2h = {v: [] for v in variants}, {}
for _ in range(reps):
    for v in variants:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = run(v)
        torch.cuda.synchronize()
        secs[v].append(round(time.perf_counter() - t0, 4))
        if v == "ii":
            d2h[v] = int(sum(w.size // 2 * 4 for w in out))   # the fp32 24 kHz copies the host path starts from (it returns 48 kHz arrays)
        else:
            d2h[v] = int(sum(w.numel() * w.element_size() for w in out))
print(json.dumps(dict(variants=variants, seconds=secs, median_s={v: round(statistics.median(t), 4) for v, t in secs.items()},
                      spread_s={v: round(max(t) - min(t), 4) for v, t in secs.items()}, d2h_bytes=d2h, gpu=torch.cuda.get_device_name(0))), flush=True)
